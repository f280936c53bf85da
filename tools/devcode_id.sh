#!/bin/bash
# developer tool: what identifies an object's gfx950 device code -- SHA-256 of the code object's .text and .rodata, and every kernel's
# registers, LDS and scratch.  (Whole objects and whole code objects differ with the source's path and text; these do not.)  No GPU needed.
#    tools/devcode_id.sh <object>...        e.g. linesegmentdetector-slam_amd/csrc/k_region_w{4,8}.o
set -euo pipefail
LLVM=${LLVM:-/opt/rocm/llvm/bin}
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
for o in "$@"; do
  echo "== $(basename "$o")"
  "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$o" "$T/fatbin"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --input="$T/fatbin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$T/co"
  for s in .text .rodata; do
    rm -f "$T/sec"
    "$LLVM/llvm-objcopy" -O binary --only-section=$s "$T/co" "$T/sec"
    if [ -s "$T/sec" ]; then echo "$s sha256 $(sha256sum < "$T/sec" | cut -d' ' -f1) ($(stat -c %s "$T/sec") bytes)"; else echo "$s none"; fi
  done
  "$LLVM/llvm-readelf" --notes "$T/co" |
    awk '/^ *(- )?\.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):/ { sub(/^ *(- )?/, ""); v[$1] = $2 }
         /^ *\.vgpr_count:/ { print v[".name:"], "vgpr", v[".vgpr_count:"], "sgpr", v[".sgpr_count:"], "lds", v[".group_segment_fixed_size:"], "scratch", v[".private_segment_fixed_size:"] }'
done
