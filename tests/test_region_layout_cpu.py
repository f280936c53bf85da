"""The 4-wave region kernel as the Makefile builds it -- four workgroups per CU -- and the inputs of tests/test_region_layout_gpu.py (no GPU
needed): the compiler's resource summary under exactly the Makefile's W4FLAGS, and, with the oracle alone, that the maps of
tests/region_layout_cases.py reach the edges of the small LDS layout that build takes."""
import os
import re
import subprocess

import numpy as np
import pytest

import region_layout_cases as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc")


def _makefile_var(name):
    txt = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, txt, flags=re.M)
    assert m, name
    return m.group(1).split()


def test_w4_build_fits_four_workgroups_per_cu(tmp_path):
    """k_region.hip under the Makefile's W4FLAGS (read from the Makefile): at most 128 registers, four waves per SIMD, and an LDS that fits a
    CU's 160 KB four times.  The scratch frame measured at this setting is 768 B per lane (592 B at three waves per SIMD: the stages save
    more callee-saved registers per call and keep a few more values of the rare paths in scratch); 5 % on top of that is the bound."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    w4 = _makefile_var("W4FLAGS")
    assert "-DLSD_REGION_NW=4" in w4
    out = str(tmp_path / "k_region_w4.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"] + w4 +
                   ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "k_region.hip")], check=True, capture_output=True)
    text = open(out).read()
    kern = text[text.index("; Kernel info:"):]
    vgprs = int(re.search(r"; NumVgprs: (\d+)", kern).group(1))
    occ = int(re.search(r"; Occupancy: (\d+)", kern).group(1))
    lds = int(re.search(r"; LDSByteSize: (\d+)", kern).group(1))
    scratch = int(re.search(r"; ScratchSize: (\d+)", kern).group(1))
    print("NumVgprs %d Occupancy %d LDSByteSize %d ScratchSize %d" % (vgprs, occ, lds, scratch))
    assert vgprs <= 128, vgprs
    assert occ >= 4, occ
    assert lds * 4 <= 160 * 1024, lds                       # (40 568 B measured)
    assert scratch <= 768 * 105 // 100, scratch             # (768 B measured)


@pytest.fixture(scope="module")
def traces(oracle):
    maps = {"strokes%d" % k: rl.strokes(k) for k in range(8)}
    maps.update(rl.single_maps())
    return {name: oracle.lsd(m.copy(), debug=True)["dbg"] for name, m in maps.items()}


def test_stroke_maps_reach_both_ends_of_the_small_window(traces):
    """At least 5 small regions of the stroke maps leave the 12-row window upwards and stay inside the 16-row one, at least 5 do so
    downwards, at least 5 stay inside the 12-row window -- each of them restated with the size the oracle's trace gives it."""
    lay = rl.layout()
    rows_small, rows_large = lay["rows"]
    assert (rows_small, rows_large) == (12, 16)
    tot = dict(up=0, down=0, inside=0, restated=0, small=0)
    for k in range(8):
        c = rl.window_classes(traces["strokes%d" % k], rows_small, rows_large)
        for f in tot:
            tot[f] += c[f]
    print(tot)
    assert tot["up"] >= 5 and tot["down"] >= 5 and tot["inside"] >= 5, tot
    assert tot["restated"] * 10 >= tot["small"] * 8, tot    # (the restatement follows the trace for most seeds: 94 % here)
    # the regions of the strokes are of 6 .. 15 pixels, several hundred of them
    nums = np.concatenate([traces["strokes%d" % k]["seeds"]["num"] for k in range(8)])
    assert ((nums >= 6) & (nums <= 15)).sum() >= 500


def test_long_edge_diagonal_and_regrown_region_have_the_sizes_the_device_test_relies_on(traces):
    lay = rl.layout()
    lcap = lay["lcap"][0]
    # a first grow's list is as long as the trace's num: longer than the small ring by 64 entries and more (and than the large one)
    s = traces["long_edge"]["seeds"]
    assert s["num"].max() >= lcap + 64 and s["num"].max() > lay["lcap"][1], s["num"].max()
    # the diagonal: the first long region, grown before any line was accepted, restated from the map -- its pixels lie in more 8 x 8 tiles
    # than a wave's tile cache has slots
    d = traces["diagonal"]
    s = d["seeds"]
    i = int(np.argmax(s["num"] > 100))
    assert s["num"][i] > 100 and not (s["outcome"][:i] == 3).any()
    xs, ys = rl.grow(d["deg"], d["used0"], int(s["x"][i]), int(s["y"][i]))
    assert len(xs) == s["num"][i]
    assert len({(x >> 3, y >> 3) for x, y in zip(xs, ys)}) > lay["nt"]
    # a region of more than 64 and fewer than 128 pixels that Refiner grows again (another size) and the NFA test rejects (outcome 2)
    s = traces["regrown"]["seeds"]
    hit = (s["num"] > 64) & (s["num"] < 128) & (s["outcome"] == 2) & (s["final_num"] != s["num"])
    assert hit.any()
