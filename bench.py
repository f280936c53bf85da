#!/usr/bin/env python3
"""bench.py -- the headline benchmark: whole-pipeline LSD throughput (Mpixels/s and lines/s) on a batch of
512 synthetic 2048x2048 occupancy maps (BASELINE.json configs[3]/[4], SURVEY 8d "C4").

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W [--scaling strong]

One process per GPU.  A "step" is one pass of the hot path (remap -> Gaussian -> gradient -> sort -> region
grow/rectangle/NFA -> line list + raster) over this rank's images, inputs resident in HBM.  Images are independent, so
ranks never exchange data on the path; for N > 1 each step ends with the RCCL gather of the ragged line lists to
rank 0 -- two regular collectives, no host synchronisation.
  --scaling weak   (default; what the driver's N = 1 line and its scaling curve use): every GPU gets its own --batch images;
  --scaling strong (BASELINE configs[4] as written): the SAME --batch images are split over the ranks, contiguous shards.
Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times --steps steps and prints the headline figure (with
--dump-outputs DIR it first writes what the last timed step computed).  With --full, after the timed region: one step at a time
(per-kernel times, roofline, region-stage cycles), the strong split and the check of the gathered results (N > 1), and (N = 1,
unless --no-cpu-baseline) the targets north_star names on mapValue_map1 (512 x replicated map1 -> lines/s; one host-ABI call
createMapCache + myLineSegmentDetector), the single-image latency, the device copy ceiling and the CPU baseline (SURVEY 8d protocol).
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

# Throughput mode keeps several steps in flight, one stream each; the HIP runtime maps streams onto 4 hardware queues unless told
# otherwise, and streams that share a queue run their kernels one after the other.  One queue per step in flight (read when the
# runtime initialises, i.e. before torch touches the GPU).  The timed region has 8 in flight; the projection
# of the sharded job (strong_scaling_projection, throughput mode) up to 32.  Measured (tools/k20_sweep.sh, tools/cumask_probe.py):
# 8 steps in flight run at the same rate on 8 and on 16 queues; 32 queues cost the single step with help 15 % and the driver's
# 20-step run 8 %; 32 small steps in flight on 16 queues (two streams per queue) run as well as on 32, on 8 queues at half the rate.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SOURCES = ["aisle1", "aisle2", "aisle3", "mapValue"]   # the four aisle-class fixtures
HBM_PEAK_GBS = 8000.0                                   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
GRAD_BYTES_PER_PX = 25.0                                # K2: 8 B read + 8+8+1 B written per scaled pixel
# the unmodified reference, single thread, survey container (it cannot be built on the GPU box)
REF_MAP1 = {"ms": 5.20, "lines_per_s": 1346.0, "Mpix_per_s": 56.1}
REF_TILE2048 = {"ms": 1362.0, "lines_per_s": 175.0, "Mpix_per_s": 3.1}


def make_image(maps, i, size):
    """Image i of the synthetic batch: tile + roll + flip of one of four fixtures, seeded by i."""
    src = maps[SOURCES[i % 4]]
    hs, ws = src.shape
    canvas = np.tile(src, (-(-size // hs) + 1, -(-size // ws) + 1))
    if i == 0:
        dy = dx = 0
    else:
        rng = np.random.default_rng(1234 + i)
        dy, dx = (int(v) for v in rng.integers(0, [hs, ws]))
    canvas = np.roll(canvas, (dy, dx), (0, 1))[:size, :size]
    f = (i // 4) % 4
    if f & 1:
        canvas = canvas[:, ::-1]
    if f & 2:
        canvas = canvas[::-1, :]
    return np.ascontiguousarray(canvas)


REAL_MAPS = ["map1", "mapValue", "aisle1", "aisle2", "aisle3", "f3key", "f4key"]   # the reference's own maps, un-tiled (data*/mapValue*.txt)


def make_pasted(maps, size=2048):
    """One size x size canvas of DIFFERENT reference maps side by side on the maps' own background value (0: every fixture's border is
    0), nothing tiled, rolled or wrapped -- so no seams and no repeated structure: f3key top left, f4key below it, aisle3 turned by 90
    degrees along the right edge.  Only defined for size >= 2048."""
    if size < 2048:
        return None
    c = np.zeros((size, size), np.uint8)
    a, b, r = maps["f3key"], maps["f4key"], np.ascontiguousarray(np.rot90(maps["aisle3"]))
    c[:a.shape[0], :a.shape[1]] = a
    c[990:990 + b.shape[0], :b.shape[1]] = b
    c[:r.shape[0], size - r.shape[1]:] = r
    return c


def make_batch(maps, n, size, first=0):
    out = np.empty((n, size, size), np.uint8)
    for j in range(n):
        out[j] = make_image(maps, first + j, size)
    return out


def source_sha():
    """Identifies the kernel sources a number was measured on (sha1 over csrc/*.hip, *.h): the PMC traffic file carries the same."""
    import glob, hashlib
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc", "*.h"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def steady_rate_ms(done_ms, slots):
    """ms per step at the steady rate of a pipeline with `slots` steps in flight: done_ms[i] = completion time of step i (which ran on
    slot i % slots, slots refilled in order).  The rate is taken between the `slots`-th completion and the moment the first slot has
    nothing left to run: the fill at the start and the drain at the end -- and, with a fixed number of steps per slot, the wait for
    the slowest slot -- stay outside.  A window of fewer than `slots` completions falls back to last completion / steps."""
    done = np.asarray(done_ms, dtype=np.float64)
    steps = len(done)
    t_dry = min(done[j::slots].max() for j in range(slots))
    order = np.sort(done)
    k1, k2 = slots, int(np.searchsorted(order, t_dry, side="right"))
    if k2 - k1 < slots:
        return float(order[-1]) / steps
    return float(order[k2 - 1] - order[k1 - 1]) / (k2 - k1)


def load_maps():
    z = np.load(os.path.join(ROOT, "tests", "golden", "maps.npz"))
    return {k: z[k] for k in z.files}


def keep_heap():
    """glibc hands blocks above 128 KB straight to mmap and gives them back on free: every oracle call would map, page-fault and
    unmap ~30 MB of work arrays (the reference's own malloc pattern).  Keeping the heap makes the calls after the first reuse it."""
    import ctypes
    libc = ctypes.CDLL("libc.so.6")
    libc.mallopt(-3, 1 << 30)       # M_MMAP_THRESHOLD
    libc.mallopt(-1, 1 << 30)       # M_TRIM_THRESHOLD


# ---- CPU baseline: the oracle = a single-threaded port of the reference path, on the GPU box's host cores ----
def _cpu_worker(args):
    """One pinned single-thread oracle instance over its own slice of the batch (the reference has no intra-image threading)."""
    core, first, count, size, reps = args
    try:
        os.sched_setaffinity(0, {core})
    except (AttributeError, OSError):
        pass
    from oracle import oracle
    maps = load_maps()
    oracle.lsd(maps["map1"].copy())                                 # warm-up
    imgs = [make_image(maps, first + k, size) for k in range(count)]
    times, nl = [], 0
    for rep in range(reps + 1):                                     # 1 warm-up pass + reps timed passes over the sample
        t0 = time.perf_counter()
        nl = 0
        for im in imgs:
            nl += len(oracle.lsd(im.copy(), want_lineim=True)["lines"])
        if rep:
            times.append(time.perf_counter() - t0)
    return times, nl


def cpu_baseline(size, first, sample=24, reps=5):
    from oracle import oracle
    oracle.build()
    cores = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    times, nl = _cpu_worker((cores[0], first, sample, size, reps))  # one pinned core: min and median of `reps` passes (this process stays pinned until unpin() below)
    def unpin():
        # the bench process must not stay on one core: threads started later inherit the mask of the thread that starts them
        try:
            os.sched_setaffinity(0, set(cores))
        except (AttributeError, OSError):
            pass
    px = sample * size * size / 1e6
    tmin, tmed = min(times), statistics.median(times)
    out = {"value": px / tmin, "unit": "Mpix/s", "cores": 1, "kind": "port",
           "sample": "images %d..%d of the same %dx%d batch, oracle/lsd_oracle.c single thread pinned to core %d, 1 warm-up + %d passes "
                     "(min %.2f s, median %.2f s)" % (first, first + sample - 1, size, size, cores[0], reps, tmin, tmed),
           "value_median": px / tmed, "lines_per_s": nl / tmin,
           # the port skips the reference's two full-image scans per region; the unmodified reference was measured in the survey
           # container (other host): 3.1 Mpix/s / 175 lines/s on the 2048^2 tile, i.e. the port is ~25-40x faster
           "true_reference_Mpix_per_s": REF_TILE2048["Mpix_per_s"], "true_reference_lines_per_s": REF_TILE2048["lines_per_s"],
           "true_reference_source": "BASELINE.md section 2 (survey container; the reference needs OpenCV/Eigen headers and cannot be built here)"}
    m1 = load_maps()["map1"]                                        # the port on mapValue_map1, same core (min of 30 calls)
    t1 = []
    for _ in range(31):
        m = m1.copy()
        t0 = time.perf_counter()
        r = oracle.lsd(m, want_lineim=True)
        t1.append(time.perf_counter() - t0)
    out["map1"] = {"ms": min(t1[1:]) * 1e3, "lines_per_s": len(r["lines"]) / min(t1[1:]), "kind": "port"}
    img0 = make_image(load_maps(), first, size)                     # the port on ONE image of the batch (what single_image_latency_ms times on the GPU)
    t0s = []
    for _ in range(4):
        m = img0.copy()
        t0 = time.perf_counter()
        oracle.lsd(m, want_lineim=True)
        t0s.append(time.perf_counter() - t0)
    out["single_image_ms"] = min(t0s[1:]) * 1e3
    # the port on the reference's own maps as they are, and on the pasted canvas (what extras() times on the GPU as `real_maps`)
    rm = {}
    mp_ = load_maps()
    todo = [(k, mp_[k]) for k in REAL_MAPS] + ([("pasted2048", make_pasted(mp_, size))] if size >= 2048 else [])
    for name, im in todo:
        ts_ = []
        for _ in range(3):
            m = im.copy()
            t0 = time.perf_counter()
            r = oracle.lsd(m, want_lineim=True)
            ts_.append(time.perf_counter() - t0)
        rm[name] = {"ms": min(ts_[1:]) * 1e3, "lines": len(r["lines"])}
    out["real_maps"] = rm
    unpin()
    try:                                                            # N-core figure: N independent pinned instances over disjoint images
        import multiprocessing as mp
        # how many cores this process may actually use: its affinity mask, cut down to the cgroup's CPU quota (a container that
        # sees 256 CPUs but is given 16 CPUs' worth of time runs 256 pinned instances 16x slower each: the measured "collapse" of the
        # all-cores figure in rounds 2-3) and to one hardware thread per physical core
        quota = None
        try:
            q, per_us = open("/sys/fs/cgroup/cpu.max").read().split()
            if q != "max":
                quota = float(q) / float(per_us)
        except (OSError, ValueError):
            pass
        sib = {}
        for c_ in cores:
            try:
                key = open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c_).read().strip()
            except OSError:
                key = str(c_)
            sib.setdefault(key, c_)
        phys = sorted(sib.values())
        use = phys[:max(1, int(quota))] if quota and quota < len(phys) else phys
        per = max(4, sample // 3)
        def run_pool(cs):
            with mp.get_context("spawn").Pool(len(cs)) as pool:
                t0 = time.perf_counter()
                res = pool.map(_cpu_worker, [(c_, first + sample + j * per, per, size, 1) for j, c_ in enumerate(cs)])
                return res, time.perf_counter() - t0
        res, wall = run_pool(use)
        slowest = max(r[0][0] for r in res)                         # timed pass of the slowest instance (start-up excluded)
        val = len(use) * per * size * size / 1e6 / slowest
        out["all_cores"] = {"cores": len(use), "value": val, "unit": "Mpix/s", "lines_per_s": sum(r[1] for r in res) / slowest,
                            "per_core_vs_one_core": val / len(use) / out["value"],
                            "host": {"logical_cpus_in_affinity_mask": len(cores), "physical_cores": len(phys), "cgroup_cpu_quota": quota},
                            "sample": "%d instances x %d images, each pinned to its own physical core; slowest instance %.2f s (wall incl. start-up %.1f s).  "
                                      "Cores = min(physical cores in the affinity mask, the cgroup's cpu.max quota): this container sees %d logical CPUs "
                                      "but is given %s CPUs' worth of time, which is why one instance per visible CPU ran ~16-27x slower each in "
                                      "rounds 2-3" % (len(use), per, slowest, wall, len(cores), "%.0f" % quota if quota else "all")}
    except Exception as e:                                          # (a sandbox without process spawning: the 1-core figure stands)
        out["all_cores"] = {"error": repr(e)}
    return out


def launch_command(argv, gpus, port=None):
    """The command line that starts one rank per GPU (what the driver's own launch looks like): used when bench.py is started with
    --gpus N > 1 and no rendezvous in the environment.  `argv` = this process's arguments without the launcher-only flags."""
    if port is None:
        import socket
        with socket.socket() as s_:                                 # a free port on the loopback interface (the container's hostname may not resolve)
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def launch_ranks(a, argv):
    """`python3 bench.py --gpus N` without an external torch.distributed.run: start the N ranks as a CHILD job, relay its output (the one
    JSON line of rank 0) and return its exit code.  Nothing in this process has touched the GPU (torch is not even imported yet) --
    replacing a process that has initialised HIP by another program takes the box down on this pool, so the ranks are children, never
    an exec.  --dry-launch prints the command instead of running it (tests/test_bench_host.py)."""
    import subprocess
    argv = [x for x in argv if x != "--dry-launch"]
    n_vis = None
    try:
        import torch                                                # device_count() alone does not initialise the GPU on this image
        n_vis = torch.cuda.device_count()
    except Exception:
        pass
    cmd = launch_command(argv, a.gpus)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")               # RCCL / dmabuf IPC on this pool (the image exports it already)
    env.setdefault("GPU_MAX_HW_QUEUES", "16")
    if a.dry_launch:
        print(json.dumps({"launch": cmd, "env": {k: env[k] for k in ("HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES")}, "visible_gpus": n_vis}), flush=True)
        return 0
    if n_vis is not None and n_vis < a.gpus:
        print("bench.py: --gpus %d but this node shows %d GPU(s)" % (a.gpus, n_vis), file=sys.stderr)
        return 2
    p = subprocess.run(cmd, env=env)
    return p.returncode


def fit_depth(depth, need_per_slot, need_fixed, free_bytes, floor=4):
    """Steps in flight that fit the free HBM of this rank: `depth` if depth x need_per_slot + need_fixed fits, else the largest depth
    >= 1 that does (never above `depth`).  Returns (depth, note or None).  DESIGN.md section 5: 4 in flight cost ~3 % against 8."""
    if depth <= 1 or depth * need_per_slot + need_fixed <= free_bytes:
        return depth, None
    fit = int((free_bytes - need_fixed) // max(1, need_per_slot))
    new = max(1, min(depth, fit))
    if new >= floor:
        new = max(floor, new)
    return new, ("%d steps in flight need %.0f GB of HBM (%.1f GB per slot), %.0f GB are free on this GPU: running %d in flight"
                 % (depth, (depth * need_per_slot + need_fixed) / 1e9, need_per_slot / 1e9, free_bytes / 1e9, new))


DUMP_BYTES = 64 << 20                                   # --dump-outputs writes at most this much in all
LINE_FIELDS = ("k", "b", "dx", "dy", "x1", "y1", "x2", "y2", "len", "orient")
NONFINITE_FIELDS = ("k", "b")                           # slope and intercept: +-inf (or NaN) for a vertical line, as the reference keeps them


def dump_outputs(path, lsd, slot, n, max_lines):
    """--dump-outputs: what the caller of the timed path received from one step (`slot` = its line records, counts and lineIm
    buffers on the device), as .npy files two builds can be compared by, at most DUMP_BYTES in all:
      counts.npy         float64 [n]         the library's line count per image (above max_lines: the list overflowed; -1: given up)
      lines.npy          float64 [rows, 13]  image index, then k b dx dy x1 y1 x2 y2 len orient of every stored line record, images in order,
                                             then the class of k and of b: 0 finite, 1 +inf, -1 -inf, 2 NaN (k or b is 0 where not finite)
      line_im.npy        float32 [k, H, W]   the lineIm rasters (0 / 255) of k images drawn with a fixed seed, as many as the budget holds
      line_im_index.npy  float64 [k]         which images those are
    Should the line records take more than half the budget (not at the default sizes), they are kept for a seeded sample of images."""
    d_lines, d_counts, d_ims = slot
    os.makedirs(path, exist_ok=True)
    order = np.random.default_rng(0).permutation(n)
    counts = d_counts[:n].cpu().numpy().astype(np.float64)
    rows = np.clip(counts, 0, max_lines).astype(np.int64)
    rec = d_lines[:n].cpu().numpy().view(lsd.LINE_DTYPE).reshape(n, max_lines)
    keep = np.zeros(n, bool)
    keep[order[np.cumsum(rows[order] * 8 * (1 + len(LINE_FIELDS) + len(NONFINITE_FIELDS))) <= DUMP_BYTES // 2]] = True
    idx = np.flatnonzero(keep)
    recs = np.concatenate([rec[i, :rows[i]] for i in idx] + [np.zeros(0, lsd.LINE_DTYPE)])
    fin = {f: np.isfinite(recs[f]) for f in NONFINITE_FIELDS}
    lines = np.column_stack([np.repeat(idx, rows[idx])] + [np.where(fin[f], recs[f], 0.0) if f in fin else recs[f] for f in LINE_FIELDS] +
                            [np.select([fin[f], np.isposinf(recs[f]), np.isneginf(recs[f])], [0.0, 1.0, -1.0], 2.0) for f in NONFINITE_FIELDS]).astype(np.float64)
    np.save(os.path.join(path, "counts.npy"), counts)
    np.save(os.path.join(path, "lines.npy"), lines)
    if d_ims is not None:
        per_image = 4 * d_ims.shape[1] * d_ims.shape[2]
        k = int(min(n, (DUMP_BYTES - (1 << 12) - 8 * n - counts.nbytes - lines.nbytes) // per_image))
        sel = np.sort(order[:max(k, 0)])
        ims = np.zeros((len(sel),) + tuple(d_ims.shape[1:]), np.float32)
        for j, i in enumerate(sel):
            ims[j] = d_ims[int(i)].cpu().numpy()
        np.save(os.path.join(path, "line_im.npy"), ims)
        np.save(os.path.join(path, "line_im_index.npy"), sel.astype(np.float64))


def dumped_line_records(lines, lsd):
    """lines.npy of dump_outputs back to (image index per record, LINE_DTYPE records), k and b +-inf / NaN again where they were."""
    rec = np.zeros(len(lines), lsd.LINE_DTYPE)
    for c, f in enumerate(LINE_FIELDS):
        rec[f] = lines[:, 1 + c]
    for c, f in enumerate(NONFINITE_FIELDS):
        cls = lines[:, 1 + len(LINE_FIELDS) + c]
        rec[f] = np.select([cls == 1, cls == -1, cls == 2], [np.inf, -np.inf, np.nan], rec[f])
    return lines[:, 0].astype(np.int64), rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (default: what the driver passes).  The timed region starts with an empty pipeline and ends "
                    "with the drain of the steps in flight -- about one step latency, 0.3 s at depth 8 -- so a short run under-reports the rate a "
                    "service sees: 20 steps ~45 ms per step, --steps 128 ~39")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512, help="images per GPU (weak scaling) or in total (strong scaling)")
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--max-lines", type=int, default=1024)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--full", action="store_true", help="besides the headline figure, measure and check everything else after the timed region: one step at a time "
                    "(per-kernel times, roofline, region-stage cycles), the strong split and the gathered results (N > 1), and, unless --no-cpu-baseline, "
                    "the CPU baseline, map1 targets, reference maps, single-image latency, strong-scaling projection and copy ceiling")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline, map1 targets, reference maps, single-image latency, "
                    "strong-scaling projection and copy ceiling (what the profiling passes use)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed region, write what rank 0's last timed step computed to DIR/*.npy (float64 / float32, "
                    "at most 64 MB): counts, every line record and the lineIm rasters of a fixed, seeded sample of images")
    ap.add_argument("--no-lineim", action="store_true")
    ap.add_argument("--force-dist", action="store_true", help="exercise the RCCL gather path even with one rank (testing)")
    ap.add_argument("--pipeline", type=int, default=8, help="steps in flight: step i runs on context / stream i %% depth, so that the tail of one step's region stage "
                    "(a few images on a CU each) overlaps the head of the next one's; 1 = one step at a time")
    ap.add_argument("--waves", type=int, default=-1, choices=(-1, 0, 4, 8), help="wavefronts per image of the region stage in the timed region: 0 = the library's choice "
                    "(8 for this batch size: lowest latency of one batch), 4 = two images per CU (highest throughput per CU); -1 = 4 with several steps in flight, else 0")
    ap.add_argument("--help-waves", type=int, default=0, help="helper wavefronts per image (lsd_set_region_help) while several steps are in flight (experiments; 0 = off)")
    ap.add_argument("--cost-history", action="store_true", help="experiments: lsd_set_cost_history(1) on every context of the timed region")
    ap.add_argument("--tail-help", type=int, default=0, help="experiments: the last N steps of the timed region are enqueued with the help across workgroups ON (no further "
                    "step will come to fill the CUs their last images leave idle); measured with 20 steps at depth 8: 0 / 4 / 7 / 8 -> 44.9 / 45.3 / 46.8 / 68.4 ms per step")
    ap.add_argument("--dry-launch", action="store_true", help="with --gpus N > 1 and no WORLD_SIZE in the environment: print the command that would start the ranks and exit")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")

    # `python3 bench.py --gpus N` started the way `--gpus 1` is (no torch.distributed.run around it): start the ranks ourselves, as a
    # child job, BEFORE anything here touches the GPU
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(a, sys.argv[1:]))

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d" % (a.gpus, world, a.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    use_dist = world > 1 or (a.force_dist and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)    # RCCL

    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    ldist = importlib.import_module("linesegmentdetector-slam_amd.dist")
    ctx = lsd.Context(local)
    maps = load_maps()

    size = a.size
    if a.scaling == "weak":
        n, n_total, first = a.batch, a.batch * world, rank * a.batch      # every GPU gets its own images
    else:
        n_total = a.batch                                                  # the same batch, contiguous shards
        lo, hi = ldist.shard_range(n_total, world, rank)
        n, first = hi - lo, lo
    host = make_batch(maps, n, size, first)
    d_maps = torch.from_numpy(host).to(dev)
    del host
    # Steps in flight (--pipeline): every slot has its own context (= workspace), stream and output buffers; all read the same
    # resident input.  With several steps in flight the help across workgroups is off: the next step's workgroups take the
    # CUs a step's last images leave idle, helpers would hold them (include/lsd_hip.h, lsd_set_region_help).
    depth = max(1, a.pipeline)
    waves = a.waves if a.waves >= 0 else (4 if depth > 1 else 0)
    # Does the depth fit this GPU?  A slot = one context's workspace (lsd_reserve: 103 B per scaled pixel on 4 wavefronts per image, 146 on
    # 8; include/lsd_hip.h) + its output buffers: ~22 GB for 512 x 2048^2 maps, ~180 GB at depth 8 of the 288 GB.  A GPU that does not
    # have that free (another tenant, a smaller part) runs fewer steps in flight -- 4 cost ~3 % -- and says so.
    ws_w, ws_h = lsd.scaled_size(size, size)
    slot_bytes = int(n * ((103 if waves == 4 else 146) * ws_w * ws_h * 1.03 + a.max_lines * 80 + 4 + (0 if a.no_lineim else size * size)))
    depth_asked = depth
    depth, depth_note = fit_depth(depth, slot_bytes, 2 << 30, torch.cuda.mem_get_info(dev)[0])
    if depth_note and rank == 0:
        print("bench.py: " + depth_note, file=sys.stderr)
    if use_dist:                                            # every rank the same depth (the gathers are issued per slot, in the same order everywhere)
        dmin = torch.tensor([depth], dtype=torch.int32, device=dev)
        dist.all_reduce(dmin, op=dist.ReduceOp.MIN)
        depth = int(dmin.item())
    waves = a.waves if a.waves >= 0 else (4 if depth > 1 else 0)
    ctxs = [ctx] + [lsd.Context(local) for _ in range(depth - 1)]
    outs = [(torch.zeros((n, a.max_lines, 10), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
             None if a.no_lineim else torch.zeros((n, size, size), dtype=torch.uint8, device=dev)) for _ in range(depth)]
    # (all of torch's 32 pool streams are taken here, back to back: the projection of the sharded job below keeps up to 32 steps in
    #  flight, and streams taken one by one between other allocations ended up unevenly spread over the hardware queues)
    tstreams = [torch.cuda.Stream(device=dev) for _ in range(max(depth, 32))]
    d_lines, d_counts, d_ims = outs[0]
    stream = tstreams[0].cuda_stream
    for c_ in ctxs:
        if depth > 1:
            c_.set_region_help(a.help_waves)
        if a.cost_history:
            c_.set_cost_history(True)
        c_.set_region_waves(waves)                          # (before reserve: the per-wave workspace is sized for the variant)
        c_.reserve(n, size, size)
    w, h = lsd.scaled_size(size, size)
    kt = {k: 0.0 for k in ("gauss", "gradient", "sort", "region", "lines", "total")}
    cap_rows = max(-(-n_total // world), 1) * 512          # slab of the per-step gather: 512 lines per image of the LARGEST shard on average (the same on every rank; flagged if exceeded)
    # the hand-off of the line lists goes through the C ABI (lsd_gather_lines: device pack + two all-gathers on the step's stream);
    # its communicator is bound to the torch.distributed group here (RCCL), a C++ host binds it with lsd_comm_from_rccl
    comm = ldist.torch_comm() if use_dist else None

    tail_help = max(0, a.tail_help) if depth > 1 else 0

    # what a step works on: this rank's images of the job (the weak job by default; the strong split of the same batch re-uses the
    # contexts and output buffers for its smaller shard, see "strong_split" below)
    job = {"maps": d_maps, "n": n, "n_total": n_total, "cap_rows": cap_rows}

    def step(i, collect, last=False):
        j = i % depth
        l_, c_, im_ = outs[j]
        m_ = job["n"]
        if depth > 1:                                      # (a host-side setting of the context, read at the enqueue)
            ctxs[j].set_region_help(-1 if last else a.help_waves)
        ctxs[j].enqueue_device(job["maps"].data_ptr(), m_, size, size, l_.data_ptr(), a.max_lines, c_.data_ptr(),
                               d_line_ims=None if im_ is None else im_.data_ptr(), stream=tstreams[j].cuda_stream)
        res = None
        if use_dist:
            with torch.cuda.stream(tstreams[j]):
                res = ldist.gather_lines_abi(ctxs[j], comm, l_[:m_], c_[:m_], job["n_total"], job["cap_rows"], stream=tstreams[j].cuda_stream)
        if collect:                                        # HIP events recorded on the launch stream by the library (this waits for the step)
            for k, v in ctxs[j].timings().items():
                kt[k] += v
        return res

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # set-up, not a step: every context's first launch (module load, attribute calls, the first touch of its workspace) happens here,
    # on one image, so that a warm-up shorter than the number of steps in flight does not leave first launches inside the timed region
    for j in range(depth):
        l_, c_, im_ = outs[j]
        ctxs[j].enqueue_device(d_maps.data_ptr(), 1, size, size, l_.data_ptr(), a.max_lines, c_.data_ptr(),
                               d_line_ims=None if im_ is None else im_.data_ptr(), stream=tstreams[j].cuda_stream)
    barrier()
    for i in range(a.warmup):
        step(i, False)
    barrier()
    t0 = time.perf_counter()
    res, res_slot = None, {}
    for i in range(a.steps):
        res = step(i, depth == 1, last=i >= a.steps - tail_help)
        res_slot[i % depth] = res                          # the gathered result of every slot's last step (checked below, all of them)
    torch.cuda.synchronize()
    barrier()
    dt = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:                       # (before anything below runs on the slots' output buffers)
        dump_outputs(a.dump_outputs, lsd, outs[(a.steps - 1) % depth], n, a.max_lines)
    # The strong split next to the weak line (N > 1, --scaling weak): the SAME --batch images (rank 0's) split over the ranks in contiguous
    # shards (BASELINE configs[4], the split north_star's "1 -> 8 GPUs on a 512-image batch" means), same contexts, same depth, same
    # protocol (barrier, K steps, barrier, max over ranks).  A shard is 1/N of the images, so a rank's GPU is 1/N as full as in the weak
    # job: DESIGN.md section 6 says what that costs and what a rank that keeps N x as many steps in flight gets back.
    strong_dt = None
    if a.full and use_dist and a.scaling == "weak":            # (use_dist: world > 1, or one rank under --force-dist -- the tests' way into this path)
        lo_s, hi_s = ldist.shard_range(a.batch, world, rank)
        strong_err = torch.zeros(1, dtype=torch.int32, device=dev)
        try:
            d_shard = torch.from_numpy(make_batch(maps, hi_s - lo_s, size, lo_s)).to(dev)
        except Exception as e:                             # (this rank cannot take part: every rank skips the pass, see below)
            print("bench.py rank %d: strong split skipped: %r" % (rank, e), file=sys.stderr)
            d_shard = None
            strong_err += 1
        dist.all_reduce(strong_err, op=dist.ReduceOp.MAX)
        if int(strong_err.item()) == 0:
            job_weak = dict(job)
            per_s = -(-a.batch // world)                   # the largest shard: the gathered slabs have the same size on every rank
            job.update({"maps": d_shard, "n": hi_s - lo_s, "n_total": a.batch, "cap_rows": max(per_s, 1) * 512})
            for i in range(min(a.warmup, depth)):
                step(i, False)
            barrier()
            t0s = time.perf_counter()
            for i in range(a.steps):
                step(i, False)
            torch.cuda.synchronize()
            barrier()
            strong_dt = time.perf_counter() - t0s
            job.update(job_weak)
            for i in range(depth):                         # the slots' outputs and gathered copies hold the weak job's step again (read and checked below)
                res_slot[i] = step(i, False)
            barrier()
        del d_shard
    # the front end inside the timed region: HIP events of every slot's LAST step, event to event -- with several steps in flight that
    # includes the wait for room beside the region stage's workgroups (one step at a time: kernel_ms below)
    tr_front = [c_.timings() for c_ in ctxs[:min(depth, a.steps)]] if a.full and depth > 1 else []
    last = outs[(a.steps - 1) % depth]
    w_, h_ = lsd.scaled_size(size, size)
    timed_cyc = np.array([ctxs[(a.steps - 1) % depth].fetch(i, lsd.DBG_STATS, (w_, h_))["cycles_total"] for i in range(n)], np.float64) if a.full and rank == 0 else None
    if timed_cyc is not None and (timed_cyc > 0).any():
        timed_cyc = timed_cyc[timed_cyc > 0]
    # One step at a time, after the timed region when that ran with several in flight: the per-kernel figures (inside an
    # overlapped region a launch's HIP events also time its wait for a CU) and the step time of a single batch, help on.
    un_steps, un_dt, hist_dt = a.steps, dt, None
    if a.full and depth > 1:
        ctx.set_region_help(-1)
        ctx.set_region_waves(0)
        un_steps = min(a.steps, 5)
        depth_saved, depth = depth, 1
        step(0, False); step(0, False)
        barrier()
        t1 = time.perf_counter()
        for i in range(un_steps):
            step(0, True)
        torch.cuda.synchronize()
        barrier()
        un_dt = time.perf_counter() - t1
        # ... and the same with the scheduling hint a caller that re-extracts the SAME maps step after step can give (lsd_set_cost_history:
        # the images start in the order of their cost in the previous call instead of by their count of gradient pixels)
        ctx.set_cost_history(True)
        step(0, False); step(0, False)
        barrier()
        t2 = time.perf_counter()
        for i in range(un_steps):
            step(0, False)
        torch.cuda.synchronize()
        barrier()
        hist_dt = time.perf_counter() - t2
        ctx.set_cost_history(False)
        depth = depth_saved
    tmax = torch.tensor([dt, un_dt, strong_dt or 0.0], dtype=torch.float64, device=dev)
    nl = last[1].sum().to(torch.float64).reshape(1)
    if use_dist:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(nl, op=dist.ReduceOp.SUM)
    dt, un_dt = float(tmax[0].item()), float(tmax[1].item())
    strong_dt = float(tmax[2].item()) if strong_dt else None
    total_lines = float(nl.item())
    overflow = int((last[1] > a.max_lines).sum().item())

    if rank == 0:
        step_s = dt / a.steps
        mpix = n_total * size * size / 1e6
        out = {
            "metric": "Mpixels/sec LSD (grad+grow+NFA)", "value": mpix / step_s, "unit": "Mpix/s", "n_gpus": world,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": step_s * 1e3, "higher_is_better": True,
            "scaling": a.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic", "source_sha": source_sha(),
            "config": {"workload": "%d x %dx%d u8 occupancy maps %s tiled/rolled/flipped from 4 aisle-class fixtures "
                                   "(SURVEY 8d C4), full pipeline incl. lineIm, params 0.3/0.6/22.5/0.7/1024" % (
                                       a.batch, size, size, "per GPU" if a.scaling == "weak" else "in total, split over the GPUs"),
                       "images_total": n_total, "images_rank0": n, "image": [size, size], "scaled": [w, h],
                       "parallelism": "image-sharded x%d, RCCL gather of line lists" % world if world > 1 else "single GPU",
                       "rccl_gather_in_step": bool(use_dist),
                       "steps_in_flight": depth, "steps_in_flight_asked": depth_asked, "steps_in_flight_note": depth_note,
                       "hbm_bytes_per_slot": slot_bytes, "region_waves_per_image": waves if waves else 8,
                       "help_across_workgroups": bool(a.help_waves),
                       # the last steps of the timed region run with the help ON: nothing follows them that could fill the idle CUs
                       "last_steps_with_help": tail_help,
                       # the steps in flight share one resident input, so the timed region runs WITHOUT LSD_FLAG_WRITEBACK_MAP: the
                       # observable in-place remap of the caller's maps (myLSD.cpp:135-142; ~0.3 ms of byte writes per step) is not in it
                       "writeback_map": False},
            "lines_per_s": total_lines / step_s, "lines_per_step": total_lines, "line_overflow_images": overflow,
        }
        if a.full:
            if use_dist:                                       # the gathered results of the last step of EVERY slot in flight: every line arrived, nothing overflowed
                per, _ = lsd.gather_layout(n_total, world)
                for j, rj in sorted(res_slot.items()):
                    counts_all, slabs = rj
                    assert int(counts_all[:, :per].sum().item()) == int(total_lines) == int(counts_all[:, per].sum().item()), "lsd_gather_lines lost lines (slot %d)" % j
                    assert not bool(counts_all[:, per + 1].any().item()), "lsd_gather_lines: a slab overflowed or an image was given up (slot %d)" % j
            grad_ms = kt["gradient"] / un_steps
            un_step_s = un_dt / un_steps
            grad_bytes = GRAD_BYTES_PER_PX * w * h * n
            achieved = grad_bytes / (grad_ms * 1e-3) / 1e9 if grad_ms > 0 else 0.0
            traffic, traffic_all, traffic_src = None, {}, None
            tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
            if os.path.exists(tpath) and n == 512 and size == 2048:
                try:
                    tj = json.load(open(tpath))
                    traffic = tj.get("k_gradient_bytes_per_launch")
                    traffic_all = {k: v["hbm_bytes_per_launch"] for k, v in tj.get("kernels", {}).items()}
                    same = tj.get("source_sha") == source_sha()
                    traffic_src = "profiles/traffic_latest.json (%s, kernel sources %s): separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload, not this run" % (
                        tj.get("build", "build not recorded"), "identical to this run's (sha %s)" % source_sha() if same else "DIFFERENT from this run's: sha %s vs %s" % (tj.get("source_sha"), source_sha()))
                except Exception:
                    traffic = None
            # per-image cycles of the region stage (s_memtime, read after the timed region): the batch time is its heaviest images
            stats = [ctx.fetch(i, lsd.DBG_STATS, (w, h)) for i in range(n)]
            ties = ctx.last_sensitivity(n)                      # decisions within the noise of the reference's libm, per image (lsd_last_sensitivity)
            cyc_raw = np.array([x["cycles_total"] for x in stats], np.int64)
            # (a record that is not a positive clock count is left out of the statistics and listed.  The count is a difference of the shader clock,
            #  s_memtime, which is a counter of the XCD: a workgroup that was preempted -- more hardware queues in use than the device has, e.g. this
            #  process beside another -- and resumed elsewhere read another counter; the kernel falls back to the constant 100 MHz clock then, so
            #  that none should show up here any more)
            bad_cyc = [(int(i), int(v)) for i, v in enumerate(cyc_raw) if v <= 0]
            cyc = cyc_raw[cyc_raw > 0].astype(np.float64) if (cyc_raw > 0).any() else np.ones(1)
            nb_mean = float(np.mean([ctx.fetch(i, lsd.DBG_NB, (w, h)) for i in range(0, n, max(1, n // 32))]))
            # SURVEY 8d algorithmic bytes of the whole path per image: K1 W*H + 8wh, K2 25wh, K3 8wh + 12 nb, K5 W*H (K4: latency-bound, none)
            alg_img = 2.0 * size * size + (8 + 25 + 8) * w * h + 12.0 * nb_mean
            reg_ms = kt["region"] / un_steps
            out.update({
                # the timed region keeps `steps_in_flight` steps in flight (one context, stream and set of output buffers each);
                # `one_step_at_a_time` is the same step run alone, measured right after it -- the source of every per-kernel figure below
                "one_step_at_a_time": {"steps": un_steps, "ms_per_step": un_step_s * 1e3, "value": mpix / un_step_s, "unit": "Mpix/s",
                                       "note": "a batch alone on the GPU, the library's defaults (8 waves per image as persistent workgroups, help across workgroups off); kernel_ms, roofline and dominant_kernel are from these steps "
                                               "(HIP events of a launch inside an overlapped region also time its wait for a CU)" if depth > 1 else "identical to the timed region"},
                "one_step_at_a_time_with_cost_history": ({"ms_per_step": hist_dt / un_steps * 1e3, "value": mpix / (hist_dt / un_steps), "unit": "Mpix/s",
                                                         "note": "lsd_set_cost_history(1): the same batch again, its images started in the order of their cost in the previous "
                                                                 "step (a caller re-extracting one site's maps); rank 0's clock, not part of `value`"} if hist_dt else None),
                # images of rank 0's batch with at least one decision inside the libm's noise (lsd_last_sensitivity): on the others any libm within
                # one ulp of correct rounding gives the reference's result; and the number of such decisions over the batch
                "libm_sensitive_images": int((ties > 0).sum()), "libm_near_ties": int(ties.sum()),
                # N > 1 only: the same --batch images split over the ranks (the strong split), timed like the weak job right after it
                "strong_split": ({"scaling": "strong", "images_total": a.batch, "ms_per_step": strong_dt / a.steps * 1e3,
                                  "value": a.batch * size * size / 1e6 / (strong_dt / a.steps), "unit": "Mpix/s", "steps": a.steps,
                                  "steps_in_flight": depth,
                                  "note": "rank 0's %d images in contiguous shards over the %d ranks, RCCL gather of the line lists in every step; same contexts and "
                                          "depth as the weak job, max over ranks; compare with the N = 1 line's value" % (a.batch, world)} if strong_dt else None),
                "kernel_ms": {k: v / un_steps for k, v in kt.items()},
                # the same kernels inside the timed region, event to event (mean over the slots' last steps): what the front end of a step
                # takes while the region stages of the other steps in flight hold the CUs
                "kernel_ms_in_timed_region": ({k: float(np.mean([t[k] for t in tr_front])) for k in ("gauss", "gradient", "sort", "region", "lines")} if tr_front else None),
                # informational: every kernel's HBM traffic (PMC, profiles/traffic_latest.json) over its live launch time
                "kernel_hbm_GBs": {k: traffic_all["k_" + k] / (kt[k] / un_steps * 1e-3) / 1e9
                                   for k in ("gauss", "gradient", "sort", "region", "lines") if ("k_" + k) in traffic_all and kt[k] > 0},
                # the kernel north_star prices: the gradient pass, algorithmic bytes over its HIP-event launch time of THIS run
                "roofline": {"kernel": "k_gradient", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                             "algorithmic_bytes_per_launch": grad_bytes, "avg_launch_ms": grad_ms,
                             "note": "k_gradient is the pass north_star prices, not the dominant kernel: see dominant_kernel / roofline_pipeline"},
                # ... and the whole truth next to it: the step is the region stage, a serial-latency / instruction-issue bound kernel
                "dominant_kernel": {"name": "k_region", "ms": reg_ms, "share_of_step": reg_ms / (un_step_s * 1e3),
                                    "Mpix_per_s": n * size * size / 1e6 / (reg_ms * 1e-3), "lines_per_s": float(d_counts.sum().item()) / (reg_ms * 1e-3),
                                    "bound": "serial dependence per image (no HBM / MFMA roofline applies): DESIGN.md section 4",
                                    "variant": "w8::k_region (the library's choice for one batch of this size: one persistent workgroup per CU; help across workgroups off)" if (depth > 1 or not waves) else "w%d::k_region" % waves,
                                    "cycles_per_image": {"mean": float(cyc.mean()), "max": float(cyc.max()), "max_over_mean": float(cyc.max() / cyc.mean()), "bad_records": bad_cyc},
                                    # the same statistics for the last step of the TIMED region (its own variant; with several steps in flight a
                                    # workgroup shares its CU with workgroups of other steps, so these cycles include that contention)
                                    "timed_region": {"variant": "w%d::k_region, help %s, %d steps in flight" % (waves if waves else 8, "off" if (depth > 1 and not a.help_waves) else "on", depth),
                                                     "cycles_per_image": {"mean": float(timed_cyc.mean()), "max": float(timed_cyc.max()), "max_over_mean": float(timed_cyc.max() / timed_cyc.mean())}},
                                    # full evaluations of the last step that wavefronts of finished workgroups did for other images
                                    "help_across_workgroups": {"evaluations": int(sum(x["help_evals"] for x in stats)),
                                                               "images_helped": int(sum(1 for x in stats if x["help_exports"] > 0))}},
                "roofline_pipeline": {"bound": "hbm", "algorithmic_bytes_per_step": alg_img * n, "achieved": alg_img * n_total / step_s / 1e9,
                                      "peak": HBM_PEAK_GBS * world, "unit": "GB/s", "frac": alg_img * n_total / step_s / 1e9 / (HBM_PEAK_GBS * world),
                                      "note": "SURVEY 8d algorithmic bytes of the whole path (K1+K2+K3+K5; %.1f MB per image) over the step time" % (alg_img / 1e6)},
            })
        if a.full and world == 1 and not a.no_cpu_baseline:
            extras(out, a, ctx, lsd, ldist, maps, d_maps, d_lines, d_counts, d_ims, stream, dev, size, n_total, ctxs, outs, tstreams, waves)
            out["cpu_baseline"] = cb = cpu_baseline(size, first)
            # same-box ratios: the GPU against the single-thread port on THIS host's cores (cpu_baseline.kind = "port": a port of the
            # reference path that skips its two accidental full-image scans per region -- NOT the reference itself, which cannot
            # be built here; the cross-host figure against the unmodified reference carries the host in its name)
            m1 = out["map1"]
            m1["vs_port_one_core"] = m1["batch512_lines_per_s"] / cb["map1"]["lines_per_s"]
            if "cores" in cb.get("all_cores", {}):
                m1["vs_port_all_cores"] = m1["batch512_lines_per_s"] / (cb["map1"]["lines_per_s"] * cb["all_cores"]["cores"])
                m1["vs_port_all_cores_note"] = "map1 port lines/s x %d host cores (one independent instance per core assumed)" % cb["all_cores"]["cores"]
            m1["single_call_vs_port"] = cb["map1"]["ms"] / m1["single_call_lsd_only_ms"]
            out["single_image_latency_vs_port"] = cb["single_image_ms"] / out["single_image_latency_ms"]
            out["vs_port_one_core"] = out["value"] / cb["value"]
            for name, rec in out.get("real_maps", {}).items():
                if name in cb.get("real_maps", {}):
                    rec["port_ms_per_map"] = cb["real_maps"][name]["ms"]
                    rec["port_lines"] = cb["real_maps"][name]["lines"]
                    rec["vs_port_one_core"] = cb["real_maps"][name]["ms"] * rec["copies"] / rec["ms"]
            if "value" in cb.get("all_cores", {}):
                out["vs_port_all_cores"] = out["value"] / cb["all_cores"]["value"]
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    for c_ in ctxs:
        c_.close()


def extras(out, a, ctx, lsd, ldist, maps, d_maps, d_lines, d_counts, d_ims, stream, dev, size, n_total, ctxs, outs, tstreams, waves):
    """Outside the timed region: what north_star asks for on mapValue_map1, single-image latency, device copy ceiling."""
    import torch
    ims = None if d_ims is None else d_ims.data_ptr()
    lat = []
    for _ in range(3):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.enqueue_device(d_maps.data_ptr(), 1, size, size, d_lines.data_ptr(), a.max_lines, d_counts.data_ptr(), d_line_ims=ims, stream=stream)
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - t1) * 1e3)
    out["single_image_latency_ms"] = min(lat)
    # -- the observable in-place remap of the caller's maps (myLSD.cpp:135-142), which the timed region leaves out because its steps in
    #    flight share one resident input (config.writeback_map): what it costs, one step at a time on a private copy of the batch
    #    (restored before every repetition), with LSD_FLAG_WRITEBACK_MAP and without
    try:
        d_priv = d_maps.clone()
        tw = {}
        for flag in (0, lsd.LSD_FLAG_WRITEBACK_MAP):
            ts = []
            for _ in range(3):
                d_priv.copy_(d_maps)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ctx.enqueue_device(d_priv.data_ptr(), n_total, size, size, d_lines.data_ptr(), a.max_lines, d_counts.data_ptr(), d_line_ims=ims, flags=flag, stream=stream)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t1) * 1e3)
            tw[flag] = (min(ts), ctx.timings()["gauss"])
        rem = ((d_maps == 1) | (d_maps == 255))
        rem[:, 0, :] = False; rem[:, :, 0] = False
        ok = bool(((d_priv != d_maps) == rem).all().item())      # exactly the cells with value 1 or 255 off row 0 / column 0 were rewritten
        out["writeback_map"] = {"step_ms_without": tw[0][0], "step_ms_with": tw[lsd.LSD_FLAG_WRITEBACK_MAP][0], "gauss_ms_without": tw[0][1],
                                "gauss_ms_with": tw[lsd.LSD_FLAG_WRITEBACK_MAP][1], "maps_rewritten_as_the_reference_does": ok,
                                "note": "one step at a time on a private copy of the batch: the in-place remap (a1) rides on K1's event window; the timed region runs without it"}
        del d_priv, rem
    except (RuntimeError, lsd.LsdError) as e:
        out["writeback_map"] = {"error": str(e)[:200]}
    # ... and the timed configuration WITH it: every step in flight on a private copy of the batch that is restored (a device copy on the
    # step's stream: the arrival of the next batch, which the reference's caller does by loading a file) before the step rewrites it
    if len(ctxs) > 1 and "error" not in out["writeback_map"]:
        try:
            privs = [d_maps.clone() for _ in ctxs]
            for c_ in ctxs:
                c_.set_region_help(a.help_waves); c_.set_region_waves(waves)
            def stepw(i, restore=True):
                j = i % len(ctxs)
                l_, c2, im_ = outs[j]
                if restore:
                    with torch.cuda.stream(tstreams[j]):
                        privs[j].copy_(d_maps, non_blocking=True)
                ctxs[j].enqueue_device(privs[j].data_ptr(), n_total, size, size, l_.data_ptr(), a.max_lines, c2.data_ptr(),
                                       d_line_ims=None if im_ is None else im_.data_ptr(), flags=lsd.LSD_FLAG_WRITEBACK_MAP, stream=tstreams[j].cuda_stream)
            for i in range(len(ctxs)):
                stepw(i)
            torch.cuda.synchronize()
            ks = 24
            t1 = time.perf_counter()
            for i in range(ks):
                stepw(i)
            torch.cuda.synchronize()
            out["writeback_map"].update({"timed_configuration_ms_per_step_with_writeback_and_restore_copy": (time.perf_counter() - t1) / ks * 1e3,
                                         "timed_configuration_note": "%d steps in flight as in the timed region, 24 steps after a fill, LSD_FLAG_WRITEBACK_MAP on a private copy per slot, "
                                                                     "each restored by a device copy (2 x %.1f GB of traffic that is not the path's) before its step" % (len(ctxs), n_total * size * size / 1e9)})
            del privs
            ctx.set_region_help(-1); ctx.set_region_waves(0)
        except (RuntimeError, lsd.LsdError) as e:
            out["writeback_map"]["timed_configuration_error"] = str(e)[:200]
    # -- mapValue_map1 (608 x 480, 7 lines): (a) the reference's usage, ONE host-ABI call createMapCache + myLineSegmentDetector
    #    (LSD/main_on_windows.cpp:67-70), wall time incl. PCIe; (b) throughput on 512 replicas resident in HBM
    m1 = maps["map1"]
    rows, cols = m1.shape
    both, lsd_only = [], []
    for _ in range(22):
        m = m1.copy()
        t1 = time.perf_counter()
        ctx.map_cache(m, 0.05)
        t2 = time.perf_counter()
        lines, _ = ctx.run(m)
        t3 = time.perf_counter()
        both.append((t3 - t1) * 1e3); lsd_only.append((t3 - t2) * 1e3)
    assert len(lines) == 7
    reps = 512
    d1 = torch.from_numpy(np.broadcast_to(m1, (reps, rows, cols)).copy()).to(dev)
    l1 = torch.zeros((reps, 64, 10), dtype=torch.int64, device=dev)
    c1 = torch.zeros(reps, dtype=torch.int32, device=dev)
    i1 = torch.zeros((reps, rows, cols), dtype=torch.uint8, device=dev)
    tt = []
    for it in range(6):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.enqueue_device(d1.data_ptr(), reps, cols, rows, l1.data_ptr(), 64, c1.data_ptr(), d_line_ims=i1.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        if it:
            tt.append(time.perf_counter() - t1)
    assert int(c1.min().item()) == int(c1.max().item()) == 7
    tb = min(tt)
    out["map1"] = {
        "single_call_ms": statistics.median(both[2:]), "single_call_lsd_only_ms": statistics.median(lsd_only[2:]),
        "single_call_note": "host ABI (lsd_map_cache + lsd_run), wall clock incl. staging and PCIe, median of 20",
        "batch512_ms": tb * 1e3, "batch512_lines_per_s": reps * 7 / tb, "batch512_Mpix_per_s": reps * rows * cols / 1e6 / tb,
        "reference_single_thread": REF_MAP1, "reference_source": "BASELINE.md section 2 (unmodified reference, survey container)",
        "lines_per_s_vs_reference_cross_host": reps * 7 / tb / REF_MAP1["lines_per_s"],
        "single_call_vs_reference_cross_host": REF_MAP1["ms"] / statistics.median(lsd_only[2:]),
        "cross_host_note": "numerator: this MI355X box; denominator: the unmodified reference on the survey container's 2.1 GHz Xeon (BASELINE.md section 2) -- "
                           "the reference cannot be built on the GPU box; same-box ratios against the port: vs_port_one_core / vs_port_all_cores",
        "kernel_ms_batch512": ctx.timings()}
    del d1, l1, c1, i1
    # -- the reference's own maps, un-tiled (LSD/main_on_windows.cpp:20-46 loads one of these per run): each replicated to a batch of
    #    512 resident in HBM and run through the device entry point with the library's defaults, + one 2048^2 canvas of different
    #    maps pasted side by side (no wrap-around seams, no repeated structure).  set_answers = evaluations the certified uniform
    #    sets answered: how much of that mechanism survives outside the tiled bench batch.
    real = {}
    pasted = make_pasted(maps, size)
    for name in REAL_MAPS + (["pasted2048"] if pasted is not None else []):
        im = pasted if name == "pasted2048" else maps[name]
        rr, cc = im.shape
        dm = torch.from_numpy(np.broadcast_to(im, (reps, rr, cc)).copy()).to(dev)
        ll = torch.zeros((reps, a.max_lines, 10), dtype=torch.int64, device=dev)
        cn = torch.zeros(reps, dtype=torch.int32, device=dev)
        li = torch.zeros((reps, rr, cc), dtype=torch.uint8, device=dev)
        tt = []
        for it in range(4):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ctx.enqueue_device(dm.data_ptr(), reps, cc, rr, ll.data_ptr(), a.max_lines, cn.data_ptr(), d_line_ims=li.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            if it:
                tt.append(time.perf_counter() - t1)
        assert int(cn.min().item()) == int(cn.max().item()) >= 0, name
        tb_ = min(tt)
        ws_, hs_ = lsd.scaled_size(cc, rr)
        st_ = ctx.fetch(0, lsd.DBG_STATS, (ws_, hs_))
        real[name] = {"image": [cc, rr], "copies": reps, "ms": tb_ * 1e3, "Mpix_per_s": reps * rr * cc / 1e6 / tb_, "lines": int(cn[0].item()),
                      "lines_per_s": reps * int(cn[0].item()) / tb_, "lit_pixels": int((li[0] != 0).sum().item()), "kernel_ms": ctx.timings(),
                      "grow_calls": st_["grow_calls"], "grown_px": st_["grown_px"], "set_answers": st_["set_answers"], "sets_founded": st_["sets_founded"],
                      "region_Mcycles": st_["cycles_total"] / 1e6}
        del dm, ll, cn, li
    out["real_maps"] = real
    out["real_maps_note"] = ("the reference's seven maps as they are (no tiling) and one 2048^2 canvas of three different maps pasted side by side, %d copies "
                             "each, resident, library defaults, best of 3; vs_port_one_core (added next to cpu_baseline) = the port's time for the "
                             "same number of maps on one core of this box / ms" % reps)
    # -- strong scaling projected from ONE GPU (BASELINE configs[4]: the same batch split over 2 / 4 / 8 GPUs, contiguous shards):
    #    every shard is run alone on this GPU; a step of the sharded job cannot be shorter than its slowest shard (+ the gather, 22 MB)
    if a.scaling == "weak" and n_total >= 8:
        def run_shard(lo, hi, src=None):
            src = d_maps if src is None else src
            best = 1e9
            for _ in range(2):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ctx.enqueue_device(src[lo:hi].data_ptr(), hi - lo, size, size, d_lines[lo:hi].data_ptr(), a.max_lines, d_counts[lo:hi].data_ptr(),
                                   d_line_ims=None if d_ims is None else d_ims[lo:hi].data_ptr(), stream=stream)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t1) * 1e3)
            return best
        t_all = run_shard(0, n_total)
        # the cost-aware deal (lsd_shard_balanced) by the cycles every image took in that run: the batch re-ordered so that the same
        # contiguous shards carry about the same cost (the gathered lists then arrive in that order, image perm[g] at position g)
        costs = ctx.last_region_cycles(n_total)
        proj = {"1": {"max_shard_ms": t_all, "speedup": 1.0}}
        perms = {}
        for world in (2, 4, 8):
            ts = [run_shard(*ldist.shard_range(n_total, world, r)) for r in range(world)]
            proj[str(world)] = {"max_shard_ms": max(ts), "min_shard_ms": min(ts), "speedup": t_all / max(ts)}
            perms[world] = lsd.shard_balanced(costs, world)
            d_bal = d_maps[torch.from_numpy(perms[world].astype(np.int64)).to(dev)]
            tb_ = [run_shard(*ldist.shard_range(n_total, world, r), src=d_bal) for r in range(world)]
            proj[str(world)].update({"balanced_max_shard_ms": max(tb_), "balanced_min_shard_ms": min(tb_), "balanced_speedup": t_all / max(tb_)})
            del d_bal
        # the same split in THROUGHPUT mode: what an N-GPU job sees when every rank keeps `depth` steps in flight on its shard
        # (contexts ctxs[], 4-wave region stage, help off -- the configuration of this line's `value`), ms per sharded step
        depth1 = len(ctxs)
        if depth1 > 1:
            # A rank of an N-GPU job has a shard of n / N images per step; to keep the GPU as full as the 1-GPU job does it keeps N times
            # as many steps in flight (the same number of images, up to 32 steps).  The 1-GPU figure comes from the timed region's own
            # contexts; they are then closed (a context's workspace is ~40 MB per image) and every shard size gets contexts and outputs
            # of its own, sized for the shard.
            def run_pipelined(lo, hi, slots, src=None):
                # ms per step at the steady RATE of the pipeline: every step's completion is time-stamped (an event on its stream), and the
                # rate is taken between the dw-th completion and the moment the first slot runs out of queued steps.  (Timing a fixed
                # number of steps per slot instead measures the most crowded hardware queue: 32 streams are dealt onto 16 queues, not
                # always two each -- rocprofv3's Queue_Id showed 3 + 1 on two of them after an earlier launch in the process -- and a
                # rank that refills whichever slot is free does not wait for that queue.  DESIGN_NOTES.md, "The strong split".)
                m, dw = hi - lo, len(slots)
                src = d_maps if src is None else src
                def go(i):
                    cx, st_, l_, c2, im_ = slots[i % dw]
                    cx.enqueue_device(src[lo:hi].data_ptr(), m, size, size, l_.data_ptr(), a.max_lines, c2.data_ptr(),
                                      d_line_ims=None if im_ is None else im_.data_ptr(), stream=st_.cuda_stream)
                for i in range(dw):
                    go(i)
                torch.cuda.synchronize()
                steps = 6 * dw
                ev0 = torch.cuda.Event(enable_timing=True)
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
                ev0.record(torch.cuda.current_stream(dev))
                torch.cuda.synchronize()
                for i in range(steps):
                    go(i)
                    evs[i].record(slots[i % dw][1])
                torch.cuda.synchronize()
                return steady_rate_ms([ev0.elapsed_time(e) for e in evs], dw)     # ms since ev0; step i ran on slot i % dw
            for c_ in ctxs:
                c_.set_region_help(a.help_waves); c_.set_region_waves(waves)
            t1_all = run_pipelined(0, n_total, [(ctxs[j], tstreams[j]) + tuple(outs[j]) for j in range(len(ctxs))])
            proj["1"].update({"pipelined_ms_per_step": t1_all, "pipelined_steps_in_flight": len(ctxs)})
            for c_ in ctxs[1:]:
                c_.close()
            del ctxs[1:], outs[1:]
            try:                                               # (outside the timed region: a projection that does not fit this device's
                                                               #  memory must not take the line with it)
                for world in (2, 4, 8):
                    dw = min(depth1 * world, 32)
                    m = -(-n_total // world)
                    torch.cuda.empty_cache()                       # (the library allocates with hipMalloc: what torch has cached is not free for it)
                    slots = []
                    for j in range(dw):
                        cx = lsd.Context(dev.index or 0)
                        cx.set_region_help(a.help_waves); cx.set_region_waves(waves); cx.reserve(m, size, size)
                        slots.append((cx, tstreams[(j + depth1) % len(tstreams)], torch.zeros((m, a.max_lines, 10), dtype=torch.int64, device=dev),
                                      torch.zeros(m, dtype=torch.int32, device=dev), None if a.no_lineim else torch.zeros((m, size, size), dtype=torch.uint8, device=dev)))
                    ts = [run_pipelined(*ldist.shard_range(n_total, world, r), slots) for r in range(world)]
                    proj[str(world)].update({"pipelined_max_shard_ms_per_step": max(ts), "pipelined_min_shard_ms_per_step": min(ts),
                                             "pipelined_speedup": t1_all / max(ts), "pipelined_steps_in_flight": dw,
                                             "pipelined_shard_ms_per_step": [round(t, 2) for t in ts]})
                    d_bal = d_maps[torch.from_numpy(perms[world].astype(np.int64)).to(dev)]          # the same with the cost-aware deal
                    tb_ = [run_pipelined(*ldist.shard_range(n_total, world, r), slots, src=d_bal) for r in range(world)]
                    proj[str(world)].update({"pipelined_balanced_max_shard_ms_per_step": max(tb_), "pipelined_balanced_min_shard_ms_per_step": min(tb_),
                                             "pipelined_balanced_speedup": t1_all / max(tb_)})
                    del d_bal
                    for sl in slots:
                        sl[0].close()
                    del slots
            except (lsd.LsdError, RuntimeError) as e:
                proj["error_throughput_mode"] = str(e)[:300]
            torch.cuda.empty_cache()
            ctx.set_region_help(-1); ctx.set_region_waves(0)
        out["strong_scaling_projection"] = {"gpus": proj, "note_throughput_mode": "pipelined_*: every shard run on this one GPU in the timed region's configuration with pipelined_steps_in_flight steps in flight "
                                            "(%d x the number of GPUs, at most 32: the same number of images in flight as the 1-GPU job); "
                                            "a sharded job in throughput mode advances at its slowest shard's rate" % depth1, "note_balanced": "balanced_*: the same with the images dealt by lsd_shard_balanced (costs = the cycles each image took in the full run before: a site's maps cost about the same from step to step)", "note": "each contiguous shard of the %d images run alone on this one GPU (best of 2); "
                                            "the sharded step takes at least its slowest shard: the region stage gives one CU per image, so a shard "
                                            "cannot finish before its heaviest image does" % n_total}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    src_t = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst_t = torch.empty_like(src_t)
    dst_t.copy_(src_t)
    ev0.record()
    for _ in range(5):
        dst_t.copy_(src_t)
    ev1.record()
    torch.cuda.synchronize()
    out["roofline"]["measured_copy_GBs"] = 5 * 2 * (1 << 30) / (ev0.elapsed_time(ev1) * 1e-3) / 1e9   # read + write
    del src_t, dst_t


if __name__ == "__main__":
    main()
