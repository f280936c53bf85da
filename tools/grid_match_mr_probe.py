#!/usr/bin/env python3
"""Developer probe: the coarse-to-fine match (csrc/k_gridmatch_mr.hip) beside the plain one (csrc/k_gridmatch.hip), in the same process on
the same inputs, on a 2048 x 2048 grid at 0.05 m.

The generated rooms of tools/grid_probe.py are integrated at their poses, the lookup plane is made from them (the default table), and the
same scans are matched around poses displaced inside the window, at na = 10.  Events around each entry, from a warm context; the median,
the minimum and the maximum of REPS launches.  One invocation measures ONE configuration (--wx, --scans, --beams) at b = 4, 8, 16, so that
a caller can give every step a time limit of its own; one JSON line per measurement:
  plain        lsd_enqueue_grid_match_device
  coarse_plane lsd_enqueue_grid_coarse_device alone
  mr           lsd_enqueue_grid_match_mr_device alone (the coarse plane is there), and "charged": the coarse plane's build in front of
               it inside the same pair of events -- what a caller pays who refreshes the plane at every match
with the statistics beside the times: refined / blocks, and the byte gathers done -- coarse (scored beams x blocks) + seed (scored beams x
b^2 per angle) + fine (scored beams x fine candidates) -- against the plain count (scored beams x candidates).  The records of the two
entries must be equal: the run fails (exit 1) where they are not.

--summarise LOG reads such lines back and states the condition DESIGN.md 8.1.8 holds the change to: at wx = wy = 63 there is a block size
at which, for every scan count and beam count in the log, the SLOWEST charged launch is below the FASTEST plain launch (exit 1 if not).
Usage: tools/grid_match_mr_probe.py --wx 63 --scans 64 --beams 1081 [--reps 20] [--size 2048]
       tools/grid_match_mr_probe.py --summarise profiles/grid_match_mr_probe.log"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NA, STEP, BLOCKS = 10, 0.5, (4, 8, 16)


def summarise(path):
    rows = [json.loads(l) for l in open(path) if l.startswith("{")]
    plain = {(r["scans"], r["beams"]): r for r in rows if r["what"] == "plain" and r["wx"] == 63}
    mr = {(r["scans"], r["beams"], r["block"]): r for r in rows if r["what"] == "mr" and r["wx"] == 63}
    ok = {}
    for b in BLOCKS:
        have = [k for k in plain if k + (b,) in mr]
        ok[b] = bool(have) and len(have) == len(plain) and all(mr[k + (b,)]["charged_ms_max"] < plain[k]["ms_min"] for k in have)
    equal = all(r["records_equal"] for r in rows if r["what"] == "mr")
    print(json.dumps(dict(what="summary", wx=63, configurations=sorted(plain), slowest_charged_below_fastest_plain=ok, records_equal=equal)))
    return 0 if equal and any(ok.values()) else 1


def timed3(fn, reps):
    import numpy as np
    import torch
    fn(); torch.cuda.synchronize()                                          # warm
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise")
    ap.add_argument("--wx", type=int, default=63)
    ap.add_argument("--scans", type=int, default=1)
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import numpy as np
    import torch
    from grid_probe import RANGE_MAX, RESOL, dev, rooms
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    W, count, beams = args.wx, args.scans, args.beams
    ctx = lsd.Context(0)
    ctx.set_scan_capacity(lsd.LSD_SCAN_MAX_LEN)
    mapper = lsd.GridMapper(args.size, args.size, RESOL, 0.0, 0.0, RANGE_MAX, ctx=ctx)
    search = lsd.grid_search(wx=W, wy=W, na=NA, ang_step=STEP, min_beams=30, min_num=1, min_den=4)
    shift = (min(41, W - 1), -min(37, W - 2), 3)                            # inside the window: (41, -37) cells at 63, (9, -8) at 10; 3 steps
    n_ang, cand = 2 * NA + 1, (2 * W + 1) ** 2 * (2 * NA + 1)
    scans, lens, poses = rooms(count, beams, args.size, 1)
    d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
    d_moved = dev(poses + np.array([shift[0], shift[1], shift[2] * STEP]))
    for _ in range(2):
        mapper.integrate_device(d_sc, d_ln, d_po)
    mapper.likelihood_device()
    s = torch.cuda.current_stream().cuda_stream
    mp, stride = mapper.map_param, scans.shape[1]
    d_plain = torch.zeros((count, 56), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((count, 56), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros((count, 16), dtype=torch.uint8, device="cuda")
    plain = lambda: ctx.enqueue_grid_match_device(d_sc.data_ptr(), d_ln.data_ptr(), count, stride, d_moved.data_ptr(), 24, mp, RANGE_MAX, mapper.d_corr,
                                                  search, d_plain.data_ptr(), s)
    med, lo, hi = timed3(plain, args.reps)
    r = d_plain.cpu().numpy().reshape(-1).view(lsd.GRID_MATCH_DTYPE)
    scored = int(r["n_beams"].sum())                                        # (of the winners' angles: the count barely moves with the angle)
    back = int(((r["di"] == -shift[0]) & (r["dj"] == -shift[1]) & (r["da"] == -shift[2])).sum())
    print(json.dumps(dict(what="plain", grid=args.size, scans=count, beams=beams, wx=W, wy=W, na=NA, candidates=cand, scored_beams=scored,
                          gathers=scored * cand, recovered=back, ms_median=med, ms_min=lo, ms_max=hi)), flush=True)
    status = 0
    for b in BLOCKS:
        d_coarse = mapper.coarse_device(b).data_ptr()
        coarse = lambda: ctx.enqueue_grid_coarse_device(mapper.d_corr, args.size, args.size, b, d_coarse, s)
        match = lambda: ctx.enqueue_grid_match_mr_device(d_sc.data_ptr(), d_ln.data_ptr(), count, stride, d_moved.data_ptr(), 24, mp, RANGE_MAX,
                                                         mapper.d_corr, d_coarse, b, search, d_rec.data_ptr(), d_stats.data_ptr(), s)
        c_med, c_lo, c_hi = timed3(coarse, args.reps)
        m_med, m_lo, m_hi = timed3(match, args.reps)
        both = lambda: (coarse(), match())
        t_med, t_lo, t_hi = timed3(both, args.reps)
        equal = bool(torch.equal(d_rec, d_plain))
        st = d_stats.cpu().numpy().reshape(-1).view(lsd.GRID_MATCH_MR_STATS_DTYPE)
        per_scan = r["n_beams"].astype(np.int64)
        gathers = int((per_scan * (st["blocks"].astype(np.int64) + n_ang * b * b + st["fine"].astype(np.int64))).sum())
        print(json.dumps(dict(what="coarse_plane", grid=args.size, block=b, ms_median=c_med, ms_min=c_lo, ms_max=c_hi,
                              gb_per_s=2 * args.size * args.size / (1e6 * c_med))), flush=True)
        print(json.dumps(dict(what="mr", grid=args.size, scans=count, beams=beams, wx=W, wy=W, na=NA, block=b, records_equal=equal,
                              blocks=int(st["blocks"].sum()), refined=int(st["refined"].sum()), fine=int(st["fine"].sum()), gathers=gathers,
                              gathers_plain=scored * cand, ms_median=m_med, ms_min=m_lo, ms_max=m_hi, charged_ms_median=t_med, charged_ms_min=t_lo,
                              charged_ms_max=t_hi, plain_ms_min=lo, speedup_median=med / t_med)), flush=True)
        if not equal:
            status = 1
    ctx.close()
    return status


if __name__ == "__main__":
    sys.exit(main())
