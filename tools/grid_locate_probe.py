#!/usr/bin/env python3
"""Developer probe: global scan-to-grid localisation (csrc/k_gridlocate.hip) over a whole 2048 x 2048 grid at 0.05 m and all headings.

The generated rooms of tools/grid_probe.py are integrated at their poses, the lookup plane is made from them (the default table), and the
same scans are located WITHOUT their poses: 720 headings of 0.5 degrees over the whole grid, at levels = 4, 6 and 8.  Events around each
entry, from a warm context; the median, the minimum and the maximum of REPS launches.  One invocation measures ONE configuration (--scans,
--beams), so that a caller can give every step a time limit of its own; one JSON line per measurement:
  publish      lsd_enqueue_grid_publish_device, the bandwidth kernel the pyramid pass is read beside
  pyramid      lsd_enqueue_grid_pyramid_device alone: levels + 1 launches; bytes = every level's cells written once and, above level 0,
               four cells read for each
  locate       lsd_enqueue_grid_locate_device alone (the pyramid is there): the milliseconds, the outcomes, the statistics' `scored` beside
               the 720 x 2048^2 candidates per scan an exhaustive search would score, the frontier per level, and how many scans came back
               within two cells and one step of the pose they were generated at (the poses are not on whole cells, and a rectangular room
               looks the same from its point mirror: the probe says what it found, it is no test)
  locate_tight (--tight) lsd_enqueue_grid_locate_tight_device (csrc/k_gridlocate_tight.hip) on the same inputs in the same
               process, once per flag word of --tight (default 1 and 3: the probe alone, the probe and the retry): the same fields, and the
               retried levels, the first counts, the bound per level of the first scan and the launches
Usage: tools/grid_locate_probe.py --scans 16 --beams 1081 [--reps 20] [--size 2048] [--max-nodes 1048576] [--tight [WORD ...]]"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ANG, STEP, ANG0, LEVELS = 720, 0.5, -180.0, (4, 6, 8)


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
    ap.add_argument("--scans", type=int, default=1)
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--max-nodes", type=int, default=1 << 20)
    ap.add_argument("--tight", type=int, nargs="*", default=None, help="also measure the tight entry at these flag words (none given: 1 3)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from grid_probe import RANGE_MAX, RESOL, dev, rooms
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    count, beams, size = args.scans, args.beams, args.size
    ctx = lsd.Context(0)
    ctx.set_scan_capacity(lsd.LSD_SCAN_MAX_LEN)
    mapper = lsd.GridMapper(size, size, RESOL, 0.0, 0.0, RANGE_MAX, ctx=ctx)
    scans, lens, poses = rooms(count, beams, size, 1)
    d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
    for _ in range(2):
        mapper.integrate_device(d_sc, d_ln, d_po)
    mapper.likelihood_device()
    s = torch.cuda.current_stream().cuda_stream
    mp, stride, cells = mapper.map_param, scans.shape[1], size * size
    med, lo, hi = timed3(lambda: mapper.publish_device(), args.reps)
    print(json.dumps(dict(what="publish", grid=size, ms_median=med, ms_min=lo, ms_max=hi, gb_per_s=9 * cells / (1e6 * med))), flush=True)
    d_rec = torch.zeros((count, 64), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros((count, 48), dtype=torch.uint8, device="cuda")
    d_tstats = torch.zeros((count, 128), dtype=torch.uint8, device="cuda")
    words = [] if args.tight is None else (args.tight or [1, 3])
    want_a = np.rint((poses[:, 2] - ANG0) / STEP).astype(np.int64) % N_ANG
    for H in LEVELS:
        par = lsd.grid_locate(cols=size, rows=size, ang0=ANG0, ang_step=STEP, n_ang=N_ANG, levels=H, max_nodes=args.max_nodes, min_beams=30,
                              min_num=1, min_den=4)
        d_pyr = mapper.pyramid_device(H).data_ptr()
        pyramid = lambda: ctx.enqueue_grid_pyramid_device(mapper.d_corr, size, size, H, d_pyr, s)
        locate = lambda: ctx.enqueue_grid_locate_device(d_sc.data_ptr(), d_ln.data_ptr(), count, stride, mp, RANGE_MAX, d_pyr, par, d_rec.data_ptr(),
                                                        d_stats.data_ptr(), s)
        p_med, p_lo, p_hi = timed3(pyramid, args.reps)
        level_cells = [(size + (1 << h) - 1) ** 2 for h in range(H + 1)]
        moved = 2 * level_cells[0] + sum(5 * c for c in level_cells[1:])    # level 0: a copy; above: four reads, one write
        print(json.dumps(dict(what="pyramid", grid=size, levels=H, bytes=moved, ms_median=p_med, ms_min=p_lo, ms_max=p_hi,
                              gb_per_s=moved / (1e6 * p_med))), flush=True)
        def report(what, ms, st, ws, **more):
            l_med, l_lo, l_hi = ms
            r = d_rec.cpu().numpy().reshape(-1).view(lsd.GRID_LOCATE_DTYPE)
            da = np.abs(r["a"] - want_a)
            near = (np.abs(r["cx"] - poses[:, 0]) <= 2) & (np.abs(r["cy"] - poses[:, 1]) <= 2) & (np.minimum(da, N_ANG - da) <= 1)
            won = (r["flags"] & (lsd.GRID_LOCATE_ACCEPTED | lsd.GRID_LOCATE_REJECTED)) != 0
            print(json.dumps(dict(what=what, grid=size, scans=count, beams=beams, headings=N_ANG, levels=H, max_nodes=args.max_nodes,
                                  workspace_mb=ws / 2 ** 20,
                                  ms_median=l_med, ms_min=l_lo, ms_max=l_hi, flags=sorted(set(int(f) for f in r["flags"])),
                                  accepted=int((r["flags"] == lsd.GRID_LOCATE_ACCEPTED).sum()), overflowed=int((r["flags"] == lsd.GRID_LOCATE_OVERFLOW).sum()),
                                  at_the_generated_pose=int((near & won).sum()), n_best_max=int(r["n_best"].max()),
                                  top_nodes=int(st["top_nodes"].astype(np.int64).sum()), scored=int(st["scored"].astype(np.int64).sum()),
                                  exhaustive=count * N_ANG * cells, frontier=[int(v) for v in st["frontier"].astype(np.int64).sum(axis=0)[:H + 1]],
                                  lower_bound_over_score=[round(float(a) / max(1, int(b)), 3) for a, b in zip(r["lower_bound"][:4], r["score"][:4])],
                                  **more)), flush=True)
            return r.copy()
        ms = timed3(locate, args.reps)
        plain = report("locate", ms, d_stats.cpu().numpy().reshape(-1).view(lsd.GRID_LOCATE_STATS_DTYPE),
                       ctx.L.lsd_grid_locate_workspace_bytes(count, stride, par))
        for word in words:
            tight = lambda: ctx.enqueue_grid_locate_tight_device(d_sc.data_ptr(), d_ln.data_ptr(), count, stride, mp, RANGE_MAX, d_pyr, par, word,
                                                                 d_rec.data_ptr(), d_tstats.data_ptr(), s)
            ms = timed3(tight, args.reps)
            st = d_tstats.cpu().numpy().reshape(-1).view(lsd.GRID_LOCATE_TIGHT_STATS_DTYPE)
            both = (plain["flags"] != lsd.GRID_LOCATE_OVERFLOW)
            r = report("locate_tight", ms, st, ctx.L.lsd_grid_locate_tight_workspace_bytes(count, stride, par), tight=word,
                       launches=H + 6 + max(H - 1, 0) * (1 + (word & 1) + (word >> 1 & 1)),
                       retried_scans=int((st["retried"] != 0).sum()), retried_levels=int(np.bitwise_or.reduce(st["retried"])),
                       first_count=[int(v) for v in st["first_count"].astype(np.int64).sum(axis=0)[:H + 1]], bound_scan0=[int(v) for v in st["bound"][0][:H + 1]])
            a, b = r.view(np.uint8).reshape(-1, 64).copy(), plain.view(np.uint8).reshape(-1, 64).copy()
            a[:, 52:56] = b[:, 52:56] = 0
            print(json.dumps(dict(what="same_records_where_the_existing_entry_does_not_overflow", levels=H, tight=word,
                                  same=bool(a[both].tobytes() == b[both].tobytes()), compared=int(both.sum()))), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
