#!/usr/bin/env python3
"""Developer probe: throughput of the device replay loop (lsd_enqueue_localize_device) on the data/ log of tests/golden/.

S sequences (S = 1, 19, 256 by default) replay FRAMES frames each of the 99-frame log, sequence s starting at frame (7 s) mod
(99 - FRAMES), so that the sequences see different scans at the same frame index.  FeatureScan runs once, outside the timing; the
timed part is the loop alone (3 launches per frame index), from a warm context, with the frames/s of all sequences together.
One JSON line per S.  Usage: tools/localize_probe.py [--seqs 1,19,256] [--frames 60] [--reps 5]"""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fa_restatement as fr

lsd = importlib.import_module("linesegmentdetector-slam_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="1,19,256")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    m, mp, lid, odom = fr.load_log("data")
    scans, lens = lsd.lidar_frames(lid)
    ctx = lsd.Context(0)
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsd.z_occ_max_dis)
    ml = lsd.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    F, pts_cap = args.frames, 8192
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_mc, d_ml = dev(mc), dev(np.ascontiguousarray(ml).view(np.uint8))
    stream = torch.cuda.current_stream().cuda_stream
    mpar = lsd.lsd_map_param(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]))
    for S in (int(v) for v in args.seqs.split(",")):
        starts = [(7 * s) % (len(scans) - F) for s in range(S)]
        sc = np.stack([scans[a:a + F] for a in starts]); ln = np.stack([lens[a:a + F] for a in starts])
        od = np.stack([odom[a:a + F + 1] for a in starts]); od[:, 0, 0] = 0.0
        n = S * F
        d_sc, d_ln, d_od = dev(sc.reshape(n, 360, 2)), dev(ln.reshape(-1)), dev(od)
        d_lines = torch.zeros(n * 360 * 80, dtype=torch.uint8, device="cuda")
        d_nl, d_np = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        d_pts = torch.zeros(n * pts_cap * 3, dtype=torch.float64, device="cuda")
        d_lp, d_sz = torch.zeros(n * 2, dtype=torch.float64, device="cuda"), torch.zeros(n * 2, dtype=torch.int32, device="cuda")
        init = np.zeros(S, lsd.FA_STATE_DTYPE); init[:] = lsd.Context.fa_initial_state()
        d_init = dev(init.view(np.uint8))
        d_states = torch.zeros(n * 720, dtype=torch.uint8, device="cuda"); d_reps = torch.zeros(n * 72, dtype=torch.uint8, device="cuda")
        ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, 360, mpar, 3, 0.08, 0.5,
                                                             d_lines.data_ptr(), d_nl.data_ptr(), d_pts.data_ptr(), pts_cap, d_np.data_ptr(),
                                                             d_lp.data_ptr(), d_sz.data_ptr(), stream))
        run = lambda: ctx.enqueue_localize_device(d_mc.data_ptr(), mc.shape[1], mc.shape[0], d_ml.data_ptr(), len(ml), S, F, [F] * S,
                                                  d_lines.data_ptr(), d_nl.data_ptr(), d_pts.data_ptr(), pts_cap, d_np.data_ptr(),
                                                  d_lp.data_ptr(), d_od.data_ptr(), float(mp[2]), d_init.data_ptr(), d_states.data_ptr(),
                                                  d_reps.data_ptr(), stream)
        run(); torch.cuda.synchronize()                       # warm: workspace sized, code loaded
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        reps = d_reps.cpu().numpy().view(lsd.FA_REPORT_DTYPE)
        t = float(np.median(ts))
        print(json.dumps(dict(seqs=S, frames_per_seq=F, map_lines=len(ml), ms_median=t * 1e3, ms_min=min(ts) * 1e3,
                              frames_per_s=S * F / t, us_per_frame_index=t / F * 1e6, pairs_mean=float(reps["n_pairs"].mean()),
                              kept_mean=float(reps["n_kept"].mean()), kept_max=int(reps["n_kept"].max()))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
