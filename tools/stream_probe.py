#!/usr/bin/env python3
"""Developer probe: the per-tick cost of the resumable loop (Localizer.step -> lsd_enqueue_localize_resume_device) on the data/ log of
tests/golden/, to set beside tools/localize_probe.py's one-call replay.

S robots (S = 1, 19, 256 by default) step one frame per call for TICKS ticks, robot s on the log from frame (7 s) mod (99 - TICKS), as
localize_probe.py staggers its sequences.  A tick is timed whole, from a warm Localizer: the host's infinite-range filter and the uploads,
FeatureScan of the S scans, the three FeatureAssociation launches, and the read-back of the tick's states and reports (one
synchronisation).  One JSON line per S.  Usage: tools/stream_probe.py [--robots 1,19,256] [--ticks 60] [--warm 3]"""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fa_restatement as fr

lsd = importlib.import_module("linesegmentdetector-slam_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="1,19,256")
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    m, mp, lid, odom = fr.load_log("data")
    ctx = lsd.Context(0)
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsd.z_occ_max_dis)
    ml = lsd.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    T = args.ticks
    for S in (int(v) for v in args.robots.split(",")):
        starts = np.array([(7 * s) % (len(lid) - T) for s in range(S)])
        od0 = odom[starts].copy(); od0[:, 0] = 0.0                       # the driver's Odom[0].x = 0
        loc = lsd.Localizer(mc, ml, mp, S, odom0=od0, ctx=ctx)
        frame = lambda t: (lid[starts + t][:, None], odom[starts + t + 1][:, None])
        for t in range(args.warm):                                       # warm: staging and workspace sized, code loaded
            loc.step(*frame(t))
        loc.reset(range(S), odom0=od0)
        torch.cuda.synchronize()
        ts, tf, kept = [], [], []
        for t in range(T):
            a = frame(t)
            t0 = time.perf_counter()
            st, rp = loc.step(*a)
            ts.append(time.perf_counter() - t0)
            kept.append(rp["n_kept"])
            t0 = time.perf_counter()
            lsd.lidar_frames_batch(a[0])                                 # the host's share: the infinite-range filter alone
            tf.append(time.perf_counter() - t0)
        ts, tf = np.array(ts) * 1e6, np.array(tf) * 1e6
        kept = np.concatenate(kept)
        print(json.dumps(dict(robots=S, ticks=T, map_lines=len(ml), us_per_tick_median=float(np.median(ts)), us_per_tick_min=float(ts.min()),
                              us_per_tick_p90=float(np.percentile(ts, 90)),
                              us_host_filter_median=float(np.median(tf)), frames_per_s=S / float(np.median(ts)) * 1e6,
                              kept_mean=float(kept.mean()), kept_max=int(kept.max()))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
