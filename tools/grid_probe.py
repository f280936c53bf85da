#!/usr/bin/env python3
"""Developer probe: the time of k_grid_integrate and k_grid_publish (csrc/k_gridmap.hip) on a 2048 x 2048 grid at 0.05 m.

Scans of one generated room each (walls 2 - 12 m from a lidar that stands somewhere in the middle half of the grid, a tenth of the
beams without a return, cut at range_max = 20 m), integrated by lsd_enqueue_grid_integrate_device between two events, from a warm
context; the median and the minimum of REPS launches.  1, 64 and 256 scans of 360, 1081 and 4096 beams, then the publish of the grid.
One JSON line per measurement, with the ray steps the launch added so that a time reads as steps per microsecond.
Usage: tools/grid_probe.py [--reps 20] [--size 2048]"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

lsd = importlib.import_module("linesegmentdetector-slam_amd")
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
RESOL, RANGE_MAX = 0.05, 20.0


def rooms(count, beams, size, seed):
    """(scans [count, beams, 2], lens, poses [count, 3]): a rectangular room around each lidar, seen over the full circle."""
    rng = np.random.default_rng((seed, count, beams))
    ang = np.linspace(-np.pi, np.pi, beams, endpoint=False)
    scans = np.zeros((count, beams, 2))
    for i in range(count):
        w = rng.uniform(2.0, 12.0, 4)                                       # the walls' distances: +x, -x, +y, -y
        c, s = np.cos(ang), np.sin(ang)
        with np.errstate(divide="ignore"):
            tx = np.where(c > 0, w[0] / c, np.where(c < 0, -w[1] / c, np.inf))
            ty = np.where(s > 0, w[2] / s, np.where(s < 0, -w[3] / s, np.inf))
        r = np.minimum(tx, ty) + rng.normal(0, 0.01, beams)
        r[rng.random(beams) < 0.1] = 2 * RANGE_MAX                          # no return: a pass up to range_max, no hit
        scans[i, :, 0], scans[i, :, 1] = r, ang
    poses = np.stack([rng.uniform(size / 4, 3 * size / 4, count), rng.uniform(size / 4, 3 * size / 4, count), rng.uniform(-180, 180, count)], 1)
    return scans, np.full(count, beams, np.int32), poses


def timed(fn, reps):
    fn(); torch.cuda.synchronize()                                          # warm
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    ctx = lsd.Context(0)
    ctx.set_scan_capacity(lsd.LSD_SCAN_MAX_LEN)
    mapper = lsd.GridMapper(args.size, args.size, RESOL, 0.0, 0.0, RANGE_MAX, ctx=ctx)
    for beams in (360, 1081, 4096):
        for count in (1, 64, 256):
            scans, lens, poses = rooms(count, beams, args.size, 1)
            d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
            mapper.clear()
            mapper.integrate_device(d_sc, d_ln, d_po)
            steps = int(mapper.counts()[0].astype(np.int64).sum())          # passes one launch adds
            med, lo = timed(lambda: mapper.integrate_device(d_sc, d_ln, d_po), args.reps)
            print(json.dumps(dict(what="grid_integrate", grid=args.size, resol=RESOL, range_max=RANGE_MAX, scans=count, beams=beams, passes=steps,
                                  ms_median=med, ms_min=lo, passes_per_us=steps / (1e3 * med))), flush=True)
    med, lo = timed(lambda: mapper.publish_device(), args.reps)
    print(json.dumps(dict(what="grid_publish", grid=args.size, cells=args.size * args.size, ms_median=med, ms_min=lo,
                          gb_per_s=9 * args.size * args.size / (1e6 * med))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
