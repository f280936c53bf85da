#!/usr/bin/env python3
"""Developer probe: the time of lsd_enqueue_grid_raycast_device (csrc/k_gridray.hip: k_grid_raycast + k_grid_ray_sum) on a 2048 x 2048
grid at 0.05 m.

The rooms are those of tools/grid_probe.py (walls 2 - 12 m from the lidar, a tenth of the beams without a return, range_max = 20 m);
the grid is the one those rooms integrate and publish to (min_pass 1: a cell one ray crossed is known).  The entry, with screened scans,
between two events from a warm context; the median and the minimum of REPS calls.  1, 64 and 256 scans of 360, 1081 and 4096 beams.
One JSON line per measurement, also written to --out: `visited` is the cells the rule looks at, k_hit + 1 for a ray that meets an
occupied cell and n + 1 for one that does not, summed over the cast beams (the kernel tests them 16 at a time and so up to 15 more per
ray); `ray_cells` is the sum of n + 1, the rays' whole lengths to range_max; `share` their ratio.  (n of a ray with a hit is recomputed
here with numpy's sin / cos: it can differ by one cell from the device's on a rounding edge.)
Usage: tools/grid_ray_probe.py [--reps 20] [--size 2048] [--out profiles/grid_ray_probe.log]"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from grid_probe import RANGE_MAX, RESOL, dev, rooms, timed

lsd = importlib.import_module("linesegmentdetector-slam_amd")


def ray_lengths(scans, poses, rays):
    """n + 1 of every beam (all are cast: the angles and poses are finite)."""
    th = scans[..., 1] + (poses[:, 2] / 180.0 * np.pi)[:, None]
    x0, y0 = np.round(poses[:, 0])[:, None], np.round(poses[:, 1])[:, None]
    x1 = np.round(poses[:, 0][:, None] + RANGE_MAX * np.cos(th) / RESOL)
    y1 = np.round(poses[:, 1][:, None] + RANGE_MAX * np.sin(th) / RESOL)
    miss = rays["k_hit"] < 0                                               # without a hit the record holds the end cell itself
    x1, y1 = np.where(miss, rays["cx"], x1), np.where(miss, rays["cy"], y1)
    return np.maximum(np.abs(x1 - x0), np.abs(y1 - y0)).astype(np.int64) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_ray_probe.log"))
    args = ap.parse_args()
    ctx = lsd.Context(0)
    ctx.set_scan_capacity(lsd.LSD_SCAN_MAX_LEN)
    mapper = lsd.GridMapper(args.size, args.size, RESOL, 0.0, 0.0, RANGE_MAX, min_pass=1, ctx=ctx)
    par = lsd.grid_ray(mapResol=RESOL)
    lines = []
    for beams in (360, 1081, 4096):
        for count in (1, 64, 256):
            scans, lens, poses = rooms(count, beams, args.size, 1)
            d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
            mapper.clear()
            mapper.integrate_device(d_sc, d_ln, d_po)
            grid = mapper.publish_device()
            d_out = torch.zeros((count, beams, 32), dtype=torch.uint8, device="cuda")
            d_sum = torch.zeros((count, 64), dtype=torch.uint8, device="cuda")
            d_so = torch.zeros((count, beams, 2), dtype=torch.float64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            call = lambda: ctx.enqueue_grid_raycast_device(d_sc.data_ptr(), d_ln.data_ptr(), count, beams, d_po.data_ptr(), 24, mapper.map_param,
                                                           RANGE_MAX, grid.data_ptr(), par, d_out.data_ptr(), d_sum.data_ptr(), d_so.data_ptr(), stream)
            med, lo = timed(call, args.reps)
            rays = d_out.cpu().numpy().reshape(-1).view(lsd.GRID_RAY_DTYPE).reshape(count, beams)
            sums = d_sum.cpu().numpy().reshape(-1).view(lsd.GRID_RAY_SUM_DTYPE)
            whole = ray_lengths(scans, poses, rays)
            visited = np.where(rays["k_hit"] >= 0, rays["k_hit"].astype(np.int64) + 1, whole)
            lines.append(json.dumps(dict(what="grid_raycast", grid=args.size, resol=RESOL, range_max=RANGE_MAX, scans=count, beams=beams,
                                         visited=int(visited.sum()), ray_cells=int(whole.sum()), share=float(visited.sum() / whole.sum()),
                                         classes=[int(v) for v in sums["n"].astype(np.int64).sum(0)], ms_median=med, ms_min=lo,
                                         visited_per_us=float(visited.sum() / (1e3 * med)))))
            print(lines[-1], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
