#!/usr/bin/env python3
"""Developer probe: the time of k_grid_likelihood, k_grid_match and k_grid_match_pick (csrc/k_gridmatch.hip) on a 2048 x 2048 grid at
0.05 m.

The generated rooms of tools/grid_probe.py are integrated at their poses, the lookup plane is made from them (the default table), and the
same scans are matched around poses displaced by (3, -2) cells and one angle step, at wx = wy = 10, na = 10 (9261 candidates a scan).
Events around each entry, from a warm context; the median and the minimum of REPS launches.  The match entry is two launches, so its
time is k_grid_match + k_grid_match_pick; the pick alone is timed on the same records with a window of one candidate and no beams
(len = 0), where k_grid_match has nothing to do but start.  One JSON line per measurement: lookups = scored beams x candidates, so a time
reads as lookups per nanosecond; the likelihood pass in GB/s of compulsory traffic (8 bytes read, 1 written per cell), to set beside
k_grid_publish (profiles/grid_probe.log).
Usage: tools/grid_match_probe.py [--reps 20] [--size 2048]"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from grid_probe import RANGE_MAX, RESOL, dev, rooms, timed

lsd = importlib.import_module("linesegmentdetector-slam_amd")
W, NA, STEP = 10, 10, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    ctx = lsd.Context(0)
    ctx.set_scan_capacity(lsd.LSD_SCAN_MAX_LEN)
    mapper = lsd.GridMapper(args.size, args.size, RESOL, 0.0, 0.0, RANGE_MAX, ctx=ctx)
    search = lsd.grid_search(wx=W, wy=W, na=NA, ang_step=STEP, min_beams=30, min_num=1, min_den=4)
    one = lsd.grid_search(wx=0, wy=0, na=NA, ang_step=STEP, min_beams=30, min_num=1, min_den=4)
    cand = (2 * W + 1) ** 2 * (2 * NA + 1)
    for beams in (360, 1081, 4096):
        for count in (1, 64, 256):
            scans, lens, poses = rooms(count, beams, args.size, 1)
            d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
            d_moved = dev(poses + np.array([3.0, -2.0, STEP]))
            d_none = torch.zeros_like(d_ln)
            mapper.clear()
            for _ in range(2):
                mapper.integrate_device(d_sc, d_ln, d_po)
            med_l, lo_l = timed(lambda: mapper.likelihood_device(), args.reps)
            rec = mapper.match_device(d_sc, d_ln, d_moved, 24, search)
            r = rec.cpu().numpy().reshape(-1).view(lsd.GRID_MATCH_DTYPE)
            scored = int(r["n_beams"].sum())                                 # (of the winners' angles: the count barely moves with the angle)
            back = int(((r["di"] == -3) & (r["dj"] == 2) & (r["da"] == -1)).sum())
            med_m, lo_m = timed(lambda: mapper.match_device(d_sc, d_ln, d_moved, 24, search), args.reps)
            med_p, lo_p = timed(lambda: mapper.match_device(d_sc, d_none, d_moved, 24, one), args.reps)
            cells = args.size * args.size
            print(json.dumps(dict(what="grid_likelihood", grid=args.size, cells=cells, ms_median=med_l, ms_min=lo_l,
                                  gb_per_s=9 * cells / (1e6 * med_l))), flush=True)
            print(json.dumps(dict(what="grid_match+pick", grid=args.size, scans=count, beams=beams, wx=W, wy=W, na=NA, candidates=cand,
                                  scored_beams=scored, lookups=scored * cand, recovered=back, ms_median=med_m, ms_min=lo_m,
                                  lookups_per_ns=scored * cand / (1e6 * med_m))), flush=True)
            print(json.dumps(dict(what="empty_match+pick", note="both launches with nothing to sum: the floor the pick and the launches set",
                                  scans=count, ms_median=med_p, ms_min=lo_p)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
