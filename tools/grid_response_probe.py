#!/usr/bin/env python3
"""Developer probe: the response stage (csrc/k_gridresponse.hip) timed alone, beside the coarse-to-fine match at block = 4
(csrc/k_gridmatch_mr.hip) that wrote its records, in the same process on the same inputs, on a 2048 x 2048 grid at 0.05 m.

The generated rooms of tools/grid_probe.py are integrated at their poses, the lookup plane is made from them (the default table), and the
same scans are matched around poses displaced inside the window (--wx, na = 10); the response is then taken around the records with
rx = ry = 3, ra = 1 (the defaults of grid_response()).  Events around each entry, from a warm context; the median, the minimum and the
maximum of REPS launches.  One JSON line per configuration (1 / 64 / 256 scans of 360 / 1081 beams):
  match_ms_*     lsd_enqueue_grid_match_mr_device alone (the coarse plane is there)
  response_ms_*  lsd_enqueue_grid_response_device alone, the volume in the context's workspace
  share          response_ms_median / match_ms_median: what the response adds to a match
with what the response found: the scans with a response, those whose centre is a peak on all three axes, the candidates used.
Usage: tools/grid_response_probe.py [--wx 63] [--reps 20] [--size 2048]"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NA, STEP, BLOCK = 10, 0.5, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wx", type=int, default=63)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    import numpy as np
    import torch
    from grid_match_mr_probe import timed3
    from grid_probe import RANGE_MAX, RESOL, dev, rooms
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    W = args.wx
    ctx = lsd.Context(0)
    ctx.set_scan_capacity(lsd.LSD_SCAN_MAX_LEN)
    mapper = lsd.GridMapper(args.size, args.size, RESOL, 0.0, 0.0, RANGE_MAX, ctx=ctx)
    search = lsd.grid_search(wx=W, wy=W, na=NA, ang_step=STEP, min_beams=30, min_num=1, min_den=4)
    rp = lsd.grid_response()
    shift = (min(41, W - 1) + 0.3, -min(37, W - 2) - 0.2, 3 * STEP + 0.2)   # inside the window, off the whole cells and steps
    s = torch.cuda.current_stream().cuda_stream
    for beams in (360, 1081):
        for count in (1, 64, 256):
            scans, lens, poses = rooms(count, beams, args.size, 1)
            d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
            d_moved = dev(poses + np.array(shift))
            mapper.clear()
            for _ in range(2):
                mapper.integrate_device(d_sc, d_ln, d_po)
            mapper.likelihood_device()
            d_coarse = mapper.coarse_device(BLOCK).data_ptr()
            mp, stride = mapper.map_param, scans.shape[1]
            d_rec = torch.zeros((count, 56), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((count, 192), dtype=torch.uint8, device="cuda")
            match = lambda: ctx.enqueue_grid_match_mr_device(d_sc.data_ptr(), d_ln.data_ptr(), count, stride, d_moved.data_ptr(), 24, mp, RANGE_MAX,
                                                             mapper.d_corr, d_coarse, BLOCK, search, d_rec.data_ptr(), None, s)
            resp = lambda: ctx.enqueue_grid_response_device(d_sc.data_ptr(), d_ln.data_ptr(), count, stride, d_moved.data_ptr(), 24, d_rec.data_ptr(),
                                                            mp, RANGE_MAX, mapper.d_corr, STEP, rp, d_out.data_ptr(), None, s)
            m_med, m_lo, m_hi = timed3(match, args.reps)
            r_med, r_lo, r_hi = timed3(resp, args.reps)
            out = d_out.cpu().numpy().reshape(-1).view(lsd.GRID_RESPONSE_DTYPE)
            valid = (out["flags"] & lsd.GRID_RESPONSE_VALID) != 0
            flat = lsd.GRID_RESPONSE_X_NOT_PEAK | lsd.GRID_RESPONSE_Y_NOT_PEAK | lsd.GRID_RESPONSE_A_NOT_PEAK
            print(json.dumps(dict(what="response", grid=args.size, scans=count, beams=beams, wx=W, wy=W, na=NA, block=BLOCK, rx=rp.rx, ry=rp.ry, ra=rp.ra,
                                  with_response=int(valid.sum()), peaks=int((valid & ((out["flags"] & flat) == 0)).sum()),
                                  mismatch=int(((out["flags"] & lsd.GRID_RESPONSE_MISMATCH) != 0).sum()), used=int(out["n_used"].sum()),
                                  match_ms_median=m_med, match_ms_min=m_lo, match_ms_max=m_hi, response_ms_median=r_med, response_ms_min=r_lo,
                                  response_ms_max=r_hi, share=r_med / m_med)), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
