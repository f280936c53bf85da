#!/usr/bin/env python3
"""Developer probe: relocalisation of the lost robots of a fleet (csrc/k_falost.hip, csrc/k_faseed.hip) beside the
route there was before it, on the set-up of tools/grid_locate_probe.py.

A Localizer of --robots robots (64) on a 2048 x 2048 grid at 0.05 m: the generated rooms of tools/grid_probe.py are integrated at their
poses, the lookup plane is made from them, and one tick is taken with those scans against a map without lines, so every robot's frame ends
in LSD_FA_RESET; then all but --lost of the robots (1, 4) are given a pose.  Events around each call, from a warm context; the median, the
minimum and the maximum of REPS calls; the carries are put back between the calls, outside the events.  One JSON line per measurement:
  relocate   Localizer.relocate_last_tick(max_lost = --max-lost): gather, pyramid, locate of max_lost rows, seed; the outcomes and the
             workspace of a locate of max_lost scans
  locate_all Localizer.locate_last_tick on the same inputs: pyramid and locate of every slot -- the only route before, which leaves the
             carries to the host --, and the workspace of a locate of every slot
  relocate_tight (--tight) relocate with tight=True on the same inputs in the same process
720 headings of 0.5 degrees over the whole grid at levels = 8, no refresh of the lookup plane in either (it is the same launch in both).
Usage: tools/relocate_probe.py --lost 1 [--robots 64] [--max-lost 4] [--beams 360] [--reps 20] [--size 2048]"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ANG, STEP, ANG0, LEVELS = 720, 0.5, -180.0, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lost", type=int, default=1)
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--max-lost", type=int, default=4)
    ap.add_argument("--beams", type=int, default=360)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tight", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from grid_probe import RANGE_MAX, RESOL, dev, rooms
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    S, beams, size = args.robots, args.beams, args.size
    ctx = lsd.Context(0)
    mapper = lsd.GridMapper(size, size, RESOL, 0.0, 0.0, RANGE_MAX, ctx=ctx)
    scans, lens, poses = rooms(S, beams, size, 1)
    d_sc, d_ln, d_po = dev(scans), dev(lens), dev(poses)
    for _ in range(2):
        mapper.integrate_device(d_sc, d_ln, d_po)
    mapper.likelihood_device()
    # a map without lines: every frame ends in LSD_FA_RESET, so the tick's states and the carries are those of lost robots
    loc = lsd.Localizer(np.zeros((size, size)), np.zeros(0, lsd.LINE_DTYPE), (size, size, RESOL, 0.0, 0.0), S, ctx=ctx, n_beams=beams)
    loc.step_device(d_sc.reshape(S, 1, beams, 2), torch.zeros((S, 1, 3), dtype=torch.float64, device="cuda"))
    carries = loc.carries
    assert (carries["state"]["x"][:, 0] == -1.0).all(), "the tick was to leave every robot without a pose"
    lost = np.linspace(0, S - 1, args.lost).round().astype(int)
    carries["state"]["x"][:, 0] = 100.0
    carries["state"]["x"][lost, 0] = -1.0
    saved = dev(carries.view(np.uint8).reshape(-1))
    par = lsd.grid_locate(cols=size, rows=size, ang0=ANG0, ang_step=STEP, n_ang=N_ANG, levels=LEVELS, max_nodes=1 << 20, min_beams=30, min_num=1,
                          min_den=4)
    ws = lambda n: ctx.L.lsd_grid_locate_workspace_bytes(n, beams, par)
    got = {}

    def relocate(tight=None):
        loc._carry.copy_(saved)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got["r"] = loc.relocate_last_tick(mapper, par, dict(max_best=1), max_lost=args.max_lost, refresh=False, tight=tight)
        b.record()
        return a, b

    def locate_all():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got["l"] = loc.locate_last_tick(mapper, par, refresh=False)
        b.record()
        return a, b

    def timed(fn):
        fn(); torch.cuda.synchronize()                                      # warm
        ms = []
        for _ in range(args.reps):
            a, b = fn(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))
    for what, fn in [("relocate", relocate)] + ([("relocate_tight", lambda: relocate(True))] if args.tight else []):
        med, lo, hi = timed(fn)
        pick, n_lost, rec, rep = (t.cpu().numpy() for t in got["r"])
        rep, rec = rep.reshape(-1).view(lsd.FA_SEED_DTYPE), rec.reshape(-1).view(lsd.GRID_LOCATE_DTYPE)
        seeded = rep["flags"] == lsd.FA_SEED_SEEDED
        near = [bool(abs(r["pose"][0] - poses[r["seq"], 0]) <= 2 and abs(r["pose"][1] - poses[r["seq"], 1]) <= 2) for r in rep[seeded]]
        print(json.dumps(dict(what=what, grid=size, robots=S, lost=args.lost, max_lost=args.max_lost, beams=beams, headings=N_ANG, levels=LEVELS,
                              ms_median=med, ms_min=lo, ms_max=hi, workspace_mb=ws(args.max_lost) / 2 ** 20, n_lost=n_lost.tolist(), pick=pick.tolist(),
                              seed_flags=[int(f) for f in rep["flags"]], locate_flags=[int(f) for f in rec["flags"]], seeded=int(seeded.sum()),
                              within_two_cells_of_the_generated_pose=int(sum(near)))), flush=True)
    med, lo, hi = timed(locate_all)
    rec = got["l"].cpu().numpy().reshape(-1).view(lsd.GRID_LOCATE_DTYPE)
    print(json.dumps(dict(what="locate_all", grid=size, robots=S, lost=args.lost, slots=S, beams=beams, headings=N_ANG, levels=LEVELS, ms_median=med,
                          ms_min=lo, ms_max=hi, workspace_mb=ws(S) / 2 ** 20, accepted=int((rec["flags"] == lsd.GRID_LOCATE_ACCEPTED).sum()))),
          flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
