#!/usr/bin/env python3
"""Developer probe: the correction of the carries (csrc/k_facorrect.hip), measured, with no threshold.  One JSON line each:

  entry     lsd_enqueue_fa_carry_correct_device alone for 1 / 64 / 1024 sequences at frames_pitch 1 and 8: events around the launch from a
            warm context, the median, minimum and maximum of REPS launches.  Every sequence takes the APPLIED path (a matching slot, a valid
            response); the carries are put back from a pristine copy in front of the first event, since the update is in place.
  tick      one Localizer.refine_and_integrate_last_tick(response=...) on a tick of the data log's first 20 frames, with and without correct=,
            in the same process, alternating: events around the call.
  waypoints the surveyed way-points (DESIGN.md 8.0's median offset, tests/fa_logs.py: way_point_errors) of the f3key and f4key logs -- the
            data log's fixture holds none --, replayed one frame per tick with a GridMapper behind every tick, once with correct=True and
            once without.  Whether the correction shrinks the offset is not known beforehand and nothing is claimed.
Usage: tools/fa_correct_probe.py [--reps 20] > profiles/fa_correct_probe.log"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

RANGE_MAX = 8.0
SEARCH = dict(wx=3, wy=2, na=1, ang_step=0.5, min_beams=30, min_num=1, min_den=8)
RESPONSE = dict(rx=2, ry=2, ra=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import fa_correct_cases as fc
    import fa_logs
    import fa_restatement as fr
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    ctx = lsd.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn, before=lambda: None):
        fn(); torch.cuda.synchronize()                                          # warm
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before(); a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    # 1. the entry alone
    for fp in (1, 8):
        for n in (1, 64, 1024):
            units = [fc.unit("probe_%d" % k, 9000 + k, fp) for k in range(min(n, 64))]
            units = [units[k % len(units)] for k in range(n)]
            pristine = dev(np.array([u["carry"] for u in units]).view(np.uint8))
            d_cy = pristine.clone()
            d_po, d_re = dev(np.concatenate([u["poses"] for u in units])), dev(np.concatenate([u["resp"] for u in units]).view(np.uint8))
            d_rp = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
            fn = lambda: ctx.enqueue_fa_carry_correct_device(d_cy.data_ptr(), n, fp, d_po.data_ptr(), 24, d_re.data_ptr(), None, 0, None, d_rp.data_ptr(), s)
            med, lo, hi = timed(fn, lambda: d_cy.copy_(pristine))
            flags = d_rp.cpu().numpy().view(lsd.FA_CORRECT_DTYPE)["flags"]
            print(json.dumps(dict(what="entry", sequences=n, frames_pitch=fp, applied=int((flags == lsd.FA_CORRECT_APPLIED).sum()),
                                  ms_median=med, ms_min=lo, ms_max=hi)), flush=True)

    # 2. one refine_and_integrate_last_tick with and without the correction
    m, mp, lid, odom = fr.load_log("data")
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsd.z_occ_max_dis)
    ml = lsd.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    mapper = lambda: lsd.GridMapper(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]), RANGE_MAX, ctx=ctx)
    loc, gm_ = lsd.Localizer(mc, ml, mp, 1, odom0=odom[0], ctx=ctx), mapper()
    d_lid, d_od = dev(lid[None, :20]), dev(odom[None, 1:21])
    saved = loc.carries
    for _ in range(2):                                                          # warm: the staging, the planes, the volume
        loc.carries = saved
        loc.step_device(d_lid, d_od)
        loc.integrate_last_tick(gm_)
        loc.refine_and_integrate_last_tick(gm_, SEARCH, response=RESPONSE, correct=True)
    torch.cuda.synchronize()
    ms = {None: [], True: []}
    for rep in range(2 * args.reps):
        correct = (None, True)[rep % 2]
        loc.carries = saved
        loc.step_device(d_lid, d_od)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); loc.refine_and_integrate_last_tick(gm_, SEARCH, response=RESPONSE, correct=correct); b.record(); torch.cuda.synchronize()
        ms[correct].append(a.elapsed_time(b))
    print(json.dumps(dict(what="tick", frames=20, without_ms_median=float(np.median(ms[None])), with_ms_median=float(np.median(ms[True])),
                          without_ms_min=float(min(ms[None])), with_ms_min=float(min(ms[True])))), flush=True)

    # 3. the surveyed way-points, with and without (the data log's fixture holds none: the two key logs that have them)
    for name in ("f3key", "f4key"):
        m, mp, lid, odom = fr.load_log(name)
        mc = ctx.map_cache(m.copy(), float(mp[2]), lsd.z_occ_max_dis)
        ml = lsd.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        real_pos, recorded = fr.load_way_points(name)
        for correct in (None, True):
            loc = lsd.Localizer(mc, ml, mp, 1, odom0=odom[0], ctx=ctx)
            gm_ = lsd.GridMapper(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]), RANGE_MAX, ctx=ctx)
            states, flags = [], []
            for t in range(len(lid)):
                st, _, _ = loc.step_device(dev(lid[None, t:t + 1]), dev(odom[None, t + 1:t + 2]))
                got = loc.refine_and_integrate_last_tick(gm_, SEARCH, response=RESPONSE, integrate_at="response", correct=correct)
                states.append(st.cpu().numpy().reshape(-1).view(lsd.FA_STATE_DTYPE)[0]["x"].copy())
                if correct:
                    flags.append(int(got[2].cpu().numpy().reshape(-1).view(lsd.FA_CORRECT_DTYPE)[0]["flags"]))
            err = fa_logs.way_point_errors(states, mp, real_pos, recorded)
            ok = err[~np.isnan(err)]
            print(json.dumps(dict(what="waypoints", log=name, correct=bool(correct), frames=len(lid), way_points=len(recorded),
                                  without_pose=int(np.isnan(err).sum()), median_error_m=float(np.median(ok)) if len(ok) else None,
                                  max_error_m=float(ok.max()) if len(ok) else None,
                                  outcomes={fc.FLAG_NAMES[f]: flags.count(f) for f in sorted(set(flags))})), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
