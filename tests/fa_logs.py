"""Replays of recorded logs on the CPU and their ground-truth anchor, shared by tests/test_localize_more_cpu.py and the survey mode of
tests/golden/make_localize_logs.py.

The anchor: realPos.txt holds surveyed way-points in metres, recored_Odom.txt the frame count at which the robot stood on each.  The
reference spreads them over the frames as sampleRealPos.colRange(rec[i] - 1, ...) (ROS/lsd/src/FeatureAssociation.cpp:363): column
rec[i] - 1 of a 0-based matrix is way-point i, so a recorded index is the driver's 1-based cnt_frame, and the pose to compare is the
state AFTER frame t = rec[i] - 1.  A pose in pixels becomes metres as x * mapResol + mapOri (:127-128 of the same file, the inverse of
FeatureScan's (metres - mapOri) / mapResol)."""
import numpy as np

import fa_restatement as fr


def replay(oracle, lsdmod, log, _lib=None):
    """The replay driver's loop on the CPU: the oracle's FeatureScan and matching (glibc, or _lib), then the restatement.
    log: a name for fr.load_log, or (map u8, map_param, lidar [n, 360, 2], odom [n + 1, 3]).  Returns [(x, report, kept)] per frame."""
    m, mp, lid, odom = fr.load_log(log) if isinstance(log, str) else log
    mc = oracle.map_cache(m.copy(), mp[2])
    ml = oracle.lsd(m.copy())["lines"]
    scans, lens = lsdmod.lidar_frames(lid)
    loop = fr.Loop(odom, mp[2])
    out = []
    for t in range(len(scans)):
        fs = oracle.feature_scan(scans[t, :lens[t]], mp)
        sp = loop.scan_pose(t)
        lp = loop.lidar_pose(fs["lidar_pos"])
        last = loop.last_pose()
        pr = np.array(fr.pairs(ml["len"], fs["lines"]["len"]), np.int32).reshape(-1, 2)
        cands = oracle.scan_to_map_match(mc, ml, fs["lines"], fs["pts"], lp, last, pr, _lib=_lib).reshape(-1, 4) if len(pr) else np.zeros((0, 4))
        x, P, rep = fr.feature_association(cands, last, sp, loop.x, loop.P, len(pr))
        loop.finish(t, x, P)
        out.append((x, rep, fr.keep_sorted(cands)))
    return out


def has_fix(x):
    """A state that holds a pose: finite, and not the reset sentinel (-1, -1)."""
    return bool(np.isfinite(x[0]) and np.isfinite(x[1]) and not abs(x[0] + 1) < 0.0001)


def way_point_errors(states, map_param, real_pos, recorded):
    """Distance in metres between each way-point and the pose after its recorded frame; NaN where that state holds no pose."""
    err = np.full(len(recorded), np.nan)
    for i, (rec, (wx, wy)) in enumerate(zip(recorded, real_pos)):
        x = states[int(rec) - 1]
        if has_fix(x):
            err[i] = np.hypot(x[0] * map_param[2] + map_param[3] - wx, x[1] * map_param[2] + map_param[4] - wy)
    return err


def resets_after_first_fix(branches):
    """RESET frames after the first FIRST frame: how often the log loses its fix."""
    b = list(branches)
    return b[b.index(fr.FIRST):].count(fr.RESET) if fr.FIRST in b else 0


def summary(run, map_param, real_pos, recorded):
    """The survey's record of one replay (the list replay() returns)."""
    br = [r["branch"] for _, r, _ in run]
    err = way_point_errors([x for x, _, _ in run], map_param, real_pos, recorded)
    ok = err[~np.isnan(err)]
    return dict(frames=len(run), branches=dict(reset=br.count(fr.RESET), first=br.count(fr.FIRST), ukf=br.count(fr.UKF)),
                resets_after_first_fix=resets_after_first_fix(br), max_n_pairs=max(r["n_pairs"] for _, r, _ in run),
                max_n_kept=max(r["n_kept"] for _, r, _ in run), llt_failures=sum(r["llt"] >= 0 for _, r, _ in run),
                nan_frames=sum(bool(np.isnan(x).any()) for x, _, _ in run), way_points=len(recorded),
                way_points_without_pose=int(np.isnan(err).sum()),
                median_error_m=float(np.median(ok)) if len(ok) else None, max_error_m=float(ok.max()) if len(ok) else None)
