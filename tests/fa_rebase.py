"""The carry re-base (lsd_enqueue_fa_carry_rebase_device, csrc/k_fa.hip: k_fa_rebase) restated on Python floats, in the header's order
of operations, and the fixture the re-base tests share: a map grown by whole cells on the left and on top, the way a SLAM map that
grows is published again.

A frame is (mapResol, mapOriX, mapOriY): metres = pixels * mapResol + mapOri.  Python's float arithmetic is IEEE double without
contraction, as the build's -ffp-contract=off, so the restatement is bit for bit."""
from fractions import Fraction

import fa_restatement as fr
from fa_resume import ResumableLoop


def frame_of(map_param):
    return tuple(float(v) for v in map_param[2:5])


def rebase_state(x, P, frm, to):
    """(x [9], P rows [9][9]) from frame `frm` to frame `to`; a state without a pose (|x[0] + 1| < 1e-4) is returned as it is."""
    x, P = [float(v) for v in x], [[float(v) for v in r] for r in P]
    if tuple(frm) == tuple(to) or abs(x[0] + 1) < 0.0001:
        return x, P
    s = frm[0] / to[0]
    tx, ty = (frm[1] - to[1]) / to[0], (frm[2] - to[2]) / to[0]
    x[0] = x[0] * s + tx
    x[1] = x[1] * s + ty
    for k in (3, 4, 6, 7):
        x[k] = x[k] * s
    d = [s if k % 3 != 2 else 1.0 for k in range(9)]
    return x, [[(P[i][j] * d[i]) * d[j] for j in range(9)] for i in range(9)]


def rebase_loop(loop, frm, to):
    """The ResumableLoop continued in frame `to`: the state re-based, the loop's resolution the new map's; odom, the angle bookkeeping
    and the frame count are untouched."""
    loop.x, loop.P = rebase_state(loop.x, loop.P, frm, to)
    loop.resol = float(to[0])
    return loop


def rebase_carry(rec, frm, to):
    """An FA_CARRY_DTYPE record re-based: a copy with the state moved, every other byte kept."""
    import numpy as np
    out = rec.copy()
    x, P = rebase_state(rec["state"]["x"], np.asarray(rec["state"]["P"], np.float64).reshape(9, 9, order="F").tolist(), frm, to)
    if not (tuple(frm) == tuple(to) or abs(float(rec["state"]["x"][0]) + 1) < 0.0001):
        out["state"]["x"] = x
        out["state"]["P"] = np.array(P, np.float64).ravel(order="F")
    return out


def metres(x, frame):
    """The exact pose in metres of pixel coordinates (x[0], x[1]) in `frame`, as Fractions."""
    return (Fraction(x[0]) * Fraction(frame[0]) + Fraction(frame[1]), Fraction(x[1]) * Fraction(frame[0]) + Fraction(frame[2]))


def metres_bound(x_from, x_to, frm, to):
    """How far the exact metres pose may move under rebase_state, per coordinate, from the roundings of the formula alone, to first
    order with a factor for the rest: x' = fl(fl(x * s) + t), s = fl(rf / rt), t = fl(fl(of - ot) / rt).  Each rounding moves its
    result by at most u = 2^-53 of its magnitude: s and the product put 2u on |x s|, the difference and the quotient 2u on |t|, the sum
    u on |x'|; in metres that is rt times as much.  (The higher-order terms are below 2^-50 of the bound: the factor 1 + 2^-40.)"""
    u = Fraction(1, 2 ** 53)
    s = Fraction(frm[0] / to[0])
    out = []
    for k in (0, 1):
        t = Fraction((frm[1 + k] - to[1 + k]) / to[0])
        b = u * (2 * abs(Fraction(x_from[k]) * s) + 2 * abs(t) + abs(Fraction(x_to[k])))
        out.append(b * Fraction(to[0]) * (1 + Fraction(1, 2 ** 40)))
    return out


def grow_map(map_cache, map_lines, map_param, d_cols, d_rows, pad):
    """Map B = map A grown by d_cols whole cells on the left and d_rows on top: the cache padded with `pad` (z_occ_max_dis: nothing
    known there), the line records shifted (x by d_cols, y by d_rows; the intercept follows), the origin moved by the same cells so
    that a point of the world keeps its metres.  Returns (cache, lines, map_param)."""
    import numpy as np
    mc = np.asarray(map_cache, np.float64)
    rows, cols = mc.shape
    out = np.full((rows + d_rows, cols + d_cols), float(pad), np.float64)
    out[d_rows:, d_cols:] = mc
    ml = np.array(map_lines, copy=True)
    for f, d in (("x1", d_cols), ("x2", d_cols), ("y1", d_rows), ("y2", d_rows)):
        ml[f] = ml[f] + float(d)
    ml["b"] = ml["b"] + float(d_rows) - ml["k"] * float(d_cols)
    res = float(map_param[2])
    mp = (float(cols + d_cols), float(rows + d_rows), res, float(map_param[3]) - d_cols * res, float(map_param[4]) - d_rows * res)
    return out, ml, mp


def grow_grid(grid, d_cols, d_rows):
    """grow_map for an OccupancyGrid (int8 [rows, cols]): the new cells are unknown (-1)."""
    import numpy as np
    rows, cols = grid.shape
    out = np.full((rows + d_rows, cols + d_cols), -1, np.int8)
    out[d_rows:, d_cols:] = grid
    return out


def replay(frames, odom, loop, map_cache, map_lines, map_param, feature_scan, match):
    """Drives `loop` (a ResumableLoop) through `frames` (indices into the log: frame t uses odom[t + 1] as its new row) on one map.
    feature_scan(t) -> (scan lines, points, lidar position) in this map's geometry; match(cache, map lines, scan lines, points, lidar
    pose, last pose, pairs) -> candidates [n, 4].  Returns the per-frame (x, P, report)."""
    import numpy as np
    out = []
    for t in frames:
        sl, pts, lidar_pos = feature_scan(t)
        sp, last = loop.scan_pose(odom[t + 1]), loop.last_pose()
        lp = (fr.c_round(lidar_pos[0]), fr.c_round(lidar_pos[1]), 0.0)
        pr = np.array(fr.pairs(map_lines["len"], sl["len"]), np.int32).reshape(-1, 2)
        cands = match(map_cache, map_lines, sl, pts, lp, last, pr) if len(pr) else np.zeros((0, 4))
        x, P, rep = fr.feature_association(cands, last, sp, loop.x, loop.P, len(pr))
        loop.finish(odom[t + 1], x, P)
        out.append((x, P, rep))
    return out


__all__ = ["ResumableLoop", "frame_of", "rebase_state", "rebase_loop", "rebase_carry", "metres", "metres_bound", "grow_map", "grow_grid",
           "replay"]
