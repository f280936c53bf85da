"""Hand-made frames for the pair list of k_fa_prepare (csrc/k_fa.hip) and a whole frame of lsd_feature_association behind it
(shared by the CPU and GPU tests).

The map is a synthetic 96 x 64 room (walls of cells 1 on free cells 255); the lsd_line records of both sides are written by hand
from real end points on its walls, with `len` then overwritten where a case needs a length that no segment of the room has.  The
scan frame is the map frame (the true pose is the identity), the lidar stands in the middle, the scan points lie on the walls.
  length cases  one special scan line with len = nextafter(40, 0), 40, NaN, inf between two ordinary ones (44 and 30), against map
                lines of len 26, the double below, 54, the double above, NaN, inf, 40 and 20: the pair conditions of myFA.cpp:32 and
                :40 on and beside their thresholds (40 * 0.35 is exactly 14), and where a NaN makes every comparison false
  count cases   (n_scan, n_map) with the product n_scan * n_map at 255 / 256 / 257 (the ordered compaction walks it in rounds of
                256), an empty side, one line a side, and the 360-record pitch; about half of the scan lines too short and every
                fourth map line too short, so that the compaction has holes
"""
import math

import numpy as np

COLS, ROWS, RES = 96, 64, 0.025
X0, X1, Y0, Y1 = 10, 85, 8, 55                            # the room's walls
LIDAR = (48.0, 32.0, 0.0)
NEAR = (49.0, 31.0, 0.0)                                  # a lastPose within maxEstiDist of every candidate of this room
FIRST = (-1.0, -1.0, 0.0)
SCAN_POSE = (1.25, -0.5, 0.75)
INF, NAN = float("inf"), float("nan")
LINE_DTYPE = np.dtype([("k", "f8"), ("b", "f8"), ("dx", "f8"), ("dy", "f8"), ("x1", "f8"), ("y1", "f8"),
                       ("x2", "f8"), ("y2", "f8"), ("len", "f8"), ("orient", "i4"), ("_pad", "i4")])
SCAN_LENGTHS = (("below40", math.nextafter(40.0, 0.0)), ("40", 40.0), ("nan", NAN), ("inf", INF))
MAP_LENGTHS = (26.0, math.nextafter(26.0, 0.0), 54.0, math.nextafter(54.0, INF), NAN, INF, 40.0, 20.0)
COUNTS = ((0, 5), (5, 0), (1, 1), (16, 16), (15, 17), (17, 15), (1, 257), (257, 1), (360, 3))


def room():
    m = np.full((ROWS, COLS), 255, np.uint8)
    m[Y0, X0:X1 + 1] = 1; m[Y1, X0:X1 + 1] = 1; m[Y0:Y1 + 1, X0] = 1; m[Y0:Y1 + 1, X1] = 1
    return m


def points():
    """40 scan points on the walls; those of the top wall three pixels inside it (mapCache is 0 up to one pixel from a wall), so that no alignment scores exactly 0 (a kept score of
    0 makes the state NaN: tests/test_localize_cpu.py has that quirk to itself)."""
    top = [(x, Y0 + 3) for x in range(X0 + 2, X1, 6)]
    bot = [(x, Y1) for x in range(X0 + 4, X1, 6)]
    left = [(X0, y) for y in range(Y0 + 3, Y1, 7)]
    right = [(X1, y) for y in range(Y0 + 5, Y1, 7)]
    p = np.zeros((len(top + bot + left + right), 3))
    p[:, :2] = top + bot + left + right
    return p


def segment(j, length):
    """Segment j of `length` pixels on wall j % 4 (top, right, bottom, left), its start moving along the wall with j."""
    wall, step = j % 4, j // 4
    if wall % 2 == 0:
        x = X0 + (3 * step) % (X1 - X0 - length + 1)
        y = Y0 if wall == 0 else Y1
        return (x, y, x + length, y)
    y = Y0 + step % (Y1 - Y0 - length + 1)
    x = X1 if wall == 1 else X0
    return (x, y, x, y + length)


def lines(segs, lens=None):
    out = np.zeros(len(segs), LINE_DTYPE)
    for i, (x1, y1, x2, y2) in enumerate(segs):
        o = out[i]
        o["x1"], o["y1"], o["x2"], o["y2"], o["dx"], o["dy"] = x1, y1, x2, y2, x2 - x1, y2 - y1
        o["len"] = math.hypot(x2 - x1, y2 - y1)
        o["orient"] = 1
    if lens is not None:
        for i, v in enumerate(lens):
            if v is not None:
                out["len"][i] = v
    return out


def length_case(ls):
    """(map lines, scan lines): scan line 1 has len = ls (its end points are 40 apart), map line j has len MAP_LENGTHS[j]."""
    scan = lines([segment(0, 44), segment(2, 40), segment(1, 30)], [None, ls, None])
    mp = lines([segment(j, 40) for j in range(len(MAP_LENGTHS))], MAP_LENGTHS)
    return mp, scan


def count_case(n_scan, n_map):
    """Scan lines 44 long, every other one 30 (too short); map lines 40..44 long, every fourth one 20 (too short for a 44)."""
    scan = lines([segment(j, 30 if j % 2 else 44) for j in range(n_scan)])
    mp = lines([segment(j, 20 if j % 4 == 3 else 40 + 2 * (j % 3)) for j in range(n_map)])
    return mp, scan


def cases():
    """[(name, map lines, scan lines, lastPose)]"""
    out = []
    for name, ls in SCAN_LENGTHS:
        mp, scan = length_case(ls)
        out.append(("len_%s_near" % name, mp, scan, NEAR))
        out.append(("len_%s_first" % name, mp, scan, FIRST))
    for n_scan, n_map in COUNTS:
        mp, scan = count_case(n_scan, n_map)
        out.append(("count_%dx%d" % (n_scan, n_map), mp, scan, NEAR))
    return out


def state():
    rng = np.random.default_rng(4)
    A = rng.normal(size=(9, 9))
    return np.linspace(-2, 2, 9) + np.array([48.0, 32.0, 0, 0, 0, 0, 0, 0, 0]), A @ A.T + 9 * np.eye(9)
