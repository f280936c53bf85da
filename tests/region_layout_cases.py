"""Maps aimed at the edges of the region stage's LDS layout (csrc/region/config.h, lds.h), shared by tests/test_region_layout_cpu.py (which
proves with the oracle alone that the maps reach those edges) and tests/test_region_layout_gpu.py (which runs them on the device).

The 4-wave build compiled for four workgroups per CU takes the small sizes of region/config.h: windows of 16 columns x 12 rows for the
small-region grower (5 rows above the seed, 6 below; 16 rows -- 7 above, 8 below -- otherwise), a list ring of 256 entries (512), 16 tile
slots.  The maps are 256 x 256 cells, 76 x 76 pixels at the default scale:

  strokes(k), k = 0 .. 7   36 one-pixel strokes of 16 .. 33 cells at the eight orientations: their gradient bands are regions of a few
                           pixels, most of them below regThre (10.4 pixels at this size), which the small-region grower ends itself -- unless
                           what it examines (the members and their neighbours) leaves the seed's window;
  long_edge()              a straight wall edge with a graded profile: one region of several hundred pixels, longer than either list ring;
  diagonal()               a one-pixel diagonal from corner to corner: one region across more 8 x 8 tiles than the tile cache has slots;
  regrown()                walls in noise: holds a region of 87 pixels that Refiner grows again and the NFA test rejects.
"""
import math
import os
import re

import numpy as np

import line_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256
DEG_THRE = 22.5 / 180.0 * math.pi                          # myLSD.cpp:148


def layout():
    """The sizes the two settings of region/config.h select: {"rows": (small, large), "lcap": (small, large), "nt": slots}; the seed sits in
    row (rows - 1) // 2 and column 7 of its window."""
    src = open(os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc", "region", "config.h")).read()

    def pair(name):
        m = re.search(r"#define LSD_REGION_%s \(LSD_REGION_DIET \? (\d+) : (\d+)\)" % name, src)
        return int(m.group(1)), int(m.group(2))
    nt = int(re.search(r"#define LSD_REGION_NT (\d+)", src).group(1))
    return dict(rows=pair("WINROWS"), lcap=pair("LCAP"), nt=nt)


def _stroke(m, cx, cy, ang, length):
    dx, dy = math.cos(ang), math.sin(ang)
    for t in np.arange(-length / 2.0, length / 2.0 + 0.25, 0.5):
        x, y = int(round(cx + t * dx)), int(round(cy + t * dy))
        if 0 <= x < m.shape[1] and 0 <= y < m.shape[0]:
            m[y, x] = lc.OCC


def strokes(k):
    m = np.full((SIZE, SIZE), lc.FREE, np.uint8)
    i = 0
    for gy in range(6):
        for gx in range(6):
            _stroke(m, 22 + gx * 42 + (i * 3 + k) % 5, 22 + gy * 42 + (i * 5 + 2 * k) % 5, ((i + k) % 8) * math.pi / 8, 16 + (i * 7 + k * 3) % 18)
            i += 1
    return m


def long_edge():
    m = np.zeros((SIZE, SIZE), np.uint8)
    ramp = np.clip((np.arange(SIZE) - 100) * 10, 0, 240).astype(np.uint8)
    m[12:SIZE - 12, :] = ramp[None, :]
    m[m == 1] = 2                                           # (1 is the loader's "occupied")
    return m


def diagonal():
    m = np.full((SIZE, SIZE), lc.FREE, np.uint8)
    t = np.arange(10, SIZE - 10)
    m[t, t] = lc.OCC
    return m


def regrown():
    return lc.noise_with_walls(4, SIZE, SIZE)


def stroke_batch():
    return np.stack([strokes(k) for k in range(8)])


def single_maps():
    return {"long_edge": long_edge(), "diagonal": diagonal(), "regrown": regrown()}


def grow(deg, used, x, y):
    """RegionGrower (myLSD.cpp:491-590) restated: the list of a first grow from seed (x, y), as (xs, ys) in grow order."""
    h, w = deg.shape
    member = {(x, y)}
    xs, ys = [x], [y]
    reg = deg[y, x]
    s, c = math.sin(reg), math.cos(reg)
    n, ex = 1, 0
    while ex != n:
        ex = n
        i = 0
        while i < n:
            for m in (ys[i] - 1, ys[i], ys[i] + 1):
                for q in (xs[i] - 1, xs[i], xs[i] + 1):
                    if 0 <= m < h and 0 <= q < w and (q, m) not in member and used[m, q] != 1:
                        d = abs(reg - deg[m, q])
                        if d > math.pi * 1.5:
                            d = abs(d - 2 * math.pi)
                        if d < DEG_THRE:
                            c += math.cos(deg[m, q])
                            s += math.sin(deg[m, q])
                            reg = math.atan2(s, c)
                            member.add((q, m))
                            xs.append(q)
                            ys.append(m)
                            n += 1
            i += 1
    return xs, ys


def reg_thre(w, h):
    return -(5 * (math.log10(h) + math.log10(w)) / 2.0) / math.log10(22.5 / 180.0)   # myLSD.cpp:207-208


def window_classes(dbg, rows_small, rows_large):
    """The small regions of an oracle run (trace records below regThre), restated from the map as it was before the seed loop (a region
    below regThre marks nothing and a rejected one stays growable, so only accepted lines change what a later seed sees: a restated
    region that differs in size from the trace's is left out).  Counts, by the box of what the grower examines -- the members and their
    neighbours inside the image, relative to the seed -- against the window of rows_small rows and the one of rows_large rows (both 16
    columns, 7 left of the seed and 8 right): "up" / "down" leave the small window upwards / downwards and stay inside the large one,
    "inside" stay inside the small one."""
    w, h = dbg["w"], dbg["h"]
    up_s, dn_s = (rows_small - 1) // 2, rows_small - 1 - (rows_small - 1) // 2
    up_l, dn_l = (rows_large - 1) // 2, rows_large - 1 - (rows_large - 1) // 2
    out = dict(up=0, down=0, inside=0, restated=0, small=0)
    thre = reg_thre(w, h)
    for sd in dbg["seeds"]:
        if sd["num"] >= thre:
            continue
        out["small"] += 1
        sx, sy = int(sd["x"]), int(sd["y"])
        xs, ys = grow(dbg["deg"], dbg["used0"], sx, sy)
        if len(xs) != sd["num"]:
            continue
        out["restated"] += 1
        x0, x1 = max(min(xs) - 1, 0) - sx, min(max(xs) + 1, w - 1) - sx
        y0, y1 = max(min(ys) - 1, 0) - sy, min(max(ys) + 1, h - 1) - sy
        if x0 < -7 or x1 > 8 or y0 < -up_l or y1 > dn_l:
            continue                                        # leaves the large window as well
        out["up"] += int(y0 < -up_s)
        out["down"] += int(y1 > dn_s)
        out["inside"] += int(y0 >= -up_s and y1 <= dn_s)
    return out
