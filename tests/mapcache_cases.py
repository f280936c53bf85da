"""The createMapCache campaign: a restatement of mylsd::createMapCache (LSD/myLSD.cpp:11-127) that records the flood, and the maps
that drive k_mapcache.hip where the fixtures and random maps do not go -- floods deeper than the spread path plans (k_mc_finish has
work), rings cut off by the radius test (:53), cells whose value depends on the FIFO order, shapes smaller than the spread path's
chunk count, frontiers on and beside the 1024-node round, every cell value.  tests/test_mapcache_cases_cpu.py shows that the
restatement equals the oracle bit for bit and that every class reaches what it was built for; tests/test_mapcache_cases_gpu.py
runs the cases on the device.  No GPU and no oracle is needed to import this module.

FIFO order is level order, and inside a level the queue order is (rank of the parent in its level, direction up/left/down/right),
so the restatement runs level by level with numpy: the offers of a level in queue order, the first offer per cell wins."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIRS = ("up", "left", "down", "right")                      # :48, :67, :86, :105
_DI = np.array([-1, 0, 1, 0])
_DJ = np.array([0, -1, 0, 1])


def cell_radius(res, z):
    return int(math.floor(z / res))                         # :13


def planned_levels(rows, cols, res, z):
    """The levels launch_mapcache_spread enqueues before k_mc_finish: int(1.5 * cell_radius) + 3, at most rows + cols."""
    return min(int(1.5 * max(cell_radius(res, z), 0)) + 3, rows + cols)


class Flood:
    """values float64 [rows, cols]; level int32 [rows, cols] (-1: never claimed, 0: occupied); depth: the highest level;
    stopped: nodes the radius test kept from expanding; sensitive: cells offered in their claiming level by at least two parents
    whose distance * res differ; winners / losers: per direction, how often it delivered the winning / a losing offer with a
    different value to such a cell; contested: per direction, how often it won a cell that at least two parents offered, whatever
    their values; frontiers: the size of every level's frontier, level 0 first."""


def flood(m, res, z=1.0):
    rows, cols = m.shape
    radius = cell_radius(res, z)
    occ = np.flatnonzero(m.reshape(-1) == 1)                # raster order :22-40
    values = np.full(rows * cols, float(z), np.float64)
    values[occ] = 0.0
    level = np.full(rows * cols, -1, np.int32)
    level[occ] = 0
    cur, src = occ.astype(np.int64), occ.astype(np.int64)
    f = Flood()
    f.stopped = f.sensitive = 0
    f.winners, f.losers, f.contested = [0] * 4, [0] * 4, [0] * 4
    f.frontiers = []
    lv = 0
    while cur.size:
        f.frontiers.append(int(cur.size))
        ci, cj, si, sj = cur // cols, cur % cols, src // cols, src % cols
        di, dj = np.abs(ci - si).astype(np.float64), np.abs(cj - sj).astype(np.float64)       # :49-50
        dist = np.sqrt(di * di + dj * dj)                                                   # :51
        go = dist <= radius                                                                 # :53
        f.stopped += int((~go).sum())
        k = np.flatnonzero(go)
        ni, nj = ci[k, None] + _DI, cj[k, None] + _DJ                                       # [parents, 4] in queue order
        inside = (ni >= 0) & (ni < rows) & (nj >= 0) & (nj < cols)
        nb = np.where(inside, ni * cols + nj, 0)
        offer = inside & (level[nb] < 0)
        cells = nb[offer]
        vals = np.broadcast_to((dist[k] * res)[:, None], nb.shape)[offer]                   # :54, the PARENT's distance
        srcs = np.broadcast_to(src[k][:, None], nb.shape)[offer]
        dirs = np.broadcast_to(np.arange(4), nb.shape)[offer]
        _, first, inv, offers = np.unique(cells, return_index=True, return_inverse=True, return_counts=True)
        for d in range(4):
            f.contested[d] += int(((dirs[first] == d) & (offers > 1)).sum())
        won = np.zeros(cells.size, bool)
        won[first] = True
        differs = vals.view(np.int64) != vals[first][inv].view(np.int64)                    # a losing offer of another value
        f.sensitive += int(np.unique(cells[differs]).size)
        for d in range(4):
            f.losers[d] += int((differs & (dirs == d)).sum())
        sens_win = np.zeros(cells.size, bool)
        sens_win[first[np.unique(inv[differs])]] = True
        for d in range(4):
            f.winners[d] += int((sens_win & (dirs == d)).sum())
        lv += 1
        values[cells[won]] = vals[won]
        level[cells[won]] = lv
        cur, src = cells[won], srcs[won]                                                    # still in queue order
    f.values, f.level = values.reshape(rows, cols), level.reshape(rows, cols)
    f.depth = int(level.max()) if level.size else 0
    f.max_frontier = max(f.frontiers) if f.frontiers else 0
    return f


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cls, name, m, res, z=1.0):
        self.cls, self.name, self.res, self.z = cls, name, float(res), float(z)
        self.map = np.ascontiguousarray(m, np.uint8)
        self.map.setflags(write=False)

    @property
    def planned(self):
        return planned_levels(self.map.shape[0], self.map.shape[1], self.res, self.z)

    def __repr__(self):
        return "%s/%s" % (self.cls, self.name)


def from_sources(rows, cols, sources, fill=0):
    m = np.full((rows, cols), fill, np.uint8)
    for i, j in sources:
        m[i, j] = 1
    return m


def _detours():
    """Source lists found by tests/golden/make_mapcache_detours.py (a seeded hill-climb over source placements): trees of different
    sources block each other into detours, so the flood outlives the planned levels.  detour_r10_witness is the list of the issue."""
    out = []
    for name, d in sorted(json.load(open(os.path.join(GOLDEN, "mapcache_detours.json"))).items()):
        out.append(Case("detour", name, from_sources(d["rows"], d["cols"], d["sources"]), d["res"], d["z"]))
    return out


def _radius():
    out = []
    one = from_sources(36, 36, [(17, 18)])
    wall = from_sources(36, 36, [(12, j) for j in range(10, 17)] + [(i, 25) for i in range(20, 24)])
    for res, r in ((2.0, 0), (1.0, 1), (0.5, 2), (0.3, 3), (0.2, 5)):
        assert cell_radius(res, 1.0) == r
        out.append(Case("radius", "single_r%d" % r, one, res))
        out.append(Case("radius", "walls_r%d" % r, wall, res))
    big = from_sources(96, 96, [(47, 48)] + [(20, j) for j in range(5, 12)])
    out.append(Case("radius", "single_r40", big, 0.025))
    # quotients on and beside an integer
    mid = from_sources(64, 64, [(31, 32)] + [(5, j) for j in range(50, 56)])
    out.append(Case("radius", "q_0.3_0.1", one, 0.1, 0.3))                      # 2.9999999999999996 -> 2
    out.append(Case("radius", "q_1.0_0.2", wall, 0.2, 1.0))                     # 5.0
    out.append(Case("radius", "q_2.0_0.05", big, 0.05, 2.0))                    # 40.0
    out.append(Case("radius", "q_res_above_0.05", mid, np.nextafter(0.05, 1.0)))   # 19.999999999999996 -> 19
    out.append(Case("radius", "q_res_below_0.05", mid, np.nextafter(0.05, 0.0)))   # 20.000000000000004 -> 20
    out.append(Case("radius", "q_res_0.05", mid, 0.05))
    # the radius is larger than the map: nothing is cut off, and the planned levels are capped at rows + cols
    out.append(Case("radius", "beyond_map", wall, 0.01))
    return out


def _ties():
    out = []
    base = {
        "pair_row": from_sources(24, 24, [(10, 6), (11, 15)]),
        "pair_knight": from_sources(24, 24, [(8, 9), (10, 14), (15, 10)]),
        "pair_diag": from_sources(24, 24, [(6, 6), (15, 17), (6, 17)]),
    }
    rng = np.random.default_rng(41)
    lat = [(i + int(rng.integers(0, 3)), j + int(rng.integers(0, 3))) for i in range(2, 44, 7) for j in range(2, 44, 6)]
    base["lattice"] = from_sources(48, 48, lat)
    for name, m in base.items():                         # every orientation
        for tag, v in (("", m), ("_ud", m[::-1]), ("_lr", m[:, ::-1]), ("_t", m.T)):
            out.append(Case("ties", name + tag, v, 0.1))
    # An "up" offer hardly ever wins against an offer of another value: the parent below a cell comes late in the queue.  One map in
    # 40 000 random ones had such a cell (radius 5: a tree stopped by the radius test leaves the cell to the parent below).
    out.append(Case("ties", "up_wins", from_sources(8, 11, [(1, 1), (2, 1), (6, 0), (6, 2), (7, 0), (7, 4), (7, 10)]), 0.2))
    return out


def _border(rows, cols):
    m = np.zeros((rows, cols), np.uint8)
    m[0, ::3] = 1; m[rows - 1, 1::3] = 1; m[::3, 0] = 1; m[1::3, cols - 1] = 1
    m[0, 0] = m[0, cols - 1] = m[rows - 1, 0] = m[rows - 1, cols - 1] = 1
    return m


def _shapes():
    out = []
    out.append(Case("shapes", "1x1_occupied", np.ones((1, 1)), 0.1))
    out.append(Case("shapes", "1x1_free", np.zeros((1, 1)), 0.1))
    out.append(Case("shapes", "1x65", from_sources(1, 65, [(0, 0), (0, 40)]), 0.05))
    out.append(Case("shapes", "65x1", from_sources(65, 1, [(64, 0), (20, 0)]), 0.05))
    out.append(Case("shapes", "2x2", from_sources(2, 2, [(1, 0)]), 0.1))
    out.append(Case("shapes", "3x3", from_sources(3, 3, [(1, 1)]), 0.1))
    out.append(Case("shapes", "3x3_corners", from_sources(3, 3, [(0, 0), (0, 2), (2, 0), (2, 2)]), 0.1))
    for rows, cols in ((9, 63), (9, 64), (9, 65), (33, 31), (32, 32), (25, 41), (1, 1023), (1024, 1), (5, 205)):
        rng = np.random.default_rng(rows * 10000 + cols)
        m = np.zeros((rows, cols), np.uint8)
        m[rng.random((rows, cols)) < 0.03] = 1
        m[0, 0] = m[0, cols - 1] = m[rows - 1, 0] = m[rows - 1, cols - 1] = 1          # all four corners
        out.append(Case("shapes", "%dx%d" % (rows, cols), m, 0.1))
    out.append(Case("shapes", "borders_36x36", _border(36, 36), 0.1))
    out.append(Case("shapes", "borders_31x64", _border(31, 64), 0.05))
    return out


def _exactly(rows, cols, k, seed):
    m = np.zeros(rows * cols, np.uint8)
    m[np.random.default_rng(seed).choice(rows * cols, k, replace=False)] = 1
    return m.reshape(rows, cols)


def _frontiers():
    out = []
    for k in (1023, 1024, 1025, 2500):
        out.append(Case("frontier", "level0_%d" % k, _exactly(64, 64, k, k), 0.05))
    checker = (np.indices((64, 64)).sum(0) & 1).astype(np.uint8)                    # 2048 sources, first ring 2048
    out.append(Case("frontier", "checker_64x64", checker, 0.05))
    lat = np.zeros((96, 96), np.uint8)
    lat[1::3, 1::3] = 1                                                             # 1024 sources, first ring 4096
    out.append(Case("frontier", "lattice3_96x96", lat, 0.05))
    return out


def _values():
    out = []
    rng = np.random.default_rng(77)
    m = rng.choice(np.array([0, 1, 2, 100, 254, 255], np.uint8), size=(40, 52), p=[0.3, 0.03, 0.17, 0.1, 0.1, 0.3])
    out.append(Case("values", "mixed_40x52", m, 0.1))
    out.append(Case("values", "mixed_40x52_z2", m, 0.1, 2.0))
    out.append(Case("values", "empty_36x36", np.zeros((36, 36)), 0.1))
    out.append(Case("values", "empty_of_255", np.full((36, 36), 255), 0.1))
    out.append(Case("values", "full_36x36", np.ones((36, 36)), 0.1))
    out.append(Case("values", "full_but_one", 1 - from_sources(36, 36, [(20, 7)]), 0.1))
    return out


CLASSES = ("detour", "radius", "ties", "shapes", "frontier", "values")
CASES = _detours() + _radius() + _ties() + _shapes() + _frontiers() + _values()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(c.res >= 0.005 and c.map.shape[0] * c.map.shape[1] <= 96 * 160 for c in CASES)


def cases(cls):
    return [c for c in CASES if c.cls == cls]


# ---- batches for lsd_enqueue_map_cache_device -----------------------------------------------------------------------------------------
# The entry spreads a map over G = min(64, 2 * num_cus // n) workgroups when G >= 4 and runs one workgroup per map otherwise.
BATCHES = ("one_workgroup", "smallest_spread", "three")
BATCH_RES, BATCH_Z = 0.05, 1.0
BATCH_CORE = ("detour_r20", "level0_2500", "checker_64x64", "ties_64x64", "empty_64x64", "full_64x64", "level0_1025", "q_res_0.05")


def batch_size(name, num_cus):
    return {"one_workgroup": num_cus // 2 + 1, "smallest_spread": num_cus // 2, "three": 3}[name]


def _core_map(name):
    if name == "ties_64x64":
        return np.pad(BY_NAME["lattice"].map, 8)
    if name == "empty_64x64":
        return np.zeros((64, 64), np.uint8)
    if name == "full_64x64":
        return np.ones((64, 64), np.uint8)
    assert BY_NAME[name].map.shape == (64, 64)
    return BY_NAME[name].map


def batch(name, num_cus):
    """n maps of 64x64 at BATCH_RES: the core maps (a detour map, more than 1024 sources, a tie map, an empty and a full one, ...) and
    after them the detour map's sources shifted and thinned differently per index, so that no two maps of the batch are equal."""
    n = batch_size(name, num_cus)
    maps = [_core_map(c) for c in BATCH_CORE[:n]]
    det = BY_NAME["detour_r20"].map
    for i in range(len(maps), n):
        rng = np.random.default_rng(1000 + i)
        m = np.roll(det, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1)).copy()
        m[rng.random(m.shape) < 0.004 * (1 + i % 5)] = 1
        m[(m != 1) & (rng.random(m.shape) < 0.2)] = 255 if i % 2 else 2          # not occupied
        maps.append(m)
    out = np.stack(maps)
    if name == "three":                                      # a detour map first, in the middle and last in turn
        out = out[[1, 0, 2]]
    return out
