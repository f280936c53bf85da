"""Writes tests/golden/mapcache_detours.json: source placements whose createMapCache flood is deeper than the levels the spread path
plans (int(1.5 * cell_radius) + 3), so that k_mc_finish claims cells.  Uniform random maps almost never get there; a seeded
hill-climb over source placements does: move, add or drop one source, keep the change if (depth, cells in the two deepest levels)
does not get worse.  Deterministic: run it again and the file comes out the same.

    python tests/golden/make_mapcache_detours.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mapcache_cases import cell_radius, flood, from_sources, planned_levels      # noqa: E402

WITNESS = [(0, 15), (0, 22), (2, 19), (2, 33), (3, 26), (5, 22), (6, 14), (6, 17), (6, 30), (9, 7), (9, 12), (14, 18), (15, 28),
           (16, 16), (17, 15), (17, 33), (19, 13), (22, 10), (25, 34), (35, 2)]


def score(rows, cols, sources, res, z):
    f = flood(from_sources(rows, cols, sources), res, z)
    return f.depth, int((f.level >= f.depth - 1).sum())


def climb(rows, cols, res, z, n_sources, seed, steps, want, start=None, exact=None):
    """Returns (sources at the end, the first placement tried whose depth was exactly `exact`)."""
    rng = np.random.default_rng(seed)
    cur = set(start) if start else set()
    while len(cur) < n_sources:
        cur.add((int(rng.integers(rows)), int(rng.integers(cols))))
    best = score(rows, cols, cur, res, z)
    at_exact = None
    for _ in range(steps):
        if best[0] >= want:
            break
        nxt = set(cur)
        kind = rng.random()
        if kind < 0.7 or len(nxt) < 4:
            i, j = sorted(nxt)[int(rng.integers(len(nxt)))]
            nxt.discard((i, j))
            if rng.random() < 0.6:
                i, j = i + int(rng.integers(-2, 3)), j + int(rng.integers(-2, 3))
            else:
                i, j = int(rng.integers(rows)), int(rng.integers(cols))
            nxt.add((min(max(i, 0), rows - 1), min(max(j, 0), cols - 1)))
        elif kind < 0.85:
            nxt.add((int(rng.integers(rows)), int(rng.integers(cols))))
        else:
            nxt.discard(sorted(nxt)[int(rng.integers(len(nxt)))])
        s = score(rows, cols, nxt, res, z)
        if s[0] == exact and at_exact is None:
            at_exact = sorted(nxt)
        if s >= best:
            cur, best = nxt, s
    return sorted(cur), at_exact


def entry(rows, cols, res, z, sources):
    depth = score(rows, cols, sources, res, z)[0]
    print("%dx%d res %g z %g: radius %d, %d sources, depth %d, planned %d" %
          (rows, cols, res, z, cell_radius(res, z), len(sources), depth, planned_levels(rows, cols, res, z)))
    return {"rows": rows, "cols": cols, "res": res, "z": z, "sources": [list(map(int, p)) for p in sources]}, depth


def main():
    out = {}
    out["detour_r10_witness"], d = entry(36, 36, 0.1, 1.0, WITNESS)
    assert d == 25
    # radius 10 from a random start: the placement that first reaches the planned count exactly (the frontier is not empty at the
    # finish, but nothing more is claimed), and the one the climb ends on
    end, exact = climb(36, 36, 0.1, 1.0, 20, 3, 6000, want=22, exact=18)
    out["detour_r10_exactly_planned"], d = entry(36, 36, 0.1, 1.0, exact)
    assert d == 18
    out["detour_r10"], d = entry(36, 36, 0.1, 1.0, end)
    assert d >= 19
    # radius 20 on 64x64, planned 33
    end, _ = climb(64, 64, 0.05, 1.0, 36, 5, 12000, want=36)
    out["detour_r20"], d = entry(64, 64, 0.05, 1.0, end)
    assert d >= 34
    # z_occ_max_dis = 2.0 (the map callback's cap): radius 20 at res 0.1
    end, _ = climb(64, 64, 0.1, 2.0, 36, 6, 12000, want=36)
    out["detour_z2_r20"], d = entry(64, 64, 0.1, 2.0, end)
    assert d >= 34
    with open(os.path.join(HERE, "mapcache_detours.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
