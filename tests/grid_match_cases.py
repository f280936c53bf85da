"""Correlative scan-to-grid matching (csrc/k_gridmatch.hip): both rules restated in plain Python / numpy on the helpers
of tests/grid_cases.py, and a generated campaign on small grids (at most 61 x 47 cells, and the 1 x 257 strip).

The restatement is the definition.  The lookup plane is a maximum over integers; the match rounds every end cell with the integration's
own helpers (fp64 in statement order, C's round(), the x86 cast, correctly rounded sin / cos) and from there on sums bytes and compares
integers.  Neither has an iteration order, so the device must give the same bytes.

A case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc

MATCH_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("score", "u4"), ("n_beams", "u4"), ("di", "i4"), ("dj", "i4"),
                        ("da", "i4"), ("flags", "u4"), ("score_prior", "u4"), ("reserved", "u4")])
assert MATCH_DTYPE.itemsize == 56
ACCEPTED, SKIPPED = 1, 2
SEARCH_KEYS = ("wx", "wy", "na", "ang_step", "min_beams", "min_num", "min_den")


# ---- the lookup plane ------------------------------------------------------------------------------------------------------------------
def occupied(pass_counts, hit_counts, min_pass=2, occ_num=1, occ_den=10):
    """bool [rows, cols]: the cells the publish rule gives 100 (uint32 x uint32 products are exact in uint64)."""
    p, h = pass_counts.astype(np.uint64), hit_counts.astype(np.uint64)
    return (p >= np.uint64(min_pass)) & (h * np.uint64(occ_den) >= p * np.uint64(occ_num))


def likelihood(pass_counts, hit_counts, min_pass, occ_num, occ_den, radius, w):
    """uint8 [rows, cols]: corr[y][x] = max of w[|v|][|u|] over |u|, |v| <= radius with (x + u, y + v) inside and occupied; 0 if none."""
    assert 0 <= radius <= 7 and occ_den > 0 and occ_num <= occ_den           # (what the entry refuses is no case)
    occ = occupied(pass_counts, hit_counts, min_pass, occ_num, occ_den)
    rows, cols = occ.shape
    corr = np.zeros((rows, cols), np.uint8)
    for oy, ox in np.argwhere(occ):
        for v in range(-radius, radius + 1):
            for u in range(-radius, radius + 1):
                y, x = oy - v, ox - u                                    # (the window is symmetric: the cell that sees (ox, oy) at (u, v))
                if 0 <= y < rows and 0 <= x < cols:
                    corr[y, x] = max(int(corr[y, x]), int(w[abs(v)][abs(u)]))
    return corr


def table(radius, fn):
    """An 8 x 8 table from fn(|dv|, |du|) within the radius, 0 elsewhere."""
    w = np.zeros((8, 8), np.uint8)
    for v in range(radius + 1):
        for u in range(radius + 1):
            w[v, u] = fn(v, u)
    return w


# ---- the match -------------------------------------------------------------------------------------------------------------------------
def scored_ends(scan, n, pose, theta, resol, range_max, trace=None):
    """int64 [nb, 2] (ex, ey) of the beams scored at the angle theta, in beam order."""
    x, y, ang = (float(v) for v in pose)
    ends = []
    for j in range(n):
        r, a = float(scan[j, 0]), float(scan[j, 1])
        why = gc.beam_skip(r, a, ang)
        if why is None and not r <= range_max:
            why = "beam_over_range"
        th = a + theta / 180.0 * gc.K_PI
        if why is None and not math.isfinite(th):
            why = "beam_bad_angle"
        if why:
            if trace is not None:
                trace.append(dict(beam=j, skip=why, range=r))
            continue
        s, c = gc.cr().cr_sin(th), gc.cr().cr_cos(th)
        fx, fy = x + r * c / resol, y + r * s / resol
        ends.append((gc.cvt_x86(gc.c_round(fx)), gc.cvt_x86(gc.c_round(fy))))
        if trace is not None:
            trace.append(dict(beam=j, skip=None, range=r, raw=(fx, fy)))
    return np.array(ends, np.int64).reshape(-1, 2)


def scores(ends, corr, wx, wy):
    """(S int64 [2 wy + 1, 2 wx + 1], inside bool [nb, 2 wy + 1, 2 wx + 1]) of one angle."""
    rows, cols = corr.shape
    i = np.arange(-wx, wx + 1, dtype=np.int64)
    j = np.arange(-wy, wy + 1, dtype=np.int64)
    cx = ends[:, 0, None, None] + i[None, None, :] + 0 * j[None, :, None]
    cy = ends[:, 1, None, None] + j[None, :, None] + 0 * i[None, None, :]
    inside = (cx >= 0) & (cx < cols) & (cy >= 0) & (cy < rows)
    vals = np.where(inside, corr[np.clip(cy, 0, rows - 1), np.clip(cx, 0, cols - 1)].astype(np.int64), 0)
    return vals.sum(axis=0), inside


def match(scans, lens, poses, resol, range_max, corr, search, trace=None):
    """The records (MATCH_DTYPE) of the scans matched on the plane corr [rows, cols].  poses: float64 [n, 3] (their BITS are what a
    record copies).  search: a dict of SEARCH_KEYS.  trace: a list that receives one dict per scan."""
    wx, wy, na, step = int(search["wx"]), int(search["wy"]), int(search["na"]), float(search["ang_step"])
    nx, ny = 2 * wx + 1, 2 * wy + 1
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    out = np.zeros(len(lens), MATCH_DTYPE)
    words = out.view(np.uint64).reshape(len(lens), 7)
    for n in range(len(lens)):
        words[n, :3] = poses[n].view(np.uint64)
        why = gc.scan_skip(poses[n])
        if why:
            out[n]["flags"] = SKIPPED
            if trace is not None:
                trace.append(dict(scan=n, skip=why))
            continue
        x, y, ang = (float(v) for v in poses[n])
        best, nbs, beams, S_all, inside_all = None, {}, {}, {}, {}
        for a in range(-na, na + 1):
            theta = ang + float(a) * step
            bt = []
            ends = scored_ends(scans[n], int(lens[n]), poses[n], theta, resol, range_max, bt)
            S, inside = scores(ends, corr, wx, wy)
            nbs[a], beams[a], S_all[a], inside_all[a] = len(ends), bt, S, inside
            for jj in range(ny):
                for ii in range(nx):
                    i, j = ii - wx, jj - wy
                    key = (-int(S[jj, ii]), i * i + j * j, abs(a), ((a + na) * ny + jj) * nx + ii, a, j, i)
                    if best is None or key < best:
                        best = key
        S_win, a, j, i = -best[0], best[4], best[5], best[6]
        nb = nbs[a]
        ok = nb >= search["min_beams"] and S_win * int(search["min_den"]) >= 255 * nb * int(search["min_num"])
        r = out[n]
        r["score"], r["n_beams"], r["di"], r["dj"], r["da"] = S_win, nb, i, j, a
        r["score_prior"], r["flags"] = int(S_all[0][wy, wx]), ACCEPTED if ok else 0
        if ok:
            r["x"], r["y"], r["ang"] = x + float(i), y + float(j), ang + float(a) * step
        if trace is not None:
            trace.append(dict(scan=n, skip=None, nb=nbs, beams=beams, S=S_all, inside=inside_all, winner=(a, j, i), score=S_win, accepted=ok))
    return out


# ---- the classes -----------------------------------------------------------------------------------------------------------------------
LIKE_CLASSES = (["radius_0", "radius_1", "radius_7"] + ["edge_%s" % e for e in ("left", "right", "top", "bottom")] +
                ["corner_%s" % c for c in ("tl", "tr", "bl", "br")] +
                ["overlap_each_wins", "non_monotone", "pass_below_min", "pass_at_min", "ratio_equal", "ratio_one_below", "ratio_one_above",
                 "grid_1x1", "grid_1x257", "grid_61x47"])


def like_classes_of(case):
    got = set()
    r, w = case["radius"], case["w"].astype(int)
    if r in (0, 1, 7):
        got.add("radius_%d" % r)
    p, h = case["pass"].astype(object), case["hit"].astype(object)            # Python integers: no product overflows
    occ = occupied(case["pass"], case["hit"], case["min_pass"], case["occ_num"], case["occ_den"])
    rows, cols = occ.shape
    if r > 0:
        for name, cells in (("edge_left", occ[:, 0]), ("edge_right", occ[:, -1]), ("edge_top", occ[0]), ("edge_bottom", occ[-1]),
                            ("corner_tl", occ[0, 0]), ("corner_tr", occ[0, -1]), ("corner_bl", occ[-1, 0]), ("corner_br", occ[-1, -1])):
            if np.any(cells) and cols > 1 and rows > 1:
                got.add(name)
    if any(w[v, u + 1] > w[v, u] or w[u + 1, v] > w[u, v] for v in range(r + 1) for u in range(r)):
        got.add("non_monotone")
    num, den, mn = case["occ_num"], case["occ_den"], case["min_pass"]
    ratio_ok = h * den >= p * num
    if np.any((p == mn - 1) & ratio_ok):
        got.add("pass_below_min")
    if np.any((p == mn) & ratio_ok):
        got.add("pass_at_min")
    live = p >= mn
    if np.any(live & (h * den == p * num)):
        got.add("ratio_equal")
    if np.any(live & ((h + 1) * den == p * num)):
        got.add("ratio_one_below")
    if np.any(live & (h >= 1) & ((h - 1) * den == p * num)):
        got.add("ratio_one_above")
    cells = np.argwhere(occ)
    if 2 <= len(cells) <= 8 and r > 0:
        for a in range(len(cells)):
            for b in range(a + 1, len(cells)):
                (ay, ax), (by, bx) = cells[a], cells[b]
                a_wins = b_wins = False
                for y in range(max(0, ay - r, by - r), min(rows, ay + r + 1, by + r + 1)):
                    for x in range(max(0, ax - r, bx - r), min(cols, ax + r + 1, bx + r + 1)):
                        wa, wb = w[abs(y - ay), abs(x - ax)], w[abs(y - by), abs(x - bx)]
                        a_wins |= wa > wb
                        b_wins |= wb > wa
                if a_wins and b_wins:
                    got.add("overlap_each_wins")
    if (cols, rows) == (1, 1):
        got.add("grid_1x1")
    if (cols, rows) in ((1, 257), (257, 1)):
        got.add("grid_1x257")
    if (cols, rows) == (61, 47):
        got.add("grid_61x47")
    return got


NB_COUNTS = (0, 1, 63, 64, 65, 256, 257, 1025)
CAND_COUNTS = (1, 255, 289)
MATCH_CLASSES = (["nb_%d" % n for n in NB_COUNTS] + ["cand_%d" % n for n in CAND_COUNTS] + ["na_0", "na_1", "na_63"] +
                 ["window_over_%s" % e for e in ("left", "right", "top", "bottom")] +
                 ["beam_outside_for_some", "beam_outside_for_all", "uniform_plane", "tie_by_index", "tie_by_distance", "tie_by_angle",
                  "accept_at_equality", "accept_one_below", "accept_one_above", "beams_below_min", "beams_at_min",
                  "beam_over_range", "range_at_max_scored", "range_one_ulp_above_max", "half_way", "winner_moved", "rejected"] +
                 gc.BEAM_SKIPS + gc.SCAN_SKIPS)


def match_classes_of(case, trace):
    got = set()
    se = case["search"]
    wx, wy, na = se["wx"], se["wy"], se["na"]
    nx, ny = 2 * wx + 1, 2 * wy + 1
    rows, cols = case["corr"].shape
    if nx * ny in CAND_COUNTS:
        got.add("cand_%d" % (nx * ny))
    if na in (0, 1, 63):
        got.add("na_%d" % na)
    for t in trace:
        if t["skip"]:
            got.add(t["skip"])
            continue
        for a, nb in t["nb"].items():
            if nb in NB_COUNTS:
                got.add("nb_%d" % nb)
            for b in t["beams"][a]:
                if b["skip"]:
                    got.add(b["skip"])
                    if b["range"] == np.nextafter(case["range_max"], np.inf):
                        got.add("range_one_ulp_above_max")
                else:
                    if b["range"] == case["range_max"]:
                        got.add("range_at_max_scored")
                    if any(gc.is_half(v) for v in b["raw"]):
                        got.add("half_way")
            ins = t["inside"][a]
            if ins.shape[0]:
                per_beam = ins.reshape(ins.shape[0], -1)
                if np.any(per_beam.any(1) & ~per_beam.all(1)):
                    got.add("beam_outside_for_some")
                if np.any(~per_beam.any(1)):
                    got.add("beam_outside_for_all")
        all_S = np.stack([t["S"][a] for a in sorted(t["S"])])
        a, j, i = t["winner"]
        top = all_S.max()
        n_top = int((all_S == top).sum())
        if all_S.min() == top and all_S.size > 1 and t["nb"][0] > 0 and top > 0:
            got.add("uniform_plane")
            assert (a, j, i) == (0, 0, 0)
        if n_top > 1 and not (all_S.min() == top):
            ii, jj = np.meshgrid(np.arange(-wx, wx + 1), np.arange(-wy, wy + 1))
            d2 = np.broadcast_to(ii * ii + jj * jj, all_S.shape)
            aa = np.broadcast_to(np.abs(np.arange(-na, na + 1))[:, None, None], all_S.shape)
            m = all_S == top
            m2 = m & (d2 == d2[m].min())
            m3 = m2 & (aa == aa[m2].min())
            if m2.sum() == 1:
                got.add("tie_by_distance")
            elif m3.sum() == 1:
                got.add("tie_by_angle")
            else:
                got.add("tie_by_index")
        if (a, j, i) != (0, 0, 0):
            got.add("winner_moved")
        nb, S = t["nb"][a], t["score"]
        thr = 255 * nb * se["min_num"]
        if nb >= se["min_beams"] and nb > 0:
            if S * se["min_den"] == thr:
                got.add("accept_at_equality")
            elif S * se["min_den"] < thr <= (S + 1) * se["min_den"]:
                got.add("accept_one_below")
            elif (S - 1) * se["min_den"] <= thr < S * se["min_den"]:
                got.add("accept_one_above")
        if nb == se["min_beams"] - 1:
            got.add("beams_below_min")
            assert not t["accepted"]
        if nb == se["min_beams"] and nb > 0:
            got.add("beams_at_min")
        if not t["accepted"]:
            got.add("rejected")
    return got


def window_classes(case, trace):
    """The edges some candidate cell of a scored beam lies beyond (from the end cells the trace's inside masks were made of)."""
    got = set()
    se = case["search"]
    rows, cols = case["corr"].shape
    for n, t in enumerate(trace):
        if t["skip"]:
            continue
        ends = scored_ends(case["scans"][t["scan"]], int(case["lens"][t["scan"]]), case["poses"][t["scan"]], float(case["poses"][t["scan"]][2]),
                           case["resol"], case["range_max"])
        if len(ends) == 0:
            continue
        inside_now = (ends[:, 0] >= 0) & (ends[:, 0] < cols) & (ends[:, 1] >= 0) & (ends[:, 1] < rows)
        e = ends[inside_now]
        if len(e) == 0:
            continue
        if (e[:, 0] - se["wx"] < 0).any():
            got.add("window_over_left")
        if (e[:, 0] + se["wx"] >= cols).any():
            got.add("window_over_right")
        if (e[:, 1] - se["wy"] < 0).any():
            got.add("window_over_top")
        if (e[:, 1] + se["wy"] >= rows).any():
            got.add("window_over_bottom")
    return got


# ---- the campaigns ---------------------------------------------------------------------------------------------------------------------
GAUSS = table(3, lambda v, u: [255, 155, 35, 3][max(v, u)] if (v == 0 or u == 0) else [0, 94, 21, 2][max(v, u)] if v == u else 9)
CONE7 = table(7, lambda v, u: max(0, 250 - 30 * max(v, u) - 3 * min(v, u)))
BUMPY = table(3, lambda v, u: [[10, 200, 30, 90], [200, 5, 250, 1], [30, 250, 0, 77], [90, 1, 77, 255]][v][u])       # not monotone
BUMPY7 = table(7, lambda v, u: (37 * v + 91 * u + 13 * v * u) % 256)


def like_case(name, cols, rows, cells, radius, w, min_pass=2, occ=(1, 10), fill=None):
    """cells: (x, y, pass, hit) of the cells that are not (0, 0) -- or not `fill`."""
    pa = np.zeros((rows, cols), np.uint32)
    hi = np.zeros((rows, cols), np.uint32)
    if fill is not None:
        pa[:], hi[:] = fill
    for x, y, p, h in cells:
        pa[y, x], hi[y, x] = p, h
    return dict(name=name, cols=cols, rows=rows, min_pass=min_pass, occ_num=occ[0], occ_den=occ[1], radius=radius, w=w.copy())|{"pass": pa, "hit": hi}


def like_campaign():
    cases = []
    rng = np.random.default_rng(20250711)
    for v in range(3):
        cols, rows = 61 - 7 * v, 47 - 5 * v
        # every edge and every corner, at radius 1, 3 and 7
        rim = [(0, 0, 5, 5), (cols - 1, 0, 5, 5), (0, rows - 1, 5, 5), (cols - 1, rows - 1, 5, 5), (cols // 2, 0, 9, 1), (cols // 2, rows - 1, 9, 1),
               (0, rows // 2, 3, 3), (cols - 1, rows // 2 + v, 3, 3)]
        cases.append(like_case("rim_r1_%d" % v, cols, rows, rim, 1, table(1, lambda a, b: 255 - 100 * a - 50 * b)))
        cases.append(like_case("rim_r3_%d" % v, cols, rows, rim, 3, GAUSS))
        cases.append(like_case("rim_r7_%d" % v, cols, rows, rim, 7, CONE7))
        cases.append(like_case("rim_r0_%d" % v, cols, rows, rim, 0, table(0, lambda a, b: 255 - v)))
        # two cells whose windows overlap: each wins its own side; and a table that is not monotone
        pair = [(20 + v, 20, 4, 4), (23 + v, 21 + v, 4, 2)]
        cases.append(like_case("pair_%d" % v, cols, rows, pair, 3, GAUSS))
        cases.append(like_case("pair_bumpy_%d" % v, cols, rows, pair + [(5, 5 + v, 2, 2)], 3, BUMPY))
        cases.append(like_case("bumpy7_%d" % v, cols, rows, pair + [(cols - 2, 3, 2, 2)], 7, BUMPY7))
        # the occupancy rule at its thresholds: pass = min_pass - 1 / min_pass; hit * den == pass * num and one either side
        mn, num, den = ((2, 1, 10), (5, 1, 3), (3, 3, 4))[v]
        p_eq = den * 2                                                          # hit = 2 num makes the ratio exact
        rule = [(3, 3, mn - 1, mn - 1), (9, 3, mn, mn), (15, 3, p_eq, 2 * num), (21, 3, p_eq, 2 * num - 1), (27, 3, p_eq, 2 * num + 1),
                (33, 3, 0xFFFFFFFF, 0xFFFFFFFF), (39, 3, 1 << 31, (1 << 31) // den * num)]
        cases.append(like_case("rule_%d" % v, cols, rows, rule, 1 + v, GAUSS if v else table(1, lambda a, b: 200 - 60 * (a + b)), min_pass=mn,
                               occ=(num, den)))
        # the smallest grid, the strip, the largest grid with random counters
        cases.append(like_case("one_cell_%d" % v, 1, 1, [(0, 0, 2 + v, 1 if v < 2 else 0)], (0, 1, 7)[v], CONE7))
        strip = [(0, y, 3, 3) for y in (0, 100 + v, 256)]
        cases.append(like_case("strip_%d" % v, 1, 257, strip, (1, 3, 7)[v], CONE7))
        cases.append(like_case("strip_wide_%d" % v, 257, 1, [(y, 0, p, h) for _, y, p, h in strip] + [(31 + v, 0, 2, 2), (32 + v, 0, 2, 2)], (7, 3, 1)[v], BUMPY7))
        pa = rng.integers(0, 12, (47, 61)).astype(np.uint32)
        hi = np.minimum(rng.integers(0, 30, (47, 61)) // 9, pa).astype(np.uint32)
        big = like_case("random_%d" % v, 61, 47, [], (2, 5, 7)[v], (GAUSS, BUMPY7, CONE7)[v])
        big["pass"], big["hit"] = pa, hi
        cases.append(big)
    return cases


def search(wx, wy, na=0, ang_step=0.0, min_beams=1, min_num=1, min_den=4):
    return dict(wx=wx, wy=wy, na=na, ang_step=float(ang_step), min_beams=min_beams, min_num=min_num, min_den=min_den)


def match_case(name, corr, resol, range_max, beams, poses, se, stride=None, capacity=1024):
    base = gc.make_case(name, min(corr.shape[1], gc.MAX_COLS), min(corr.shape[0], gc.MAX_ROWS), resol, range_max, beams, poses, stride, capacity)
    base.update(cols=corr.shape[1], rows=corr.shape[0], corr=np.ascontiguousarray(corr, np.uint8), search=se)
    return base


def random_plane(rng, cols, rows, density=0.25):
    corr = rng.integers(1, 256, (rows, cols)).astype(np.uint8)
    corr[rng.random((rows, cols)) > density] = 0
    return corr


def beams_at_cells(pose, cells, resol, nudge=0.0):
    """Beams (range, angle) from `pose` (ang = 0) whose end points are the centres of the cells (x, y), moved by `nudge` of a cell."""
    out = []
    for cx, cy in cells:
        dx, dy = (cx + nudge - pose[0]) * resol, (cy + nudge - pose[1]) * resol
        out.append((math.hypot(dx, dy), math.atan2(dy, dx)))
    return out


def match_campaign():
    cases = []
    rng = np.random.default_rng(20250712)
    # scored-beam counts around the wavefront, the workgroup and beyond the short capacity; candidate counts 1, 255, 289; na 0, 1
    for n in NB_COUNTS:
        for v in range(3 if n != 1025 else 1):
            cols, rows = 61 - 3 * v, 47 - 2 * v
            corr = random_plane(rng, cols, rows)
            scored = np.stack([rng.uniform(0.05, 1.2, n), rng.uniform(-math.pi, math.pi, n)], 1)
            extra = np.array([(math.nan, 0.1), (-0.5, 0.2), (5.0, 0.3)])             # never scored: NaN, non-positive, beyond range_max
            b = np.concatenate([scored, extra])
            b = b[rng.permutation(len(b))]
            se = (search(0, 0, 1, 0.75), search(7, 8, 0), search(8, 8, 1, 1.5))[v] if n != 1025 else search(2, 1, 1, 0.5)
            cases.append(match_case("nb%d_%d" % (n, v), corr, 0.05, 1.5, [b, b[: max(1, len(b) // 2)]],
                                    [(rng.uniform(22, 38), rng.uniform(18, 28), rng.uniform(-180, 180)), (30.0, 20.0, 0.0)], se,
                                    stride=len(b) + 5 * v, capacity=1024 if len(b) <= 1024 else 2048))
    # na = 63 on few beams
    for v in range(3):
        corr = random_plane(rng, 40 + v, 31, 0.5)
        b = np.stack([rng.uniform(0.2, 0.9, 6 + v), rng.uniform(-math.pi, math.pi, 6 + v)], 1)
        cases.append(match_case("na63_%d" % v, corr, 0.05, 1.0, [b], [(20.0 + v, 15.5, 30.0 * v)], search(1, v, 63, 0.7 + 0.1 * v)))
    # windows over every edge; end cells outside for some candidates and for all of them
    for v in range(3):
        corr = random_plane(rng, 33 + v, 29, 0.6)
        fan = [(0.45 + 0.02 * k, k * 2 * math.pi / 16) for k in range(16)]
        far = [(1.45, 0.1 * k) for k in range(4)]                                  # 29 cells away: outside for every candidate
        cases.append(match_case("edges_%d" % v, corr, 0.05, 1.5, [fan + far, fan, fan, fan, fan],
                                [(16.0, 14.0, 0.0), (6.0 + v, 14.0, 0.0), (27.0 + v, 14.0, 0.0), (16.0, 5.0 + v, 0.0), (16.0, 23.0 - v, 0.0)],
                                search(5, 6, 1, 2.0)))
    # a uniform plane returns the zero offset; a mirror-symmetric plane where the linear index decides; ties by distance and by |a|
    for v in range(3):
        fan = [(0.3 + 0.01 * k, k * 2 * math.pi / 12 + 0.05) for k in range(12)]
        cases.append(match_case("uniform_%d" % v, np.full((31, 41), 17 + 100 * v, np.uint8), 0.05, 1.0, [fan], [(20.0, 15.0, 10.0 * v)],
                                search(3, 2 + v, v, 1.0)))
        # one beam along +x ending at cell (24, 15); the plane has two equal peaks at (22, 15) and (26, 15): i = -2 and i = +2 tie in
        # S, in i^2 + j^2 and in |a|, the smaller linear index (i = -2) wins
        one = beams_at_cells((20.0, 15.0), [(24, 15)], 0.05)
        corr = np.zeros((31, 41), np.uint8)
        corr[15, 22] = corr[15, 26] = 200 + v
        cases.append(match_case("mirror_%d" % v, corr, 0.05, 1.0, [one], [(20.0, 15.0, 0.0)], search(3, 1 + v, 0)))
        # equal peaks at distances 1 and 3: the nearer one wins although its linear index is larger
        corr = np.zeros((31, 41), np.uint8)
        corr[15, 21] = corr[15, 25 + (v > 1)] = 90 + v
        corr[15 + v, 25] = 90 + v
        cases.append(match_case("nearer_%d" % v, corr, 0.05, 1.0, [one], [(20.0, 15.0, 0.0)], search(3, 2, 0)))
        # a beam of 4 cells turned by +-14.5 degrees ends one cell up or down: with a column of equal values the angles a = -1, 0, +1 tie
        # at the zero translation, and |a| = 0 wins; with the middle cell empty a = -1 and a = +1 tie and the index (a = -1) decides
        corr = np.zeros((31, 41), np.uint8)
        corr[14:17, 24] = 150 + v
        cases.append(match_case("angle_tie_%d" % v, corr, 0.05, 1.0, [one], [(20.0, 15.0, 0.0)], search(0, 0, 1, 14.5)))
        corr = corr.copy()
        corr[15, 24] = 0
        cases.append(match_case("angle_mirror_%d" % v, corr, 0.05, 1.0, [one], [(20.0, 15.0, 0.0)], search(0, 0, 1, 14.5)))
    # acceptance at equality and one either side (one beam: S is one byte; 255 * 1 * num <= S * 255 iff S >= num), min_beams - 1 / min_beams
    for v in range(3):
        one = beams_at_cells((20.0, 15.0), [(24, 15)], 0.05)
        for d in (-1, 0, 1):
            corr = np.zeros((31, 41), np.uint8)
            corr[15, 24] = 100 + v + d
            cases.append(match_case("accept%+d_%d" % (d, v), corr, 0.05, 1.0, [one], [(20.0, 15.0, 0.0)], search(1, 1, 0, min_num=100 + v, min_den=255)))
        three = beams_at_cells((20.0, 15.0), [(24, 15), (20, 19), (16, 15)], 0.05)
        corr = np.full((31, 41), 255, np.uint8)
        cases.append(match_case("min_beams_%d" % v, corr, 0.05, 1.0, [three, three[:2]], [(20.0, 15.0, 0.0)] * 2, search(1, 1, v, 1.0, min_beams=3)))
    # readings and poses that are skipped (the integration's lists), the cut at range_max
    for v in range(3):
        corr = random_plane(rng, 47, 41, 0.5)
        good = (0.6 + 0.1 * v, 0.5)
        b = [good, (math.nan, 0.1), (0.0, 0.2), (-0.7, 0.3), (-math.inf, 0.4), (math.inf, 0.5), (0.6, math.nan), (0.6, math.inf),
             (0.6, -math.inf), (-0.0, 0.0), good]
        cases.append(match_case("skipped_beams_%d" % v, corr, 0.05, 2.0, [b], [(20.0 + v, 19.0, 5.0 * v)], search(2, 2, 1, 1.0)))
        poses = [(math.nan, 10, 0), (10, math.inf, 0), (10, 10, math.nan), (10, 10, -math.inf), (-1.0, 12, 0), (-1.00005, 12, 3),
                 (-0.99995, 12, 3), (1048577.0, 3, 0), (5, -1048576.5, 0), (-0.9998, 12.0, 0.0), (21.0 + v, 17.0, 0.0)]
        cases.append(match_case("skipped_scans_%d" % v, corr, 0.05, 2.0, [[good, (0.9, 2.0 + v)]] * len(poses), poses, search(1, 2, 1, 2.0)))
        rmax = (1.0, 0.73, 1.9)[v]
        up = float(np.nextafter(rmax, np.inf))
        b = [(rmax, 0.3 + v), (up, 0.3 + v), (rmax, 2.0 + v), (up, -1.0 - v), (3 * rmax, 1.1), (0.5 * rmax, 1.1)]
        cases.append(match_case("range_max_%d" % v, random_plane(rng, 61, 47, 0.7), 0.05, rmax, [b], [(30.4, 22.7, 12.0 * v)], search(2, 2, 1, 3.0)))
        # half-way coordinates: c = 1 exactly at th = 0 and rr / mapResol = 4.5 at a resolution of 0.5
        b = [(2.25, 0.0), (1.0, math.pi / 2), (2.0, 0.0)]
        poses = [(10.0 + 2 * v, 8.0, 0.0), (12.5 + 2 * v, 6.5, 0.0), (2.5, 3.0 + v, 0.0)]
        cases.append(match_case("half_way_%d" % v, random_plane(rng, 40, 30, 0.8), 0.5, 8.0, [b] * 3, poses, search(2, 2, 0)))
    return cases


def run_match_case(case, corr=None):
    trace = []
    rec = match(case["scans"], case["lens"], case["poses"], case["resol"], case["range_max"], case["corr"] if corr is None else corr,
                case["search"], trace)
    return rec, trace


# ---- recovery --------------------------------------------------------------------------------------------------------------------------
ROOM = dict(cols=61, rows=47, resol=0.05, range_max=4.0, x0=8, y0=6, x1=52, y1=40)      # the walls' cell lines
RECOVERY_OFFSETS = [(2, -1, 1), (-3, 2, -2), (0, 3, 0), (1, 1, 2), (-2, -2, -1)]         # (cells in x, cells in y, angle steps) added to the truth
RECOVERY_SEARCH = search(3, 3, 2, 2.0, min_beams=30, min_num=1, min_den=2)


def room_scan(pose, n_beams=90):
    """A scan of the rectangular room from `pose` (x, y in cells, ang in degrees): ranges in metres to the walls' cell centres."""
    x, y, ang = pose
    out = []
    for k in range(n_beams):
        a = -math.pi + 2 * math.pi * (k + 0.5) / n_beams
        th = a + math.radians(ang)
        c, s = math.cos(th), math.sin(th)
        ts = []
        if c > 0: ts.append((ROOM["x1"] - x) / c)
        if c < 0: ts.append((ROOM["x0"] - x) / c)
        if s > 0: ts.append((ROOM["y1"] - y) / s)
        if s < 0: ts.append((ROOM["y0"] - y) / s)
        out.append((min(t for t in ts if t > 0) * ROOM["resol"], a))
    return np.array(out)


def recovery():
    """(corr, scans, lens, true poses, displaced poses): a room integrated twice at the true poses, smeared by GAUSS."""
    truth = np.array([(30.25, 22.5, 10.0), (24.5, 27.25, -35.0), (36.75, 18.5, 80.0)])
    scans = np.stack([room_scan(p) for p in truth])
    lens = np.full(len(truth), scans.shape[1], np.int32)
    pa = np.zeros((ROOM["rows"], ROOM["cols"]), np.uint32)
    hi = np.zeros_like(pa)
    for _ in range(2):
        gc.integrate(scans, lens, truth, ROOM["cols"], ROOM["rows"], ROOM["resol"], ROOM["range_max"], pa, hi)
    corr = likelihood(pa, hi, 2, 1, 10, 3, GAUSS)
    return corr, scans, lens, truth
