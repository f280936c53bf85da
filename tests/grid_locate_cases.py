"""Global scan-to-grid localisation (csrc/k_gridlocate.hip): the rule restated in plain Python / numpy on the helpers of
tests/grid_cases.py and tests/grid_match_cases.py, and a generated campaign on small grids (at most 61 x 47 cells, and the 1 x 257 strip).

The restatement is the definition.  The beam offsets are the match's end cells at the pose (0, 0, theta_a) (fp64 in statement order, C's
round(), the x86 cast, correctly rounded sin / cos); everything behind them is integer sums and comparisons with no iteration order, so the
device must give the same bytes.  The restatement scores EVERY node of every level densely and states the frontier as masks over those
arrays: what the device never visits is still defined here.

A case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import functools
import math

import numpy as np

import grid_cases as gc
import grid_match_cases as gm

LOCATE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("score", "u4"), ("n_beams", "u4"), ("cx", "i4"), ("cy", "i4"), ("a", "i4"),
                         ("flags", "u4"), ("n_best", "u4"), ("lower_bound", "u4"), ("reserved", "u4", (2,))])
STATS_DTYPE = np.dtype([("top_nodes", "u4"), ("frontier", "u4", (9,)), ("scored", "u4"), ("reserved", "u4")])
assert LOCATE_DTYPE.itemsize == 64 and STATS_DTYPE.itemsize == 48
ACCEPTED, REJECTED, NOT_FOUND, OVERFLOW, EMPTY = 1, 2, 4, 8, 16
PAR_KEYS = ("x0", "y0", "nx", "ny", "ang0", "ang_step", "n_ang", "levels", "max_nodes", "score_floor", "min_beams", "min_num", "min_den")
LOWER_BOUND_BYTES = slice(52, 56)                                   # the record's only field that depends on `levels`


def par(x0, y0, nx, ny, ang0=0.0, ang_step=0.0, n_ang=1, levels=4, max_nodes=1 << 16, score_floor=0, min_beams=1, min_num=1, min_den=4):
    return dict(x0=x0, y0=y0, nx=nx, ny=ny, ang0=float(ang0), ang_step=float(ang_step), n_ang=n_ang, levels=levels, max_nodes=max_nodes,
                score_floor=score_floor, min_beams=min_beams, min_num=min_num, min_den=min_den)


# ---- the pyramid -----------------------------------------------------------------------------------------------------------------------
def plane(corr, h):
    """uint8 [rows + 2^h - 1, cols + 2^h - 1]: plane[y + 2^h - 1][x + 2^h - 1] = the maximum of corr over [x, x + 2^h) x [y, y + 2^h) inside
    the grid, 0 if none.  From the definition (a maximum has no order: rows first, then columns), not level from level."""
    b = 1 << h
    m = b - 1
    rows, cols = corr.shape
    pad = np.zeros((rows + 2 * m, cols + 2 * m), np.uint8)
    pad[m:m + rows, m:m + cols] = corr
    row_max = np.zeros((rows + 2 * m, cols + m), np.uint8)
    for u in range(b):
        np.maximum(row_max, pad[:, u:u + cols + m], out=row_max)
    out = np.zeros((rows + m, cols + m), np.uint8)
    for v in range(b):
        np.maximum(out, row_max[v:v + rows + m], out=out)
    return out


def pyramid_offset(cols, rows, h):
    return sum((cols + (1 << l) - 1) * (rows + (1 << l) - 1) for l in range(h))


def pyramid(corr, levels):
    """The buffer lsd_enqueue_grid_pyramid_device writes: the planes 0..levels one behind the other."""
    return np.concatenate([plane(corr, h).reshape(-1) for h in range(levels + 1)])


# ---- the search ------------------------------------------------------------------------------------------------------------------------
def offsets(scan, n, theta, resol, range_max, trace=None):
    """int64 [nb, 2] (ox, oy) of the beams scored at the heading theta: the match's end cells at the pose (0, 0, theta)."""
    return gm.scored_ends(scan, n, (0.0, 0.0, theta), theta, resol, range_max, trace)


def node_sums(pl, h, offs, x0, y0, nbx, nby):
    """int64 [nby, nbx]: U_h of every node (Q, P) of one heading, pl = plane(corr, h)."""
    m = (1 << h) - 1
    pr, pc = pl.shape
    if len(offs) == 0:
        return np.zeros((nby, nbx), np.int64)
    xs = x0 + m + offs[:, 0, None] + (np.arange(nbx, dtype=np.int64) << h)[None, :]         # [nb, nbx] plane columns
    ys = y0 + m + offs[:, 1, None] + (np.arange(nby, dtype=np.int64) << h)[None, :]
    okx, oky = (xs >= 0) & (xs < pc), (ys >= 0) & (ys < pr)
    vals = pl[np.clip(ys, 0, pr - 1)[:, :, None], np.clip(xs, 0, pc - 1)[:, None, :]].astype(np.int64)
    return (vals * (oky[:, :, None] & okx[:, None, :])).sum(axis=0)


def locate(scans, lens, resol, range_max, corr, p, ge=True, trace=None):
    """(records LOCATE_DTYPE [n], statistics STATS_DTYPE [n]) of the scans located on the plane corr [rows, cols] with the parameters p (a
    dict of PAR_KEYS).  ge=False: the frontier test as `>` -- NOT the rule; one test shows the difference.  trace: a list that receives
    one dict per scan."""
    H, nx, ny, n_ang, x0, y0 = p["levels"], p["nx"], p["ny"], p["n_ang"], p["x0"], p["y0"]
    planes = [plane(corr, h) for h in range(H + 1)]
    dims = [((nx + (1 << h) - 1) >> h, (ny + (1 << h) - 1) >> h) for h in range(H + 1)]   # (nbx, nby) per level
    out = np.zeros(len(lens), LOCATE_DTYPE)
    stats = np.zeros(len(lens), STATS_DTYPE)
    out["x"], out["y"] = -1.0, -1.0
    for n in range(len(lens)):
        thetas = [p["ang0"] + float(a) * p["ang_step"] for a in range(n_ang)]
        beams = [[] for _ in range(n_ang)]
        offs = [offsets(scans[n], int(lens[n]), thetas[a], resol, range_max, beams[a]) for a in range(n_ang)]
        nb = [len(o) for o in offs]
        t = dict(scan=n, nb=nb, beams=beams, flags=EMPTY, frontier={}, n_best=0)
        if trace is not None:
            trace.append(t)
        if not any(nb):
            out[n]["flags"] = EMPTY
            continue
        # U of every node of every level: [n_ang, nby, nbx]
        U = [np.stack([node_sums(planes[h], h, offs[a], x0, y0, *dims[h]) for a in range(n_ang)]) for h in range(H + 1)]
        for h in range(H):                                          # beam by beam a node bounds its children
            up = np.repeat(np.repeat(U[h + 1], 2, axis=1), 2, axis=2)[:, :dims[h][1], :dims[h][0]]
            assert (up >= U[h]).all()
        # the lower bound: the greedy descent of every heading
        la = []
        for a in range(n_ang):
            Q, P = divmod(int(np.argmax(U[H][a])), dims[H][0])      # the first maximum in the order Q nbx + P
            for h in range(H, 0, -1):
                kids = [(int(U[h - 1][a, 2 * Q + dq, 2 * P + dp]), -dq, -dp) for dq in (0, 1) for dp in (0, 1)
                        if 2 * Q + dq < dims[h - 1][1] and 2 * P + dp < dims[h - 1][0]]
                _, dq, dp = max(kids)                               # the largest U, among equals the smallest (Q, P)
                Q, P = 2 * Q - dq, 2 * P - dp
            la.append(int(U[0][a, Q, P]))
        L = max(max(la), p["score_floor"])
        keep = (lambda u: u >= L) if ge else (lambda u: u > L)
        st = stats[n]
        st["top_nodes"] = n_ang * dims[H][0] * dims[H][1]
        scored = int(st["top_nodes"])
        F = keep(U[H])
        overflow = False
        for h in range(H, 0, -1):
            st["frontier"][h] = t["frontier"][h] = int(F.sum())
            if F.sum() > p["max_nodes"]:
                overflow = True
                break
            kids = np.repeat(np.repeat(F, 2, axis=1), 2, axis=2)[:, :dims[h - 1][1], :dims[h - 1][0]]      # the existing children of F_h
            scored += int(kids.sum())
            F = kids & keep(U[h - 1])
        st["scored"] = scored
        r = out[n]
        r["lower_bound"] = L
        t.update(L=L, la=la, S=U[0])
        if overflow:
            r["flags"] = t["flags"] = OVERFLOW
            continue
        st["frontier"][0] = t["frontier"][0] = int(F.sum())
        if not F.any():
            r["flags"] = t["flags"] = NOT_FOUND
            continue
        S = np.where(F, U[0], -1)
        lin = int(np.argmax(S))                                     # the largest S, then the smallest lin
        a, rem = divmod(lin, ny * nx)
        q, pp = divmod(rem, nx)
        S_win = int(S.reshape(-1)[lin])
        ok = nb[a] >= p["min_beams"] and S_win * p["min_den"] >= 255 * nb[a] * p["min_num"]
        r["score"], r["n_beams"], r["cx"], r["cy"], r["a"], r["n_best"] = S_win, nb[a], x0 + pp, y0 + q, a, int((S == S_win).sum())
        r["flags"] = ACCEPTED if ok else REJECTED
        if ok:
            r["x"], r["y"], r["ang"] = float(x0 + pp), float(y0 + q), thetas[a]
        t.update(flags=int(r["flags"]), winner=(a, q, pp), score=S_win, n_best=int(r["n_best"]), n_beams=nb[a])
    return out, stats


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
def case(name, corr, resol, range_max, beams, p, stride=None, capacity=1024):
    base = gc.make_case(name, min(corr.shape[1], gc.MAX_COLS), min(corr.shape[0], gc.MAX_ROWS), resol, range_max, beams, [(0, 0, 0)] * len(beams),
                        stride, capacity)
    base.update(cols=corr.shape[1], rows=corr.shape[0], corr=np.ascontiguousarray(corr, np.uint8), par=p)
    del base["poses"]
    return base


def whole(corr, **kw):
    """The parameters whose box is the whole grid."""
    return par(0, 0, corr.shape[1], corr.shape[0], **kw)


def run_case(c, levels=None, ge=True):
    """(records, statistics, trace) of a case, at its own levels or at the given ones."""
    trace = []
    p = c["par"] if levels is None else dict(c["par"], levels=levels)
    rec, st = locate(c["scans"], c["lens"], c["resol"], c["range_max"], c["corr"], p, ge, trace)
    return rec, st, trace


def random_beams(rng, n, extras=True):
    scored = np.stack([rng.uniform(0.05, 1.2, n), rng.uniform(-math.pi, math.pi, n)], 1).reshape(-1, 2)
    if not extras:
        return scored
    b = np.concatenate([scored, np.array([(math.nan, 0.1), (-0.5, 0.2), (5.0, 0.3)])])       # never scored: NaN, non-positive, over range_max
    return b[rng.permutation(len(b))]


def one_beam(ox, oy, resol=0.05):
    """A beam whose offset at the heading 0 is (ox, oy) cells."""
    return gm.beams_at_cells((0.0, 0.0), [(ox, oy)], resol)


def largest_frontier(c):
    """The largest |F_h|, h >= 1, of the case's first scan when nothing overflows."""
    _, st, _ = run_case(dict(c, par=dict(c["par"], max_nodes=1 << 24)))
    return int(st[0]["frontier"][1:].max())


@functools.lru_cache(maxsize=None)
def campaign():
    """The cases, deterministic."""
    cases = []
    rng = np.random.default_rng(20250919)
    # scored-beam counts around the wavefront, the workgroup and beyond the short capacity
    for n in gm.NB_COUNTS:
        for v in range(3 if n != 1025 else 1):
            corr = gm.random_plane(rng, 61 - 3 * v, 47 - 2 * v)
            b = random_beams(rng, n)
            p = whole(corr, ang0=-30.0 * v, ang_step=41.5, n_ang=(1, 2, 3)[v] if n != 1025 else 2, levels=(1, 4, 5)[v])
            cases.append(case("nb%d_%d" % (n, v), corr, 0.05, 1.5, [b, b[: max(1, len(b) // 2)]], p, stride=len(b) + 5 * v,
                              capacity=1024 if len(b) <= 1024 else 2048))
    # the levels, with 1, 2 and 65 headings; 2^8 exceeds every box: one top node
    for H in (0, 1, 4, 5, 8):
        for v in range(3):
            corr = gm.random_plane(rng, 61, 47 - v, 0.3)
            p = whole(corr, ang0=10.0 * v, ang_step=5.5, n_ang=(1, 2, 65)[v], levels=H)
            cases.append(case("levels%d_%d" % (H, v), corr, 0.05, 1.5, [random_beams(rng, (40, 17, 9)[v])], p))
    # box sizes 1, 2^H - 1, 2^H and 2^H + 1 (an overhanging last node)
    for v, H in enumerate((1, 3, 4)):
        sizes = (1, (1 << H) - 1, 1 << H, (1 << H) + 1)
        corr = gm.random_plane(rng, 61, 47, 0.5)
        for k, nx in enumerate(sizes):
            p = par(20 + v, 12 - v, nx, sizes[(k + 1 + v) % 4], ang_step=90.0, n_ang=2, levels=H)
            cases.append(case("box%d_%d" % (nx, v), corr, 0.05, 1.5, [random_beams(rng, 12 + v)], p))
    # boxes at a negative x0, partly outside and wholly outside the grid
    for v in range(3):
        corr = gm.random_plane(rng, 40 + v, 31, 0.5)
        b = [random_beams(rng, 20)]
        cases.append(case("box_negative_%d" % v, corr, 0.05, 1.5, b, par(-9 - v, -3, 30, 20 + v, levels=3)))
        cases.append(case("box_high_%d" % v, corr, 0.05, 1.5, b, par(25, 20 + v, 40, 33, ang_step=7.0, n_ang=2, levels=2 + v)))
        cases.append(case("box_outside_%d" % v, corr, 0.05, 1.5, b, par(200 + v, -150, 9 + v, 8, levels=2)))
    # the smallest grid and the strip
    for v in range(3):
        cases.append(case("one_cell_%d" % v, np.array([[200 + v]], np.uint8), 0.05, 1.5, [one_beam(0, 0) + one_beam(1, 0)],
                          par(-2, -2, 5, 5, levels=(0, 1, 2)[v])))
        strip = gm.random_plane(rng, 1, 257, 0.4)
        b = [(0.05 * k, math.pi / 2) for k in (1, 3, 4 + v, 9, 20)]
        cases.append(case("strip_%d" % v, strip, 0.05, 1.5, [b], par(0, 0, 1, 257, levels=(4, 5, 8)[v])))
    # max_nodes at the largest |F_h| and one below it
    for v in range(3):
        corr = gm.random_plane(rng, 61, 47, 0.6)
        c = case("max_nodes_at_%d" % v, corr, 0.05, 1.5, [random_beams(rng, 6 + v)], whole(corr, ang_step=3.0, n_ang=2, levels=3 + v))
        m = largest_frontier(c)
        assert m >= 2
        c["par"]["max_nodes"] = m
        cases.append(c)
        cases.append(dict(c, name="max_nodes_below_%d" % v, par=dict(c["par"], max_nodes=m - 1)))
    # ties: mirror-symmetric planes where lin decides (n_best 2 and 4), and a uniform plane in a small box (all tie, lin = 0 wins)
    for v in range(3):
        corr = np.zeros((31, 41), np.uint8)
        corr[15, 12] = corr[15, 28] = 200 + v
        cases.append(case("mirror2_%d" % v, corr, 0.05, 1.0, [one_beam(4, 0)], whole(corr, levels=2 + v)))
        corr = corr.copy()
        corr[9 - v, 12] = corr[9 - v, 28] = 200 + v
        cases.append(case("mirror4_%d" % v, corr, 0.05, 1.0, [one_beam(4, 0)], whole(corr, levels=2 + v)))
        cases.append(case("uniform_%d" % v, np.full((31, 41), 17 + 100 * v, np.uint8), 0.05, 1.0, [random_beams(rng, 5, False) * (0.2, 1.0)],
                          par(10, 10, 6 + v, 5, ang_step=10.0, n_ang=2, levels=2)))
    # score_floor at S_win and one above it
    for v in range(3):
        corr = gm.random_plane(rng, 50, 40, 0.5)
        c = case("floor_at_%d" % v, corr, 0.05, 1.5, [random_beams(rng, 15 + v)], whole(corr, levels=3))
        s_win = int(run_case(c)[0][0]["score"])
        c["par"]["score_floor"] = s_win
        cases.append(c)
        cases.append(dict(c, name="floor_above_%d" % v, par=dict(c["par"], score_floor=s_win + 1)))
    # acceptance at equality and one either side (one beam: S is one byte); n_beams at min_beams - 1 and min_beams
    for v in range(3):
        for d in (-1, 0, 1):
            corr = np.zeros((31, 41), np.uint8)
            corr[15, 24] = 100 + v + d
            cases.append(case("accept%+d_%d" % (d, v), corr, 0.05, 1.0, [one_beam(4, 0)], whole(corr, levels=3, min_num=100 + v, min_den=255)))
        three = gm.beams_at_cells((0.0, 0.0), [(4, 0), (0, 4), (-4, 0)], 0.05)
        cases.append(case("min_beams_%d" % v, np.full((31, 41), 255, np.uint8), 0.05, 1.0, [three, three[:2]],
                          par(12, 12, 4, 4 + v, levels=1, min_beams=3)))
    # readings that are skipped (the integration's list), the cut at range_max
    for v in range(3):
        corr = gm.random_plane(rng, 47, 41, 0.5)
        good = (0.6 + 0.1 * v, 0.5)
        b = [good, (math.nan, 0.1), (0.0, 0.2), (-0.7, 0.3), (-math.inf, 0.4), (math.inf, 0.5), (0.6, math.nan), (0.6, math.inf),
             (0.6, -math.inf), (-0.0, 0.0), good]
        cases.append(case("skipped_beams_%d" % v, corr, 0.05, 2.0, [b], whole(corr, ang0=5.0 * v, ang_step=1.0, n_ang=2, levels=2)))
        rmax = (1.0, 0.73, 1.9)[v]
        up = float(np.nextafter(rmax, np.inf))
        b = [(rmax, 0.3 + v), (up, 0.3 + v), (rmax, 2.0 + v), (up, -1.0 - v), (3 * rmax, 1.1), (0.5 * rmax, 1.1)]
        cases.append(case("range_max_%d" % v, gm.random_plane(rng, 61, 47, 0.7), 0.05, rmax, [b], par(3, 2, 50, 40, ang0=12.0 * v, levels=4)))
    # three scans with an empty one in the middle
    for v in range(3):
        corr = gm.random_plane(rng, 45, 38 + v, 0.4)
        cases.append(case("empty_middle_%d" % v, corr, 0.05, 1.5, [random_beams(rng, 30), [], random_beams(rng, 11)],
                          whole(corr, ang_step=120.0, n_ang=3, levels=3), stride=40))
    return cases


# ---- the classes -----------------------------------------------------------------------------------------------------------------------
CLASSES = (["levels_%d" % h for h in (0, 1, 4, 5, 8)] + ["one_top_node"] + ["box_1", "box_pow_minus_1", "box_pow", "box_pow_plus_1"] +
           ["box_negative_x0", "box_partly_outside", "box_wholly_outside", "grid_1x1", "grid_1x257", "grid_61x47"] +
           ["n_ang_%d" % n for n in (1, 2, 65)] + ["nb_%d" % n for n in gm.NB_COUNTS] +
           ["max_nodes_at_largest", "overflow", "n_best_2", "n_best_4", "all_tie_lin_0", "floor_at_win", "floor_above_win", "not_found",
            "accept_at_equality", "accept_one_below", "accept_one_above", "beams_below_min", "beams_at_min", "rejected", "empty",
            "empty_scan_in_the_middle", "beam_over_range", "range_at_max_scored", "range_one_ulp_above_max"] + gc.BEAM_SKIPS)
ONCE = {"nb_1025"}                                                  # a raised scan capacity: one case


def classes_of(c, rec, st, trace):
    got = set()
    p = c["par"]
    H, nx, ny = p["levels"], p["nx"], p["ny"]
    rows, cols = c["corr"].shape
    if H in (0, 1, 4, 5, 8):
        got.add("levels_%d" % H)
    if H >= 1 and (1 << H) >= max(nx, ny):
        got.add("one_top_node")
        assert all(s["top_nodes"] in (0, p["n_ang"]) for s in st)
    if 1 in (nx, ny):
        got.add("box_1")
    if H >= 1:
        for d, name in ((-1, "box_pow_minus_1"), (0, "box_pow"), (1, "box_pow_plus_1")):
            if (1 << H) + d in (nx, ny):
                got.add(name)
    if p["x0"] < 0:
        got.add("box_negative_x0")
    inside_x, inside_y = min(p["x0"] + nx, cols) - max(p["x0"], 0), min(p["y0"] + ny, rows) - max(p["y0"], 0)
    if inside_x <= 0 or inside_y <= 0:
        got.add("box_wholly_outside")
    elif inside_x < nx or inside_y < ny:
        got.add("box_partly_outside")
    for name, shape in (("grid_1x1", (1, 1)), ("grid_1x257", (257, 1)), ("grid_61x47", (47, 61))):
        if (rows, cols) == shape:
            got.add(name)
    if p["n_ang"] in (1, 2, 65):
        got.add("n_ang_%d" % p["n_ang"])
    for i, t in enumerate(trace):
        for a, nb in enumerate(t["nb"]):
            if nb in gm.NB_COUNTS:
                got.add("nb_%d" % nb)
            for b in t["beams"][a]:
                if b["skip"]:
                    got.add(b["skip"])
                    if b["range"] == np.nextafter(c["range_max"], np.inf):
                        got.add("range_one_ulp_above_max")
                elif b["range"] == c["range_max"]:
                    got.add("range_at_max_scored")
        if t["flags"] == EMPTY:
            got.add("empty")
            if 0 < i < len(trace) - 1 and c["lens"][i] == 0:
                got.add("empty_scan_in_the_middle")
            continue
        front = [t["frontier"].get(h, 0) for h in range(1, H + 1)]
        if t["flags"] == OVERFLOW:
            got.add("overflow")
            assert max(front) == p["max_nodes"] + 1 or max(front) > p["max_nodes"]
            continue
        if front and max(front) == p["max_nodes"]:
            got.add("max_nodes_at_largest")
        if t["flags"] == NOT_FOUND:
            got.add("not_found")
            if p["score_floor"] == int(t["S"].max()) + 1:
                got.add("floor_above_win")
            continue
        if p["score_floor"] == t["score"] > 0:
            got.add("floor_at_win")
        if t["n_best"] in (2, 4) and t["S"].min() < t["score"]:
            got.add("n_best_%d" % t["n_best"])
        if t["n_best"] == t["S"].size > 1 and t["score"] > 0:
            got.add("all_tie_lin_0")
            assert t["winner"] == (0, 0, 0)
        nb, S = t["n_beams"], t["score"]
        thr = 255 * nb * p["min_num"]
        if nb >= p["min_beams"] and nb > 0:
            if S * p["min_den"] == thr:
                got.add("accept_at_equality")
            elif S * p["min_den"] < thr <= (S + 1) * p["min_den"]:
                got.add("accept_one_below")
            elif (S - 1) * p["min_den"] <= thr < S * p["min_den"]:
                got.add("accept_one_above")
        if nb == p["min_beams"] - 1:
            got.add("beams_below_min")
            assert t["flags"] == REJECTED
        if nb == p["min_beams"] and nb > 0:
            got.add("beams_at_min")
        if t["flags"] == REJECTED:
            got.add("rejected")
    return got


@functools.lru_cache(maxsize=None)
def expected():
    """Per case of the campaign (records, statistics, trace) of the restatement at the case's own levels: computed once, shared, never
    changed."""
    return [run_case(c) for c in campaign()]


# ---- recovery --------------------------------------------------------------------------------------------------------------------------
RECOVERY_STEP, RECOVERY_HEADINGS = 3.0, 120
# an L-shaped room with a pillar, walls on whole cell lines: (x0, y0, x1, y1) segments, axis-parallel
WALLS = [(8, 6, 52, 6), (52, 6, 52, 24), (52, 24, 34, 24), (34, 24, 34, 40), (34, 40, 8, 40), (8, 40, 8, 6),
         (18, 14, 21, 14), (21, 14, 21, 18), (21, 18, 18, 18), (18, 18, 18, 14)]


def room_scan(pose, n_beams=180, resol=0.05):
    """The scan of the room from `pose` (x, y in cells, ang in degrees): ranges in metres to the nearest wall, the beams evenly spread."""
    x, y, ang = pose
    out = []
    for k in range(n_beams):
        a = -math.pi + 2 * math.pi * (k + 0.5) / n_beams
        th = a + math.radians(ang)
        c, s = math.cos(th), math.sin(th)
        best = math.inf
        for x0, y0, x1, y1 in WALLS:
            if x0 == x1 and c != 0:
                t = (x0 - x) / c
                if t > 0 and min(y0, y1) <= y + t * s <= max(y0, y1):
                    best = min(best, t)
            if y0 == y1 and s != 0:
                t = (y0 - y) / s
                if t > 0 and min(x0, x1) <= x + t * c <= max(x0, x1):
                    best = min(best, t)
        out.append((best * resol, a))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def recovery():
    """(corr, scans, lens, the true (cx, cy, a) of every scan, parameters): the room integrated at known whole-cell poses and smeared by
    GAUSS, and scans simulated from three OTHER whole-cell poses at headings that are multiples of the step."""
    cols, rows, resol, range_max = 61, 47, 0.05, 4.0
    mapped = np.array([(14.0, 11.0, 0.0), (44.0, 14.0, 90.0), (26.0, 30.0, 180.0), (14.0, 34.0, 270.0), (28.0, 12.0, 45.0)])
    sc = np.stack([room_scan(q, 360) for q in mapped])
    pa = np.zeros((rows, cols), np.uint32)
    hi = np.zeros_like(pa)
    for _ in range(2):
        gc.integrate(sc, np.full(len(mapped), 360, np.int32), mapped, cols, rows, resol, range_max, pa, hi)
    corr = gm.likelihood(pa, hi, 2, 1, 10, 3, gm.GAUSS)
    truth = [(40, 12, 7), (12, 28, 50), (27, 33, 101)]             # (cx, cy, a): the heading is a * RECOVERY_STEP degrees
    scans = np.stack([room_scan((cx, cy, a * RECOVERY_STEP)) for cx, cy, a in truth])
    lens = np.full(len(truth), scans.shape[1], np.int32)
    p = par(0, 0, cols, rows, ang0=0.0, ang_step=RECOVERY_STEP, n_ang=RECOVERY_HEADINGS, levels=4, max_nodes=1 << 16, min_beams=90, min_num=1,
            min_den=2)
    return dict(name="recovery", cols=cols, rows=rows, resol=resol, range_max=range_max, corr=corr, scans=scans, lens=lens, par=p,
                capacity=1024), truth
