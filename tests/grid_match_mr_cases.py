"""Coarse-to-fine correlative matching (csrc/k_gridmatch_mr.hip): the rule restated in plain Python / numpy on the helpers
of tests/grid_match_cases.py, and a generated campaign on grids of at most 61 x 47 cells.

The restatement is the definition.  The coarse plane is a maximum over bytes; U, the seeds, L and the refined set are integer sums and
comparisons of the same end cells the plain rule rounds, so neither has an iteration order and the device must give the same bytes -- the
records AND the statistics.  The winner is taken over the refined candidates ONLY: that it equals the plain winner is what the tests show.

A case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
import grid_match_cases as gm

STATS_DTYPE = np.dtype([("blocks", "u4"), ("refined", "u4"), ("fine", "u4"), ("lower_bound", "u4")])
assert STATS_DTYPE.itemsize == 16
BLOCKS = (2, 3, 4, 8, 16)                       # the block sizes every parity test runs


# ---- the coarse plane ------------------------------------------------------------------------------------------------------------------
def coarse_plane(corr, b):
    """uint8 [rows + b - 1, cols + b - 1]: coarse[y + b - 1][x + b - 1] = max corr[y + v][x + u] over 0 <= u, v < b inside the grid, 0 if
    none, for x = -(b - 1) .. cols - 1 and y likewise."""
    assert 2 <= b <= 16
    rows, cols = corr.shape
    h = b - 1
    padded = np.zeros((rows + 2 * h, cols + 2 * h), np.uint8)
    padded[h:h + rows, h:h + cols] = corr
    out = np.zeros((rows + h, cols + h), np.uint8)
    for v in range(b):
        for u in range(b):
            np.maximum(out, padded[v:v + rows + h, u:u + cols + h], out=out)
    return out


# ---- the match -------------------------------------------------------------------------------------------------------------------------
def prepare(scans, lens, poses, resol, range_max, corr, search):
    """What does not depend on the block size, per scan: None for a skipped scan, else the end cells, the beam traces, nb and the FULL score
    table S of every angle (the table is the trace's and the bound check's; the rule below reads it only where it refines)."""
    wx, wy, na, step = int(search["wx"]), int(search["wy"]), int(search["na"]), float(search["ang_step"])
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    out = []
    for n in range(len(lens)):
        why = gc.scan_skip(poses[n])
        if why:
            out.append(dict(skip=why))
            continue
        ang = float(poses[n][2])
        p = dict(skip=None, ends={}, beams={}, nb={}, S={})
        for a in range(-na, na + 1):
            bt = []
            ends = gm.scored_ends(scans[n], int(lens[n]), poses[n], ang + float(a) * step, resol, range_max, bt)
            p["ends"][a], p["beams"][a], p["nb"][a] = ends, bt, len(ends)
            p["S"][a] = gm.scores(ends, corr, wx, wy)[0]
        out.append(p)
    return out


def block_bounds(ends, coarse, b, wx, wy):
    """U int64 [nby, nbx] of one angle: the sum over the scored beams of coarse[ey - wy + J b + b - 1][ex - wx + I b + b - 1], 0 where that
    index is outside the coarse plane."""
    crows, ccols = coarse.shape
    nbx, nby = -(-(2 * wx + 1) // b), -(-(2 * wy + 1) // b)
    I = np.arange(nbx, dtype=np.int64)
    J = np.arange(nby, dtype=np.int64)
    cx = ends[:, 0, None, None] - wx + I[None, None, :] * b + (b - 1) + 0 * J[None, :, None]
    cy = ends[:, 1, None, None] - wy + J[None, :, None] * b + (b - 1) + 0 * I[None, None, :]
    inside = (cx >= 0) & (cx < ccols) & (cy >= 0) & (cy < crows)
    vals = np.where(inside, coarse[np.clip(cy, 0, crows - 1), np.clip(cx, 0, ccols - 1)].astype(np.int64), 0)
    return vals.sum(axis=0), (cx, cy, inside, vals)


def match_mr(scans, lens, poses, resol, range_max, corr, search, b, trace=None, strict=False, prepared=None, coarse=None):
    """(records MATCH_DTYPE, stats STATS_DTYPE) of the scans matched coarse to fine with blocks of b x b translations.  strict: the WRONG rule
    that refines only U > L (and keeps the seeds' own candidates) -- for the test that shows why the comparison is >=.  trace: a list that
    receives one dict per scan."""
    wx, wy, na, step = int(search["wx"]), int(search["wy"]), int(search["na"]), float(search["ang_step"])
    nx, ny = 2 * wx + 1, 2 * wy + 1
    nbx, nby = -(-nx // b), -(-ny // b)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    prepared = prepared if prepared is not None else prepare(scans, lens, poses, resol, range_max, corr, search)
    coarse = coarse if coarse is not None else coarse_plane(corr, b)
    out = np.zeros(len(lens), gm.MATCH_DTYPE)
    stats = np.zeros(len(lens), STATS_DTYPE)
    words = out.view(np.uint64).reshape(len(lens), 7)
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny))
    d2 = (ii - wx) ** 2 + (jj - wy) ** 2
    blk_of = (jj // b) * nbx + ii // b                                   # the block of every candidate of the window
    for n in range(len(lens)):
        words[n, :3] = poses[n].view(np.uint64)
        p = prepared[n]
        if p["skip"]:
            out[n]["flags"] = gm.SKIPPED
            if trace is not None:
                trace.append(dict(scan=n, skip=p["skip"]))
            continue
        x, y, ang = (float(v) for v in poses[n])
        U, rim, seeds, La = {}, {}, {}, {}
        for a in range(-na, na + 1):
            U[a], detail = block_bounds(p["ends"][a], coarse, b, wx, wy)
            cx, cy, inside, vals = detail
            rim[a] = bool((inside & ((cx < b - 1) | (cy < b - 1)) & (vals > 0)).any())
            seed = int(np.argmax(U[a].reshape(-1)))                       # the first of the largest: the smallest J nbx + I
            seeds[a] = (seed // nbx, seed % nbx)
            La[a] = int(p["S"][a][blk_of == seed].max())
        L = max(La.values())
        refined, best, n_fine = {}, None, 0
        for a in range(-na, na + 1):
            refined[a] = (U[a] > L) if strict else (U[a] >= L)
            mask = refined[a].reshape(-1)[blk_of]
            n_fine += int(mask.sum())
            if strict:
                mask = mask | (blk_of == seeds[a][0] * nbx + seeds[a][1])
            if not mask.any():
                continue
            S = p["S"][a]
            top = S[mask].max()
            m = mask & (S == top)
            m = m & (d2 == d2[m].min())
            j_i = np.argwhere(m)[0]                                     # row-major: the smallest linear index of this angle
            key = (-int(top), int(d2[m].min()), abs(a), ((a + na) * ny + int(j_i[0])) * nx + int(j_i[1]), a, int(j_i[0]) - wy, int(j_i[1]) - wx)
            if best is None or key < best:
                best = key
        S_win, a, j, i = -best[0], best[4], best[5], best[6]
        nb = p["nb"][a]
        ok = nb >= search["min_beams"] and S_win * int(search["min_den"]) >= 255 * nb * int(search["min_num"])
        r = out[n]
        r["score"], r["n_beams"], r["di"], r["dj"], r["da"] = S_win, nb, i, j, a
        r["score_prior"], r["flags"] = int(p["S"][0][wy, wx]), gm.ACCEPTED if ok else 0
        if ok:
            r["x"], r["y"], r["ang"] = x + float(i), y + float(j), ang + float(a) * step
        n_ref = sum(int(refined[a].sum()) for a in refined)
        stats[n] = ((2 * na + 1) * nbx * nby, n_ref, n_fine, L)
        if trace is not None:
            trace.append(dict(scan=n, skip=None, nb=p["nb"], beams=p["beams"], S=p["S"], U=U, rim=rim, seeds=seeds, La=La, L=L, refined=refined,
                              winner=(a, j, i), score=S_win, accepted=ok, prior=int(p["S"][0][wy, wx])))
    return out, stats


def bound_holds(trace, b, wx, wy):
    """S <= U on every block of every angle of every scan of a trace."""
    nx, ny = 2 * wx + 1, 2 * wy + 1
    for t in trace:
        if t["skip"]:
            continue
        for a, S in t["S"].items():
            Uc = np.repeat(np.repeat(t["U"][a], b, axis=0), b, axis=1)[:ny, :nx]       # every candidate's own block bound
            if not (S <= Uc).all():
                return False
    return True


# ---- the classes -----------------------------------------------------------------------------------------------------------------------
SURVIVORS = (0, 1, 63, 64, 65)
NB_COUNTS = (0, 1, 64, 65, 257, 1025)
MR_CLASSES = (["b_%d" % b for b in (2, 3, 8, 16)] + ["window_multiple", "window_overhang", "window_one_block", "low_rim", "winner_outside_seeds",
              "L_from_other_angle", "angle_no_survivor", "U_equals_L_wins", "zero_block_pruned", "all_refined", "refined_1"] +
              ["survivors_%d" % k for k in SURVIVORS] + ["survivors_over_256", "fine_over_256"] + ["nb_%d" % k for k in NB_COUNTS] +
              ["w63_na1", "scan_skipped", "beam_skipped", "beam_over_range", "half_way", "room"])


def mr_classes_of(case, trace, stats):
    got = set()
    b, se = case["block"], case["search"]
    wx, wy, na = se["wx"], se["wy"], se["na"]
    nx, ny = 2 * wx + 1, 2 * wy + 1
    nbx = -(-nx // b)
    if b in (2, 3, 8, 16):
        got.add("b_%d" % b)
    got.add("window_one_block" if nx < b else "window_multiple" if nx % b == 0 else "window_overhang")
    if (wx, wy, na) == (63, 63, 1):
        got.add("w63_na1")
    for t in trace:
        if t["skip"]:
            got.add("scan_skipped")
            continue
        for a, nb in t["nb"].items():
            if nb in NB_COUNTS:
                got.add("nb_%d" % nb)
            for bm in t["beams"][a]:
                if bm["skip"] == "beam_over_range":
                    got.add("beam_over_range")
                elif bm["skip"]:
                    got.add("beam_skipped")
                elif any(gc.is_half(v) for v in bm["raw"]):
                    got.add("half_way")
            k = int(t["refined"][a].sum())
            if k in SURVIVORS:
                got.add("survivors_%d" % k)
            if k == 0:
                got.add("angle_no_survivor")
            if k > 256:
                got.add("survivors_over_256")
            jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
            if int(t["refined"][a][jj // b, ii // b].sum()) > 256:
                got.add("fine_over_256")
            if t["rim"][a]:
                got.add("low_rim")
        a, j, i = t["winner"]
        JI = ((j + wy) // b, (i + wx) // b)
        st = stats[t["scan"]]
        if JI != t["seeds"][a]:
            got.add("winner_outside_seeds")
            if t["U"][a][JI] == t["L"]:
                got.add("U_equals_L_wins")
        if t["La"][a] < t["L"]:
            got.add("L_from_other_angle")
        if not t["refined"][0][wy // b, wx // b] and t["prior"] > 0:
            got.add("zero_block_pruned")
        if st["refined"] == st["blocks"] and st["blocks"] > 1 and t["L"] > 0:
            got.add("all_refined")
        if st["refined"] == 1:
            got.add("refined_1")
        if "offset" in case and (i, j, a) == tuple(-v for v in case["offset"]):
            got.add("room")
    return got


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
def with_block(case, b, name=None):
    c = dict(case, block=b)
    c["name"] = name or "%s_b%d" % (case["name"], b)
    return c


def one_beam(name, b, se, cells, pose=(20.0, 23.0), end=(30, 23), cols=61, rows=47, capacity=1024):
    """One beam from `pose` ending in the cell `end`; the plane is 0 but for cells: {(x, y): value}."""
    corr = np.zeros((rows, cols), np.uint8)
    for (x, y), v in cells.items():
        corr[y, x] = v
    case = gm.match_case(name, corr, 0.05, 4.0, [gm.beams_at_cells(pose, [end], 0.05)], [pose + (0.0,)], se, capacity=capacity)
    return with_block(case, b, name)


def peaks_in_blocks(name, b, W, k, spread, value=200):
    """One beam, a window of +-W, and k blocks -- every `spread`-th of the window's -- holding one cell of `value` at their low corner: exactly
    those k blocks have U = L = value."""
    ex, ey = 30, 23
    nbx = -(-(2 * W + 1) // b)
    nblk = nbx * nbx
    picked = [(m * spread) % nblk for m in range(k)]
    assert len(set(picked)) == k and ey - W >= 0 and ey + W < 47
    cells = {(ex - W + (q % nbx) * b, ey - W + (q // nbx) * b): value for q in picked}
    return one_beam(name, b, gm.search(W, W, 0), cells)


ROOM_OFFSETS = [(15, 15, 3), (-15, 9, -2), (7, -15, 1), (-11, -13, -3), (15, -6, 0)]      # (cells in x, cells in y, angle steps) added to the truth
ROOM_SEARCH = gm.search(15, 15, 3, 2.0, min_beams=30, min_num=1, min_den=2)

PLAIN_REUSED = ("skipped_scans_", "skipped_beams_", "range_max_", "half_way_", "nb0_", "nb1_", "nb64_", "nb65_", "nb257_", "nb1025_", "edges_",
                "uniform_")


def mr_campaign():
    cases = []
    rng = np.random.default_rng(20250801)
    # the plain campaign's skipped-scan, skipped-beam, range_max and half-way cases, its beam counts, its windows over the edges and its
    # uniform planes, each variant at another block size
    for c in gm.match_campaign():
        if c["name"].startswith(PLAIN_REUSED):
            v = int(c["name"].rsplit("_", 1)[1])
            cases.append(with_block(c, (2, 3, 8)[v] if not c["name"].startswith(("nb65_", "half_way_")) else (16, 4, 2)[v]))
    # random planes: every block size against windows that are a multiple of it, overhang it, and are smaller than it
    # (2 wx + 1 is odd: only an odd block size divides it)
    for b in (2, 3, 4, 5, 7, 8, 16):
        for v, (wx, wy) in enumerate(((b, b - 1), ((b - 2) // 2, b // 2), ((3 * b - 1) // 2 if b % 2 else b + b // 2, 2))):
            corr = gm.random_plane(rng, 61 - v, 47 - v, 0.3)
            beams = np.stack([rng.uniform(0.2, 1.0, 40 + v), rng.uniform(-math.pi, math.pi, 40 + v)], 1)
            poses = [(rng.uniform(25, 35), rng.uniform(18, 28), rng.uniform(-180, 180)), (30.0, 22.0, 0.0)]
            cases.append(with_block(gm.match_case("random_%d_%d" % (b, v), corr, 0.05, 1.5, [beams, beams[:17]], poses, gm.search(wx, wy, 1, 1.5)),
                                    b, "random_b%d_%d" % (b, v)))
    # structured planes: a few walls smeared by GAUSS -- the planes the bound is loose on, so most blocks go
    for v, b in enumerate((2, 3, 4, 8, 16, 8)):
        corr, scans, lens, truth = gm.recovery()
        se = gm.search(5 + v, 4 + v, 1, 2.0, min_beams=30, min_num=1, min_den=2)
        moved = truth + np.array([2 - v, v - 1, 2.0 * (v % 3 - 1)])
        case = gm.match_case("walls_%d" % v, corr, gm.ROOM["resol"], gm.ROOM["range_max"], list(scans), moved, se)
        cases.append(with_block(case, b, "walls_b%d_%d" % (b, v)))
    # the room at five large displacements
    corr, scans, lens, truth = gm.recovery()
    for v, off in enumerate(ROOM_OFFSETS):
        moved = truth + np.array([off[0], off[1], off[2] * ROOM_SEARCH["ang_step"]])
        case = gm.match_case("room_%d" % v, corr, gm.ROOM["resol"], gm.ROOM["range_max"], list(scans), moved, ROOM_SEARCH)
        case["offset"] = off
        cases.append(with_block(case, (4, 8, 2, 16, 3)[v], "room_b%d_%d" % ((4, 8, 2, 16, 3)[v], v)))
    # survivors per angle around the wavefront and beyond the workgroup: one beam, k blocks with a peak
    for k in (1, 63, 64, 65):
        for v in range(3):
            cases.append(peaks_in_blocks("peaks%d_%d" % (k, v), (2, 3, 2)[v], (9, 14, 11)[v], k, (7, 3, 5)[v], 200 + v))
    for v in range(3):
        cases.append(peaks_in_blocks("peaks_many_%d" % v, 2, 17, 300 - 10 * v, 1, 90 + v))             # beyond 256 survivors, and 4 x that fine
        cases.append(peaks_in_blocks("peaks_fine_%d" % v, (8, 16, 4)[v], (12, 17, 9)[v], (5, 2, 20)[v], 2, 77))   # few survivors, many fine items
    for v in range(3):
        b = (4, 8, 3)[v]
        # equal peaks at i = -3 and i = +1: the seed is the block of i = -3, L its score; the block of i = +1 has U == L and holds the winner
        # by i^2 + j^2
        se = gm.search(3, v, 0)
        cases.append(one_beam("equal_peaks_%d" % v, 4, se, {(27, 23): 150 + v, (31, 23): 150 + v}))
        # the zero offset's block pruned although score_prior is not 0
        cases.append(one_beam("prior_pruned_%d" % v, b, gm.search(2 * b, b, 0), {(30, 23): 40 + v, (30 + b + 1, 23 + 1): 220}))
        # an end cell near the left / top edge: the low rim of the coarse plane carries the cells of the grid's first columns and rows
        end = ((1, 20), (25, 0), (0, 1))[v]
        pose = (end[0] + 6.0, end[1] + 8.0)
        cells = {(0, y): 60 + y for y in range(0, 47, 3)}
        cells.update({(x, 0): 90 + x for x in range(0, 61, 4)})
        cells[(1, 1)] = 255
        cases.append(one_beam("low_rim_%d" % v, (4, 16, 8)[v], gm.search(3 + v, 4, 0), cells, pose=pose, end=end))
        # angles that see nothing: a long beam and a large step carry the end cell off the only peak
        cases.append(one_beam("lonely_%d" % v, b, gm.search(3, 3, 1, 50.0 + 5 * v), {(50, 23): 180 + v}, pose=(22.0, 23.0), end=(50, 23)))
        # L from another angle than the winner's: at a = 0 the seed's best cell (250) lies in the block's OVERHANG, beyond the window, so
        # L_0 is the 10 inside it; the winner (100) sits in another block of a = 0; a = +1, far away, finds 90 in its seed: L = 90
        bb = (4, 8, 3)[v]
        W = {4: 5, 8: 11, 3: 3}[bb]                                                           # 2 W + 1 no multiple of bb: the last block overhangs
        assert (2 * W + 1) % bb
        pose, end = (20.0, 23.0), (44, 23)                                                  # 24 cells: +50 degrees moves the end by ~20 cells
        th = math.radians(50.0)
        far = (int(round(20 + 24 * math.cos(th))), int(round(23 + 24 * math.sin(th))))
        cells = {(end[0] + W + 1, end[1]): 250, (end[0] + W, end[1]): 10, (end[0] + W - 1, end[1] - W): 100 + v, far: 90}
        cases.append(one_beam("other_angle_%d" % v, bb, gm.search(W, W, 1, 50.0), cells, pose=pose, end=end))
    # the widest window on a handful of beams
    for v, b in enumerate((8, 16, 4)):
        corr = gm.random_plane(rng, 61, 47, 0.15)
        beams = np.stack([rng.uniform(0.3, 1.0, 5 + v), rng.uniform(-math.pi, math.pi, 5 + v)], 1)
        cases.append(with_block(gm.match_case("w63_%d" % v, corr, 0.05, 1.5, [beams], [(30.0 + v, 23.0, 20.0 * v)], gm.search(63, 63, 1, 3.0)), b,
                                "w63_b%d_%d" % (b, v)))
    return cases


def run_mr_case(case, b=None, strict=False, prepared=None):
    trace = []
    rec, stats = match_mr(case["scans"], case["lens"], case["poses"], case["resol"], case["range_max"], case["corr"], case["search"],
                          case["block"] if b is None else b, trace, strict, prepared)
    return rec, stats, trace


def prepare_case(case):
    return prepare(case["scans"], case["lens"], case["poses"], case["resol"], case["range_max"], case["corr"], case["search"])
