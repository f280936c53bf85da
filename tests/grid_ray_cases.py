"""Ray casting on the grid (csrc/k_gridray.hip): the rule restated in plain Python / numpy on the helpers of
tests/grid_cases.py, a second formulation that walks every ray cell by cell, and a generated campaign on small grids (at most 61 x 47
cells; strips of up to 300 x 5 for the long rays).

The restatement is the definition: fp64 in the statement order of include/lsd_hip.h, C's round() and the x86 (int) cast, sin / cos from
the correctly rounded build of the oracle, the ray in its closed form, one sqrt and three products per distance.  It has no iteration
order to agree on, so the device must give the same bytes.

A case class is a predicate on the restatement's own TRACE (one record per beam and per skipped scan), never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
from grid_cases import K_PI, c_rint, c_round, cvt_x86, ray_cells, scan_skip

RAY_DTYPE = np.dtype([("r_exp", "f8"), ("r_unk", "f8"), ("cx", "i4"), ("cy", "i4"), ("k_hit", "i4"), ("cls", "u4")])
SUM_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("n", "u4", (7,)), ("judged", "u4"), ("flags", "u4"), ("pad", "u4")])
assert RAY_DTYPE.itemsize == 32 and SUM_DTYPE.itemsize == 64
NOT_CAST, NO_MEASUREMENT, AGREE_FREE, AGREE, SHORT, LONG, UNEXPLORED = range(7)
CONSISTENT, SKIPPED = 1, 2
QUIET_NAN = 0x7FF8000000000000
MAX_STRIP = 300                            # the long side of a strip grid (the short one: 5)
FREE, OCC, UNK = 0, 1, 2                   # cell kinds


def ray_par(tol=0.1, drop_mask=1 << SHORT, min_beams=1, ok_num=1, ok_den=2, gate=0):
    return dict(tol=float(tol), drop_mask=int(drop_mask), min_beams=int(min_beams), ok_num=int(ok_num), ok_den=int(ok_den), gate=int(gate))


def cell_kinds(grid, cells):
    """(kind, inside, byte) of the cells [n, 2] of an int8 [rows, cols] grid, read as k_occ.hip reads a cell: byte 255 unknown, 0 free,
    every other byte occupied; a cell outside the grid is unknown (its byte is given as 255)."""
    rows, cols = grid.shape
    x, y = cells[:, 0], cells[:, 1]
    inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
    v = np.full(len(cells), 255, np.uint8)
    v[inside] = grid.view(np.uint8)[y[inside], x[inside]]
    return np.where(v == 255, UNK, np.where(v == 0, FREE, OCC)), inside, v


def beam_cast(a, ang):
    """None, or why beam (angle a) of a scan at rotation ang is not cast."""
    if not math.isfinite(a):
        return "beam_bad_angle"
    if not math.isfinite(a + ang / 180.0 * K_PI):
        return "beam_th_overflow"
    return None


def cast_ends(pose, a, resol, range_max, rnd=c_round):
    """(x0, y0, x1, y1, the four values before rounding) of a beam that is cast: the ray runs to the range_max end cell."""
    x, y, ang = (float(v) for v in pose)
    th = a + ang / 180.0 * K_PI
    s, c = gc.cr().cr_sin(th), gc.cr().cr_cos(th)
    ex, ey = x + range_max * c / resol, y + range_max * s / resol
    return cvt_x86(rnd(x)), cvt_x86(rnd(y)), cvt_x86(rnd(ex)), cvt_x86(rnd(ey)), (x, y, ex, ey)


def dist(cell, x, y, resol):
    """Two products, one sum, one square root, one product."""
    ddx, ddy = float(cell[0]) - x, float(cell[1]) - y
    return math.sqrt(ddx * ddx + ddy * ddy) * resol


def first_cells(kinds):
    """(k_hit, k_unk) of the kinds along a ray, vectorised."""
    occ = np.flatnonzero(kinds == OCC)
    k_hit = int(occ[0]) if len(occ) else -1
    unk = np.flatnonzero(kinds[:k_hit] == UNK) if k_hit >= 0 else np.flatnonzero(kinds == UNK)
    return k_hit, (int(unk[0]) if len(unk) else -1)


def first_cells_brute(x0, y0, x1, y1, grid):
    """The same two numbers by walking the ray cell by cell in Python integers, stopping at the first occupied cell."""
    rows, cols = grid.shape
    g = grid.view(np.uint8)
    dx, dy = x1 - x0, y1 - y0
    n, m = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
    sx, sy = (-1 if dx < 0 else 1), (-1 if dy < 0 else 1)
    k_unk = -1
    for k in range(n + 1):
        minor = (2 * k * m + n) // (2 * n) if n else 0
        cx, cy = (x0 + sx * k, y0 + sy * minor) if abs(dx) >= abs(dy) else (x0 + sx * minor, y0 + sy * k)
        v = int(g[cy, cx]) if 0 <= cx < cols and 0 <= cy < rows else 255
        if v == 255:
            if k_unk < 0:
                k_unk = k
        elif v != 0:
            return k, k_unk, (cx, cy)
    return -1, k_unk, (x1, y1)


def classify(m, k_hit, k_unk, r_exp, r_unk, range_max, tol):
    if math.isnan(m) or m <= 0:
        return NO_MEASUREMENT
    if m == math.inf or m > range_max:
        return LONG if k_hit >= 0 else (UNEXPLORED if k_unk >= 0 else AGREE_FREE)
    d = m - r_exp
    if abs(d) <= tol:
        return AGREE
    if d > tol:
        return LONG
    return UNEXPLORED if r_unk <= m else SHORT


def record_of(pose, x1, y1, cells, k_hit, k_unk, m, resol, range_max, tol):
    """The beam record (a tuple in RAY_DTYPE's order) of a cast beam."""
    x, y = float(pose[0]), float(pose[1])
    r_exp = dist(cells[k_hit], x, y, resol) if k_hit >= 0 else math.inf
    r_unk = dist(cells[k_unk], x, y, resol) if k_unk >= 0 else math.inf
    cx, cy = (int(cells[k_hit][0]), int(cells[k_hit][1])) if k_hit >= 0 else (x1, y1)
    return (r_exp, r_unk, cx, cy, k_hit, classify(m, k_hit, k_unk, r_exp, r_unk, range_max, tol))


def summary_flags(n, par):
    """(judged, consistent) of the seven class counts; Python's integers are unbounded: no product overflows."""
    judged = int(n[2]) + int(n[3]) + int(n[4]) + int(n[5])
    return judged, judged >= par["min_beams"] and (int(n[2]) + int(n[3])) * par["ok_den"] >= judged * par["ok_num"]


def raycast(scans, lens, poses, grid, resol, range_max, par, out, sums, scans_out=None, rnd=c_round, trace=None):
    """Writes the beam records out [n, stride] (RAY_DTYPE; i < len only), the summaries sums [n] (SUM_DTYPE) and, if given, the screened
    scans scans_out [n, stride, 2] (i < len only), in place.  scans_out may be `scans` itself.  trace: a list that receives one dict per
    beam and one per skipped scan."""
    bits_in = np.ascontiguousarray(scans).view(np.uint64)
    for i in range(len(lens)):
        pose = [float(v) for v in poses[i]]
        why = scan_skip(pose)
        counts = [0] * 7
        for j in range(int(lens[i])):
            m, a = float(scans[i, j, 0]), float(scans[i, j, 1])
            rec, t = (0.0, 0.0, 0, 0, 0, NOT_CAST), None
            if not why:
                no = beam_cast(a, pose[2])
                if no:
                    t = dict(scan=i, beam=j, skip=no)
                else:
                    x0, y0, x1, y1, raw = cast_ends(pose, a, resol, range_max, rnd)
                    cells = ray_cells(x0, y0, x1, y1)
                    kinds, inside, byte = cell_kinds(grid, cells)
                    k_hit, k_unk = first_cells(kinds)
                    rec = record_of(pose, x1, y1, cells, k_hit, k_unk, m, resol, range_max, par["tol"])
                    t = dict(scan=i, beam=j, skip=None, x0=x0, y0=y0, x1=x1, y1=y1, raw=raw, cells=cells, kinds=kinds, inside=inside, byte=byte,
                             k_hit=k_hit, k_unk=k_unk, r_exp=rec[0], r_unk=rec[1], m=m, cls=rec[5])
                counts[rec[5]] += 1
            out[i, j] = rec
            if scans_out is not None:
                dropped = (par["drop_mask"] >> rec[5]) & 1
                b = (QUIET_NAN if dropped else bits_in[i, j, 0], bits_in[i, j, 1])
                scans_out.view(np.uint64)[i, j] = b
            if trace is not None and t is not None:
                trace.append(t)
        if why:
            counts = [0] * 7
            if trace is not None:
                trace.append(dict(scan=i, skip=why))
        judged, ok = summary_flags(counts, par)
        ok = ok and not why
        s = np.zeros((), SUM_DTYPE)
        s["n"], s["judged"], s["flags"] = counts, judged, (CONSISTENT if ok else 0) | (SKIPPED if why else 0)
        sums[i] = s
        sums.view(np.uint64).reshape(len(sums), 8)[i, :3] = np.array(poses[i], np.float64).view(np.uint64)        # the pose's bits
        if par["gate"] and not why and not ok:
            sums["x"][i] = -1.0                                   # the "no pose" sentinel


def run_case(case, rnd=c_round, fill=None, in_place=False):
    """(out, sums, scans_out, trace) of a case.  fill: None (zeroed outputs), or a function(shape_bytes, seed) -> uint8 pattern the
    three outputs start from."""
    n, stride = case["scans"].shape[:2]
    out, sums, so = np.zeros((n, stride), RAY_DTYPE), np.zeros(n, SUM_DTYPE), np.zeros((n, stride, 2))
    if fill is not None:
        out = fill(out.nbytes, 1).view(RAY_DTYPE).reshape(n, stride).copy()
        sums = fill(sums.nbytes, 2).view(SUM_DTYPE).copy()
        so = fill(so.nbytes, 3).view(np.float64).reshape(n, stride, 2).copy()
    if in_place:
        so = case["scans"].copy()
    trace = []
    raycast(case["scans"] if not in_place else so, case["lens"], case["poses"], case["grid"], case["resol"], case["range_max"], case["par"], out, sums,
            so, rnd, trace)
    return out, sums, so, trace


# ---- the classes -----------------------------------------------------------------------------------------------------------------------
SCAN_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 360, 1025)
K_HITS = (15, 16, 17, 63, 64, 65, 255, 256, 257)
OCTANTS, AXES, SCAN_SKIPS = gc.OCTANTS, gc.AXES, gc.SCAN_SKIPS
BEAM_SKIPS = ["beam_bad_angle", "beam_th_overflow"]
NO_MEAS = ["m_nan", "m_zero", "m_negative", "m_minus_inf"]
CLASSES = (["khit_0", "khit_1", "khit_n", "khit_none", "occupied_behind_unknown", "unknown_behind_hit", "leaves_grid", "enters_from_outside",
            "wholly_outside"] + OCTANTS + AXES + ["diagonal", "n_zero"] + ["khit_%d" % k for k in K_HITS] +
           ["scan_len_%d" % n for n in SCAN_LENGTHS] + ["len_zero", "len_is_stride"] + SCAN_SKIPS + BEAM_SKIPS + ["all_256_bytes"] +
           ["cls_%d" % c for c in range(7)] +
           ["d_at_tol", "d_ulp_outside_tol", "d_ulp_inside_tol", "tol_zero_agree", "tol_zero_disagree", "m_at_range_max", "m_ulp_above_range_max",
            "r_unk_at_m", "r_unk_ulp_below_m", "r_unk_ulp_above_m"] + NO_MEAS +
           ["half_way", "sum_at_equality", "sum_one_below", "sum_one_above", "judged_at_min", "judged_below_min", "sum_products_beyond_2_32",
            "gate_on_gated", "gate_on_passed", "gate_off_inconsistent", "drop_mask_0", "drop_mask_127"] + ["drop_bit_%d" % c for c in range(7)])


def classes_of(case, trace, sums):
    """The classes a case reaches, from its trace and the restatement's summaries."""
    got = set()
    par, rmax = case["par"], case["range_max"]
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    bytes_read = set()
    for t in trace:
        if t["skip"]:
            got.add(t["skip"])
            if "beam" in t or case["lens"][t["scan"]] > 0:
                got.add("cls_0")                     # (a beam that is not cast, or the beams of a scan that is not)
            continue
        got.add("cls_%d" % t["cls"])
        dx, dy = t["x1"] - t["x0"], t["y1"] - t["y0"]
        n, m_ = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
        if n == 0:
            got.add("n_zero")
        elif m_ == n:
            got.add("diagonal")
        elif m_ == 0:
            got.add("axis_%s%s" % ("+-"[(dx or dy) < 0], "x" if dx else "y"))
        else:
            got.add("octant_%s%s_%s" % ("+-"[dx < 0], "+-"[dy < 0], "x" if abs(dx) > abs(dy) else "y"))
        k_hit, k_unk, kinds, ins = t["k_hit"], t["k_unk"], t["kinds"], t["inside"]
        if k_hit in (0, 1):
            got.add("khit_%d" % k_hit)
        if k_hit == n and n > 1:
            got.add("khit_n")
        if k_hit < 0:
            got.add("khit_none")
        if k_hit in K_HITS:
            got.add("khit_%d" % k_hit)
        if k_hit >= 0 and k_unk >= 0:
            got.add("occupied_behind_unknown")
            assert k_unk < k_hit
        if k_hit >= 0 and k_unk < 0 and (kinds[k_hit + 1:] == UNK).any():
            got.add("unknown_behind_hit")
        if ins[0] and not ins[-1]:
            got.add("leaves_grid")
        if not ins[0] and ins.any():
            got.add("enters_from_outside")
        if not ins.any():
            got.add("wholly_outside")
        bytes_read.update(t["byte"][ins][:(k_hit + 1) if k_hit >= 0 else None].tolist())
        m = t["m"]
        if math.isnan(m):
            got.add("m_nan")
        elif m == 0:
            got.add("m_zero")
        elif m == -math.inf:
            got.add("m_minus_inf")
        elif m < 0:
            got.add("m_negative")
        elif m == rmax:
            got.add("m_at_range_max")
            assert t["cls"] in (AGREE, SHORT, LONG, UNEXPLORED)
        elif m == up(rmax):
            got.add("m_ulp_above_range_max")
            assert t["cls"] in (AGREE_FREE, LONG, UNEXPLORED)
        if 0 < m <= rmax:                            # a return
            d, tol = m - t["r_exp"], par["tol"]
            near = [abs(dn(m) - t["r_exp"]), abs(up(m) - t["r_exp"])]
            if tol > 0 and abs(d) == tol:
                got.add("d_at_tol")
                assert t["cls"] == AGREE
            if tol > 0 and abs(d) > tol and tol in near:
                got.add("d_ulp_outside_tol")
                assert t["cls"] != AGREE
            if tol > 0 and abs(d) < tol and tol in near:
                got.add("d_ulp_inside_tol")
                assert t["cls"] == AGREE
            if tol == 0:
                got.add("tol_zero_agree" if d == 0 else "tol_zero_disagree")
                assert (t["cls"] == AGREE) == (d == 0)
            if d < -tol and math.isfinite(t["r_unk"]):
                if t["r_unk"] == m:
                    got.add("r_unk_at_m")
                    assert t["cls"] == UNEXPLORED
                if t["r_unk"] == dn(m):
                    got.add("r_unk_ulp_below_m")
                    assert t["cls"] == UNEXPLORED
                if t["r_unk"] == up(m):
                    got.add("r_unk_ulp_above_m")
                    assert t["cls"] == SHORT
        if any(gc.is_half(v) for v in t["raw"]):
            got.add("half_way")
    if len(bytes_read) == 256:
        got.add("all_256_bytes")
    stride = case["scans"].shape[1]
    for i, ln in enumerate(case["lens"]):
        skipped = scan_skip(case["poses"][i]) is not None
        if ln == 0:
            got.add("len_zero")
        if ln == stride:
            got.add("len_is_stride")
        if ln in SCAN_LENGTHS and not skipped:
            got.add("scan_len_%d" % ln)
        if skipped:
            continue
        n = [int(v) for v in sums["n"][i]]
        judged, ok = summary_flags(n, par)
        lhs, rhs, agree = (n[2] + n[3]) * par["ok_den"], judged * par["ok_num"], n[2] + n[3]
        if judged >= max(1, par["min_beams"]):
            if lhs == rhs:
                got.add("sum_at_equality")
            if (agree + 1) * par["ok_den"] == rhs:
                got.add("sum_one_below")
                assert not ok
            if (agree - 1) * par["ok_den"] == rhs:
                got.add("sum_one_above")
                assert ok
            if lhs >= 1 << 32 and rhs >= 1 << 32:
                got.add("sum_products_beyond_2_32")
        if par["min_beams"] > 0 and judged == par["min_beams"]:
            got.add("judged_at_min")
        if par["min_beams"] > 0 and judged == par["min_beams"] - 1:
            got.add("judged_below_min")
            assert not ok
        if par["gate"]:
            got.add("gate_on_passed" if ok else "gate_on_gated")
        elif not ok:
            got.add("gate_off_inconsistent")
    mask = par["drop_mask"]
    if mask in (0, 127):
        got.add("drop_mask_%d" % mask)
    for c in range(7):
        if mask == 1 << c:
            got.add("drop_bit_%d" % c)
    return got


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
MASKS = [0, 127] + [1 << c for c in range(7)]


def make_case(name, grid, resol, range_max, beams, poses, par=None, stride=None, capacity=1024):
    """grid: int8 [rows, cols]; beams: per scan a list of (range, angle); stride: the pitch (default: the longest scan, at least 1)."""
    rows, cols = grid.shape
    assert (cols <= gc.MAX_COLS and rows <= gc.MAX_ROWS) or (max(cols, rows) <= MAX_STRIP and min(cols, rows) <= 5)
    stride = stride or max(1, max(len(b) for b in beams))
    scans = np.zeros((len(beams), stride, 2))
    for i, b in enumerate(beams):
        if len(b):
            scans[i, :len(b)] = np.asarray(b, np.float64).reshape(-1, 2)
    return dict(name=name, cols=cols, rows=rows, resol=float(resol), range_max=float(range_max), scans=scans,
                lens=np.array([len(b) for b in beams], np.int32), poses=np.asarray(poses, np.float64).reshape(-1, 3), capacity=capacity,
                grid=np.ascontiguousarray(grid, np.int8), par=par or ray_par())


def room(cols, rows, wall=100, margin=1, outside=-1):
    """Free inside, a closed wall `margin` cells from the border, `outside` beyond it."""
    g = np.full((rows, cols), outside, np.int8)
    g[margin:rows - margin, margin:cols - margin] = wall
    g[margin + 1:rows - margin - 1, margin + 1:cols - margin - 1] = 0
    return g


def noisy_room(rng, cols, rows):
    """A room with unknown blotches and obstacles of every byte value."""
    g = room(cols, rows, margin=int(rng.integers(0, 3)))
    for _ in range(6):
        x, y = int(rng.integers(2, cols - 4)), int(rng.integers(2, rows - 4))
        g[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = -1
    for _ in range(8):
        g[int(rng.integers(2, rows - 2)), int(rng.integers(2, cols - 2))] = np.uint8(rng.integers(1, 255)).view(np.int8)
    return g


def measured(rng, case_args, share_agree=0.5):
    """Ranges for the beams of a case under construction: about half within a cell of what the map expects (the restatement's own
    expected range is an INPUT here, nothing is compared with it), the rest anywhere, and a few readings of every unusable kind."""
    grid, resol, range_max, beams, poses = case_args
    out = []
    for b, pose in zip(beams, poses):
        b = np.array(b, np.float64).reshape(-1, 2)
        if scan_skip(pose) is None:
            for j in range(len(b)):
                if beam_cast(float(b[j, 1]), float(pose[2])) is None and rng.random() < share_agree:
                    x0, y0, x1, y1, _ = cast_ends(pose, float(b[j, 1]), resol, range_max)
                    cells = ray_cells(x0, y0, x1, y1)
                    k_hit, _ = first_cells(cell_kinds(grid, cells)[0])
                    if k_hit >= 0:
                        b[j, 0] = dist(cells[k_hit], float(pose[0]), float(pose[1]), resol) + rng.uniform(-1.5, 1.5) * resol
        if len(b) >= 8:
            for v in (math.nan, -0.3, 0.0, math.inf, -math.inf, 10 * range_max):
                b[rng.integers(0, len(b)), 0] = v
        out.append(b)
    return out


def campaign():
    """The cases, deterministic."""
    cases = []
    rng = np.random.default_rng(20250914)
    deg = math.pi / 180
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))

    def add(name, grid, resol, range_max, beams, poses, **kw):
        i = len(cases)
        par = dict(ray_par(tol=kw.pop("tol", 2 * resol), drop_mask=MASKS[i % len(MASKS)], gate=(i // 2) % 2), **kw.pop("par", {}))
        cases.append(make_case(name, grid, resol, range_max, beams, poses, par=par, **kw))

    # the eight octants, the four axes, exact diagonals, n = 0, in rooms whose walls the rays reach (or not: range_max 1 m in the last)
    for v, (px, py, ang) in enumerate([(30.0, 23.0, 0.0), (20.3, 11.6, 37.0), (41.7, 30.2, -171.5)]):
        rmax = (4.0, 2.5, 1.0)[v]
        g = room(61, 47, wall=(100, 1, -128)[v])
        octs = [(0.45 + 0.4 * k, (22.5 + 45 * k) * deg - ang * deg) for k in range(8)]
        add("octants%d" % v, g, 0.05, rmax, [octs], [(px, py, ang)])
        ipx, ipy = round(px), round(py)
        axes = [(0.4 + 0.35 * k, k * math.pi / 2) for k in range(4)]
        add("axes%d" % v, g, 0.05, rmax, [axes], [(ipx, ipy, 0.0)])
        diag = [(0.5 + 0.3 * k, (45 + 90 * k) * deg) for k in range(4)]
        add("diagonals%d" % v, g, 0.05, rmax, [diag], [(ipx, ipy, 0.0)])
        tiny = [(0.004 + 0.003 * k, 0.7 * k + v) for k in range(5)]
        add("n_zero%d" % v, room(33 + v, 29 - v), 0.05, 0.02, [tiny], [(ipx % 29, ipy % 23, 10.0 * v)])
    # k_hit = 0, 1, n and none; an occupied cell behind an unknown one, an unknown one behind the first occupied one: along +x at
    # a resolution of 0.5 and range_max 4, i.e. rays of exactly 8 cells
    for v in range(3):
        g = np.zeros((12 + v, 30), np.int8)
        g[1, 10] = 100                       # the start cell itself
        g[2, 11] = 50                        # the neighbour
        g[3, 18] = 100 - v                   # the last cell (n = 8)
        g[5, 14], g[5, 16] = -1, 100         # occupied behind unknown
        g[6, 14], g[6, 16] = 100, -1         # unknown behind occupied
        g[7, 12:15], g[7, 17] = -1, 1        # several unknown cells, then occupied
        beams = [[(1.0 + 0.5 * v, 0.0), (3.0, 0.0)]] * 7
        poses = [(10.0, r, 0.0) for r in (1, 2, 3, 4, 5, 6, 7)]
        add("k_hit_small%d" % v, g, 0.5, 4.0, beams, poses, tol=0.25)
    # rays that leave the grid, start outside and enter, stay outside
    for v in range(3):
        g = room(31 + 5 * v, 23 + 3 * v, margin=0)
        g[1:-1, -1] = 0                      # an open side: rays leave through it
        fan = [(1.5 + 0.2 * v, k * 2 * math.pi / 24 + 0.01 * v) for k in range(24)]
        add("leaves%d" % v, g, 0.05, 4.0, [fan], [(15.2 + v, 11.4 + v, 3.0 * v)])
        g2 = np.zeros((30 + v, 40), np.int8)
        g2[10:20, 20] = 100
        inward = [(1.2 + 0.1 * k, (-20 + 5 * k) * deg) for k in range(9)]
        add("enters%d" % v, g2, 0.05, 4.0, [inward, inward], [(-6.4 - v, 14.0 + v, 0.0), (12.0 + v, -5.5, 90.0)])
        away = [(0.8 + 0.05 * k, (160 + 5 * k) * deg) for k in range(9)]
        add("outside%d" % v, g2, 0.05, 4.0, [away, inward], [(-9.0 - v, 15.0, 0.0), (300.0 + v, 200.0, 0.0)])
    # k_hit on and beside the strides of a lane group, a wavefront and a workgroup: strips, one beam along the strip per scan
    for v in range(3):
        horizontal = v != 1
        g = np.zeros((5, MAX_STRIP) if horizontal else (MAX_STRIP, 5), np.int8)
        wall = 290 if v != 2 else 9
        if horizontal:
            g[:, wall] = 100
            g[4, :] = -1                     # one row of unknown cells: a slanted ray reports it
        else:
            g[wall, :] = 100
        sgn = -1 if v == 2 else 1
        poses, beams = [], []
        for j, k in enumerate(K_HITS):
            poses.append((wall - sgn * k, j % 4, 0.0) if horizontal else (j % 5, wall - sgn * k, 0.0))
            a = (0.0 if sgn > 0 else math.pi) if horizontal else math.pi / 2
            beams.append([(k * 0.05, a), (1.0, a + 0.004), (14.5, a - 0.002), (math.inf, a)])
        add("k_hit_strides%d" % v, g, 0.05, 14.0, beams, poses)
    # every byte value: 256 scans of one beam along +x, each with its own cell three steps ahead (range_max: 6 cells)
    for v in range(3):
        g = np.zeros((47, 61), np.int8)
        vals = np.roll(np.arange(256), 37 * v)
        poses, beams = [], []
        for s in range(256):
            y, x = s % 40 + 3, 8 * (s // 40) + 1
            g.view(np.uint8)[y, x + 3] = vals[s]
            poses.append((x, y, 0.0))
            beams.append([(0.15 + 0.01 * (s % 3), 0.0)])
        add("bytes%d" % v, g, 0.05, 0.3, beams, poses)
    # the class edges.  resol 0.5 and integer poses make every distance along an axis exact: the wall is 6 cells (3.0) ahead along +x,
    # an unknown cell 4 cells (2.0) ahead along +y with nothing behind it
    for v, tol in enumerate([0.25, 0.5, 0.125]):
        g = np.zeros((30, 40), np.int8)
        g[:, 16 + v] = 100
        g[14 + v, 10 + v] = -1
        pose = (10.0 + v, 10.0 + v, 0.0)
        r, ru, rmax, h = 3.0, 2.0, 4.0, math.pi / 2
        edges = [(r + tol, 0.0), (up(r + tol), 0.0), (dn(r + tol), 0.0), (r - tol, 0.0), (dn(r - tol), 0.0), (up(r - tol), 0.0), (r, 0.0),
                 (rmax, 0.0), (up(rmax), 0.0), (rmax, math.pi), (up(rmax), math.pi), (rmax, h), (up(rmax), h),
                 (ru, h), (up(ru), h), (dn(ru), h), (1.0, h), (3.5, h),
                 (math.nan, 0.0), (0.0, 0.0), (-0.0, 0.0), (-1.5, 0.0), (-math.inf, 0.0), (math.inf, 0.0), (math.inf, h), (math.inf, math.pi)]
        add("edges%d" % v, g, 0.5, rmax, [edges], [pose], tol=tol)
        add("tol_zero%d" % v, g, 0.5, rmax, [[(r, 0.0), (up(r), 0.0), (dn(r), 0.0), (ru, h), (1.0, math.pi)]], [pose], tol=0.0)
    # beams and scans that are not cast
    for v in range(3):
        good = (0.6 + 0.1 * v, 0.5)
        g = room(47, 41)
        b = [good, (0.6, math.nan), (0.6, math.inf), (0.6, -math.inf), (math.nan, math.nan), good]
        add("uncast_beams%d" % v, g, 0.05, 2.0, [b, [good, (1.0, 1.79e308), (1.0, 0.3)]], [(20.0 + v, 19.0, 5.0 * v), (20.0, 19.0 + v, 1e308)])
        poses = [(math.nan, 10, 0), (10, math.inf, 0), (10, 10, math.nan), (10, 10, -math.inf), (-1.0, 12, 0), (-1.00005, 12, 3),
                 (-0.99995, 12, 3), (1048577.0, 3, 0), (5, -1048576.5, 0), (-0.9998, 12.0, 0.0), (21.0 + v, 17.0, 0.0)]
        add("skipped_scans%d" % v, g, 0.05, 2.0, [[good, (0.9, 2.0 + v)]] * len(poses), poses)
    # len = 0, len = stride, and the scan lengths around the wavefront and the workgroup, in noisy rooms
    def random_case(name, cols, rows, lengths, **kw):
        g = noisy_room(rng, cols, rows)
        beams = [np.stack([rng.uniform(0.05, 3.5, n), rng.uniform(-math.pi, math.pi, n)], 1) if n else [] for n in lengths]
        poses = [(rng.uniform(5, cols - 5), rng.uniform(5, rows - 5), rng.uniform(-180, 180)) for _ in lengths]
        add(name, g, 0.05, 3.0, measured(rng, (g, 0.05, 3.0, beams, poses)), poses, **kw)
    for v in range(3):
        random_case("len_zero%d" % v, 29, 31, [0, 5, 0], stride=5 + v)
    for n in SCAN_LENGTHS:
        for v in range(3 if n != 1025 else 1):
            random_case("len%d_%d" % (n, v), 61 - v, 47 - 2 * v, [n, max(1, n // 2)], stride=n + (0 if v == 0 else 7 * v),
                        capacity=1024 if n <= 1024 else 2048)
    # coordinates exactly half-way between two cells, where round and rint part: in the pose and in the end point (c = 1 exactly at
    # th = 0, and range_max / mapResol = 4.5 exactly)
    for v in range(3):
        g = room(40, 30, margin=2)
        g[8, 15 + 2 * v], g[7, 16 + 2 * v] = 100, 100
        b = [(2.25, 0.0), (1.0, math.pi / 2), (2.0, 0.0)]
        poses = [(10.0 + 2 * v, 8.0, 0.0), (12.5 + 2 * v, 6.5, 0.0), (2.5, 3.5 + v, 0.0)]
        add("half_way%d" % v, g, 0.5, 2.25, [b] * 3, poses)
    # the summary rule: four beams along the axes of a closed room, k of them agreeing and the rest short, at ok = 1 / 2 (k = 1, 2, 3), with
    # min_beams at judged and one above, and the same ratio as 2^30 / 2^31
    for v in range(3):
        g = room(21, 21)                     # the walls 9 cells (0.45 m) from the centre, along every axis
        want = 9 * 0.05
        scans = [[(want if k < agree else 0.1, k * math.pi / 2) for k in range(4)] for agree in (1, 2, 3)]
        scans.append([(want, 0.0), (want, math.pi / 2), (0.1, math.pi), (math.nan, 0.0)])                # judged = 3
        poses = [(10.0, 10.0, 0.0)] * 4
        add("summary_half%d" % v, g, 0.05, 1.0, scans, poses, par=dict(min_beams=4, ok_num=1, ok_den=2), tol=0.01)
        add("summary_big%d" % v, g, 0.05, 1.0, scans, poses, par=dict(min_beams=3 + (v == 2), ok_num=1 << 30, ok_den=1 << 31), tol=0.01)
        add("summary_gate%d" % v, g, 0.05, 1.0, scans, poses, par=dict(min_beams=1 + v, ok_num=3, ok_den=4, gate=1), tol=0.01)
        add("summary_open%d" % v, g, 0.05, 1.0, scans, poses, par=dict(min_beams=5, ok_num=0, ok_den=1 + v, gate=0), tol=0.01)
    return cases
