"""Mapping with known poses (csrc/k_gridmap.hip): the rule restated in plain Python / numpy, and a generated campaign on
small grids (at most 61 x 47 cells).

The restatement is the definition: fp64 in the statement order of include/lsd_hip.h (Python floats are IEEE doubles and never fuse a
multiply with an add), C's round() and the x86 (int) cast written out, sin / cos from the correctly rounded build of the oracle
(oracle.lib_cr(): cr_sin / cr_cos, which is what sincos_g computes on the device for |th| <= 64), the ray in its closed form, counters
modulo 2^32.  It has no iteration order to agree on, so the device must give the same bytes.

A case class is a predicate on the restatement's own TRACE (one record per beam and per skipped scan), never on what the device gives.
"""
import ctypes as C
import math

import numpy as np

K_PI = 3.14159265358979323846              # lsd_internal.h: kPi
INT_MIN = -(1 << 31)
MAX_COLS, MAX_ROWS = 61, 47                # the campaign's largest grid

_cr = None


def cr():
    global _cr
    if _cr is None:
        from oracle import oracle
        L = oracle.lib_cr()
        for f in (L.cr_sin, L.cr_cos):
            f.restype, f.argtypes = C.c_double, [C.c_double]
        _cr = L
    return _cr


def c_round(v):
    """C's round(): to the nearest integer, half-way cases away from zero (v - trunc(v) is exact in fp64)."""
    t = float(math.trunc(v))
    return t + math.copysign(1.0, v) if abs(v - t) >= 0.5 else t


def c_rint(v):
    """rint() in the default rounding mode: half-way cases to even.  NOT the rule; the half-way class shows the difference."""
    return float(np.rint(v))


def cvt_x86(v):
    """cvttsd2si: lsd_internal.h cvt_x86."""
    if not (v > -2147483649.0 and v < 2147483648.0):
        return INT_MIN
    return int(v)


def scan_skip(pose):
    """None, or why the whole scan is skipped."""
    x, y, ang = (float(v) for v in pose)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(ang)):
        return "scan_nonfinite"
    if abs(x + 1) < 1e-4:
        return "scan_sentinel"
    if abs(x) > 1048576.0 or abs(y) > 1048576.0:
        return "scan_far"
    return None


def beam_skip(r, a, ang):
    """None, or why the beam is skipped."""
    if math.isnan(r):
        return "beam_nan_range"
    if r <= 0:
        return "beam_nonpos_range"
    if r == math.inf:
        return "beam_inf_range"
    if not math.isfinite(a) or not math.isfinite(a + ang / 180.0 * K_PI):
        return "beam_bad_angle"
    return None


def beam_ends(pose, r, a, resol, range_max, rnd=c_round):
    """(x0, y0, x1, y1, hits, the four values before rounding) of a beam that is not skipped."""
    x, y, ang = (float(v) for v in pose)
    rr = r if r < range_max else range_max
    th = a + ang / 180.0 * K_PI
    s, c = cr().cr_sin(th), cr().cr_cos(th)
    ex, ey = x + rr * c / resol, y + rr * s / resol
    return cvt_x86(rnd(x)), cvt_x86(rnd(y)), cvt_x86(rnd(ex)), cvt_x86(rnd(ey)), r <= range_max, (x, y, ex, ey)


def ray_cells(x0, y0, x1, y1):
    """The n + 1 cells of the ray, int64 [n + 1, 2] as (x, y), k = 0 .. n."""
    dx, dy = x1 - x0, y1 - y0
    n, m = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
    k = np.arange(n + 1, dtype=np.int64)
    minor = (2 * k * m + n) // (2 * n) if n else k
    sx, sy = (-1 if dx < 0 else 1), (-1 if dy < 0 else 1)
    if abs(dx) >= abs(dy):
        return np.stack([x0 + sx * k, y0 + sy * minor], 1)
    return np.stack([x0 + sx * minor, y0 + sy * k], 1)


def integrate(scans, lens, poses, cols, rows, resol, range_max, pass_counts, hit_counts, rnd=c_round, trace=None):
    """Adds the scans to the two uint32 [rows, cols] planes, in place.  trace: a list that receives one dict per beam (and one per
    skipped scan)."""
    pa = pass_counts.reshape(-1).astype(np.int64)
    hi = hit_counts.reshape(-1).astype(np.int64)
    for i in range(len(lens)):
        why = scan_skip(poses[i])
        if why:
            if trace is not None:
                trace.append(dict(scan=i, skip=why))
            continue
        for j in range(int(lens[i])):
            r, a = float(scans[i, j, 0]), float(scans[i, j, 1])
            why = beam_skip(r, a, float(poses[i][2]))
            if why:
                if trace is not None:
                    trace.append(dict(scan=i, beam=j, skip=why))
                continue
            x0, y0, x1, y1, hits, raw = beam_ends(poses[i], r, a, resol, range_max, rnd)
            cells = ray_cells(x0, y0, x1, y1)
            inside = (cells[:, 0] >= 0) & (cells[:, 0] < cols) & (cells[:, 1] >= 0) & (cells[:, 1] < rows)
            idx = cells[inside, 1] * cols + cells[inside, 0]
            pa[idx] += 1                                  # (the cells of one ray are distinct)
            if hits and inside[-1]:
                hi[cells[-1, 1] * cols + cells[-1, 0]] += 1
            if trace is not None:
                trace.append(dict(scan=i, beam=j, skip=None, x0=x0, y0=y0, x1=x1, y1=y1, hits=hits, range=r, raw=raw, cells=cells,
                                  inside=inside))
    pass_counts.reshape(-1)[:] = (pa & 0xFFFFFFFF).astype(np.uint32)
    hit_counts.reshape(-1)[:] = (hi & 0xFFFFFFFF).astype(np.uint32)


def publish(pass_counts, hit_counts, min_pass=2, occ_num=1, occ_den=10):
    """The int8 grid of the two planes, integers only (Python's are unbounded: no product overflows)."""
    p, h = pass_counts.reshape(-1), hit_counts.reshape(-1)
    out = np.empty(len(p), np.int8)
    for i in range(len(p)):
        out[i] = -1 if int(p[i]) < min_pass else (100 if int(h[i]) * occ_den >= int(p[i]) * occ_num else 0)
    return out.reshape(pass_counts.shape)


def run_case(case, rnd=c_round, pass_counts=None, hit_counts=None):
    """(pass, hit, trace) of a case on zeroed planes (or on the given ones, which are not modified)."""
    shape = (case["rows"], case["cols"])
    pa = np.zeros(shape, np.uint32) if pass_counts is None else pass_counts.copy()
    hi = np.zeros(shape, np.uint32) if hit_counts is None else hit_counts.copy()
    trace = []
    integrate(case["scans"], case["lens"], case["poses"], case["cols"], case["rows"], case["resol"], case["range_max"], pa, hi, rnd, trace)
    return pa, hi, trace


# ---- the classes -----------------------------------------------------------------------------------------------------------------------
SCAN_LENGTHS = (1, 63, 64, 65, 360, 1025)
OCTANTS = ["octant_%s%s_%s" % ("+-"[sx], "+-"[sy], major) for sx in (0, 1) for sy in (0, 1) for major in ("x", "y")]
AXES = ["axis_+x", "axis_-x", "axis_+y", "axis_-y"]
BEAM_SKIPS = ["beam_nan_range", "beam_nonpos_range", "beam_inf_range", "beam_bad_angle"]
SCAN_SKIPS = ["scan_nonfinite", "scan_sentinel", "scan_far"]
CLASSES = (OCTANTS + AXES + ["diagonal", "n_zero", "ends_outside", "enters_from_outside", "wholly_outside", "range_at_max_hits",
                             "range_one_ulp_above_max", "len_zero", "len_is_stride", "two_scans_share_a_cell", "half_way"] +
           BEAM_SKIPS + SCAN_SKIPS + ["scan_len_%d" % n for n in SCAN_LENGTHS])


def is_half(v):
    return math.isfinite(v) and abs(v - math.trunc(v)) == 0.5


def classes_of(case, trace):
    """The classes a case reaches, from its trace."""
    got = set()
    by_scan = {}
    for t in trace:
        if t["skip"]:
            got.add(t["skip"])
            continue
        dx, dy = t["x1"] - t["x0"], t["y1"] - t["y0"]
        n, m = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
        if n == 0:
            got.add("n_zero")
        elif m == n:
            got.add("diagonal")
        elif m == 0:
            got.add("axis_%s%s" % ("+-"[(dx or dy) < 0], "x" if dx else "y"))
        else:
            got.add("octant_%s%s_%s" % ("+-"[dx < 0], "+-"[dy < 0], "x" if abs(dx) > abs(dy) else "y"))
        ins = t["inside"]
        if ins[0] and not ins[-1]:
            got.add("ends_outside")
        if not ins[0] and ins.any():
            got.add("enters_from_outside")
        if not ins.any():
            got.add("wholly_outside")
        if t["range"] == case["range_max"]:
            got.add("range_at_max_hits")
            assert t["hits"]
        if t["range"] == np.nextafter(case["range_max"], np.inf):
            got.add("range_one_ulp_above_max")
            assert not t["hits"]
        if any(is_half(v) for v in t["raw"]):
            got.add("half_way")
        cells = t["cells"][ins]
        by_scan.setdefault(t["scan"], set()).update(map(tuple, cells.tolist()))
    sets = list(by_scan.values())
    if any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets))):
        got.add("two_scans_share_a_cell")
    stride = case["scans"].shape[1]
    for i, ln in enumerate(case["lens"]):
        if ln == 0:
            got.add("len_zero")
        if ln == stride:
            got.add("len_is_stride")
        if ln in SCAN_LENGTHS and scan_skip(case["poses"][i]) is None:
            got.add("scan_len_%d" % ln)
    return got


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
def make_case(name, cols, rows, resol, range_max, beams, poses, stride=None, capacity=1024):
    """beams: per scan a list of (range, angle); stride: the pitch (default: the longest scan, at least 1)."""
    assert cols <= MAX_COLS and rows <= MAX_ROWS
    stride = stride or max(1, max(len(b) for b in beams))
    scans = np.zeros((len(beams), stride, 2))
    for i, b in enumerate(beams):
        if len(b):
            scans[i, :len(b)] = np.asarray(b, np.float64).reshape(-1, 2)
    return dict(name=name, cols=cols, rows=rows, resol=float(resol), range_max=float(range_max), scans=scans,
                lens=np.array([len(b) for b in beams], np.int32), poses=np.asarray(poses, np.float64).reshape(-1, 3), capacity=capacity)


def random_scan(rng, n, range_hi=3.0):
    b = np.stack([rng.uniform(0.05, range_hi, n), rng.uniform(-math.pi, math.pi, n)], 1)
    if n >= 8:                                   # a few readings no map takes
        b[rng.integers(0, n, max(1, n // 40)), 0] = np.nan
        b[rng.integers(0, n, max(1, n // 40)), 0] = -rng.uniform(0, 1)
    return b


def campaign():
    """The cases, deterministic."""
    cases = []
    rng = np.random.default_rng(20250607)
    deg = math.pi / 180
    # the eight octants, the four axes, exact diagonals, n = 0: three poses each
    for v, (px, py, ang) in enumerate([(30.0, 23.0, 0.0), (20.3, 11.6, 37.0), (41.7, 30.2, -171.5)]):
        octs = [(0.45 + 0.1 * v, (22.5 + 45 * k) * deg - ang * deg) for k in range(8)]
        cases.append(make_case("octants%d" % v, 61, 47, 0.05, 2.0, [octs], [(px, py, ang)]))
        ipx, ipy = round(px), round(py)
        axes = [(0.4 + 0.15 * v, k * math.pi / 2) for k in range(4)]
        cases.append(make_case("axes%d" % v, 61, 47, 0.05, 2.0, [axes], [(ipx, ipy, 0.0)]))
        diag = [((3 + 2 * v + k) * math.sqrt(2.0) * 0.05, (45 + 90 * k) * deg) for k in range(4)]
        cases.append(make_case("diagonals%d" % v, 61, 47, 0.05, 2.0, [diag], [(ipx, ipy, 0.0)]))
        tiny = [(0.004 + 0.003 * k, 0.7 * k + v) for k in range(5)]
        cases.append(make_case("n_zero%d" % v, 33 + v, 29 - v, 0.05, 2.0, [tiny], [(ipx % 29, ipy % 23, 10.0 * v)]))
    # rays that end outside, start outside and enter, stay outside
    for v in range(3):
        fan = [(1.5 + 0.2 * v, k * 2 * math.pi / 24 + 0.01 * v) for k in range(24)]
        cases.append(make_case("ends_outside%d" % v, 31 + 5 * v, 23 + 3 * v, 0.05, 4.0, [fan], [(15.2 + v, 11.4 + v, 3.0 * v)]))
        inward = [(1.2 + 0.1 * k, (-20 + 5 * k) * deg) for k in range(9)]
        cases.append(make_case("enters%d" % v, 40, 30 + v, 0.05, 4.0, [inward, inward], [(-6.4 - v, 14.0 + v, 0.0), (12.0 + v, -5.5, 90.0)]))
        away = [(0.8 + 0.05 * k, (160 + 5 * k) * deg) for k in range(9)]
        cases.append(make_case("outside%d" % v, 40, 30, 0.05, 4.0, [away, inward], [(-9.0 - v, 15.0, 0.0), (300.0 + v, 200.0, 0.0)]))
    # the cut at range_max: exactly at it (a hit) and one ulp above (a pass without a hit)
    for v, rmax in enumerate([1.0, 0.73, 1.9]):
        b = [(rmax, 0.3 + v), (float(np.nextafter(rmax, np.inf)), 0.3 + v), (rmax, 2.0 + v), (float(np.nextafter(rmax, np.inf)), -1.0 - v),
             (3 * rmax, 1.1), (0.5 * rmax, 1.1)]
        cases.append(make_case("range_max%d" % v, 61, 47, 0.05, rmax, [b], [(30.4, 22.7, 12.0 * v)]))
    # readings and poses that are skipped
    for v in range(3):
        good = (0.6 + 0.1 * v, 0.5)
        b = [good, (math.nan, 0.1), (0.0, 0.2), (-0.7, 0.3), (-math.inf, 0.4), (math.inf, 0.5), (0.6, math.nan), (0.6, math.inf),
             (0.6, -math.inf), (-0.0, 0.0), good]
        cases.append(make_case("skipped_beams%d" % v, 47, 41, 0.05, 2.0, [b], [(20.0 + v, 19.0, 5.0 * v)]))
        poses = [(math.nan, 10, 0), (10, math.inf, 0), (10, 10, math.nan), (10, 10, -math.inf), (-1.0, 12, 0), (-1.00005, 12, 3),
                 (-0.99995, 12, 3), (1048577.0, 3, 0), (5, -1048576.5, 0), (-0.9998, 12.0, 0.0), (21.0 + v, 17.0, 0.0)]
        cases.append(make_case("skipped_scans%d" % v, 47, 41, 0.05, 2.0, [[good, (0.9, 2.0 + v)]] * len(poses), poses))
    # len = 0, len = stride, and the scan lengths around the wavefront and the workgroup
    for v in range(3):
        cases.append(make_case("len_zero%d" % v, 29, 31, 0.05, 2.0, [[], random_scan(rng, 5), []], [(14, 15, 0), (13.5, 12.2, 40.0 * v), (3, 3, 0)],
                               stride=5 + v))
    for n in SCAN_LENGTHS:
        for v in range(3 if n != 1025 else 1):
            beams = [random_scan(rng, n), random_scan(rng, max(1, n // 2))]
            cases.append(make_case("len%d_%d" % (n, v), 61 - v, 47 - 2 * v, 0.05, 2.0, beams,
                                   [(rng.uniform(5, 55), rng.uniform(5, 40), rng.uniform(-180, 180)), (rng.uniform(5, 55), rng.uniform(5, 40), 0.0)],
                                   stride=n + (0 if v == 0 else 7 * v), capacity=1024 if n <= 1024 else 2048))
    # two scans whose rays cross
    for v in range(3):
        a = [(1.0 + 0.1 * v, 0.0), (1.0, 0.05)]
        b = [(1.0 + 0.1 * v, math.pi / 2), (1.0, math.pi / 2 + 0.05)]
        cases.append(make_case("crossing%d" % v, 50, 40, 0.05, 2.0, [a, b], [(10.0, 20.0 + v, 0.0), (20.0, 10.0 + v, 0.0)]))
    # coordinates exactly half-way between two cells, where round and rint part: in the pose, and in the end point (c = 1 exactly at
    # th = 0, and rr / mapResol = 4.5 exactly at a resolution of 0.5)
    for v in range(3):
        b = [(2.25, 0.0), (1.0, math.pi / 2), (2.0, 0.0)]
        poses = [(10.0 + 2 * v, 8.0, 0.0), (12.5 + 2 * v, 6.5, 0.0), (-2.5, 3.0 + v, 0.0)]
        cases.append(make_case("half_way%d" % v, 40, 30, 0.5, 8.0, [b] * 3, poses))
    return cases
