"""Seeded, deterministic lidar scans and parameter sets for the scan-side parity campaign (shared by the CPU and GPU tests).

FeatureScan (k_rdp.hip) takes its thresholds and its map_param once per launch, so the campaign is a handful of GROUPS: one
parameter set each, a few hundred scans each, every scan length of LENGTHS in every group.  The families are built to reach what a
lidar log never does: the cluster that wraps from the last reading to the first, a first cluster that is dropped before that wrap,
ranges on and beside every step of getThresholdDeltaDist and beside 9, exactly vertical and 0/0 chords, repeated readings, more
than 64 chords, pixel columns that are all negative, lines on pixel row / column 0.

The reference's domain is kept: finite ranges in (0, 60] m, resolution >= 0.025, region_point_limit >= 1.  The raster loops of
k_rdp run once per pixel of a line's extent, so every group bounds its ranges by RMAX_PIXELS * resolution: the image stays below
~1000 px (check_bounds() asserts <= 5000 on the oracle's result before anything goes to a GPU).

The second half builds scan-to-map matching cases (match_cases): FeatureScan's own integer-coordinate lines against the fixture
maps' lines and mapCache, and small hand-made frames that sit exactly on the edges of thread_ScanToMapMatch.
"""
import numpy as np

LENGTHS = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 359, 360, 361, 1023, 1024)
LOG_MAP_PARAM = (1377, 428, 0.025, -4.43187, -5.49357)              # data/mapParam.txt
DELTA_STEPS = np.array([0.3, 0.5, 0.8, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])   # getThresholdDeltaDist, myRDP.cpp:347-368
DELTA_VALS = np.array([0.02, 0.05, 0.11, 0.17, 0.6, 0.7, 0.85, 0.9, 1.0, 1.1])
RMAX_PIXELS = 480                                                    # ranges <= RMAX_PIXELS * resolution (and <= 60 m)
PTS_CAP = 4096                                                       # what the GPU campaign stores per scan; check_bounds() holds the generator to it
PTS_CAP_SMALL = 64                                                   # the truncation test's
STRIDE = 1024
IMAGE_LIMIT = 5000

# (name, map_param, region_point_limit, thre_line, line_dist_thre_m).  Origins: the log's own; ordinary; beyond every reading (all
# pixel columns / rows negative, so maxX / maxY stay at their initial 0); on a wall of the room (a line on absolute pixel row / column 0).
GROUPS = (
    ("log_defaults", LOG_MAP_PARAM, 3, 0.08, 0.5),
    ("log_fine", LOG_MAP_PARAM, 1, 0.01, 0.0),
    ("res05", (800, 800, 0.05, -20.0, -20.0), 2, 0.08, 0.0),
    ("all_negative", (10, 10, 0.1, 70.0, 65.0), 3, 0.3, 2.0),
    ("neg_columns", (10, 10, 0.1, 70.0, -30.0), 8, 0.01, 0.5),
    ("edge_coarse", (400, 300, 0.2, -4.0, -3.0), 1, 0.08, 0.0),
    ("edge_fine", (400, 300, 0.025, -4.0, -3.0), 2, 0.3, 0.5),
    ("coarse", (500, 500, 0.2, -40.0, -40.0), 8, 0.08, 2.0),
)
REPS = 45                                                            # scans per length and group


def thre_delta(r):
    return DELTA_VALS[np.searchsorted(DELTA_STEPS, r, side="left")]


def _rmax(res):
    return min(60.0, RMAX_PIXELS * res)


# ---- ray casting ------------------------------------------------------------------------------------------------------------
def _cast(ang, rect, boxes):
    """Range of each ray from the origin to the rectangle (x0, x1, y0, y1) around it, or to the nearest axis-aligned box in front."""
    c, s = np.cos(ang), np.sin(ang)
    x0, x1, y0, y1 = rect
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(c > 0, x1 / c, np.where(c < 0, x0 / c, np.inf))
        ty = np.where(s > 0, y1 / s, np.where(s < 0, y0 / s, np.inf))
        t = np.minimum(tx, ty)
        for bx0, bx1, by0, by1 in boxes:
            ax, bx = bx0 / c, bx1 / c
            ay, by = by0 / s, by1 / s
            lo = np.maximum(np.minimum(ax, bx), np.minimum(ay, by))
            hi = np.minimum(np.maximum(ax, bx), np.maximum(ay, by))
            hit = (hi >= lo) & (lo > 0)
            t = np.where(hit & (lo < t), lo, t)
    return t


def _room(rng, res, origin, corridor=False):
    rm = _rmax(res)
    a = rng.uniform(0.2, 0.6, 4) * rm
    if corridor:
        a[2:] = rng.uniform(0.05, 0.1, 2) * rm
    rect = [-a[0], a[1], -a[2], a[3]]
    if origin is not None:                                           # walls through the middle of absolute pixel column 0 and row 0
        rect[0], rect[2] = origin[0] + res / 2, origin[1] + res / 2
    boxes = []
    for _ in range(int(rng.integers(0, 4))):
        cx, cy = rng.uniform(rect[0], rect[1]), rng.uniform(rect[2], rect[3])
        w, h = rng.uniform(0.03, 0.15, 2) * rm
        if abs(cx) - w > 0.02 * rm or abs(cy) - h > 0.02 * rm:       # not around the lidar
            boxes.append((cx - w, cx + w, cy - h, cy + h))
    return rect, boxes


def _finish(rng, r, ang, res, noise):
    # a tenth of a millimetre of jitter in every range: the two readings beside a corner, or two mirror-image peaks, are then not
    # within an ulp of the same distance from a chord, where which one is the farthest would depend on the last bit of sin / cos
    r = r + 1e-4 * rng.uniform(-1, 1, len(r))
    if noise > 0:
        r = r + noise * rng.standard_normal(len(r))
    return np.stack([np.clip(r, 0.05, _rmax(res)), ang], 1)


def fam_room(rng, n, g, full, noise, corridor=False):
    res = g[1][2]
    origin = (g[1][3], g[1][4]) if g[0].startswith("edge") else None
    rect, boxes = _room(rng, res, origin, corridor)
    if full:
        ang = -np.pi + 2 * np.pi * np.arange(n) / n + rng.uniform(0, 0.01)
    else:
        fov = rng.uniform(0.5, 1.5) * np.pi
        ang = rng.uniform(-np.pi, np.pi) + np.linspace(-fov / 2, fov / 2, n)
    return _finish(rng, _cast(ang, rect, boxes), ang, res, noise * g[3])


def fam_wrap_drop(rng, n, g):
    """A full scan whose first cluster is shorter than region_point_limit (a post right behind it) and whose last cluster runs into
    the first reading: RegionSegmentation overwrites cs[0] of a LATER cluster (myRDP.cpp:361-365)."""
    sc = fam_room(rng, n, g, True, 0.0)
    j = int(rng.integers(0, g[2])) + 1                               # the first gap over the threshold is behind reading j - 1 < limit
    if j < n:
        sc[j, 0] *= 0.4
    return sc


def fam_delta_steps(rng, n, g):
    """Readings on and one ulp beside each step of getThresholdDeltaDist, each followed by a reading whose distance lies between the
    two thresholds the step separates: which side of the step the range is on decides the break.  Runs of equal range in between."""
    rm = _rmax(g[1][2])
    steps = DELTA_STEPS[DELTA_STEPS < rm - 1.2]
    r = np.empty(n)
    i = 0
    while i < n:
        k = int(rng.integers(0, len(steps)))
        s = steps[k]
        v = (np.nextafter(s, 0), s, np.nextafter(s, 9))[int(rng.integers(0, 3))]
        run = int(rng.integers(1, 6))
        r[i:i + run] = v
        i += run
        if i < n:
            r[i] = v + 0.5 * (DELTA_VALS[k] + DELTA_VALS[k + 1])
            i += 1
    ang = rng.uniform(-3, 2) + 1e-4 * np.arange(n)
    return np.stack([r, ang], 1)


def _filler(n, a0):
    """n isolated readings (alternately 3 m and 5 m away, opposite a0): every one a cluster of its own, which is dropped."""
    return np.stack([np.where(np.arange(n) % 2 == 0, 3.0, 5.0), a0 + np.pi + 1e-3 * np.arange(n)], 1)


def fam_nine(rng, n, g, variant):
    """One straight cluster with its middle reading sticking out by 2 * thre_line at a range of 9 (variant 0), one ulp below (1) or
    one ulp above (2): at 9 and below the reading splits the chord, above it the threshold is 9 times larger and it does not."""
    limit, tl = g[2], g[3]
    m = max(limit, 5)
    if n < 2 * m + 2 or _rmax(g[1][2]) < 10:
        return fam_room(rng, n, g, False, 0.0)
    a0 = rng.uniform(-1.0, 1.0)
    r9 = (9.0, np.nextafter(9.0, 0), np.nextafter(9.0, 10))[variant]
    D = 9.0 - 2 * tl
    th = np.arange(-m, m + 1) * (3.0 / 9.0 / m)                       # half a chord of ~3 m: longer than every line_dist_thre_m
    r = D / np.cos(th)
    r[m] = r9
    cl = np.stack([r, a0 + th], 1)
    return np.concatenate([cl, _filler(n - len(cl), a0)])


def fam_symmetric(rng, n, g, bumpy):
    """Angles symmetric about 0 with ranges symmetric in them: cos(-a) == cos(a) exactly, so the cluster's chord is exactly vertical
    (k = +-inf, every distance NaN, nothing is split: myRDP.cpp:245-257) and so is the pixel line."""
    rm = _rmax(g[1][2])
    rho = rng.uniform(2.0, min(5.0, 0.5 * rm))
    th = np.linspace(-1.2, 1.2, n) if n > 1 else np.zeros(1)
    th = (th - th[::-1]) / 2                                         # exactly antisymmetric
    r = rho * (1 + (0.1 * np.cos(3 * th) if bumpy else np.zeros(n)))
    r = (r + r[::-1]) / 2
    return np.stack([r, th], 1)


def fam_repeats(rng, n, g):
    """Runs of identical readings (zero gap; a cluster whose ends coincide has a 0/0 chord) and runs that come back to their first reading."""
    out = np.empty((n, 2))
    i = 0
    far = False
    while i < n:
        run = int(rng.integers(2, 13))
        r0 = (5.0 if far else 3.0) + rng.uniform(0, 0.2)
        a0 = rng.uniform(-3, 3)
        blk = np.tile([r0, a0], (run, 1))
        if run > 3 and rng.integers(0, 2):
            blk[1:-1, 0] += rng.uniform(0, 0.15, run - 2)
            blk[1:-1, 1] += rng.uniform(0, 0.02, run - 2)
        out[i:i + run] = blk[:n - i]
        i += run
        far = not far
    return out


def fam_zigzag(rng, n, g):
    """An arc whose first <= 300 readings alternate in range: every one of them becomes a split point where thre_line allows it."""
    rm = _rmax(g[1][2])
    rho = rng.uniform(3.0, min(5.0, 0.45 * rm))
    ang = rng.uniform(-3, 0) + np.arange(n) * min(0.003, 3.0 / max(n, 1))
    r = np.full(n, rho)
    z = min(n, 300)
    per = int(rng.integers(2, 5))
    r[:z] += np.where(np.arange(z) % per == 0, 0.12, 0.0)
    return _finish(rng, r, ang, g[1][2], 0.0)


def fam_tie(rng, n, g):
    """Two readings EXACTLY as far from their cluster's chord, whatever the last bit of sin / cos: the chord lies on the x axis
    (angle 0: k = 0, d = 0, the distance is |py|) and the readings are (r, +a) and (r, -a).  The reference takes the first; taking
    the second gives other lines: it is just beside the chord's start, so the first reading is then not split off any more."""
    limit, tl = g[2], g[3]
    m = max(limit, 3)
    if n < m + 5:
        return fam_room(rng, n, g, False, 0.0)
    h, dx = 1.5 * tl, 0.2 * tl
    rp = np.hypot(5.5 + dx, h)
    a = np.arcsin(h / rp)
    cl = [(5.5, 0.0), (rp, a), (rp, -a)] + [(5.9 + 0.3 * j, 0.0) for j in range(m)]
    return np.concatenate([np.array(cl), _filler(n - len(cl), 0.0)])


def _family(k, rng, n, g):
    k %= 15
    if k == 0: return "room_full", fam_room(rng, n, g, True, 0.0)
    if k == 1: return "room_full_noise", fam_room(rng, n, g, True, 0.3)
    if k == 2: return "room_partial", fam_room(rng, n, g, False, 0.0)
    if k == 3: return "room_partial_noise", fam_room(rng, n, g, False, 1.0)
    if k == 4: return "corridor", fam_room(rng, n, g, True, 0.0, corridor=True)
    if k == 5: return "wrap_drop", fam_wrap_drop(rng, n, g)
    if k == 6: return "delta_steps", fam_delta_steps(rng, n, g)
    if k in (7, 8, 9): return "nine_%d" % (k - 7), fam_nine(rng, n, g, k - 7)
    if k == 10: return "symmetric", fam_symmetric(rng, n, g, False)
    if k == 11: return "symmetric_bumpy", fam_symmetric(rng, n, g, True)
    if k == 12: return "repeats", fam_repeats(rng, n, g)
    if k == 13: return "zigzag", fam_zigzag(rng, n, g)
    return "tie", fam_tie(rng, n, g)


def campaign(reps=REPS):
    """[dict(name, map_param, limit, thre_line, line_dist, scans=[float64 [len, 2]], tags=[family name])], one per GROUPS entry.
    The three nine_* scans of one (length, repetition) share their random draws: they differ in the one range only."""
    out = []
    for gi, g in enumerate(GROUPS):
        scans, tags = [], []
        for li, n in enumerate(LENGTHS):
            for rep in range(reps):
                k = rep % 15
                seed = (gi, li, rep - (k - 7) if k in (7, 8, 9) else rep)
                tag, sc = _family(k, np.random.default_rng(seed), n, g)
                assert sc.shape == (n, 2) and np.isfinite(sc).all() and (sc[:, 0] > 0).all() and (sc[:, 0] <= 60).all()
                scans.append(np.ascontiguousarray(sc)); tags.append(tag)
        out.append(dict(name=g[0], map_param=g[1], limit=g[2], thre_line=g[3], line_dist=g[4], scans=scans, tags=tags))
    return out


def reference(oracle, group, lib, idx=None):
    """The oracle's FeatureScan of every scan of a group (or of those in idx), with room for every pixel."""
    return [oracle.feature_scan(group["scans"][i], group["map_param"], group["limit"], group["thre_line"], group["line_dist"],
                                pts_cap=65536, _lib=lib) for i in (range(len(group["scans"])) if idx is None else idx)]


def check_bounds(refs):
    """What the generator promises about its scans, asserted on the oracle's results before anything is sent to a GPU."""
    for r in refs:
        assert max(r["im_size"]) <= IMAGE_LIMIT and len(r["pts"]) <= PTS_CAP, (r["im_size"], len(r["pts"]))


def pack(scans, stride=STRIDE, fill=0.0):
    """scans -> (float64 [n, stride, 2] with `fill` behind each scan's readings, int32 lens)."""
    out = np.full((len(scans), stride, 2), fill, np.float64)
    lens = np.zeros(len(scans), np.int32)
    for i, s in enumerate(scans):
        out[i, :len(s)] = s; lens[i] = len(s)
    return out, lens


def clusters(scan, limit):
    """RegionSegmentation's walk (myRDP.cpp:297-330) restated for counting what the campaign reaches:
    (number of clusters, the last cluster wraps into cs[0], the first cluster had been dropped before that)."""
    r, a = scan[:, 0], scan[:, 1]
    px, py = r * np.cos(a), r * np.sin(a)
    brk = np.hypot(px - np.roll(px, -1), py - np.roll(py, -1)) > thre_delta(r)
    cells, start, first_dropped = 0, 0, False
    for i in np.nonzero(brk)[0]:
        if i - start >= limit:
            cells += 1
        elif start == 0:
            first_dropped = True
        start = i + 1
    wrapped = cells > 0 and not brk[-1]
    return cells, wrapped, wrapped and first_dropped


# ---- what is compared, and how ---------------------------------------------------------------------------------------------------
LINE_FIELDS = ("k", "b", "dx", "dy", "x1", "y1", "x2", "y2", "len", "orient", "_pad")


def bits(a):
    """float64 array -> its bit patterns with every NaN mapped to one pattern (IEEE 754 leaves the sign and payload of a generated
    NaN to the implementation: x86 SSE gives 0xFFF8..., other hardware 0x7FF8...); everything else, -0.0 included, stays as it is."""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b


def line_diffs(got, ref):
    """Names of the line-record fields that differ bit for bit (NaN == NaN, see bits())."""
    bad = []
    for f in LINE_FIELDS:
        g, r = got[f], ref[f]
        same = np.array_equal(bits(g), bits(r)) if g.dtype == np.float64 else np.array_equal(g, r)
        if not same:
            bad.append(f)
    return bad


# ---- scan-to-map matching cases --------------------------------------------------------------------------------------------------
LINE_DTYPE = np.dtype([("k", "f8"), ("b", "f8"), ("dx", "f8"), ("dy", "f8"), ("x1", "f8"), ("y1", "f8"),
                       ("x2", "f8"), ("y2", "f8"), ("len", "f8"), ("orient", "i4"), ("_pad", "i4")])
FREE = (-1.0, -1.0, 0.0)                                             # lastPose of the first frame: no distance gate (myFA.cpp:330)


def mk_lines(segs):
    out = np.zeros(len(segs), LINE_DTYPE)
    for o, (x1, y1, x2, y2) in zip(out, segs):
        o["x1"], o["y1"], o["x2"], o["y2"] = x1, y1, x2, y2
    return out


def line_direction(sx, sy, ex, ey):
    """NormalizedLineDirection (myFA.cpp:272-305) restated for checking which branch a case takes: (angle, branch, fix-up)."""
    if sx == ex and sy != ey:
        a, br = (90.0 if sy < ey else -90.0), "vertical"
    elif sx != ex and sy == ey:
        a, br = (0.0 if sx < ex else 180.0), "horizontal"
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            a, br = float(np.degrees(np.arctan(np.float64(ey - sy) / np.float64(ex - sx)))), "atan"
    if a < 0 and sx > ex: return a + 180, br, "+180"
    if a > 0 and sx > ex: return a - 180, br, "-180"
    return a, br, ""


def candidate_ends(ml, sl, i):
    """The start and end points matching i = 1..4 gives the map line and the scan line (myFA.cpp:205-249)."""
    m = (ml["x2"], ml["y2"], ml["x1"], ml["y1"]) if i >= 3 else (ml["x1"], ml["y1"], ml["x2"], ml["y2"])
    s = (sl["x2"], sl["y2"], sl["x1"], sl["y1"]) if i in (2, 4) else (sl["x1"], sl["y1"], sl["x2"], sl["y2"])
    return tuple(float(v) for v in m), tuple(float(v) for v in s)


def case(name, map_cache, map_lines, scan_lines, pts, lidar, last=FREE, pairs=None, z_occ=1.0, max_esti_dist=60.0, **expect):
    if pairs is None:
        pairs = [(i, j) for i in range(len(map_lines)) for j in range(len(scan_lines))]
    return dict(name=name, map_cache=np.ascontiguousarray(map_cache, np.float64), map_lines=map_lines, scan_lines=scan_lines,
                pts=np.ascontiguousarray(pts, np.float64).reshape(-1, 3), lidar=lidar, last=last,
                pairs=np.ascontiguousarray(pairs, np.int32).reshape(-1, 2), z_occ=z_occ, max_esti_dist=max_esti_dist, expect=expect)


def case_args(c):
    return (c["map_cache"], c["map_lines"], c["scan_lines"], c["pts"], c["lidar"], c["last"], c["pairs"], c["z_occ"], c["max_esti_dist"])


def _pts(xy):
    p = np.zeros((len(xy), 3))
    if len(xy):
        p[:, :2] = xy
    return p


# every kind of line NormalizedLineDirection tells apart, in both directions; the last three have a slope so small that
# atand(k) -+ 180 rounds to exactly -+180, the only way to an angDiff of +-360 (a right-to-left horizontal line gets 180 and then
# the fix-up for positive angles: 0)
_TINY = 1e-300
DIRECTION_SEGS = [(2, 5, 12, 5), (12, 7, 2, 7), (6, 2, 6, 11), (8, 11, 8, 2), (3, 3, 3, 3), (1, 1, 9, 7), (1, 9, 9, 2), (10, 0, 0, -_TINY), (0, 0, 10, _TINY), (10, 0, 0, _TINY)]


def edge_cases():
    """Hand-made frames on the edges of thread_ScanToMapMatch.  expect: what the oracle's result must show before the GPU is asked."""
    rng = np.random.default_rng(2024)
    out = []
    # 1. directions: all three branches of line_direction, both sign fix-ups, angDiff of exactly +-180 and +-360 before the wrap
    mc = rng.integers(0, 65, (30, 40)) / 64.0                        # dyadic, some cells exactly z_occ_max_dis = 1.0
    ml = mk_lines(DIRECTION_SEGS)
    sl = mk_lines([(x1 + 1, y1 + 2, x2 + 1, y2 + 2) for x1, y1, x2, y2 in DIRECTION_SEGS[:7]] + [(11, 0, 1, -_TINY), (1, 0, 11, _TINY), (11, 0, 1, _TINY)])
    pts17 = _pts(rng.integers(0, 25, (17, 2)))
    out.append(case("directions", mc, ml, sl, pts17, (5.0, 5.0, 0.0), directions=True))
    for n in (0, 1, 7, 8, 9, 17):                                    # the 8-point batches of the point loop and their tail
        out.append(case("points_%d" % n, mc, ml, sl, pts17[:n], (5.0, 5.0, 0.0), n_points=n))
    all_pairs = [(i, j) for i in range(len(ml)) for j in range(len(sl))]
    for n in (1, 15, 16, 17, 1000):                                  # candidates: 4 per pair, 64 to a wavefront
        out.append(case("pairs_%d" % n, mc, ml, sl, pts17, (5.0, 5.0, 0.0), pairs=[all_pairs[k % len(all_pairs)] for k in range(n)], n_pairs=n))
    # the frames below use matching 1 of ONE pair with angDiff = 0 exactly (cosd = 1, sind = 0): the rotation is the shift by
    # (msx - ssx, msy - ssy), exact in binary, so what is inside the map and what its mapCache cell holds is known by construction
    ident = mk_lines([(0, 0, 10, 0)])
    zeros = np.zeros((20, 20))
    inside = [(k % 5 + 1, k // 5 + 1) for k in range(20)]
    # 2. numValidPoint against 0.7 * numAllPoint: 7 of 10 (0.7 * 10 == 7.0 in binary64: accepted), 9 of 13 (9 < 9.1: rejected)
    out.append(case("seventy_exact", zeros, ident, ident, _pts(inside[:7] + [(-5, 0), (0, -5), (99, 0)]), (5.0, 5.0, 0.0), score0=3.0))
    out.append(case("seventy_under", zeros, ident, ident, _pts(inside[:9] + [(-5, 0), (0, -5), (99, 0), (0, 99)]), (5.0, 5.0, 0.0), score0=np.inf))
    # 3. points rotated off each of the four edges, onto -0.5 (rounds away from zero: outside) and just inside
    rows, cols = 16, 24
    mc3 = (1.0 + np.arange(rows * cols).reshape(rows, cols)) / 1024.0
    shift = mk_lines([(2, 3, 12, 3)])                                # rx = x + 2, ry = y + 3
    off = [(-3, 0), (22, 0), (0, -4), (0, 13), (-2.5, 0), (0, -3.5), (21.5, 0), (0, 12.5)]
    on = [(-2.25, 0), (21.25, 0), (0, -3.25), (0, 12.25)] + inside
    vals = [mc3[int(np.floor(y + 3 + 0.5)), int(np.floor(x + 2 + 0.5))] for x, y in on]
    n3 = len(off) + len(on)
    s3 = 0.0
    order = off[:4] + on[:2] + off[4:] + on[2:]
    for x, y in order:                                               # the reference's sum, term by term in point order
        if (x, y) in on:
            s3 += vals[on.index((x, y))]
    out.append(case("map_edges", mc3, shift, ident, _pts(order), (5.0, 5.0, 0.0), score0=s3 / len(on) + 10.0 * (n3 - len(on)) / n3))
    # 4. mapCache values equal to z_occ_max_dis count 10, one ulp below counts itself
    mc4 = np.full((20, 20), 0.5)
    mc4[1, 1:4] = 1.0
    mc4[2, 1:3] = np.nextafter(1.0, 0)
    p4 = [(1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (1, 3), (2, 3), (3, 3)]
    s4 = 0.0
    for x, y in p4:
        if mc4[y, x] < 1.0:
            s4 += mc4[y, x]
    out.append(case("z_occ", mc4, ident, ident, _pts(p4), (5.0, 5.0, 0.0), score0=(s4 + 30.0) / 8))
    # 5. lastPose exactly max_esti_dist from the rotated lidar position (7, 8): rejected ('<'); one ulp nearer: accepted
    out.append(case("max_dist_at", zeros, shift, ident, _pts(inside), (5.0, 5.0, 0.0), last=(7.0 - 60.0, 8.0, 0.0), score0=np.inf))
    out.append(case("max_dist_inside", zeros, shift, ident, _pts(inside), (5.0, 5.0, 0.0), last=(np.nextafter(7.0 - 60.0, 0), 8.0, 0.0), score0=0.0))
    return out


def feature_scan_match_cases(oracle, maps, maps_meta, lib):
    """FeatureScan's own output (integer end points: horizontal and vertical lines) for generated rooms against a fixture map's
    lines and mapCache, every (map line, scan line) pair up to 1000."""
    m = maps["aisle1"]; res = maps_meta["aisle1"]["res"]
    map_cache = oracle.map_cache(m.copy(), res)
    map_lines = oracle.lsd(m.copy())["lines"]
    out = []
    for g in campaign(reps=15):
        if g["name"] not in ("log_defaults", "res05", "edge_coarse"):
            continue
        idx = [i for i, t in enumerate(g["tags"]) if t in ("room_full", "corridor") and len(g["scans"][i]) in (359, 360, 361)]
        for i, r in zip(idx, reference(oracle, g, lib, idx)):
            if len(r["lines"]) == 0 or len(r["pts"]) == 0:
                continue
            pairs = [(a, b) for a in range(len(map_lines)) for b in range(len(r["lines"]))][:1000]
            out.append(case("fs_%s_%d" % (g["name"], i), map_cache, map_lines, r["lines"], r["pts"], (r["lidar_pos"][0], r["lidar_pos"][1], 0.0),
                            pairs=pairs, feature_scan=True))
    return out
