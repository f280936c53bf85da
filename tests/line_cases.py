"""The line-record campaign: small deterministic maps that drive K5 (k_lines.hip: accepted rectangles -> structLinesInfo records and
the lineIm raster) and the batch compaction (k_scan_counts / k_compact_lines) where the fixtures do not go, and a plain numpy
restatement of myLSD.cpp:280-368 from the four end points.  tests/test_line_cases_cpu.py shows that the restatement equals the
oracle bit for bit and that every class below is reached; tests/test_line_cases_gpu.py runs the cases on the device.  No GPU and no
oracle is needed to import this module.

A class is a predicate on the RECORDS of the correctly rounded oracle (oracle.lib_cr()) and on the image's shape, never on what a
generator meant to draw: classes_of() is the only judge.

k NaN (x1 == x2 and y1 == y2, a rectangle of no length) is NOT reached by a map: none of the four kinds below nor of the aimed shapes
gave such a record, and tools/line_probe.py counts none over further random maps.  Neither is a sample that lies exactly half-way
between two cells (where C's round and rint part).  Both reach K5 as hand-made end points instead: HAND_RECS below, through
lsd_debug_lines on the device (test f) and through the restatement against K5's statement order here (test_line_cases_cpu.py)."""
import numpy as np

INT_MIN = -2 ** 31
CLASSES = ("k_inf", "k_zero", "tie", "orient_neg", "orient_pos", "below_0", "beyond", "row0_col0", "over_64", "over_128",
           "over_4_lines", "over_8_lines", "no_line")
NEED = {c: 3 for c in CLASSES}                              # cases that must reach each class ...
NEED["over_128"] = NEED["over_8_lines"] = 1                 # ... (the two that need aimed shapes: one)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _cvt(v):
    """(int) of a double as x86 does it (cvttsd2si): truncation, INT_MIN for NaN and for what does not fit."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
        ok = np.isfinite(t) & (t >= INT_MIN) & (t < 2.0 ** 31)
        return np.where(ok, np.where(ok, t, 0.0).astype(np.int64), INT_MIN)


def _round(v):
    """C's round(): to nearest, halves away from zero (v - trunc(v) is exact)."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
        return np.where(np.abs(v - t) >= 0.5, t + np.copysign(1.0, v), t)


def fields_from_endpoints(x1, y1, x2, y2):
    """k, b, len, orient of myLSD.cpp:289-295, :359, :366-367 for arrays of end points.  orient is the sign test on atand(k), which
    has the sign of k: -1 iff k < 0 (atan(-0.0) is -0.0, not below 0; NaN compares false)."""
    x1, y1, x2, y2 = (np.asarray(v, np.float64) for v in (x1, y1, x2, y2))
    with np.errstate(all="ignore"):
        k = (y2 - y1) / (x2 - x1)                                                          # :289
        b = (y1 + y2) / 2.0 - k * (x1 + x2) / 2.0                                          # :359
        ey, ex = y2 - y1, x2 - x1
        ln = np.sqrt(ey * ey + ex * ex)                                                    # :366
        orient = np.where(k < 0, -1, 1).astype(np.int32)                                   # :291-295
    return k, b, ln, orient


class Samples:
    """One record's walk of the longer axis (:297-342): xx, yy int64 (INT_MIN where the conversion overflows), along_x, inside (the
    bounds test of :325 / :337 passes), marked (inside and neither coordinate 0, :346 / :352)."""


def samples(x1, y1, x2, y2, rows, cols):
    x1, y1, x2, y2 = (np.float64(v) for v in (x1, y1, x2, y2))
    with np.errstate(all="ignore"):
        k = (y2 - y1) / (x2 - x1)
        if x1 > x2: xLow, xHigh = int(_cvt(np.floor(x2))), int(_cvt(np.ceil(x1)))            # :298-305
        else:       xLow, xHigh = int(_cvt(np.floor(x1))), int(_cvt(np.ceil(x2)))
        if y1 > y2: yLow, yHigh = int(_cvt(np.floor(y2))), int(_cvt(np.ceil(y1)))            # :306-313
        else:       yLow, yHigh = int(_cvt(np.floor(y1))), int(_cvt(np.ceil(y2)))
        xRang, yRang = np.abs(x2 - x1), np.abs(y2 - y1)                                    # :314
        s = Samples()
        s.along_x = bool(xRang > yRang)                                                    # :319
        if s.along_x:
            s.xx = np.arange(max(xHigh - xLow + 1, 0), dtype=np.int64) + xLow              # :322-324
            s.yy = _cvt(_round((s.xx.astype(np.float64) - x1) * k + y1))
        else:
            s.yy = np.arange(max(yHigh - yLow + 1, 0), dtype=np.int64) + yLow              # :334-336
            s.xx = _cvt(_round((s.yy.astype(np.float64) - y1) / k + x1))
    s.inside = (s.xx >= 0) & (s.xx < cols) & (s.yy >= 0) & (s.yy < rows)                   # :325 / :337
    s.marked = s.inside & (s.xx != 0) & (s.yy != 0)                                        # :346 / :352
    return s


def raster(lines, rows, cols):
    """lineIm (:215, :319-355) of the records' end points, in the records' order (marking is idempotent)."""
    im = np.zeros((rows, cols), np.uint8)
    for r in lines:
        s = samples(r["x1"], r["y1"], r["x2"], r["y2"], rows, cols)
        im[s.yy[s.marked], s.xx[s.marked]] = 255
    return im


def classes_of(lines, rows, cols):
    """The classes the records of one image reach -> {class: number of lines (1 for the per-image classes)}."""
    out = dict.fromkeys(CLASSES, 0)
    n = len(lines)
    out["no_line"] = int(n == 0)
    out["over_4_lines"], out["over_8_lines"] = int(n > 4), int(n > 8)
    for r in lines:
        x1, y1, x2, y2 = (float(r[f]) for f in ("x1", "y1", "x2", "y2"))
        out["k_inf"] += int(np.isinf(r["k"]))
        out["k_zero"] += int(r["k"] == 0)
        out["tie"] += int(abs(x2 - x1) == abs(y2 - y1))
        out["orient_neg"] += int(r["orient"] == -1)
        out["orient_pos"] += int(r["orient"] == 1)
        out["below_0"] += int(min(x1, y1, x2, y2) < 0)
        out["beyond"] += int(max(x1, x2) > cols - 1 or max(y1, y2) > rows - 1)
        s = samples(x1, y1, x2, y2, rows, cols)
        out["row0_col0"] += int(bool((s.inside & ~s.marked).any()))
        out["over_64"] += int(len(s.xx) > 64)
        out["over_128"] += int(len(s.xx) > 128)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------
FREE, OCC, UNKNOWN = 255, 1, 0                              # the loader's values; the detector turns 1 -> 255 and 255 -> 0 (:135-142)


class Case:
    def __init__(self, kind, name, m, sca):
        self.kind, self.name, self.sca = kind, name, float(sca)
        self.map = np.ascontiguousarray(m, np.uint8)
        self.map.setflags(write=False)

    @property
    def params(self):
        return dict(sca=self.sca)

    def __repr__(self):
        return "%s/%s@%g" % (self.kind, self.name, self.sca)


_REF = {}


def reference(case, oracle):
    """The correctly rounded oracle's answer for a case, computed once per process and read-only: lines (LINE_DTYPE, _pad == 0),
    lineIm, used (usedMap), w / h (the scaled size) and map (the input as the detector rewrites it in place)."""
    key = repr(case)
    if key not in _REF:
        m = case.map.copy()
        r = oracle.lsd(m, debug=True, _lib=oracle.lib_cr(), **case.params)
        d = r["dbg"]
        ref = dict(lines=r["lines"], lineIm=r["lineIm"], used=d.get("used"), w=d["w"], h=d["h"], map=m)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _free(rows, cols):
    return np.full((rows, cols), FREE, np.uint8)


def _bars():
    """One-pixel bars: vertical (k infinite), horizontal (k == 0), 45 degrees either way (the xRang == yRang tie when the rectangle
    comes out symmetric)."""
    out = []
    for rows, cols in ((96, 128), (120, 160)):
        v = _free(rows, cols); v[10:rows - 10, cols // 2] = OCC
        h = _free(rows, cols); h[rows // 2, 12:cols - 12] = OCC
        t = np.arange(10, rows - 10)
        d = _free(rows, cols); d[t, t + 8] = OCC
        a = _free(rows, cols); a[t, cols - 9 - t] = OCC
        x = _free(rows, cols); x[10:rows - 10, cols // 3] = OCC; x[rows // 3, 12:cols - 12] = OCC
        for tag, m in (("v", v), ("h", h), ("d", d), ("a", a), ("cross", x)):
            for sca in (0.3, 0.5, 1.0):
                out.append(Case("bars", "%s_%dx%d" % (tag, rows, cols), m, sca))
    return out


def _borders():
    """Bars three cells from each border, over the whole side: end points below 0 and beyond the image, samples on row 0 / column 0."""
    out = []
    for rows, cols in ((96, 128), (101, 131)):
        for tag, sl in (("left", (slice(None), 3)), ("right", (slice(None), cols - 4)), ("top", (3, slice(None))),
                        ("bottom", (rows - 4, slice(None)))):
            m = _free(rows, cols); m[sl] = OCC
            for sca in (0.3, 0.5, 1.0):
                out.append(Case("borders", "%s_%dx%d" % (tag, rows, cols), m, sca))
        m = _free(rows, cols); m[:, 3] = OCC; m[:, cols - 4] = OCC; m[3, :] = OCC; m[rows - 4, :] = OCC
        for sca in (0.3, 0.5, 1.0):
            out.append(Case("borders", "frame_%dx%d" % (rows, cols), m, sca))
    return out


def _unknown_blocks():
    """A block of unknown cells in free space: row 0 and column 0 keep their free cells as 255 (:135-142 starts at 1), so the edge
    lies on the border itself and stops where the block meets it."""
    out = []
    for rows, cols, y0, y1, x0, x1 in ((96, 128, 0, 40, 30, 90), (96, 128, 20, 96, 0, 50), (120, 160, 0, 120, 60, 100)):
        m = _free(rows, cols); m[y0:y1, x0:x1] = UNKNOWN
        for sca in (0.3, 0.5, 1.0):
            out.append(Case("unknown", "block_%d_%d_%d_%d_%dx%d" % (y0, y1, x0, x1, rows, cols), m, sca))
    return out


def noise_with_walls(seed, rows, cols, walls=8, unknown=0.35):
    rng = np.random.default_rng(seed)
    m = np.zeros((rows, cols), np.uint8)
    m[rng.random((rows, cols)) < unknown] = FREE
    for _ in range(walls):                                                                 # axis-aligned and slanted
        x0, y0 = rng.integers(5, cols - 5), rng.integers(5, rows - 5)
        L = int(rng.integers(30, 160)); a = rng.choice([0, np.pi / 2, rng.uniform(0, np.pi)])
        t = np.arange(L)
        xs = np.clip((x0 + t * np.cos(a)).astype(int), 0, cols - 1); ys = np.clip((y0 + t * np.sin(a)).astype(int), 0, rows - 1)
        m[ys, xs] = OCC
    return m


def _noise():
    out = []
    for seed, rows, cols, sca in ((1, 96, 128, 0.5), (2, 96, 128, 1.0), (3, 120, 160, 0.3), (4, 150, 200, 0.5), (5, 240, 200, 0.3),
                                  (6, 240, 200, 0.5), (7, 200, 240, 1.0), (8, 333, 517, 0.3), (9, 97, 129, 1.0), (10, 180, 190, 0.5)):
        out.append(Case("noise", "seed%d_%dx%d" % (seed, rows, cols), noise_with_walls(seed, rows, cols), sca))
    return out


def _aimed():
    """Shapes for what the four kinds reach rarely: the tie, more than 128 samples, more than 8 lines."""
    out = []
    # 45-degree bars alone in a square (cells, margin, thickness, mirrored, sca): the rectangles that come out symmetric
    for n, off, thick, flip, sca in ((75, 6, 3, True, 0.3), (75, 6, 3, True, 1.0), (90, 8, 1, True, 0.3), (69, 11, 3, False, 0.5),
                                     (81, 8, 2, False, 1.0), (78, 6, 3, True, 0.5), (60, 8, 2, True, 0.5)):
        size = n + 2 * off
        m = _free(size, size)
        t = np.arange(off, n + off)
        for d in range(thick):
            tt = t[:len(t) - d]
            m[tt + d, (size - 1 - tt) if flip else tt] = OCC
        out.append(Case("aimed", "diag%d_m%d_t%d%s" % (n, off, thick, "_flip" if flip else ""), m, sca))
    long_v = _free(333, 64); long_v[6:327, 30] = OCC          # 321 cells: over 128 samples at sca 0.5 and 1.0
    long_h = _free(64, 333); long_h[30, 6:327] = OCC
    long_s = _free(200, 333); t = np.arange(300); long_s[10 + (t * 0.55).astype(int), 12 + t] = OCC
    for tag, m in (("long_v", long_v), ("long_h", long_h), ("long_slant", long_s)):
        for sca in (0.5, 1.0):
            out.append(Case("aimed", tag, m, sca))
    grid = _free(150, 200)                                   # a comb of walls: more than 8 lines
    for x in range(15, 190, 18):
        grid[12:138, x] = OCC
    for sca in (0.5, 1.0):
        out.append(Case("aimed", "comb", grid, sca))
    return out


def _edges():
    """Structure on the border itself: a map of occupied cells only (row 0 and column 0 keep the value 1 under 254 elsewhere; an end
    point below 0), bars on row 0 and on column 1 (samples on row 0 / column 0), a bar on column 0 (no line)."""
    out = []
    for (rows, cols), sca in (((64, 80), 0.3), ((101, 131), 0.5), ((120, 90), 1.0), ((96, 128), 0.3)):
        out.append(Case("edges", "occupied_%dx%d" % (rows, cols), np.full((rows, cols), OCC, np.uint8), sca))
        v1 = _free(rows, cols); v1[:, 1] = OCC
        h0 = _free(rows, cols); h0[0, :] = OCC
        v0 = _free(rows, cols); v0[:, 0] = OCC
        for tag, m in (("col1", v1), ("row0", h0), ("col0", v0)):
            out.append(Case("edges", "%s_%dx%d" % (tag, rows, cols), m, sca))
    return out


def _empty():
    out = []
    rng = np.random.default_rng(11)
    out.append(Case("empty", "free_96x128", _free(96, 128), 0.3))
    out.append(Case("empty", "unknown_96x128", np.zeros((96, 128), np.uint8), 0.5))
    out.append(Case("empty", "unknown_120x160", np.zeros((120, 160), np.uint8), 1.0))
    out.append(Case("empty", "dots_96x128", np.where(rng.random((96, 128)) < 0.01, OCC, FREE).astype(np.uint8), 0.3))
    return out


CASES = _bars() + _borders() + _unknown_blocks() + _noise() + _aimed() + _edges() + _empty()
BY_NAME = {repr(c): c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(c.map.shape[0] <= 333 and c.map.shape[1] <= 517 for c in CASES)


# ---- batches for the compaction (k_scan_counts / k_compact_lines behind lsd_run_batch) ---------------------------------------------
# k_scan_counts gives each of its 256 threads per = ceil(n / 256) images: one each up to 256, two from 257 (the last threads idle),
# three at 513.  16 distinct 96 x 128 maps are cycled; two of them have no line, and a map without lines is also put first and last.
BATCH_SIZES = (1, 255, 256, 257, 513)
BATCH_SCA = 0.5
BATCH_MAPS = ("empty/unknown_96x128@0.5", "bars/v_96x128@0.5", "noise/seed1_96x128@0.5", "bars/h_96x128@0.5", "bars/cross_96x128@0.5",
              "borders/frame_96x128@0.5", "bars/d_96x128@0.5", "edges/col0_96x128@0.3", "noise/seed2_96x128@1", "bars/a_96x128@0.5",
              "borders/left_96x128@0.5", "borders/right_96x128@0.5", "unknown/block_0_40_30_90_96x128@0.5", "borders/top_96x128@0.5",
              "empty/dots_96x128@0.3", "borders/bottom_96x128@0.5")
BATCH_NO_LINE = (0, 7)                                      # positions in BATCH_MAPS of the maps without lines at BATCH_SCA


def batch_cases():
    """The 16 maps as cases at BATCH_SCA (a map taken from a case of another scale is a new case here)."""
    return [Case("batch", BY_NAME[k].name, BY_NAME[k].map, BATCH_SCA) for k in BATCH_MAPS]


def batch_indices(n):
    """Which of the 16 maps image i of a batch of n is: the cycle, with a map without lines first and last."""
    idx = [i % len(BATCH_MAPS) for i in range(n)]
    idx[0] = BATCH_NO_LINE[0]
    idx[-1] = BATCH_NO_LINE[1] if n > 1 else BATCH_NO_LINE[0]
    return idx


# ---- hand-made end points for K5 alone (lsd_debug_lines) ------------------------------------------------------------------------------
# What no map gives.  round() and rint() part only where the unrounded sample is an even integer plus one half, so every record of the
# first group puts such samples on its walk: (xx - x1) * k + y1 and (yy - y1) / k + x1 are exact in these numbers.
HAND_ROWS, HAND_COLS = 72, 200
HAND_RECS = np.array([
    # the x walk (xRang > yRang)
    (2.0, 2.5, 10.0, 2.5),            # k == 0: every sample is 2.5 -> row 3 (rint: 2)
    (1.0, 1.5, 9.0, 5.5),             # k == 0.5: 1.5 2 2.5 ... -> 2.5 and 4.5 are even + 0.5
    (30.0, 8.5, 12.0, 4.0),           # x1 > x2, k == 0.25: 4.5 and 6.5 at xx = 14 and 22
    (3.0, 0.5, 40.0, 0.5),            # 0.5 -> row 1, marked (rint: row 0, which :346 leaves unmarked)
    (20.0, 10.5, 190.0, 10.5),        # 171 samples: three 64-lane strides, all on a half
    # the y walk
    (2.5, 2.0, 2.5, 10.0),            # k == +inf: (yy - y1) / k == 0, every sample is 2.5 -> column 3
    (6.5, 30.0, 6.5, 12.0),           # k == -inf
    (11.5, 1.0, 15.5, 9.0),           # k == 2: 11.5 12 12.5 ... -> 12.5 and 14.5
    (24.5, 20.0, 16.5, 36.0),         # k == -2: 24.5 24 ... -> 22.5 20.5 18.5 16.5
    (50.0, 40.0, 60.0, 50.0),         # the tie xRang == yRang walks y
    (0.5, 44.0, 0.5, 60.0),           # 0.5 -> column 1, marked (rint: column 0, unmarked)
    (70.5, 1.0, 70.5, 70.0),          # 70 samples, all on a half
    # no length: k NaN, b NaN, len 0, orient 1, no pixel (the sample is NaN -> INT_MIN)
    (100.0, 30.0, 100.0, 30.0),
    # partly outside
    (-3.5, 66.5, 20.0, 66.5),         # 66.5 -> row 67; the samples left of column 0 are outside
    (196.0, 5.0, 203.0, 12.0),
], np.float64)
HAND_RECS.setflags(write=False)
