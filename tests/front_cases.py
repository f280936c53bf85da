"""The front-end campaign: small deterministic maps aimed at the branch structure of K1 (k_gauss.hip), K2 (k_grad.hip), the fused
k_front.hip and K3 (k_sort.hip: k_sort / k_order), where the whole-map tests do not go.  tests/test_front_cases_cpu.py shows on the
CPU that every class below is reached and that the restatements hold; tests/test_front_cases_gpu.py runs the cases on the device with
the pipeline cut behind the sort.  Plain numpy: no GPU and no oracle is needed to import this module.

A class is a predicate on the DEBUG ARRAYS of the correctly rounded oracle (oracle.lib_cr()) and on shapes, never on what the device
returns and never on what a generator meant to draw: classes_of() is the only judge.  Where a class needs a count to land on a value
(a wave's kept count of exactly 63 ... 257), seeds and densities were searched once with the oracle on the CPU and are committed as
constants (KEPT_FOUND); no image is committed.

The kernels' constants restated here (they define the classes, not the expected results): K1 / k_front tile 32 x 24, K2 strip 64 x 8
with a list of 256 entries flushed once it holds more than 192, k_sort 16 waves whose segments are ceil(npx / 1024) * 64 pixels long,
a wave's kept list walked in chunks of 64 and steps of 256."""
import numpy as np

DEFAULTS = dict(sca=0.3, sig=0.6, angThre=22.5, denThre=0.7, pseBin=1024)
TW, TH = 32, 24                                            # K1 / k_front tile
GX, GR, CAP = 64, 8, 256                                   # K2 strip and its list
SWAVES = 16                                                # k_sort
TAPR = 8                                                   # tap radius at sca 0.3 / sig 0.6 (17 taps: the fused kernel applies)
PSEBINS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024)
KEPT_COUNTS = (63, 64, 65, 255, 256, 257)

CLASSES = (
    # shapes
    "one_tile", "tiles_not_x8", "strips_not_x8", "other_taps",
    # remap and empty windows
    "window_zero_after_remap", "blank_in_batch",
    # K2 arithmetic
    "pi_to_zero", "border_gauss_no_gradient", "mid_strip_flush", "front_tile_full", "grad_thre_2", "all_code_1",
    # K3 segments
    "npx_4", "npx_63", "npx_1023", "npx_1024", "npx_1025", "npx_4096", "npx_4097",
    "empty_segments", "one_pixel_segment_kept", "first_wave_only", "last_wave_only",
) + tuple("kept_%d" % k for k in KEPT_COUNTS) + (
    # K3 bins
    "one_bin_over_64_in_a_wave", "bin_in_all_waves", "ties_at_max", "top_bin_empty", "nb0_not_blank", "bins_span_waves_300",
    "top_bit_peers",
    # batches
    "mixed_blank", "batch_over_256", "order_keys_collide",
)


# ---- restatements (the GPU test reuses them) ------------------------------------------------------------------------------------
def pw_of(deg, code):
    """The packed pixel word (lsd_internal.h): float32(deg) -- round to nearest even -- with its two lowest mantissa bits replaced by
    the code."""
    return (np.asarray(deg, np.float64).astype(np.float32).view(np.uint32) & np.uint32(0xfffffffc)) | np.asarray(code).astype(np.uint32)


def sort_rule(mag, max_grad, pse_bin):
    """K3's rule (myLSD.cpp:177-204) -> (pixels y * w + x, bin values): v = min(floor(mag * (pseBin / maxGrad)), pseBin), keep
    v != 0, descending v, raster order among ties.  A blank image (maxGrad == 0) has an empty list by definition (k_sort.hip)."""
    if not max_grad > 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    zoom = 1.0 * pse_bin / max_grad
    v = np.minimum(np.floor(np.asarray(mag, np.float64).ravel() * zoom), pse_bin).astype(np.int64)
    px = np.flatnonzero(v != 0)
    px = px[np.argsort(-v[px], kind="stable")]
    return px, v[px]


def gradients(gauss):
    """gradX, gradY (myLSD.cpp:161-162) of a Gaussian image, 0 on row 0 / column 0 (exact in numpy: the same fp64 operations)."""
    A, B, C, D = gauss[1:, 1:], gauss[1:, :-1], gauss[:-1, 1:], gauss[:-1, :-1]
    gx, gy = np.zeros_like(gauss), np.zeros_like(gauss)
    gx[1:, 1:] = (B + D - A - C) / 2.0
    gy[1:, 1:] = (C + D - A - B) / 2.0
    return gx, gy


def grad_ties(d, atan2):
    """The gradient pass's near-tie count of one image (grad_px.h: grad_angle) from the oracle's arrays: the pixels with a gradient
    whose angle BEFORE the "pi -> 0" rule, a = atan2(gradX, -gradY), has | |a - pi| - 1e-6 | <= 1e-14.  atan2: the correctly rounded
    one (oracle.lib_cr(): cr_atan2).  Only angles that the rule turned into 0 or that lie next to pi can count, so only those are
    evaluated."""
    pi = 3.14159265358979323846
    gx, gy = gradients(d["gauss"])
    heavy = (gx != 0) | (gy != 0)
    near = heavy & ((d["deg"] == 0) | (np.abs(d["deg"] - pi) < 1e-5))
    n = 0
    for x, y in zip(gx[near], gy[near]):
        a = atan2(float(x), -float(y))
        n += abs(abs(a - pi) - 0.000001) <= 1e-14
    return int(n)


def scrambled(batch):
    """A batch of the same shape and size with other content in every image (random bytes): what a test runs before the call it
    measures, so that no array holds that call's answer beforehand."""
    return np.random.default_rng(batch.size).integers(0, 256, size=batch.shape, dtype=np.uint8)


def seg_len(npx):
    return -(-npx // (64 * SWAVES)) * 64


def kept_per_wave(d):
    """Kept pixels of every k_sort wave, from the oracle's sorted list."""
    px = d["ord_y"].astype(np.int64) * d["w"] + d["ord_x"]
    return np.bincount(px // seg_len(d["w"] * d["h"]), minlength=SWAVES)


def chunks_of_bins(d, pse_bin):
    """The bin numbers b = pseBin - v of every 64-entry chunk of every wave's kept list (raster order), as pass 2 of k_sort walks
    them."""
    px = d["ord_y"].astype(np.int64) * d["w"] + d["ord_x"]
    o = np.argsort(px)
    px, b = px[o], pse_bin - d["ord_v"][o].astype(np.int64)
    wave = px // seg_len(d["w"] * d["h"])
    out = []
    for s in range(SWAVES):
        bs = b[wave == s]
        out += [bs[i:i + 64] for i in range(0, len(bs), 64)]
    return out


def order_key(nb, npx):
    """k_order's key of an image (without a cost history)."""
    return 255 - min(255, nb * 2048 // (npx + 1))


# ---- the images -----------------------------------------------------------------------------------------------------------------
def src(n, sca=0.3):
    """A source extent whose scaled extent is n (the census holds every case's size against the oracle's w, h)."""
    return int((n + 0.5) / sca)


def tri(seed, rows, cols):
    """Free, occupied and unknown cells at random (test_parity_gpu.synth_tiny)."""
    return np.random.default_rng(seed).choice(np.array([0, 1, 255], np.uint8), size=(rows, cols), p=[0.4, 0.3, 0.3])


def dense(seed, rows, cols):
    """Uniformly random bytes: every interior pixel has a non-zero gradient."""
    return np.random.default_rng(seed).integers(0, 256, size=(rows, cols), dtype=np.uint8)


def blocks(seed, rows, cols, p, cell=12):
    """Random bytes in a share p of the cell x cell blocks, zeros elsewhere: a kept count anywhere below the dense one."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)
    on = rng.random((-(-rows // cell), -(-cols // cell))) < p
    return m * np.kron(on, np.ones((cell, cell), bool))[:rows, :cols].astype(np.uint8)


def step(rows, cols, kind, value=100):
    """A step edge: 'l' / 'r' the left / right half filled, 't' / 'b' the top / bottom half, 'd' below the diagonal."""
    m = np.zeros((rows, cols), np.uint8)
    if kind == "l": m[:, :cols // 2] = value
    elif kind == "r": m[:, cols // 2:] = value
    elif kind == "t": m[:rows // 2] = value
    elif kind == "b": m[rows // 2:] = value
    else: m[np.arange(rows)[:, None] * cols > np.arange(cols)[None, :] * rows] = value
    return m


def two_edges(rows, cols, value, width):
    """A strong vertical edge (the right half occupied: 1 -> 255) and a weak thin vertical line: pixels in the top bin and pixels in
    the lowest bins in every row, so in every chunk of a wave's kept list."""
    m = np.zeros((rows, cols), np.uint8)
    m[:, cols // 2:] = 1
    m[:, cols // 4:cols // 4 + width] = value
    return m


def filled(rows, cols, value):
    return np.full((rows, cols), value, np.uint8)


def bar(rows, cols, r0, r1, value=1):
    """Zeros and one horizontal bar over source rows r0 .. r1 - 1 (value 1 is remapped to 255)."""
    m = np.zeros((rows, cols), np.uint8)
    m[r0:r1, cols // 4:3 * cols // 4] = value
    return m


class Case:
    """name, the scaled size it is built for, a batch of equally sized maps (made on demand, read-only) and the parameters."""

    def __init__(self, name, wh, make, **params):
        self.name, self.wh, self._make, self._batch = name, wh, make, None
        self.params = dict(DEFAULTS)
        self.params.update(params)

    @property
    def batch(self):
        if self._batch is None:
            b = np.ascontiguousarray(np.stack([np.asarray(m, np.uint8) for m in self._make()]))
            b.setflags(write=False)
            self._batch = b
        return self._batch

    @property
    def fused_applies(self):
        """17 taps: the call takes k_front unless lsd_set_fused_front(0)."""
        return self.params["sca"] == 0.3 and self.params["sig"] == 0.6

    def __repr__(self):
        return self.name


def _shape_cases():
    """About 24 scaled (w, h) pairs around the tile, strip and halo sizes, each with tri-valued and with dense content (one batch of
    two), the one-tile shapes also as single images (7 of the 8 launched workgroups return at once), three at sca = 0.5 (11 taps:
    k_gauss / k_gradient whatever the setting) where the Gaussian pitch, a multiple of 16, is above, at and below the width."""
    pairs = [(2, 2), (2, 49), (97, 2), (32, 24), (33, 25), (64, 8), (65, 9), (3, 3), (31, 23), (32, 25), (33, 24), (63, 7), (64, 9),
             (65, 8), (97, 49), (31, 3), (3, 23), (63, 24), (64, 23), (33, 49), (97, 7), (2, 9), (65, 25), (63, 2)]
    out = []
    for i, (w, h) in enumerate(pairs):
        out.append(Case("shape_%dx%d" % (w, h), (w, h),
                        lambda w=w, h=h, i=i: [tri(100 + i, src(h), src(w)), dense(200 + i, src(h), src(w))]))
    for w, h in ((32, 24), (31, 23), (2, 2)):
        out.append(Case("single_%dx%d" % (w, h), (w, h), lambda w=w, h=h: [dense(300 + w, src(h), src(w))]))
    for w in (15, 16, 17):
        out.append(Case("taps11_%dx10" % w, (w, 10), lambda w=w: [tri(310 + w, src(10, 0.5), src(w, 0.5)), dense(320 + w, src(10, 0.5), src(w, 0.5))],
                        sca=0.5))
    return out


def _remap_cases():
    r, c = src(3 * TH), src(3 * TW)
    return [
        # 3 x 3 tiles of one value: the centre tile's raw window is non-zero and all zero after the remap (255 -> 0), the border
        # tiles keep the raw row 0 / column 0; the same with 1 (-> 255: a plateau, no gradient away from the border); a blank image
        # between them in the batch
        Case("remap_255_blank_1", (3 * TW, 3 * TH), lambda: [filled(r, c, 255), filled(r, c, 0), filled(r, c, 1)]),
        Case("remap_255_alone", (3 * TW, 3 * TH), lambda: [filled(r, c, 255)]),
    ]


def _k2_cases():
    r, c = src(30), src(45)
    steps = lambda: [step(r, c, k) for k in "lrtbd"]
    out = [Case("steps_45x30", (45, 30), steps)]
    for a in (45.0, 90.0, 1.0):
        # (at 1 degree gradThre is 114.6: random bytes, smoothed, stay far below it -- every pixel off row 0 / column 0 is code 1)
        out.append(Case("ang%g_45x30" % a, (45, 30), lambda a=a: steps()[:3] + [dense(400, r, c), tri(401, r, c)], angThre=a))
    # four fully heavy rows of a 64-column strip (k_gradient's list flushed in mid-strip), a fused tile with all 768 pixels listed
    out.append(Case("dense_97x49", (97, 49), lambda: [dense(410, src(49), src(97))]))
    out.append(Case("dense_130x17", (130, 17), lambda: [dense(411, src(17), src(130)), blocks(412, src(17), src(130), 0.7)]))
    return out


# Found once with the oracle on the CPU (seeds from 1000 upwards, p in 0.3 .. 1.0 by 0.1, first hit): blocks(seed, ., ., p) at the scaled
# size (w, h) has k_sort waves whose kept counts are exactly the listed ones.  63 / 64 / 65: segments of 64 and 128 pixels; 255 / 256 /
# 257: segments of 320 (80 x 64, where the dense image keeps 316 per wave).  The census judges them again on every run.
KEPT_FOUND = ((97, 10, 1000, 0.5, (63, 64)), (65, 25, 1038, 0.3, (65,)), (80, 64, 1002, 0.3, (255, 256)), (80, 64, 1001, 0.4, (257,)))


def _segment_cases():
    out = []
    for w, h in ((2, 2), (21, 3), (31, 33), (32, 32), (25, 41), (64, 64), (17, 241)):
        out.append(Case("npx_%dx%d" % (w, h), (w, h), lambda w=w, h=h: [dense(500 + w, src(h), src(w)), tri(520 + w, src(h), src(w))]))
    for w, h, seed, p, counts in KEPT_FOUND:
        out.append(Case("kept_" + "_".join(str(k) for k in counts), (w, h), lambda w=w, h=h, seed=seed, p=p: [blocks(seed, src(h), src(w), p)]))
    r, c = src(64), src(64)
    # 64 x 64: a wave owns four rows.  A bar in source row 1 reaches the Gaussian rows 0 .. 2, so the gradient rows 1 .. 3: wave 0
    # only; one in the last three source rows reaches the rows 61 .. 63: wave 15 only.
    out.append(Case("first_last_wave_64x64", (64, 64), lambda: [bar(r, c, 1, 2), bar(r, c, r - 3, r)]))
    return out


def _bin_cases():
    out = []
    r, c = src(13), src(40)
    for pb in PSEBINS:
        out.append(Case("bins_%d" % pb, (40, 13), lambda pb=pb: [tri(600 + pb, r, c), dense(700 + pb, r, c), step(r, c, "r"), step(r, c, "b")],
                        pseBin=pb))
    # a non-blank image whose maximum rounds below bin 1 (test_parity_gpu.synth_tiny(3, 10, 400)), next to one that keeps a pixel
    out.append(Case("nb0_120x3", (120, 3), lambda: [tri(3, 10, 400), tri(4, 10, 400)], pseBin=1))
    # a horizontal edge over 241 columns: a third of its pixels sit exactly at the maximum (the x-pass has three tap phases), all
    # kept pixels in one bin and all in one wave's segment of 320
    for pb in (1, 2, 3):
        out.append(Case("edge_241x17_bins_%d" % pb, (241, 17), lambda: [step(src(17), src(241), "b"), step(src(17), src(241), "t")], pseBin=pb))
    out.append(Case("dense_80x64", (80, 64), lambda: [dense(5, src(64), src(80))]))
    # pseBin - 1 a power of two: bin number pseBin - 1 (v == 1) is the only one with the top bit of the peer search set, and differs
    # from bin number 0 (v == pseBin) in that bit alone.  A line of value 9, two cells wide, puts v == 1 next to the strong edge's
    # v == pseBin in one chunk (found with the oracle: values 2 .. 11, widths 1 .. 3 tried)
    for pb in (65, 257):
        out.append(Case("top_bit_%d" % pb, (40, 13), lambda: [two_edges(r, c, 9, 2)], pseBin=pb))
    return out


def _batch_cases():
    r, c = src(24), src(40)
    d3 = lambda: [dense(800, r, c), dense(801, r, c), dense(802, r, c)]
    mixed = lambda: [dense(800, r, c), filled(r, c, 0), dense(802, r, c)]
    out = [Case("seq_dense", (40, 24), d3), Case("seq_blank_at_1", (40, 24), mixed),
           Case("seq_all_blank", (40, 24), lambda: [filled(r, c, 0)] * 3)]
    # 257 images of 12 x 12: ten different ones (two blank) dealt so that equal images, and with them equal k_order keys, recur
    s = src(12)
    pool = lambda: [tri(900, s, s), filled(s, s, 0), dense(901, s, s), tri(902, s, s), step(s, s, "r"), tri(903, s, s), filled(s, s, 0),
                    dense(904, s, s), step(s, s, "d"), tri(905, s, s)]
    out.append(Case("batch_257", (12, 12), lambda: (lambda P: [P[(i * 7 + i // 10) % 10] for i in range(257)])(pool())))
    return out


# the calls of a sequence run one after the other on one context (same shape, same batch size)
SEQUENCES = (("dense_then_blank", ("seq_dense", "seq_blank_at_1")), ("blank_then_dense", ("seq_blank_at_1", "seq_dense")),
             ("dense_then_all_blank", ("seq_dense", "seq_all_blank", "seq_dense")))
FULL_PIPELINE = ("batch_257",)                             # run through the whole pipeline as a batch
CASES = _shape_cases() + _remap_cases() + _k2_cases() + _segment_cases() + _bin_cases() + _batch_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the oracle's answers -------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case, oracle, cr=True):
    """The oracle's debug arrays for every image of a case (correctly rounded build, or glibc's), computed once per process and
    read-only; the full pipeline's lines and lineIm ride along."""
    key = (case.name, cr)
    if key not in _REF:
        out = []
        seen = {}
        for im in case.batch:
            k = im.tobytes()
            if k not in seen:
                r = oracle.lsd(im.copy(), debug=True, _lib=oracle.lib_cr() if cr else None, **case.params)
                d = r["dbg"]
                d["lines"], d["lineIm"] = r["lines"], r["lineIm"]
                for v in d.values():
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
                seen[k] = d
            out.append(seen[k])
        _REF[key] = out
    return _REF[key]


# ---- the judge ------------------------------------------------------------------------------------------------------------------
def _centre(x, sca):
    return int(np.floor(x / sca + 0.5))                    # K1's window centre (myLSD.cpp:428 / :460)


def _mid_strip_flushes(heavy):
    """Strips of k_gradient whose list is flushed before their last row and has entries again afterwards."""
    h, w = heavy.shape
    n = 0
    for y0 in range(0, h, GR):
        for x0 in range(0, w, GX):
            cnt, flushed = 0, False
            for row in heavy[y0:y0 + GR, x0:x0 + GX]:
                k = int(row.sum())
                if flushed and k:
                    n += 1
                    break
                cnt += k
                if cnt > CAP - GX:
                    cnt, flushed = 0, True
    return n


def classes_of(case, refs):
    """The classes a case reaches -> {class: count} (images, pixels, strips or bins, whichever the class counts)."""
    out = dict.fromkeys(CLASSES, 0)
    n = len(case.batch)
    p = case.params
    d0 = refs[0]
    w, h = d0["w"], d0["h"]
    npx = w * h
    tiles = -(-w // TW) * -(-h // TH) * n
    strips = -(-w // GX) * -(-h // GR) * n
    out["one_tile"] = int(tiles == 1)
    out["tiles_not_x8"] = int(tiles % 8 != 0)
    out["strips_not_x8"] = int(strips % 8 != 0)
    out["other_taps"] = int(not case.fused_applies)
    for k in (4, 63, 1023, 1024, 1025, 4096, 4097):
        out["npx_%d" % k] = int(npx == k)
    blank = [not im.any() for im in case.batch]
    out["blank_in_batch"] = int(n > 1 and any(blank))
    out["mixed_blank"] = int(any(blank) and not all(blank))
    out["batch_over_256"] = int(n > 256)
    keys = [order_key(d["nb"], npx) for d in refs]
    out["order_keys_collide"] = int(n > 256) * (n - len(set(keys)))
    sl = seg_len(npx)
    for im, d in zip(case.batch, refs):
        gx, gy = gradients(d["gauss"])
        heavy = (gx != 0) | (gy != 0)
        for by in range(0, h, TH):
            for bx in range(0, w, TW):
                g = d["gauss"][by:by + TH, bx:bx + TW]
                r0, r1 = _centre(by, p["sca"]) - TAPR, _centre(min(by + TH, h) - 1, p["sca"]) + TAPR
                c0, c1 = _centre(bx, p["sca"]) - TAPR, _centre(min(bx + TW, w) - 1, p["sca"]) + TAPR
                raw = im[max(r0, 0):r1 + 1, max(c0, 0):c1 + 1]
                if case.fused_applies and raw.any() and not g.any() and not np.signbit(g).any():
                    out["window_zero_after_remap"] += 1
                if heavy[by:by + TH, bx:bx + TW].sum() == TW * TH:
                    out["front_tile_full"] += 1
        out["pi_to_zero"] += int(((d["deg"] == 0) & (d["mag"] > 0)).sum())
        border = np.zeros((h, w), bool)
        border[0], border[:, 0] = True, True
        out["border_gauss_no_gradient"] += int((border & (d["gauss"] != 0) & (d["mag"] == 0)).sum())
        out["mid_strip_flush"] += _mid_strip_flushes(heavy)
        if p["angThre"] == 90.0:
            out["grad_thre_2"] += int(((d["mag"] > 0) & (d["mag"] < 2.0)).any() and (d["mag"] >= 2.0).any())
        out["all_code_1"] += int(heavy.any() and (d["used0"][1:, 1:] == 1).all() and (d["used0"][0] == 0).all() and (d["used0"][:, 0] == 0).all())
        kw = kept_per_wave(d)
        own = np.clip(npx - sl * np.arange(SWAVES), 0, sl)                     # pixels every wave owns
        out["empty_segments"] += int((own == 0).any())
        out["one_pixel_segment_kept"] += int(((own == 1) & (kw == 1)).any())
        out["first_wave_only"] += int(d["nb"] > 0 and kw[0] == d["nb"] and own[1] > 0)
        out["last_wave_only"] += int(d["nb"] > 0 and kw[SWAVES - 1] == d["nb"])
        for k in KEPT_COUNTS:
            out["kept_%d" % k] += int((kw == k).any())
        v = d["ord_v"]
        out["one_bin_over_64_in_a_wave"] += int(d["nb"] > 0 and len(np.unique(v)) == 1 and kw.max() > 64)
        if d["nb"]:
            wave = (d["ord_y"].astype(np.int64) * w + d["ord_x"]) // sl
            span = np.zeros((p["pseBin"] + 1, SWAVES), bool)
            span[v, wave] = True
            per_bin = span.sum(1)
            out["bin_in_all_waves"] += int((per_bin == SWAVES).sum())
            out["bins_span_waves_300"] += int((per_bin > 1).sum() >= 300)
            out["top_bin_empty"] += int(v.max() < p["pseBin"])
            top = 1 << (max(p["pseBin"] - 1, 1).bit_length() - 1)              # the highest bit of a bin number
            if top == p["pseBin"] - 1 and top > 1:
                out["top_bit_peers"] += sum(1 for ch in chunks_of_bins(d, p["pseBin"]) if (ch == 0).any() and (ch == top).any())
        out["ties_at_max"] += int(d["maxGrad"] > 0 and (d["mag"] == d["maxGrad"]).sum() > 1)
        out["nb0_not_blank"] += int(d["nb"] == 0 and d["maxGrad"] > 0)
    return out
