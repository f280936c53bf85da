"""The fused front end (csrc/k_front.hip: Gaussian + gradient pass as one kernel, no GaussImage in device memory) against the oracle
and against the two-kernel path it replaces (-m gpu).

Every case runs twice through the device entry point, with set_fused_front(0) and with set_fused_front(1).  Both runs are held
against the oracle with test_parity_gpu.py's own tolerances (GaussImage, magMap, maxGrad, usedMap, lineIm bit for bit, degMap within
DEG_ULP), and against each other bit for bit: magMap, degMap, the packed state, maxGrad, the sorted seed list, the line records and
last_sensitivity.

last_sensitivity is the sum of two counts: the gradient pass's near ties, which the front end produces and which are a function of the
input alone, and the region stage's, which include speculative evaluations that were discarded and so move a little with the schedule
from one run to the next of the very same kernels (test_parity_gpu.py::test_sensitivity_of_the_reference_maps_and_of_a_batch says
so; measured here on the empty-next-to-full pair, three runs of the two-kernel path: [46, 14], [42, 12], [48, 13]; three of the fused
one: [40, 14], [40, 14], [41, 12]; the gradient part 0 in all six).  The
gradient pass's part -- last_sensitivity minus the region stage's own counter (DBG_STATS near_ties) -- is compared bit for bit; of
the sum, what does not move: whether an image has any.
"""
import numpy as np
import pytest

from test_parity_gpu import DEG_ULP, full_check, ulps

pytestmark = pytest.mark.gpu

MAX_LINES = 2048


# ---- the inputs (plain numpy: tests/test_fused_front_inputs.py checks on the CPU that the oracle takes each of them) -------------
def one_tile_plus_one():
    """112 x 84 -> 33 x 25 scaled pixels: one full K1 tile (32 x 24), a partial tile to its right and one below, so the halo crosses a
    tile border in both directions; occupancy values that the remap touches (1, 255) and that it does not."""
    rng = np.random.default_rng(11)
    return rng.choice(np.array([0, 1, 100, 200, 255], np.uint8), size=(1, 84, 112))


def dense():
    """Uniformly random bytes: every interior pixel has a non-zero gradient, so a full tile lists all of its 768 pixels."""
    rng = np.random.default_rng(12)
    return rng.integers(0, 256, size=(1, 200, 200), dtype=np.uint8)


def empty_next_to_full():
    """Zeros and one filled rectangle.  Image 0: the rectangle starts at source column 112, so the window of scaled column 32 (source
    columns 99 .. 115) sees it and that of column 31 (95 .. 111), with it all of tile column 0, does not: the first column of a
    non-empty tile takes its halo from an empty neighbour.  Image 1: the same for rows, at scaled row 24 (source rows 72 .. 88 against
    69 .. 85 of row 23).  The far edges of the rectangles lie inside tiles, where a non-empty tile borders on empty ones the other
    way round."""
    b = np.zeros((2, 400, 400), np.uint8)
    b[0, 150:300, 112:250] = 100
    b[1, 86:260, 130:330] = 100
    return b


def batch_of_three(maps):
    """Three different 320 x 240 crops (96 x 72 scaled: 3 x 3 tiles each, 27 tiles in all -- not a multiple of the 8 XCDs)."""
    return np.stack([np.ascontiguousarray(maps["map1"][100:340, 150:470]), np.ascontiguousarray(maps["mapValue"][60:300, 500:820]),
                     np.ascontiguousarray(maps["aisle1"][200:440, 600:920])])


# ---- one case through both settings ------------------------------------------------------------------------------------------------
_refs = {}


def _oracle_refs(oracle, key, batch, kw):
    """The oracle's answers for a batch, computed once per module (they are only read)."""
    if key not in _refs:
        out = []
        for im in batch:
            m = im.copy()
            r = oracle.lsd(m, debug=True, **kw)
            r["map_after"] = m
            out.append(r)
        _refs[key] = out
    return _refs[key]


def _run(lsdmod, ctx, batch, fused, flags=0, params=None):
    import torch
    n, rows, cols = batch.shape
    ctx.set_fused_front(fused)
    d_maps = torch.from_numpy(batch.copy()).cuda()
    d_lines = torch.zeros((n, MAX_LINES, 10), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ims = torch.full((n, rows, cols), 7, dtype=torch.uint8, device="cuda")          # the front end clears lineIm on the way
    ctx.enqueue_device(d_maps.data_ptr(), n, cols, rows, d_lines.data_ptr(), MAX_LINES, d_counts.data_ptr(), d_line_ims=d_ims.data_ptr(),
                       params=params, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    p = params or lsdmod.make_params()
    wh = lsdmod.scaled_size(cols, rows, p.sca)
    out = {"counts": d_counts.cpu().numpy(), "lines": d_lines.cpu().numpy(), "line_ims": d_ims.cpu().numpy(), "timings": ctx.timings(),
           "ties": ctx.last_sensitivity(n), "wh": wh}
    for name, what in (("gauss", lsdmod.DBG_GAUSS), ("mag", lsdmod.DBG_MAG), ("deg", lsdmod.DBG_DEG), ("state", lsdmod.DBG_STATE),
                       ("maxgrad", lsdmod.DBG_MAXGRAD), ("order", lsdmod.DBG_ORDER)):
        out[name] = [ctx.fetch(i, what, wh) for i in range(n)]                        # (GAUSS reads d_maps: still alive here)
    out["grad_ties"] = out["ties"] - np.array([ctx.fetch(i, lsdmod.DBG_STATS, wh)["near_ties"] for i in range(n)], np.int64)
    out["maps_after"] = d_maps.cpu().numpy()
    return out


def _against_oracle(got, refs, batch, writeback):
    for i, ref in enumerate(refs):
        d = ref["dbg"]
        assert got["wh"] == (d["w"], d["h"])
        assert got["counts"][i] == len(ref["lines"]) <= MAX_LINES, i
        assert np.array_equal(got["gauss"][i], d["gauss"]), i
        assert np.array_equal(got["mag"][i], d["mag"]), i
        assert got["maxgrad"][i] == d["maxGrad"], i
        assert ulps(got["deg"][i], d["deg"]).max() <= DEG_ULP, i
        assert np.array_equal((got["state"][i] & 3).astype(np.uint8), d["used"]), i
        assert np.array_equal(got["line_ims"][i], ref["lineIm"]), i
        assert np.array_equal(got["order"][i].astype(np.int64), d["ord_y"].astype(np.int64) * d["w"] + d["ord_x"]), i
        assert np.array_equal(got["maps_after"][i], ref["map_after"] if writeback else batch[i]), i


def _same_bits(a, b):
    assert np.array_equal(a["counts"], b["counts"])
    for i in range(len(a["counts"])):
        for k in ("mag", "deg", "state", "order"):
            assert a[k][i].tobytes() == b[k][i].tobytes(), (k, i)
        assert a["maxgrad"][i] == b["maxgrad"][i]
        c = int(a["counts"][i])
        assert a["lines"][i, :c].tobytes() == b["lines"][i, :c].tobytes(), i
    assert np.array_equal(a["grad_ties"], b["grad_ties"]) and (a["grad_ties"] >= 0).all()
    assert np.array_equal(a["ties"] > 0, b["ties"] > 0)
    assert np.array_equal(a["line_ims"], b["line_ims"]) and np.array_equal(a["maps_after"], b["maps_after"])


def _both(lsdmod, ctx, oracle, key, batch, flags=0):
    refs = _oracle_refs(oracle, key, batch, {})
    two = _run(lsdmod, ctx, batch, 0, flags)
    one = _run(lsdmod, ctx, batch, 1, flags)
    writeback = bool(flags & lsdmod.LSD_FLAG_WRITEBACK_MAP)
    _against_oracle(two, refs, batch, writeback)
    _against_oracle(one, refs, batch, writeback)
    _same_bits(two, one)
    # the fused kernel's time is all under "gauss"; K2 has a time of its own
    assert one["timings"]["gradient"] == 0.0 and one["timings"]["gauss"] > 0
    assert two["timings"]["gradient"] > 0
    return one


@pytest.fixture
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def test_one_tile_plus_one(lsdmod, ctx, oracle):
    one = _both(lsdmod, ctx, oracle, "tile", one_tile_plus_one())
    assert one["wh"] == (33, 25)
    # Q3: row 0 / column 0 have no gradient and stay growable
    assert not one["mag"][0][0].any() and not one["mag"][0][:, 0].any() and not one["deg"][0][0].any() and not one["deg"][0][:, 0].any()


def test_dense(lsdmod, ctx, oracle):
    one = _both(lsdmod, ctx, oracle, "dense", dense())
    assert (one["mag"][0][1:, 1:] > 0).all()                                          # every interior pixel went through the list


def test_empty_next_to_full(lsdmod, ctx, oracle):
    b = empty_next_to_full()
    one = _both(lsdmod, ctx, oracle, "empty", b)
    g0, g1 = one["gauss"]
    assert not g0[:, :32].any() and g0[50:85, 32].all()                               # tile column 0 is empty, column 32 is not
    assert not g1[:24].any() and g1[24, 45:95].all()                                  # ... and the same for rows


def test_batch_of_three(lsdmod, ctx, oracle, maps):
    one = _both(lsdmod, ctx, oracle, "batch", batch_of_three(maps))
    assert len(set(float(v) for v in one["maxgrad"])) == 3                            # per-image maxima


def test_writeback_then_fetch(lsdmod, ctx, oracle, maps):
    """The caller's map is rewritten in place (1 -> 255, 255 -> 0, not idempotent); GAUSS fetched afterwards is recomputed from the
    rewritten map without the remap and equals the oracle's all the same (_against_oracle)."""
    b = maps["map1"][None].copy()
    one = _both(lsdmod, ctx, oracle, "map1", b, flags=lsdmod.LSD_FLAG_WRITEBACK_MAP)
    assert not np.array_equal(one["maps_after"], b)


def test_fallbacks_take_the_two_kernel_path(lsdmod, ctx, oracle, maps):
    img = maps["map1"]
    # another scale: 11 taps
    kw = dict(sca=0.5, sig=0.6, angThre=22.5, denThre=0.7, pseBin=1024)
    for fused in (0, 1):
        ctx.set_fused_front(fused)
        full_check(lsdmod, ctx, oracle, img, lsdmod.make_params(**kw), kw=kw)
        assert ctx.timings()["gradient"] > 0
    # the pipeline cut behind the Gaussian: GaussImage itself is the result
    refs = _oracle_refs(oracle, "map1", img[None], {})
    try:
        ctx.set_stop_after(lsdmod.STAGE_GAUSS)
        for fused in (0, 1):
            ctx.set_fused_front(fused)
            got_map = img.copy()
            lines, line_im = ctx.run(got_map)
            assert len(lines) == 0 and not line_im.any()
            assert np.array_equal(got_map, refs[0]["map_after"])
            assert np.array_equal(ctx.fetch(0, lsdmod.DBG_GAUSS, (refs[0]["dbg"]["w"], refs[0]["dbg"]["h"])), refs[0]["dbg"]["gauss"])
            assert ctx.timings()["gradient"] > 0
    finally:
        ctx.set_stop_after(lsdmod.STAGE_ALL)
    # ... and the default parameters on the same context afterwards take the fused path again
    ctx.set_fused_front(1)
    full_check(lsdmod, ctx, oracle, img)
    assert ctx.timings()["gradient"] == 0.0
