"""RegionGrower by tolerance class (-m gpu): csrc/region/grow.h compiles one text into grow() for tolerances below 1.5 rad and grow_any()
for every other tolerance, and eval_seed() chooses between them by the wave-uniform tolerance.  Nothing of the decisions changes, so every
case is compared with the oracle as tests/test_parity_gpu.py compares (usedMap and lineIm bit-exact, the records within
assert_lines_close's tolerances against the glibc build), on 4 and on 8 wavefronts per image, and the counter of grow_any() calls
(DBG_STATS: "grow_any_calls") says which function ran.  The inputs are the smallest at which the split can go wrong: the map that
reaches Refiner and RegionRadiusReducer's sentinel, the reference's heaviest map per pixel, a batch of five different images, that batch
on fewer persistent workgroups than images, and tolerances on both sides of the threshold between the two functions.
"""
import numpy as np
import pytest

from test_parity_gpu import assert_lines_close

pytestmark = pytest.mark.gpu

BATCH_IMAGES = (0, 1, 27, 187, 396)     # of the bench generator; 187 founds certified sets


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """The oracle's answers, computed once per (image, parameters) and shared by the tests of this module."""
    return {}


def _ref(refs, oracle, key, img, kw):
    if key not in refs:
        refs[key] = oracle.lsd(img.copy(), debug=True, **kw)
    return refs[key]


def _single_against_oracle(lsdmod, ctx, oracle, refs, key, img, waves, kw):
    """One image through lsd_run on the given wave count, against the oracle -> (counter record, oracle's answer)."""
    ref = _ref(refs, oracle, (key, tuple(sorted(kw.items()))), img, kw)
    ctx.set_region_waves(waves)
    try:
        lines, line_im = ctx.run(img.copy(), lsdmod.make_params(**kw))
        rows, cols = img.shape
        wh = lsdmod.scaled_size(cols, rows)
        used = ctx.fetch(0, lsdmod.DBG_STATE, wh)
        st = ctx.fetch(0, lsdmod.DBG_STATS, wh)
    finally:
        ctx.set_region_waves(0)
    assert len(lines) == len(ref["lines"])
    assert np.array_equal((used & 3).astype(np.uint8), ref["dbg"]["used"])
    assert np.array_equal(line_im, ref["lineIm"])
    assert_lines_close(lines, ref["lines"])
    assert st["grow_calls"] >= ref["dbg"]["grow_calls"] and st["rrr_oob_reads"] == 0
    return st, ref


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("name", ["map1", "f4key"])
def test_reference_maps_at_the_default_tolerance(name, waves, maps, lsdmod, ctx, oracle, refs):
    """map1 (608 x 480) reaches Refiner and RegionRadiusReducer's sentinel; f4key (1404 x 707) is the heaviest of the reference's maps
    per pixel, with many regrows.  Every first grow runs at 0.39 rad: grow().  On map1 Refiner never asks for 1.5 rad or more either."""
    st, ref = _single_against_oracle(lsdmod, ctx, oracle, refs, name, maps[name], waves, {})
    print("%s, %d waves: grow_any calls %d of %d" % (name, waves, st["grow_any_calls"], st["grow_calls"]))
    if name == "map1":
        assert maps[name].shape == (480, 608)
        assert ref["dbg"]["rrr_sentinel_drops"] > 0 and st["rrr_calls"] > 0 and st["rrr_sentinel_drops"] > 0
        assert st["grow_any_calls"] == 0


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("ang", [90.0, 85.0, 1.0])
def test_other_tolerances(ang, waves, maps, lsdmod, ctx, oracle, refs):
    """angThre = 90 is a tolerance of 1.5708 rad >= 1.5: every first grow takes grow_any(); 85 (1.4835 rad) is the other side of the
    threshold, where grow() still classifies whole batches with a wide tolerance.  (angThre = 1 puts the gradient threshold above every
    gradient of the map: no seed, no line, on the device as in the oracle.)"""
    st, ref = _single_against_oracle(lsdmod, ctx, oracle, refs, "map1", maps["map1"], waves, dict(angThre=ang))
    print("angThre %g, %d waves: grow_any calls %d of %d" % (ang, waves, st["grow_any_calls"], st["grow_calls"]))
    if ang == 90.0:
        assert ref["dbg"]["grow_calls"] > 0 and st["grow_any_calls"] >= ref["dbg"]["grow_calls"] // 2   # every first grow, and the regrows Refiner leaves wide
    if ang == 1.0:
        assert st["grow_calls"] == 0 == st["grow_any_calls"]


@pytest.fixture(scope="module")
def crops(maps):
    import bench
    return np.stack([bench.make_image(maps, i, 2048)[:512, :512] for i in BATCH_IMAGES])


@pytest.mark.parametrize("waves,groups", [(4, -1), (8, -1), (8, 2)])
def test_batch_of_five_images(waves, groups, crops, lsdmod, ctx, oracle, refs):
    """Five different images (more than four: no helper pool), 512 x 512 crops of the bench generator's images, through the device entry
    point; with GROUPS = 2 the 8-wave kernel's persistent workgroups are fewer than the images."""
    import torch
    n, rows, cols = crops.shape
    max_lines = 1024
    d_maps = torch.from_numpy(crops.copy()).cuda()
    d_lines = torch.zeros((n, max_lines, 10), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ims = torch.full((n, rows, cols), 7, dtype=torch.uint8, device="cuda")
    ctx.set_region_waves(waves)
    ctx.debug_set_tuning("GROUPS", groups)
    try:
        ctx.enqueue_device(d_maps.data_ptr(), n, cols, rows, d_lines.data_ptr(), max_lines, d_counts.data_ptr(),
                           d_line_ims=d_ims.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        wh = lsdmod.scaled_size(cols, rows)
        used = [ctx.fetch(i, lsdmod.DBG_STATE, wh) for i in range(n)]
    finally:
        ctx.debug_set_tuning("GROUPS", -1)
        ctx.set_region_waves(0)
    counts, raw, ims = d_counts.cpu().numpy(), d_lines.cpu().numpy(), d_ims.cpu().numpy()
    for i in range(n):
        ref = _ref(refs, oracle, ("crop", i), crops[i], {})
        assert counts[i] == len(ref["lines"]), i
        assert np.array_equal((used[i] & 3).astype(np.uint8), ref["dbg"]["used"]), i
        assert np.array_equal(ims[i], ref["lineIm"]), i
        got = raw[i, :counts[i]].copy().view(np.uint8).reshape(-1, 80).view(lsdmod.LINE_DTYPE).reshape(-1)
        assert_lines_close(got, ref["lines"])
