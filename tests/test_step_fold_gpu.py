"""Lines in the region stage (lsd_set_fused_lines: the workgroup that finishes an image writes its line records and lineIm marks) against
the kernel of its own behind the batch, in the same context, byte for byte.

What is compared after every call: the counts, the whole line-record buffer (filled with 0xFF before the call, so the stored records,
their padding word and every byte the call must leave alone), lineIm (filled with 0xFF too: the library clears it), and per image
DBG_STATE, DBG_ORDER, the gradient maximum and last_sensitivity.  The shapes are small and sit on the edges of the code that moved:
lists that overflow max_lines, no lineIm, a raster that is not made of whole 16-byte words, 4 and 8 wavefronts per image, the
persistent workgroups' loop, launches of different n in a row, pipelines cut short (no lines at all), and the cost history.

last_sensitivity is the sum of two counts.  The gradient pass's near ties are a function of the input alone and are compared bit for
bit (last_sensitivity minus the region stage's own counter, DBG_STATS near_ties).  The region stage's count includes speculative
evaluations that were discarded and moves with the schedule from one run to the next of the very same kernels
(tests/test_fused_front_gpu.py has the precedent and more figures); measured here on the map1 crop alone, 4 wavefronts, run after run on
one context: the kernel of its own 83, 82; lines fused 75 -- the gradient part 0 in all three.  So of the sum, what does not move is
compared: whether an image has any.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 200, 160                                             # the crops' size (cols, rows)

# REF runs k_lines behind the batch; the mode under test has the region stage write the lines
REF = 0
MODES = {"lines": 1}


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def images(maps):
    """Nine images of H x W, no two equal: crops of map1, mapValue and aisle1 (two), and flipped / rolled copies of them."""
    a = maps["aisle1"]
    base = [maps["map1"][150:150 + H, 200:200 + W], maps["mapValue"][120:120 + H, 500:500 + W], a[100:100 + H, 300:300 + W], a[380:380 + H, 900:900 + W]]
    out = [np.ascontiguousarray(b) for b in base]
    out += [np.ascontiguousarray(b[::-1]) for b in base]
    out.append(np.ascontiguousarray(np.roll(base[2], 37, axis=1)))
    assert len({o.tobytes() for o in out}) == 9 and all(o.shape == (H, W) and o.any() for o in out)
    return np.stack(out)


def set_mode(ctx, mode):
    ctx.set_fused_lines(mode)


def run(lsdmod, ctx, batch, max_lines=64, with_im=True, stop_after=0):
    """One call on `batch` [n, rows, cols] with every output filled with 0xFF first -> dict of what the call left, as bytes."""
    import torch
    n, rows, cols = batch.shape
    d_maps = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    d_lines = torch.full((n * max_lines * 80,), 0xFF, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((n,), -1, dtype=torch.int32, device="cuda")           # (0xFF bytes)
    d_im = torch.full((n, rows, cols), 0xFF, dtype=torch.uint8, device="cuda") if with_im else None
    ctx.set_stop_after(stop_after)
    ctx.enqueue_device(d_maps.data_ptr(), n, cols, rows, d_lines.data_ptr(), max_lines, d_counts.data_ptr(),
                       d_line_ims=d_im.data_ptr() if with_im else None, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    wh = lsdmod.scaled_size(cols, rows)
    got = {"counts": d_counts.cpu().numpy().tobytes(), "lines": d_lines.cpu().numpy().tobytes(),
           "lineIm": d_im.cpu().numpy().tobytes() if with_im else b""}
    if stop_after == 0 or stop_after >= lsdmod.STAGE_SORT:
        got["order"] = b"".join(ctx.fetch(i, lsdmod.DBG_ORDER, wh).tobytes() for i in range(n))
        got["maxgrad"] = b"".join(np.float64(ctx.fetch(i, lsdmod.DBG_MAXGRAD, wh)).tobytes() for i in range(n))
    if stop_after == 0 or stop_after >= lsdmod.STAGE_REGION:
        got["state"] = b"".join(ctx.fetch(i, lsdmod.DBG_STATE, wh).tobytes() for i in range(n))
        # last_sensitivity: the gradient pass's share, and whether the image has any (see the head of this file)
        sens = ctx.last_sensitivity(n).astype(np.int64)
        region = np.array([ctx.fetch(i, lsdmod.DBG_STATS, wh)["near_ties"] for i in range(n)], np.int64)
        got["sensitivity, gradient pass"] = (sens - region).tobytes()
        got["sensitivity, any"] = (sens > 0).tobytes()
    ctx.set_stop_after(0)
    return got


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if a[k] != b[k]]


def check_modes(lsdmod, ctx, batch, **kw):
    """Every mode against the reference mode on `batch`; the reference is run before and after them (it must not move either)."""
    set_mode(ctx, REF)
    ref = run(lsdmod, ctx, batch, **kw)
    bad = []
    for name, mode in MODES.items():
        set_mode(ctx, mode)
        for rep in range(2):
            d = differing(run(lsdmod, ctx, batch, **kw), ref)
            if d:
                bad.append((name, rep, d))
    set_mode(ctx, REF)
    d = differing(run(lsdmod, ctx, batch, **kw), ref)
    if d:
        bad.append(("reference again", d))
    set_mode(ctx, MODES["lines"])
    assert not bad, bad
    return ref


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("n", [1, 3, 9])
def test_crops_in_batches(lsdmod, ctx, images, waves, n):
    ctx.set_region_waves(waves)
    try:
        ref = check_modes(lsdmod, ctx, images[:n])
        counts = np.frombuffer(ref["counts"], np.int32)
        assert (counts > 0).all() and (counts <= 64).all(), counts      # every image has lines, none overflows: the records were compared
        assert ref["lineIm"].count(b"\xff") > 0 and ref["lineIm"].count(b"\x00") > 0
    finally:
        ctx.set_region_waves(0)


@pytest.mark.parametrize("name", ["map1", "mapValue"])
def test_whole_maps(lsdmod, ctx, maps, name):
    ref = check_modes(lsdmod, ctx, maps[name][None], max_lines=256)
    assert 0 < np.frombuffer(ref["counts"], np.int32)[0] <= 256


def test_lists_that_overflow(lsdmod, ctx, images):
    ref = check_modes(lsdmod, ctx, images[:3], max_lines=4)
    assert (np.frombuffer(ref["counts"], np.int32) > 4).all()            # the counts say how many there were; four records each are stored


def test_without_lineim(lsdmod, ctx, images):
    check_modes(lsdmod, ctx, images[:3], with_im=False)


def test_raster_that_is_not_whole_words(lsdmod, ctx, images):
    batch = np.ascontiguousarray(images[:3, :157, :199])
    assert (157 * 199) % 16 != 0
    ref = check_modes(lsdmod, ctx, batch)
    assert (np.frombuffer(ref["counts"], np.int32) > 0).all()


def test_persistent_workgroups(lsdmod, ctx, images):
    ctx.set_region_waves(8)
    ctx.debug_set_tuning("GROUPS", 2)                       # nine images through two workgroups: the loop around the image's code
    try:
        check_modes(lsdmod, ctx, images)
    finally:
        ctx.debug_set_tuning("GROUPS", -1)
        ctx.set_region_waves(0)


def test_launches_of_different_n_in_a_row(lsdmod, ctx, images):
    """9, 3, 1, 9 images on one context without anything in between: the records of a larger batch before lie in the workspace the
    smaller one's workgroups read their own from."""
    seq = [images, images[3:6], images[8:9], images]
    set_mode(ctx, REF)
    refs = [run(lsdmod, ctx, b) for b in seq]
    assert not differing(refs[0], refs[3])
    for name, mode in MODES.items():
        set_mode(ctx, mode)
        for rnd in range(2):
            for b, ref in zip(seq, refs):
                assert not differing(run(lsdmod, ctx, b), ref), (name, rnd, len(b))
    set_mode(ctx, MODES["lines"])


@pytest.mark.parametrize("stage", ["STAGE_SORT", "STAGE_REGION"])
def test_pipelines_cut_short(lsdmod, ctx, images, stage):
    """A call that stops after the sort or the region stage between whole ones: it leaves the line records alone (stopping at the region
    stage: neither the kernel nor the region stage writes lines), and the whole call behind it is what it was."""
    stop = getattr(lsdmod, stage)
    batch = images[:3]
    set_mode(ctx, REF)
    ref_cut = run(lsdmod, ctx, batch, stop_after=stop)
    ref_cut2 = run(lsdmod, ctx, images[:2], stop_after=stop)
    ref_all = run(lsdmod, ctx, batch)
    assert ref_cut["lines"] == b"\xff" * len(ref_cut["lines"])
    if stop == lsdmod.STAGE_REGION:
        assert ref_cut["counts"] == ref_all["counts"] and ref_cut["state"] == ref_all["state"]
    for name, mode in MODES.items():
        set_mode(ctx, mode)
        for rnd in range(2):
            assert not differing(run(lsdmod, ctx, batch), ref_all), (name, rnd, "whole")
            assert not differing(run(lsdmod, ctx, batch, stop_after=stop), ref_cut), (name, rnd, "cut")
            assert not differing(run(lsdmod, ctx, images[:2], stop_after=stop), ref_cut2), (name, rnd, "cut, n 2")
            assert not differing(run(lsdmod, ctx, batch), ref_all), (name, rnd, "whole behind cut")
    set_mode(ctx, MODES["lines"])


def test_cost_history(lsdmod, ctx, images):
    """The images taken in the order of the last launch's counter records (lsd_set_cost_history): a workgroup writes the lines of the image
    the order gave it, not of the one at its own index (the clocks the order is made from differ from run to run; no result does)."""
    set_mode(ctx, REF)
    ref = run(lsdmod, ctx, images)
    ctx.set_cost_history(1)
    try:
        for name, mode in list(MODES.items()) + [("reference", REF)]:
            set_mode(ctx, mode)
            for rnd in range(3):                            # the first may still order by the list lengths
                assert not differing(run(lsdmod, ctx, images), ref), (name, rnd)
    finally:
        ctx.set_cost_history(0)
        set_mode(ctx, MODES["lines"])


def test_timings_report_fused_lines_as_zero(lsdmod, ctx, images):
    set_mode(ctx, MODES["lines"])
    run(lsdmod, ctx, images[:3])
    t = ctx.timings()
    assert t["lines"] == 0.0 and t["gradient"] == 0.0 and t["region"] > 0.0, t
    set_mode(ctx, REF)
    run(lsdmod, ctx, images[:3])
    assert ctx.timings()["lines"] > 0.0
    set_mode(ctx, MODES["lines"])
