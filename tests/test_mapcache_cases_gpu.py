"""The createMapCache campaign (tests/mapcache_cases.py) on the device: every case through lsd_map_cache, the batches through
lsd_enqueue_map_cache_device on both of its paths (one workgroup per map; a map spread over G workgroups with k_mc_finish behind the
planned levels), against the oracle byte for byte.  tests/test_mapcache_cases_cpu.py shows what the cases reach."""
import numpy as np
import pytest

import mapcache_cases as mc
from test_map_update_gpu import Outputs, dev, grid_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


_want = {}


def want_of(oracle, c):
    if c.name not in _want:
        _want[c.name] = oracle.map_cache(c.map.copy(), c.res, c.z)
    return _want[c.name]


def same_bytes(got, want, what):
    """Byte equality (-0.0 and NaN would show); on a difference, the first differing cells."""
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        raise AssertionError("%s: %d cells differ, first %s: got %r want %r" %
                             (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("cls", mc.CLASSES)
def test_cases(cls, ctx, oracle):
    for c in mc.cases(cls):
        m = c.map.copy()
        got = ctx.map_cache(m, c.res, c.z)
        same_bytes(got, want_of(oracle, c), repr(c))
        assert np.array_equal(m, c.map), c                                       # the caller's map is unchanged


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_batch(ctx, maps, fill=0xFF):
    """maps uint8 [n, rows, cols] through lsd_enqueue_map_cache_device into an output pre-filled with 0xFF bytes (NaN)."""
    import torch
    n, rows, cols = maps.shape
    d = dev(maps)
    out = torch.full((n * rows * cols * 8,), fill, dtype=torch.uint8, device="cuda")
    ctx.enqueue_map_cache_device(d.data_ptr(), n, cols, rows, mc.BATCH_RES, mc.BATCH_Z, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), maps)
    return out.cpu().numpy().view(np.float64).reshape(n, rows, cols)


_batch_want = {}


def batch_want(oracle, maps):
    out = np.empty(maps.shape, np.float64)
    for i, m in enumerate(maps):
        key = m.tobytes()
        if key not in _batch_want:
            _batch_want[key] = oracle.map_cache(m.copy(), mc.BATCH_RES, mc.BATCH_Z)
        out[i] = _batch_want[key]
    return out


@pytest.mark.parametrize("name", mc.BATCHES)
def test_batches(name, ctx, oracle):
    """one_workgroup: num_cus // 2 + 1 maps, G < 4, k_mapcache; smallest_spread: G = 4; three: G capped at 64."""
    cus = num_cus()
    maps = mc.batch(name, cus)
    got = run_batch(ctx, maps)
    want = batch_want(oracle, maps)
    for i in range(len(maps)):
        same_bytes(got[i], want[i], "%s map %d" % (name, i))
    if name == "one_workgroup":                              # the same maps on the spread path, in groups that spread (G >= 4)
        step = min(64, cus // 2)
        for i0 in range(0, len(maps), step):
            spread = run_batch(ctx, maps[i0:i0 + step])
            same_bytes(spread, got[i0:i0 + step], "spread maps %d.." % i0)


def test_row_stride_larger_than_cols(ctx, oracle):
    c = mc.BY_NAME["detour_r10_witness"]
    rows, cols = c.map.shape
    wide = np.full((rows, cols + 29), 1, np.uint8)           # occupied cells beyond the row: read by a kernel that ignores the stride
    wide[:, :cols] = c.map
    view = wide[:, :cols]
    assert view.strides[0] == cols + 29 and not view.flags.c_contiguous
    same_bytes(ctx.map_cache(view, c.res, c.z), want_of(oracle, c), "strided")
    assert (wide[:, cols:] == 1).all() and np.array_equal(view, c.map)


def test_detour_map_through_the_map_update(lsdmod, ctx, oracle):
    """lsd_enqueue_map_update_device on the grid of a detour map, with the callback's cap of 2.0: its mapCache is the oracle's."""
    import torch
    c = mc.BY_NAME["detour_z2_r20"]
    assert c.z == 2.0
    rows, cols = c.map.shape
    grid = grid_of(c.map)
    assert np.array_equal(oracle.occupancy_to_map(grid), c.map)
    ctx.reserve_map_update(cols, rows)
    out = Outputs(rows, cols)
    ctx.enqueue_map_update_device(dev(grid).data_ptr(), cols, rows, c.res, c.z, out.map.data_ptr(), out.mc.data_ptr(), out.lines.data_ptr(),
                                  out.max_lines, out.count.data_ptr(), out.line_im.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same_bytes(out.mc.cpu().numpy().view(np.float64).reshape(rows, cols), want_of(oracle, c), "map update")
    n = int(out.count.cpu().numpy().view(np.int32)[0])
    assert 0 <= n <= out.max_lines


def test_workspace_reuse(ctx, oracle):
    """A large case, a tiny one and the large one again on one context: stale claim words or frontier counts would show.  The same
    for the one-workgroup kernel: its batch, three maps, its batch again."""
    big, tiny = mc.BY_NAME["lattice3_96x96"], mc.BY_NAME["3x3_corners"]
    first = ctx.map_cache(big.map.copy(), big.res, big.z)
    same_bytes(first, want_of(oracle, big), "large")
    same_bytes(ctx.map_cache(tiny.map.copy(), tiny.res, tiny.z), want_of(oracle, tiny), "tiny")
    same_bytes(ctx.map_cache(big.map.copy(), big.res, big.z), first, "large again")
    cus = num_cus()
    maps, three = mc.batch("one_workgroup", cus), mc.batch("three", cus)
    a = run_batch(ctx, maps)
    same_bytes(run_batch(ctx, three), batch_want(oracle, three), "three")
    b = run_batch(ctx, maps[::-1].copy())[::-1]              # and in the other order: every map on another image's scratch
    same_bytes(b, a, "one workgroup again")
    same_bytes(a, batch_want(oracle, maps), "one workgroup")
