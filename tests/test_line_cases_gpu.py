"""The line-record campaign on the device (-m gpu; tests/line_cases.py): K5 (k_lines.hip) and the batch compaction (k_scan_counts /
k_compact_lines) against the correctly rounded build of the oracle (oracle.lib_cr()), to the bit: every byte of every record, the
tail padding of structLinesInfo included, lineIm and usedMap.

  a  every case through lsd_run;
  b  every case through lsd_enqueue_batch_device into a record buffer filled with 0xFF: the records, their padding word, and
     nothing written behind them; with and without a lineIm;
  c  the clamp count > max_lines: the true count, the first records, nothing behind them, the raster of the kept records only;
  d  K5 alone: k, b, len, orient and the raster are the restatement of myLSD.cpp:280-368 applied to the DEVICE's own end points
     (a failure of a without a failure of d is a deviation of the region stage or of the rescale, not of K5);
  e  the compaction through lsd_run_batch: n = 1, 255, 256, 257, 513 images, maps without lines first, last and in between, with the
     default host capacity and with a capacity of 2 (LSD_ERR_CAPACITY, the first records of every image);
  f  K5 on hand-made end points (lsd_debug_lines, line_cases.HAND_RECS): what no map reaches -- samples exactly half-way between two
     cells in either walk (round, not rint), and k NaN.

Every test collects what differs over all cases and asserts once, so a failure names the cases and fields."""
import numpy as np
import pytest

import line_cases as lc

pytestmark = pytest.mark.gpu

FIELDS = ("k", "b", "dx", "dy", "x1", "y1", "x2", "y2", "len", "orient", "_pad")
GUARD = 4                                                   # records of 0xFF kept behind the capacity


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def differing_fields(got, ref):
    """Names of the fields whose bytes differ ("count" if the lengths do)."""
    if len(got) != len(ref):
        return ["count %d != %d" % (len(got), len(ref))]
    return [f for f in FIELDS if np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(ref[f]).tobytes()]


@pytest.fixture(scope="module")
def device_runs(lsdmod, ctx, oracle):
    """Every case once through lsd_run: {case: (lines, lineIm, usedMap, the rewritten map)}."""
    out = {}
    for c in lc.CASES:
        ref = lc.reference(c, oracle)
        m = c.map.copy()
        lines, im = ctx.run(m, lsdmod.make_params(**c.params))
        used = (ctx.fetch(0, lsdmod.DBG_STATE, (ref["w"], ref["h"])) & 3).astype(np.uint8) if ref["used"] is not None else None
        out[repr(c)] = (lines, im, used, m)
    return out


def test_a_records_raster_and_used_map_equal_the_correctly_rounded_oracle(device_runs, oracle):
    bad = []
    for c in lc.CASES:
        ref = lc.reference(c, oracle)
        lines, im, used, m = device_runs[repr(c)]
        what = differing_fields(lines, ref["lines"])
        if lines.tobytes() != ref["lines"].tobytes() and not what:
            what.append("bytes")
        if not np.array_equal(im, ref["lineIm"]):
            what.append("lineIm")
        if ref["used"] is not None and not np.array_equal(used, ref["used"]):
            what.append("usedMap")
        if not np.array_equal(m, ref["map"]):
            what.append("map")
        if what:
            bad.append((repr(c), what))
    assert not bad, bad


def test_d_k5_alone_equals_the_restatement_on_the_device_end_points(device_runs):
    bad = []
    for c in lc.CASES:
        lines, im, _, _ = device_runs[repr(c)]
        k, b, ln, orient = lc.fields_from_endpoints(lines["x1"], lines["y1"], lines["x2"], lines["y2"])
        what = [name for name, v in (("k", k), ("b", b), ("len", ln), ("orient", orient))
                if v.tobytes() != np.ascontiguousarray(lines[name]).tobytes()]
        if lines["_pad"].any():
            what.append("_pad")
        if not np.array_equal(im, lc.raster(lines, *c.map.shape)):
            what.append("lineIm")
        if what:
            bad.append((repr(c), what))
    assert not bad, bad


def enqueue(torch, ctx, lsdmod, case, max_lines, with_im):
    """One case through the device entry point -> (count, the whole record buffer as bytes [max_lines + GUARD, 80], lineIm or None);
    the buffer was filled with 0xFF before the call."""
    rows, cols = case.map.shape
    d_map = torch.from_numpy(case.map.copy()).cuda()
    d_lines = torch.full(((max_lines + GUARD) * 80,), 0xFF, dtype=torch.uint8, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_im = torch.full((rows, cols), 0x55, dtype=torch.uint8, device="cuda") if with_im else None
    ctx.enqueue_device(d_map.data_ptr(), 1, cols, rows, d_lines.data_ptr(), max_lines, d_count.data_ptr(),
                       d_line_ims=d_im.data_ptr() if with_im else None, params=lsdmod.make_params(**case.params),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_map.cpu().numpy(), case.map)    # read-only without LSD_FLAG_WRITEBACK_MAP
    return int(d_count.item()), d_lines.cpu().numpy().reshape(-1, 80), d_im.cpu().numpy() if with_im else None


def test_b_device_entry_writes_the_records_with_their_padding_and_nothing_else(lsdmod, ctx, oracle):
    import torch
    max_lines = 32
    bad = []
    for c in lc.CASES:
        ref = lc.reference(c, oracle)
        want = ref["lines"]
        assert len(want) <= max_lines and not want["_pad"].any()
        got = {}
        for with_im in (True, False):
            n, buf, im = enqueue(torch, ctx, lsdmod, c, max_lines, with_im)
            what = []
            if n != len(want):
                what.append("count %d != %d" % (n, len(want)))
            else:
                what += differing_fields(buf[:n].copy().view(lsdmod.LINE_DTYPE).reshape(-1), want)
            if not (buf[min(max(n, 0), max_lines):] == 0xFF).all():
                what.append("bytes behind the records")
            if with_im and not np.array_equal(im, ref["lineIm"]):
                what.append("lineIm")
            got[with_im] = buf.tobytes()
            if what:
                bad.append((repr(c), "with lineIm" if with_im else "without lineIm", what))
        if got[True] != got[False]:
            bad.append((repr(c), "the records depend on d_line_ims"))
    assert not bad, bad


@pytest.mark.parametrize("name", ["noise/seed1_96x128@0.5", "aimed/comb@0.5"])
@pytest.mark.parametrize("max_lines", [2, 5])
def test_c_clamp_keeps_the_first_records_and_rasters_only_those(name, max_lines, lsdmod, ctx, oracle):
    import torch
    c = lc.BY_NAME[name]
    ref = lc.reference(c, oracle)
    assert len(ref["lines"]) > 8
    n, buf, im = enqueue(torch, ctx, lsdmod, c, max_lines, True)
    assert n == len(ref["lines"])                           # the true count
    kept = buf[:max_lines].copy().view(lsdmod.LINE_DTYPE).reshape(-1)
    assert differing_fields(kept, ref["lines"][:max_lines]) == [] and kept.tobytes() == ref["lines"][:max_lines].tobytes()
    assert (buf[max_lines:] == 0xFF).all()
    assert np.array_equal(im, lc.raster(ref["lines"][:max_lines], *c.map.shape))
    assert not np.array_equal(im, ref["lineIm"])            # (the dropped lines do leave pixels in the full raster)


def test_e_compaction_through_run_batch(lsdmod, ctx, oracle):
    cases = lc.batch_cases()
    params = lsdmod.make_params(sca=lc.BATCH_SCA)
    single = []
    for c in cases:                                         # the single-image results, and they are the oracle's
        ref = lc.reference(c, oracle)
        m = c.map.copy()
        lines, im = ctx.run(m, params)
        assert lines.tobytes() == ref["lines"].tobytes() and np.array_equal(im, ref["lineIm"]) and np.array_equal(m, ref["map"]), repr(c)
        single.append((lines, im, m))
    for n in lc.BATCH_SIZES:
        idx = lc.batch_indices(n)
        maps = np.stack([cases[i].map for i in idx])
        counts = np.array([len(single[i][0]) for i in idx])
        # the default capacity
        got_maps = maps.copy()
        lines, offsets, ims = ctx.run_batch(got_maps, params)
        assert offsets.dtype == np.int32 and np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)])), n
        assert len(lines) == offsets[n] == counts.sum()
        assert lines.tobytes() == b"".join(single[i][0].tobytes() for i in idx), n
        for j in range(n):
            assert lines[offsets[j]:offsets[j + 1]].tobytes() == single[idx[j]][0].tobytes(), (n, j)
        assert np.array_equal(ims, np.stack([single[i][1] for i in idx])) and np.array_equal(got_maps, np.stack([single[i][2] for i in idx])), n
        # a capacity of 2 (after the run above, so the staging buffers are those of the default capacity)
        ctx.set_host_max_lines(2)
        try:
            if (counts > 2).any():
                with pytest.raises(lsdmod.LsdError) as e:
                    ctx.run_batch(maps.copy(), params)
                assert e.value.status == lsdmod.LSD_ERR_CAPACITY and e.value.partial is not None
                lines2, offsets2, ims2 = e.value.partial
            else:
                lines2, offsets2, ims2 = ctx.run_batch(maps.copy(), params)
        finally:
            ctx.set_host_max_lines(lsdmod.HOST_MAX_LINES_DEFAULT)
        kept = np.minimum(counts, 2)
        assert np.array_equal(offsets2, np.concatenate([[0], np.cumsum(kept)])), n
        assert len(lines2) == offsets2[n]
        assert lines2.tobytes() == b"".join(single[i][0][:2].tobytes() for i in idx), n
        want_ims = np.stack([lc.raster(single[i][0][:2], 96, 128) for i in range(len(cases))])
        assert np.array_equal(ims2, want_ims[idx]), n


def test_f_k5_on_hand_made_end_points_rounds_halves_away_and_takes_k_nan(ctx):
    """The device's K5 on line_cases.HAND_RECS against the restatement.  Every field but dx / dy (they need the correctly rounded
    functions; the cases hold them) is compared to the bit, k and b of the k-NaN record as NaN: IEEE 754 leaves the sign and payload
    of the NaN of 0 / 0 open, and x86 sets the sign bit where other hardware does not."""
    recs = lc.HAND_RECS
    lines, im = ctx.debug_lines(recs, lc.HAND_ROWS, lc.HAND_COLS)
    lines2, none = ctx.debug_lines(recs, lc.HAND_ROWS, lc.HAND_COLS, want_lineim=False)
    assert none is None and lines2.tobytes() == lines.tobytes()
    k, b, ln, orient = lc.fields_from_endpoints(*recs.T)
    nan = np.isnan(k)
    assert nan.sum() == 1 and np.isnan(b[nan]).all()                      # (the restatement's own k NaN record)
    bad = []
    for name, v in (("x1", recs[:, 0]), ("y1", recs[:, 1]), ("x2", recs[:, 2]), ("y2", recs[:, 3]), ("len", ln), ("orient", orient)):
        if np.ascontiguousarray(lines[name]).tobytes() != np.ascontiguousarray(v).tobytes():
            bad.append(name)
    for name, v in (("k", k), ("b", b)):
        got = np.ascontiguousarray(lines[name])
        if got[~nan].tobytes() != v[~nan].tobytes() or not np.isnan(got[nan]).all():
            bad.append(name)
    if not (np.isnan(lines["dx"][nan]).all() and np.isnan(lines["dy"][nan]).all()):    # sind / cosd of NaN
        bad.append("dx dy of k NaN")
    if not np.isfinite(lines["dx"][~nan]).all() or not np.isfinite(lines["dy"][~nan]).all():
        bad.append("dx dy")
    if lines["_pad"].any():
        bad.append("_pad")
    want = lc.raster(lines[:0], lc.HAND_ROWS, lc.HAND_COLS)
    for i, r in enumerate(recs):                                          # record by record, so a failure names the record
        one = np.zeros(1, lines.dtype)
        one["x1"], one["y1"], one["x2"], one["y2"] = r
        one_im = lc.raster(one, lc.HAND_ROWS, lc.HAND_COLS)
        if not (im[one_im == 255] == 255).all():
            bad.append("lineIm lacks pixels of record %d %s" % (i, r))
        want |= one_im
    if not np.array_equal(im, want):
        bad.append("lineIm")
    assert not bad, bad
