"""The front-end campaign on the device (tests/front_cases.py; -m gpu): K1, K2, the fused k_front and K3 with the pipeline cut behind
the sort (lsd_set_stop_after(LSD_STAGE_SORT)): no region code runs.

Every image of every case, through the device entry point, with the two-kernel path and -- where the 17 taps apply -- the fused kernel:
  * GaussImage, magMap, maxGrad, the list length, the sorted list and its bin values bit for bit against BOTH builds of the oracle
    (tests/test_front_cases_cpu.py shows that they agree on these);
  * degMap bit for bit against the correctly rounded build (oracle.lib_cr()) and within DEG_ULP of glibc's;
  * the whole packed pixel word (LSD_DBG_PW: the fp32 angle and the code) against front_cases.pw_of, STATE against usedMap;
  * the (sin, cos) table (LSD_DBG_SINCOS) at every pixel of code 0: (0, 1) on row 0 / column 0, cr_sin / cr_cos of the angle elsewhere,
    to the bit;
  * the order's properties on their own: a permutation of the kept set, bin values non-increasing, raster order inside a bin;
  * the gradient pass's near-tie count (LSD_DBG_GRAD_TIES) against front_cases.grad_ties on the oracle's arrays;
  * fused and two-kernel runs identical byte for byte;
  * every image of a batch equal to the same image run alone.
Every measured call starts from poisoned arrays: a call on other content of the same shape comes first, then
lsd_debug_poison_front (_run says why).  The sequences run their calls one after the other on one context, the first one primed
that way, the later ones directly after the call before; the 257-image batch and every image of the pseBin cases also run the
whole pipeline.  One context per module; the oracle's answers are computed once (front_cases.reference).

GPU time of this file on an MI355X: see DESIGN.md 2.2."""
import ctypes as C

import numpy as np
import pytest

import front_cases as fc
import grid_cases as gc
from test_parity_gpu import DEG_ULP, assert_lines_close, full_check, ulps

pytestmark = pytest.mark.gpu

MAX_LINES = 256
SINGLE = [c.name for c in fc.CASES]
BIN_CASES = [c.name for c in fc.CASES if c.name.startswith(("bins_", "nb0_", "edge_", "top_bit_"))]


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


class _stop_after:
    def __init__(self, lsdmod, ctx, stage):
        self.lsdmod, self.ctx, self.stage = lsdmod, ctx, stage

    def __enter__(self):
        self.ctx.set_stop_after(self.stage)

    def __exit__(self, *exc):
        self.ctx.set_stop_after(self.lsdmod.STAGE_ALL)
        self.ctx.set_fused_front(1)


def _run(lsdmod, ctx, batch, params, fused, full=False, prime=True):
    """One call of the device entry point -> what the front end left, per image (prime=False: directly after the context's last call,
    for the sequences)."""
    import torch
    n, rows, cols = batch.shape
    ctx.set_fused_front(fused)
    P = lsdmod.make_params(**params)
    # Nothing clears magMap, degMap, the packed words or the (sin, cos) table between calls, and both paths store to the same
    # addresses: a call after one on the same batch would find its answers in place.  So a call on other content of the same shape
    # and size comes first (it sizes the workspace), then every array the front end fills is poisoned (0xFF bytes), then the call
    # that is measured: a store it leaves out shows.
    if prime:
        d_other = torch.from_numpy(fc.scrambled(batch)).cuda()
        d_scratch = torch.zeros((n, MAX_LINES, 10), dtype=torch.int64, device="cuda")
        d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx.enqueue_device(d_other.data_ptr(), n, cols, rows, d_scratch.data_ptr(), MAX_LINES, d_cnt.data_ptr(), params=P,
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ctx.debug_poison_front()
    d_maps = torch.from_numpy(batch.copy()).cuda()
    d_lines = torch.zeros((n, MAX_LINES, 10), dtype=torch.int64, device="cuda")
    d_counts = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    d_ims = torch.full((n, rows, cols), 7, dtype=torch.uint8, device="cuda")
    ctx.enqueue_device(d_maps.data_ptr(), n, cols, rows, d_lines.data_ptr(), MAX_LINES, d_counts.data_ptr(), d_line_ims=d_ims.data_ptr(),
                       params=P, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    wh = lsdmod.scaled_size(cols, rows, P.sca)
    out = {"wh": wh, "counts": d_counts.cpu().numpy(), "timings": ctx.timings()}
    for name, what in (("gauss", lsdmod.DBG_GAUSS), ("mag", lsdmod.DBG_MAG), ("deg", lsdmod.DBG_DEG), ("pw", lsdmod.DBG_PW),
                       ("state", lsdmod.DBG_STATE), ("sincos", lsdmod.DBG_SINCOS), ("maxgrad", lsdmod.DBG_MAXGRAD), ("nb", lsdmod.DBG_NB),
                       ("order", lsdmod.DBG_ORDER), ("order_val", lsdmod.DBG_ORDER_VAL), ("grad_ties", lsdmod.DBG_GRAD_TIES)):
        out[name] = [ctx.fetch(i, what, wh) for i in range(n)]                            # (GAUSS reads d_maps: still alive here)
    if full:
        out["lines"], out["line_ims"] = d_lines.cpu().numpy(), d_ims.cpu().numpy()
    assert np.array_equal(d_maps.cpu().numpy(), batch)                                    # read-only without the write-back flag
    return out


_sincos = {}


def _want_sincos(case, i, d):
    """(sin, cos) of the correctly rounded oracle's angle at every pixel of code 0 after the gradient pass, from the same library's
    cr_sin / cr_cos; computed once per image."""
    key = (case.name, i)
    if key not in _sincos:
        free = d["used0"] == 0
        L = gc.cr()
        a = d["deg"][free]
        _sincos[key] = (free, np.array([[L.cr_sin(float(v)), L.cr_cos(float(v))] for v in a], np.float64).reshape(-1, 2))
    return _sincos[key]


_ties = {}


def _want_ties(case, i, d):
    key = case.batch[i].tobytes() + repr(sorted(case.params.items())).encode()
    if key not in _ties:
        L = gc.cr()
        L.cr_atan2.restype, L.cr_atan2.argtypes = C.c_double, [C.c_double, C.c_double]
        _ties[key] = fc.grad_ties(d, L.cr_atan2)
    return _ties[key]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _check_image(case, i, got, cr, glibc, after_sort=True):
    """Image i of a run against the oracle's two builds (after_sort: the pipeline ended behind K3, the codes are K2's)."""
    tag = (case.name, i)
    w, h = cr["w"], cr["h"]
    assert got["wh"] == (w, h), tag
    for ref in (cr, glibc):
        assert _bits(got["gauss"][i]) == _bits(ref["gauss"]), tag
        assert _bits(got["mag"][i]) == _bits(ref["mag"]), tag
        assert _bits(np.float64(got["maxgrad"][i])) == _bits(np.float64(ref["maxGrad"])), tag
        assert got["nb"][i] == ref["nb"] == len(got["order"][i]) == len(got["order_val"][i]), tag
    # the order's properties on their own, then the list itself
    order, val = got["order"][i].astype(np.int64), got["order_val"][i].astype(np.int64)
    kept_px, kept_v = fc.sort_rule(cr["mag"], cr["maxGrad"], case.params["pseBin"])
    assert np.array_equal(np.sort(order), np.sort(kept_px)), ("not a permutation of the kept set", tag)
    assert (np.diff(val) <= 0).all(), ("bin values increase", tag)
    assert (np.diff(order)[np.diff(val) == 0] > 0).all(), ("raster order inside a bin", tag)
    for ref in (cr, glibc):
        assert np.array_equal(order, ref["ord_y"].astype(np.int64) * w + ref["ord_x"]), tag
        assert np.array_equal(val, ref["ord_v"]), tag
    # the angle: to the bit against the correctly rounded build
    assert _bits(got["deg"][i]) == _bits(cr["deg"]), (tag, int((got["deg"][i] != cr["deg"]).sum()), int(ulps(got["deg"][i], cr["deg"]).max()))
    assert ulps(got["deg"][i], glibc["deg"]).max() <= DEG_ULP, tag
    assert got["grad_ties"][i] == _want_ties(case, i, cr), tag                            # the gradient pass's near ties, restated
    if after_sort:
        assert np.array_equal(got["state"][i].astype(np.uint8), cr["used0"]), tag
        assert np.array_equal(got["pw"][i], fc.pw_of(cr["deg"], cr["used0"])), tag
        free, want = _want_sincos(case, i, cr)
        assert np.array_equal(got["pw"][i] & 3 == 0, free), tag
        sc = got["sincos"][i]
        assert _bits(sc[free]) == _bits(want), (tag, int((sc[free] != want).any(1).sum()))
        border = np.zeros((h, w), bool)
        border[0], border[:, 0] = True, True
        assert free[border].all() and _bits(sc[border]) == _bits(np.tile(np.array([0.0, 1.0]), (int(border.sum()), 1))), tag
        assert got["counts"][i] == 0, tag
    else:
        assert np.array_equal(got["pw"][i] & np.uint32(0xfffffffc), fc.pw_of(cr["deg"], 0)), tag


def _same_bits(a, b, ia, ib, tag):
    """Image ia of run a and image ib of run b, byte for byte ((sin, cos) where the code is 0: the rest is not defined)."""
    for k in ("gauss", "mag", "deg", "pw", "state", "order", "order_val"):
        assert _bits(a[k][ia]) == _bits(b[k][ib]), (k, tag)
    for k in ("nb", "grad_ties"):
        assert a[k][ia] == b[k][ib], (k, tag)
    assert _bits(np.float64(a["maxgrad"][ia])) == _bits(np.float64(b["maxgrad"][ib])), tag
    free = a["pw"][ia] & 3 == 0
    assert _bits(a["sincos"][ia][free]) == _bits(b["sincos"][ib][free]), ("sincos", tag)


def _case_through_the_front_end(lsdmod, ctx, oracle, case, alone=True):
    cr, glibc = fc.reference(case, oracle), fc.reference(case, oracle, cr=False)
    runs = []
    for fused in ((0, 1) if case.fused_applies else (0,)):
        got = _run(lsdmod, ctx, case.batch, case.params, fused)
        assert (got["timings"]["gradient"] == 0.0) == bool(fused), case                   # the path the setting asks for
        for i in range(len(case.batch)):
            _check_image(case, i, got, cr[i], glibc[i])
        runs.append(got)
    for i in range(len(case.batch)):
        if len(runs) == 2:
            _same_bits(runs[0], runs[1], i, i, (case.name, i, "fused against two kernels"))
    if alone and len(case.batch) > 1:
        seen = set()
        for i, im in enumerate(case.batch):
            if im.tobytes() not in seen:
                seen.add(im.tobytes())
                one = _run(lsdmod, ctx, im[None], case.params, 1)
                _same_bits(runs[-1], one, i, 0, (case.name, i, "in the batch against alone"))
    return runs[-1]


@pytest.mark.parametrize("name", SINGLE)
def test_case_against_both_oracle_builds(name, lsdmod, ctx, oracle):
    with _stop_after(lsdmod, ctx, lsdmod.STAGE_SORT):
        _case_through_the_front_end(lsdmod, ctx, oracle, fc.BY_NAME[name])


@pytest.mark.parametrize("name,calls", fc.SEQUENCES)
@pytest.mark.parametrize("fused", (0, 1))
def test_sequence_of_calls_on_one_context(name, calls, fused, lsdmod, ctx, oracle):
    """A blank image at the batch index where the call before, at the same shape, had a dense one (and the other way round): its
    maximum and its list length are this call's, not the last one's."""
    with _stop_after(lsdmod, ctx, lsdmod.STAGE_SORT):
        for k, cname in enumerate(calls):
            case = fc.BY_NAME[cname]
            cr, glibc = fc.reference(case, oracle), fc.reference(case, oracle, cr=False)
            got = _run(lsdmod, ctx, case.batch, case.params, fused, prime=k == 0)          # (each later call directly after the one before)
            for i in range(len(case.batch)):
                _check_image(case, i, got, cr[i], glibc[i])
                if not case.batch[i].any():
                    assert got["nb"][i] == 0 and got["maxgrad"][i] == 0 and not got["mag"][i].any(), (cname, i)


def test_batch_of_257_through_the_whole_pipeline(lsdmod, ctx, oracle):
    """More images than k_order's 256 threads, equal images among them (equal keys), some blank: counts, usedMap and lineIm bit for
    bit, the lines within assert_lines_close, the front end's arrays as in every other case, on either path.  (The same batch cut
    behind the sort, with every distinct image also alone, is one of test_case_against_both_oracle_builds' cases.)"""
    case = fc.BY_NAME["batch_257"]
    cr, glibc = fc.reference(case, oracle), fc.reference(case, oracle, cr=False)
    try:
        runs = [_run(lsdmod, ctx, case.batch, case.params, fused, full=True) for fused in (0, 1)]
    finally:
        ctx.set_fused_front(1)
    assert len(case.batch) == 257
    for got, i in ((g, i) for g in runs for i in range(257)):
        _check_image(case, i, got, cr[i], glibc[i], after_sort=False)
        ref = glibc[i]
        assert got["counts"][i] == len(ref["lines"]) <= MAX_LINES, i
        assert np.array_equal(got["state"][i].astype(np.uint8), ref["used"]), i
        assert np.array_equal(got["line_ims"][i], ref["lineIm"]), i
        lines = got["lines"][i, :got["counts"][i]].copy().view(np.uint8).reshape(-1, 80).view(lsdmod.LINE_DTYPE).reshape(-1)
        assert_lines_close(lines, ref["lines"])
    for i in range(257):
        for k in ("gauss", "mag", "deg", "order", "order_val", "state", "pw"):
            assert _bits(runs[0][k][i]) == _bits(runs[1][k][i]), (k, i)
        assert runs[0]["grad_ties"][i] == runs[1]["grad_ties"][i] and runs[0]["counts"][i] == runs[1]["counts"][i], i
        free = cr[i]["used0"] == 0                                                         # (the region stage does not touch the table)
        assert _bits(runs[0]["sincos"][i][free]) == _bits(runs[1]["sincos"][i][free]) == _bits(_want_sincos(case, i, cr[i])[1]), i


@pytest.mark.parametrize("name", BIN_CASES)
def test_bin_cases_through_the_whole_pipeline(name, lsdmod, ctx, oracle):
    case = fc.BY_NAME[name]
    for im in case.batch:
        full_check(lsdmod, ctx, oracle, np.array(im), lsdmod.make_params(**case.params), kw=case.params)
