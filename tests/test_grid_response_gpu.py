"""The response around a correlative match on the device (csrc/k_gridresponse.hip: lsd_enqueue_grid_response_device, lsd_grid_response;
GridMapper.response_device / match*(response=); Localizer.refine_and_integrate_last_tick(response=)) against the restatement of
tests/grid_response_cases.py.  The rule is integer sums and one fp64 division per output, without an iteration order, so every comparison
is byte equality: the records' 192 bytes and the whole volume."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import grid_cases as gc
import grid_match_cases as gm
import grid_response_cases as gr

pytestmark = pytest.mark.gpu

GUARD = 256                                    # bytes behind every output
FILL = 0x5A


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_long(lsdmod):
    c = lsdmod.Context(0)
    c.set_scan_capacity(2048)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """(case, records, volume) of the campaign: the restatement, computed once."""
    return [(c,) + gr.run_case(c)[:2] for c in gr.campaign()]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n_bytes):
    """A CUDA uint8 tensor of n_bytes + GUARD bytes of the fill pattern."""
    import torch
    return torch.full((n_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def back(t, n_bytes):
    """(the first n_bytes, True if the guard is untouched)."""
    a = t.cpu().numpy()
    return a[:n_bytes], bool((a[n_bytes:] == FILL).all())


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def mp_of(case):
    return (case["cols"], case["rows"], case["resol"], -1.5, 2.25)


def device_response(lsdmod, cx, case, d_out, d_vol, d_poses=None, pitch=24, d_records=None):
    import torch
    d_sc, d_ln, d_co = dev(case["scans"]), dev(case["lens"]), dev(case["corr"])
    d_po = dev(case["poses"]) if d_poses is None else d_poses
    d_re = dev(case["records"].view(np.uint8)) if d_records is None else d_records
    st = cx.L.lsd_enqueue_grid_response_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), len(case["lens"]), case["scans"].shape[1], d_po.data_ptr(), pitch,
                                               d_re.data_ptr(), lsdmod.lsd_map_param(*mp_of(case)), case["range_max"], d_co.data_ptr(),
                                               case["search"]["ang_step"], lsdmod.grid_response(case["response"]), d_out.data_ptr(),
                                               d_vol.data_ptr() if d_vol is not None else None, stream())
    torch.cuda.synchronize()
    return st


# ---- 1. the campaign through both entries, with and without the volume -------------------------------------------------------------------
def test_campaign_device_entry(lsdmod, ctx, ctx_long, cases):
    for case, want, want_vol in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        n = len(case["lens"])
        assert lsdmod.load_library().lsd_grid_response_volume_bytes(n, lsdmod.grid_response(case["response"])) == want_vol.nbytes
        d_out, d_vol = filled(192 * n), filled(want_vol.nbytes)
        assert device_response(lsdmod, cx, case, d_out, d_vol) == lsdmod.LSD_OK, case["name"]
        got, ok = back(d_out, 192 * n)
        vol, ok_vol = back(d_vol, want_vol.nbytes)
        assert ok and ok_vol, case["name"]
        where = np.argwhere(vol.view(np.uint32).reshape(want_vol.shape) != want_vol)
        assert vol.tobytes() == want_vol.tobytes(), (case["name"], "first difference at (scan, a', j', i') =", where[:1])
        assert got.tobytes() == want.tobytes(), (case["name"], got.view(gr.RESPONSE_DTYPE), want)
        d_out = filled(192 * n)                                           # the volume in the context's workspace
        assert device_response(lsdmod, cx, case, d_out, None) == lsdmod.LSD_OK, case["name"]
        got, ok = back(d_out, 192 * n)
        assert ok and got.tobytes() == want.tobytes(), case["name"]


def test_campaign_host_entry(lsdmod, ctx, ctx_long, cases):
    for case, want, want_vol in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        a = (case["scans"], case["lens"], case["poses"], case["records"], mp_of(case), case["range_max"], case["corr"], case["search"]["ang_step"],
             case["response"])
        got, vol = cx.grid_response(*a, volume=True)
        assert got.dtype == lsdmod.GRID_RESPONSE_DTYPE == gr.RESPONSE_DTYPE and vol.dtype == np.uint32 and vol.shape == want_vol.shape
        assert got.tobytes() == want.tobytes() and vol.tobytes() == want_vol.tobytes(), case["name"]
        assert cx.grid_response(*a).tobytes() == want.tobytes(), case["name"]


def test_no_scans_is_a_no_op(lsdmod, ctx, cases):
    import torch
    case = cases[0][0]
    d_out, d_vol = filled(192), filled(64)
    d = dev(np.zeros(8))
    st = ctx.L.lsd_enqueue_grid_response_device(ctx.h, d.data_ptr(), d.data_ptr(), 0, 4, d.data_ptr(), 24, d.data_ptr(), lsdmod.lsd_map_param(*mp_of(case)),
                                                2.0, dev(case["corr"]).data_ptr(), 1.0, lsdmod.grid_response(), d_out.data_ptr(), d_vol.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK and (d_out.cpu().numpy() == FILL).all() and (d_vol.cpu().numpy() == FILL).all()


# ---- 2. poses inside lsd_fa_state and lsd_fa_carry records of noise -------------------------------------------------------------------------
def test_poses_as_carries_and_states(lsdmod, ctx, cases):
    rng = np.random.default_rng(6)
    picked = [c for c in cases if c[0]["name"] in ("nb65_1", "skipped_0", "edges_1", "sizes_2_331", "altered_1")]
    assert len(picked) == 5
    for case, want, want_vol in picked:
        n = len(case["lens"])
        for dtype, pitch in ((lsdmod.FA_CARRY_DTYPE, 768), (lsdmod.FA_STATE_DTYPE, 720)):
            rec = rng.integers(0, 256, n * pitch, dtype=np.uint8).view(dtype)        # everything but the pose is noise
            st = rec["state"] if pitch == 768 else rec
            st["x"][:, :3] = case["poses"]
            d_out, d_vol = filled(192 * n), filled(want_vol.nbytes)
            assert device_response(lsdmod, ctx, case, d_out, d_vol, dev(rec.view(np.uint8)), pitch) == lsdmod.LSD_OK
            got, ok = back(d_out, 192 * n)
            vol, ok_vol = back(d_vol, want_vol.nbytes)
            assert ok and ok_vol and got.tobytes() == want.tobytes() and vol.tobytes() == want_vol.tobytes(), (case["name"], pitch)


# ---- 3. records from the device's own plain entry and from its block = 4 entry ---------------------------------------------------------------
def test_records_of_the_device_searches(lsdmod, ctx, cases):
    import torch
    picked = [c for c in cases if c[0]["name"].startswith(("sizes_", "edges_", "room_", "rim_", "uniform_", "keep_"))]
    assert len(picked) >= 30
    for case, want, want_vol in picked:
        n = len(case["lens"])
        d_sc, d_ln, d_po, d_co = dev(case["scans"]), dev(case["lens"]), dev(case["poses"]), dev(case["corr"])
        mp, se = lsdmod.lsd_map_param(*mp_of(case)), lsdmod.grid_search(case["search"])
        d_plain, d_mr = filled(56 * n), filled(56 * n)
        assert ctx.L.lsd_enqueue_grid_match_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, case["scans"].shape[1], d_po.data_ptr(), 24, mp,
                                                   case["range_max"], d_co.data_ptr(), se, d_plain.data_ptr(), stream()) == lsdmod.LSD_OK
        d_cs = torch.zeros(lsdmod.load_library().lsd_grid_coarse_bytes(case["cols"], case["rows"], 4), dtype=torch.uint8, device="cuda")
        ctx.enqueue_grid_coarse_device(d_co.data_ptr(), case["cols"], case["rows"], 4, d_cs.data_ptr(), stream())
        ctx.enqueue_grid_match_mr_device(d_sc.data_ptr(), d_ln.data_ptr(), n, case["scans"].shape[1], d_po.data_ptr(), 24, mp_of(case), case["range_max"],
                                         d_co.data_ptr(), d_cs.data_ptr(), 4, case["search"], d_mr.data_ptr(), None, stream())
        for d_rec in (d_plain, d_mr):
            d_out, d_vol = filled(192 * n), filled(want_vol.nbytes)
            assert device_response(lsdmod, ctx, case, d_out, d_vol, d_records=d_rec) == lsdmod.LSD_OK
            assert back(d_rec, 56 * n)[0].tobytes() == case["records"].tobytes(), case["name"]
            got, ok = back(d_out, 192 * n)
            vol, ok_vol = back(d_vol, want_vol.nbytes)
            assert ok and ok_vol and got.tobytes() == want.tobytes() and vol.tobytes() == want_vol.tobytes(), case["name"]


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, cases):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    case, _, want_vol = next(c for c in cases if c[0]["name"] == "sizes_0_331")
    n = len(case["lens"])
    d_out, d_vol = filled(192 * n), filled(want_vol.nbytes)
    wide = np.zeros((1, 1025, 2)); wide[..., 0] = 0.5
    d_sc, d_ln, d_po, d_co, d_re = dev(case["scans"]), dev(case["lens"]), dev(case["poses"]), dev(case["corr"]), dev(case["records"].view(np.uint8))
    d_wide = dev(wide)
    base = dict(case["response"])

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=n, stride=case["scans"].shape[1], po=d_po.data_ptr(), pitch=24, re=d_re.data_ptr(),
             cols=case["cols"], rows=case["rows"], resol=0.05, range_max=1.5, co=d_co.data_ptr(), ang_step=1.5, out=d_out.data_ptr(),
             vol=d_vol.data_ptr(), **rp):
        p = dict(base, **rp)
        r = lsdmod.lsd_grid_response(p["rx"], p["ry"], p["ra"], p["keep_num"], p["keep_den"])
        return ctx.L.lsd_enqueue_grid_response_device(h, sc, ln, n, stride, po, pitch, re, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max,
                                                      co, ang_step, r, out, vol, stream())
    assert ctx.scan_capacity == 1024
    refused = [call(h=None), call(sc=None), call(ln=None), call(po=None), call(re=None), call(co=None), call(out=None), call(n=-1), call(stride=0),
               call(sc=d_wide.data_ptr(), n=1, stride=1025), call(cols=0), call(cols=65536), call(rows=-3), call(rows=65536), call(resol=0.0),
               call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf), call(range_max=32767 * 0.05),
               call(pitch=16), call(pitch=28), call(sc=d_sc.data_ptr() + 8), call(po=d_po.data_ptr() + 4), call(re=d_re.data_ptr() + 4),
               call(out=d_out.data_ptr() + 4), call(vol=d_vol.data_ptr() + 2), call(rx=0), call(rx=8), call(ry=0), call(ry=8), call(ra=-1), call(ra=8),
               call(keep_den=0), call(keep_num=3, keep_den=2), call(ang_step=math.nan), call(ang_step=math.inf), call(ang_step=-0.5),
               call(ra=1, ang_step=0.0)]
    assert refused == [INV] * len(refused), refused
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_vol.cpu().numpy() == FILL).all()
    # the host entry refuses the same before anything travels, and a length outside 0..stride
    out = np.full(n, FILL, np.uint8).repeat(192).view(gr.RESPONSE_DTYPE)
    vol = np.full(want_vol.shape, 0x5A5A5A5A, np.uint32)
    keep, keep_vol = out.tobytes(), vol.tobytes()

    def host(lens=case["lens"], cols=case["cols"], range_max=1.5, ang_step=1.5, **rp):
        p = dict(base, **rp)
        r = lsdmod.lsd_grid_response(p["rx"], p["ry"], p["ra"], p["keep_num"], p["keep_den"])
        ln = np.ascontiguousarray(lens, np.int32)
        return ctx.L.lsd_grid_response(ctx.h, case["scans"].ctypes.data, ln.ctypes.data, n, case["scans"].shape[1], case["poses"].ctypes.data,
                                       case["records"].ctypes.data, lsdmod.lsd_map_param(cols, case["rows"], 0.05, 0.0, 0.0), range_max,
                                       case["corr"].ctypes.data, ang_step, r, out.ctypes.data, vol.ctypes.data)
    bad_len = case["lens"].copy(); bad_len[0] = case["scans"].shape[1] + 1
    refused = [host(lens=bad_len), host(cols=65536), host(range_max=32767 * 0.05), host(rx=8), host(ra=2, ang_step=0.0), host(keep_den=0)]
    assert refused == [INV] * len(refused) and out.tobytes() == keep and vol.tobytes() == keep_vol
    # ang_step == 0 is accepted where ra == 0
    assert call(ra=0, ang_step=0.0, vol=None) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert back(d_out, 192 * n)[1]


# ---- 5. GridMapper -------------------------------------------------------------------------------------------------------------------------
def test_grid_mapper_response(lsdmod, ctx, oracle):
    import torch
    corr, scans, lens, truth = gm.recovery()
    R = gm.ROOM
    se = dict(gm.RECOVERY_SEARCH, min_num=1, min_den=8)
    rp = gr.params(2, 2, 1)
    sm = lsdmod.grid_smear((3, gm.GAUSS))
    moved = truth + np.array([2.3, -1.2, se["ang_step"] + 0.4])
    want_rec = gm.match(scans, lens, moved, R["resol"], R["range_max"], corr, se)
    want, want_vol = gr.response(scans, lens, moved, want_rec, R["resol"], R["range_max"], corr, se["ang_step"], rp)
    assert (want["flags"] & gr.VALID).all() and want["sub"].any()

    def room():
        m = lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx)
        m.integrate(scans, lens, truth)
        m.integrate(scans, lens, truth)
        return m
    a, b, c = room(), room(), room()
    assert a.likelihood_device(sm).cpu().numpy().tobytes() == corr.tobytes()
    d_sc, d_ln, d_po = dev(scans), dev(lens), dev(moved)
    # match_device(response=) is match_device followed by response_device, for either search
    for block in (0, 4):
        rec, resp = a.match_device(d_sc, d_ln, d_po, 24, se, block=block, response=rp)
        rec2 = a.match_device(d_sc, d_ln, d_po, 24, se, block=block)
        resp2, vol2 = a.response_device(d_sc, d_ln, d_po, rec2, 24, se, rp, volume=True)
        torch.cuda.synchronize()
        assert tuple(resp.shape) == (3, 192) and resp.dtype == torch.uint8 and tuple(vol2.shape) == want_vol.shape
        assert rec.cpu().numpy().tobytes() == rec2.cpu().numpy().tobytes() == want_rec.tobytes()
        assert resp.cpu().numpy().tobytes() == resp2.cpu().numpy().tobytes() == want.tobytes()
        assert vol2.cpu().numpy().view(np.uint32).tobytes() == want_vol.tobytes()
    rec, st, resp = a.match_device(d_sc, d_ln, d_po, 24, se, block=4, stats=True, response=rp)
    assert tuple(st.shape) == (3, 16) and resp.cpu().numpy().tobytes() == want.tobytes()
    got_rec, got = a.match(scans, lens, moved, se, response=rp)
    assert got.dtype == lsdmod.GRID_RESPONSE_DTYPE and got.tobytes() == want.tobytes() and got_rec.tobytes() == want_rec.tobytes()
    # integrate_at="response" is integrate_device at pitch 192 on those records: planes and counters byte for byte
    pa0, hi0 = a.counts()
    rec_a, resp_a = a.match_and_integrate_device(d_sc, d_ln, d_po, 24, se, smear=sm, response=rp, integrate_at="response")
    b.likelihood_device(sm)
    rec_b, resp_b = b.match_device(d_sc, d_ln, d_po, 24, se, response=rp)
    b.integrate_device(d_sc, d_ln, resp_b, 192)
    torch.cuda.synchronize()
    assert resp_a.cpu().numpy().tobytes() == resp_b.cpu().numpy().tobytes() == want.tobytes()
    (pa, ha), (pb, hb) = a.counts(), b.counts()
    assert pa.tobytes() == pb.tobytes() and ha.tobytes() == hb.tobytes()
    pw, hw = pa0.copy(), hi0.copy()
    gc.integrate(scans, lens, np.stack([want["x"], want["y"], want["ang"]], 1), R["cols"], R["rows"], R["resol"], R["range_max"], pw, hw)
    assert pa.tobytes() == pw.tobytes() and ha.tobytes() == hw.tobytes()
    # integrate_at="match" with response= given leaves the planes exactly as they are without it
    rec_c, resp_c = c.match_and_integrate_device(d_sc, d_ln, d_po, 24, se, smear=sm, response=rp)
    b2 = room()
    rec_d = b2.match_and_integrate_device(d_sc, d_ln, d_po, 24, se, smear=sm)
    torch.cuda.synchronize()
    (pc, hc), (pd, hd) = c.counts(), b2.counts()
    assert pc.tobytes() == pd.tobytes() and hc.tobytes() == hd.tobytes() and rec_c.cpu().numpy().tobytes() == rec_d.cpu().numpy().tobytes()
    assert resp_c.cpu().numpy().tobytes() == want.tobytes() and pc.tobytes() != pa.tobytes()
    with pytest.raises(lsdmod.LsdError):
        c.match_and_integrate_device(d_sc, d_ln, d_po, 24, se, integrate_at="response")          # no response to integrate at
    with pytest.raises(lsdmod.LsdError):
        c.match_and_integrate_device(d_sc, d_ln, d_po, 24, se, response=rp, integrate_at="refined")
    with pytest.raises(lsdmod.LsdError):
        c.response_device(d_sc, d_ln, d_po, rec_c[:2], 24, se, rp)


# ---- 6. end to end: the data log's first 20 frames -----------------------------------------------------------------------------------------
FRAMES = 20
RANGE_MAX = 8.0
LOG_SEARCH = gm.search(3, 2, 1, 0.5, min_beams=30, min_num=1, min_den=8)
LOG_RESPONSE = gr.params(2, 2, 1)


class DataLog:
    def __init__(self, lsdmod, ctx):
        m, self.mp, lid, odom = fr.load_log("data")
        self.lid, self.odom = lid[:FRAMES], odom[:FRAMES + 1]
        self.mc = ctx.map_cache(m.copy(), float(self.mp[2]), lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.cols, self.rows, self.resol = int(self.mp[0]), int(self.mp[1]), float(self.mp[2])
        self.scans, self.lens = lsdmod.lidar_frames_batch(self.lid)                  # what k_ingest writes (tests/test_scan_ingest_gpu.py)

    def mapper(self, lsdmod, ctx):
        return lsdmod.GridMapper(self.cols, self.rows, self.resol, float(self.mp[3]), float(self.mp[4]), RANGE_MAX, ctx=ctx)


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    return DataLog(lsdmod, ctx)


def test_localizer_refines_at_the_response(lsdmod, ctx, log):
    """The tick's frames entered once at the localiser's poses, then matched on that grid, refined by the response and entered again at the
    refined poses: records, response records and planes equal the restatement fed with the device's own states and the ingested scans,
    whichever search wrote the records."""
    import torch
    want = None
    for block in (0, 4):
        loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
        m = log.mapper(lsdmod, ctx)
        out = loc.step_device(dev(log.lid[None]), dev(log.odom[None, 1:]))
        loc.integrate_last_tick(m)
        rec, resp = loc.refine_and_integrate_last_tick(m, LOG_SEARCH, block=block, response=LOG_RESPONSE, integrate_at="response")
        torch.cuda.synchronize()
        st = out[0]
        states = st.cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(st.shape[:2])
        poses = np.ascontiguousarray(states["x"][0, :, :3])
        if want is None:
            pa, hi = np.zeros((log.rows, log.cols), np.uint32), np.zeros((log.rows, log.cols), np.uint32)
            gc.integrate(log.scans, log.lens, poses, log.cols, log.rows, log.resol, RANGE_MAX, pa, hi)
            r, w = lsdmod.grid_smear_table(lsdmod.grid_smear_default(1.0, 3))
            corr = gm.likelihood(pa, hi, 2, 1, 10, r, w)
            want_rec = gm.match(log.scans, log.lens, poses, log.resol, RANGE_MAX, corr, LOG_SEARCH)
            want_resp, _ = gr.response(log.scans, log.lens, poses, want_rec, log.resol, RANGE_MAX, corr, LOG_SEARCH["ang_step"], LOG_RESPONSE)
            gc.integrate(log.scans, log.lens, np.stack([want_resp["x"], want_resp["y"], want_resp["ang"]], 1), log.cols, log.rows, log.resol, RANGE_MAX,
                         pa, hi)
            want = (poses.tobytes(), corr, want_rec, want_resp, pa, hi)
            assert (want_resp["flags"] & gr.VALID).any() and want_resp["sub"].any()      # the response took part
        assert poses.tobytes() == want[0]
        assert m._corr.cpu().numpy().tobytes() == want[1].tobytes()
        assert rec.cpu().numpy().tobytes() == want[2].tobytes(), block
        assert tuple(resp.shape) == (FRAMES, 192) and resp.cpu().numpy().tobytes() == want[3].tobytes(), block
        gp, gh = m.counts()
        assert gp.tobytes() == want[4].tobytes() and gh.tobytes() == want[5].tobytes(), block


def test_response_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    d_lid, d_od = dev(log.lid[None, :4]), dev(log.odom[None, 1:5])
    kw = dict(response=LOG_RESPONSE, integrate_at="response")
    loc.step_device(d_lid, d_od)                                                       # warm: the staging, the slots and the volume have their size
    loc.refine_and_integrate_last_tick(m, LOG_SEARCH, **kw)
    loc.refine_and_integrate_last_tick(m, LOG_SEARCH, block=4, **kw)
    d_sc, d_ln, d_po = dev(log.scans[:4]), dev(log.lens[:4]), dev(np.tile([300.0, 300.0, 0.0], (4, 1)))
    m.match_and_integrate_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, **kw)
    rec0 = m.match_device(d_sc, d_ln, d_po, 24, LOG_SEARCH)
    m.response_device(d_sc, d_ln, d_po, rec0, 24, LOG_SEARCH, LOG_RESPONSE, volume=True)
    a = torch.randn(4096, 4096, device="cuda")

    def burn(count):
        for _ in range(count):
            a @ a
    burn(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    burn(10)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 10                                              # the trial run: seconds per matmul
    count = max(10, min(5000, int(math.ceil(0.08 / per))))                             # ~80 ms of work in front of the calls
    done = torch.cuda.Event()
    burn(count)
    done.record()
    if done.query():
        pytest.skip("the stream drained before the calls were made (%d matmuls of %.3f ms): the host was too slow to tell" % (count, per * 1e3))
    loc.step_device(d_lid, d_od)
    rec, resp = loc.refine_and_integrate_last_tick(m, LOG_SEARCH, **kw)
    rec2, resp2 = m.match_and_integrate_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, block=4, **kw)
    rec3, resp3 = m.match_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, response=LOG_RESPONSE)
    resp4, vol4 = m.response_device(d_sc, d_ln, d_po, rec3, 24, LOG_SEARCH, LOG_RESPONSE, volume=True)
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "a call of the response stage returned only after the work in front of it had finished"
    assert resp.is_cuda and resp2.is_cuda and resp4.is_cuda and vol4.is_cuda and torch.equal(resp3, resp4)
