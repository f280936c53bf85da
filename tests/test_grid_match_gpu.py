"""Correlative scan-to-grid matching on the device (csrc/k_gridmatch.hip: lsd_enqueue_grid_likelihood_device,
lsd_enqueue_grid_match_device, lsd_grid_match; GridMapper.likelihood_device / match* ; Localizer.refine_and_integrate_last_tick) against
the restatement of tests/grid_match_cases.py.  Both rules are exact and have no iteration order, so every comparison is byte equality."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import grid_cases as gc
import grid_match_cases as gm

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
def like_cases():
    """(case, plane) of the likelihood campaign: the restatement, computed once."""
    return [(c, gm.likelihood(c["pass"], c["hit"], c["min_pass"], c["occ_num"], c["occ_den"], c["radius"], c["w"])) for c in gm.like_campaign()]


@pytest.fixture(scope="module")
def match_cases(oracle):
    """(case, records) of the match campaign: the restatement, computed once."""
    return [(c, gm.run_match_case(c)[0]) for c in gm.match_campaign()]


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


def device_likelihood(lsdmod, cx, case, d_corr, **kw):
    import torch
    a = dict(h=cx.h, pa=dev(case["pass"].view(np.int32)), hi=dev(case["hit"].view(np.int32)), cols=case["cols"], rows=case["rows"],
             mn=case["min_pass"], num=case["occ_num"], den=case["occ_den"], radius=case["radius"], co=d_corr.data_ptr())
    a.update(kw)
    ptr = lambda t: t.data_ptr() if t is not None else None
    sm = lsdmod.grid_smear((0, case["w"]))
    sm.radius = a["radius"]
    st = cx.L.lsd_enqueue_grid_likelihood_device(a["h"], ptr(a["pa"]), ptr(a["hi"]), a["cols"], a["rows"], a["mn"], a["num"], a["den"], sm,
                                                 a["co"], stream())
    torch.cuda.synchronize()
    return st


def device_match(lsdmod, cx, case, d_out, d_poses=None, pitch=24):
    import torch
    d_sc, d_ln, d_co = dev(case["scans"]), dev(case["lens"]), dev(case["corr"])
    d_po = dev(case["poses"]) if d_poses is None else d_poses
    st = cx.L.lsd_enqueue_grid_match_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), len(case["lens"]), case["scans"].shape[1], d_po.data_ptr(), pitch,
                                            lsdmod.lsd_map_param(*mp_of(case)), case["range_max"], d_co.data_ptr(),
                                            lsdmod.grid_search(case["search"]), d_out.data_ptr(), stream())
    torch.cuda.synchronize()
    return st


# ---- 1. the lookup plane -----------------------------------------------------------------------------------------------------------------
def test_likelihood_campaign(lsdmod, ctx, like_cases):
    for case, want in like_cases:
        cells = case["cols"] * case["rows"]
        d_corr = filled(cells)
        assert device_likelihood(lsdmod, ctx, case, d_corr) == lsdmod.LSD_OK, case["name"]
        got, ok = back(d_corr, cells)
        assert ok, case["name"]
        assert got.tobytes() == want.tobytes(), case["name"]


def test_smear_default_is_read_back(lsdmod, ctx, like_cases):
    """The convenience table: read back, never recomputed here; the default plane of a mapper is made with it."""
    r, w = lsdmod.grid_smear_table(lsdmod.grid_smear_default(1.0, 3))
    assert r == 3 and w[0, 0] == 255 and (w[4:] == 0).all() and (w[:, 4:] == 0).all() and (w == w.T).all() and w[0, 1] > w[0, 2] > w[0, 3]
    for bad in ((0.0, 3), (math.nan, 3), (1.0, 8), (1.0, -1), (math.inf, 2)):
        with pytest.raises(lsdmod.LsdError):
            lsdmod.grid_smear_default(*bad)
    case = next(c for c, _ in like_cases if c["name"] == "pair_0")
    m = lsdmod.GridMapper(case["cols"], case["rows"], 0.05, 0.0, 0.0, 2.0, ctx=ctx)
    m._planes.copy_(dev(np.stack([case["pass"].reshape(-1), case["hit"].reshape(-1)]).view(np.int32)))
    plane = m.likelihood_device()
    assert plane.cpu().numpy().tobytes() == gm.likelihood(case["pass"], case["hit"], 2, 1, 10, r, w).tobytes()


# ---- 2. the match campaign through both entries -------------------------------------------------------------------------------------------
def test_match_campaign_device_entry(lsdmod, ctx, ctx_long, match_cases):
    for case, want in match_cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        n = len(case["lens"])
        d_out = filled(56 * n)
        assert device_match(lsdmod, cx, case, d_out) == lsdmod.LSD_OK, case["name"]
        got, ok = back(d_out, 56 * n)
        assert ok, case["name"]
        assert got.tobytes() == want.tobytes(), (case["name"], got.view(gm.MATCH_DTYPE), want)


def test_match_campaign_host_entry(lsdmod, ctx, ctx_long, match_cases):
    for case, want in match_cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        got = cx.grid_match(case["scans"], case["lens"], case["poses"], mp_of(case), case["range_max"], case["corr"], case["search"])
        assert got.dtype == lsdmod.GRID_MATCH_DTYPE == gm.MATCH_DTYPE
        assert got.tobytes() == want.tobytes(), case["name"]


def test_recovery_on_the_device(lsdmod, ctx, oracle):
    corr, scans, lens, truth = gm.recovery()
    se = gm.RECOVERY_SEARCH
    mp = (gm.ROOM["cols"], gm.ROOM["rows"], gm.ROOM["resol"], 0.0, 0.0)
    for dx, dy, k in gm.RECOVERY_OFFSETS:
        moved = truth + np.array([dx, dy, k * se["ang_step"]])
        got = ctx.grid_match(scans, lens, moved, mp, gm.ROOM["range_max"], corr, se)
        assert got.tobytes() == gm.match(scans, lens, moved, gm.ROOM["resol"], gm.ROOM["range_max"], corr, se).tobytes()
        assert got["di"].tolist() == [-dx] * 3 and got["dj"].tolist() == [-dy] * 3 and got["da"].tolist() == [-k] * 3
        assert got[["x", "y", "ang"]].tolist() == [tuple(t) for t in truth]


def test_no_scans_is_a_no_op(lsdmod, ctx, match_cases):
    import torch
    case = match_cases[0][0]
    d_out = filled(56)
    d = dev(np.zeros(4))
    st = ctx.L.lsd_enqueue_grid_match_device(ctx.h, d.data_ptr(), d.data_ptr(), 0, 4, d.data_ptr(), 24, lsdmod.lsd_map_param(*mp_of(case)), 2.0,
                                             dev(case["corr"]).data_ptr(), lsdmod.grid_search(case["search"]), d_out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK and (d_out.cpu().numpy() == FILL).all()


# ---- 3. poses inside lsd_fa_state and lsd_fa_carry records --------------------------------------------------------------------------------
def test_poses_as_carries_and_states(lsdmod, ctx, match_cases):
    rng = np.random.default_rng(5)
    picked = [c for c in match_cases if c[0]["name"] in ("nb65_1", "skipped_scans_0", "edges_1", "min_beams_2")]
    assert len(picked) == 4
    for case, want in picked:
        n = len(case["lens"])
        for dtype, pitch in ((lsdmod.FA_CARRY_DTYPE, 768), (lsdmod.FA_STATE_DTYPE, 720)):
            rec = rng.integers(0, 256, n * pitch, dtype=np.uint8).view(dtype)        # everything but the pose is noise
            st = rec["state"] if pitch == 768 else rec
            st["x"][:, :3] = case["poses"]
            d_out = filled(56 * n)
            assert device_match(lsdmod, ctx, case, d_out, dev(rec.view(np.uint8)), pitch) == lsdmod.LSD_OK
            got, ok = back(d_out, 56 * n)
            assert ok and got.tobytes() == want.tobytes(), (case["name"], pitch)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, like_cases, match_cases):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    case = next(c for c, _ in like_cases if c["name"] == "pair_0")
    cells = case["cols"] * case["rows"]
    d_corr = filled(cells)
    lk = lambda **kw: device_likelihood(lsdmod, ctx, case, d_corr, **kw)
    refused = [lk(h=None), lk(pa=None), lk(hi=None), lk(co=None), lk(cols=0), lk(cols=65536), lk(rows=0), lk(rows=65536), lk(rows=-1),
               lk(radius=-1), lk(radius=8), lk(den=0), lk(num=11), lk(num=2, den=1)]
    assert refused == [INV] * len(refused), refused
    assert (d_corr.cpu().numpy() == FILL).all()

    mcase = next(c for c, _ in match_cases if c["name"] == "nb65_0")
    n = len(mcase["lens"])
    d_out = filled(56 * n)
    wide = np.zeros((1, 1025, 2)); wide[..., 0] = 0.5
    d_sc, d_ln, d_po, d_co = dev(mcase["scans"]), dev(mcase["lens"]), dev(mcase["poses"]), dev(mcase["corr"])
    d_wide = dev(wide)
    base = dict(mcase["search"])

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=n, stride=mcase["scans"].shape[1], po=d_po.data_ptr(), pitch=24, cols=mcase["cols"],
             rows=mcase["rows"], resol=0.05, range_max=1.5, co=d_co.data_ptr(), out=d_out.data_ptr(), **se):
        s = lsdmod.lsd_grid_search(*[dict(base, **se)[k] for k in gm.SEARCH_KEYS])
        return ctx.L.lsd_enqueue_grid_match_device(h, sc, ln, n, stride, po, pitch, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max, co,
                                                   s, out, stream())
    assert ctx.scan_capacity == 1024
    refused = [call(h=None), call(sc=None), call(ln=None), call(po=None), call(co=None), call(out=None), call(n=-1), call(stride=0),
               call(sc=d_wide.data_ptr(), n=1, stride=1025), call(cols=0), call(cols=65536), call(rows=-3), call(rows=65536), call(resol=0.0),
               call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf), call(range_max=32767 * 0.05),
               call(pitch=16), call(pitch=28), call(sc=d_sc.data_ptr() + 8), call(po=d_po.data_ptr() + 4), call(out=d_out.data_ptr() + 4),
               call(wx=-1), call(wx=64), call(wy=-1), call(wy=64), call(na=-1), call(na=64), call(ang_step=math.nan), call(ang_step=math.inf),
               call(ang_step=-0.5), call(na=1, ang_step=0.0), call(min_den=0), call(min_num=5, min_den=4)]
    assert refused == [INV] * len(refused), refused
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    # the host entry refuses the same before anything travels, and a length outside 0..stride
    out = np.full(n, FILL, np.uint8).repeat(56).view(gm.MATCH_DTYPE)
    keep = out.tobytes()

    def host(lens=mcase["lens"], cols=mcase["cols"], range_max=1.5, **se):
        s = lsdmod.lsd_grid_search(*[dict(base, **se)[k] for k in gm.SEARCH_KEYS])
        ln = np.ascontiguousarray(lens, np.int32)
        return ctx.L.lsd_grid_match(ctx.h, mcase["scans"].ctypes.data, ln.ctypes.data, n, mcase["scans"].shape[1], mcase["poses"].ctypes.data,
                                    lsdmod.lsd_map_param(cols, mcase["rows"], 0.05, 0.0, 0.0), range_max, mcase["corr"].ctypes.data, s, out.ctypes.data)
    bad_len = mcase["lens"].copy(); bad_len[0] = mcase["scans"].shape[1] + 1
    refused = [host(lens=bad_len), host(cols=65536), host(range_max=32767 * 0.05), host(wx=64), host(na=2, ang_step=0.0), host(min_den=0)]
    assert refused == [INV] * len(refused) and out.tobytes() == keep
    # ang_step == 0 is accepted where na == 0
    assert call(na=0, ang_step=0.0) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert back(d_out, 56 * n)[1]


# ---- 5. GridMapper -------------------------------------------------------------------------------------------------------------------------
def test_grid_mapper_matches_and_integrates(lsdmod, ctx, oracle):
    """The room: integrate at the truth, then displaced scans come back to it -- match, match_device and match_and_integrate_device."""
    import torch
    corr, scans, lens, truth = gm.recovery()
    se, R = gm.RECOVERY_SEARCH, gm.ROOM
    m = lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx)
    m.integrate(scans, lens, truth)
    m.integrate(scans, lens, truth)
    sm = lsdmod.grid_smear((3, gm.GAUSS))
    plane = m.likelihood_device(sm)
    torch.cuda.synchronize()
    assert plane.cpu().numpy().tobytes() == corr.tobytes()
    moved = truth + np.array([2, -1, se["ang_step"]])
    want = gm.match(scans, lens, moved, R["resol"], R["range_max"], corr, se)
    assert m.match(scans, lens, moved, se).tobytes() == want.tobytes()
    pa0, hi0 = m.counts()
    rec = m.match_and_integrate_device(dev(scans), dev(lens), dev(moved), 24, se, smear=sm)
    assert tuple(rec.shape) == (3, 56) and rec.dtype == torch.uint8
    assert rec.cpu().numpy().tobytes() == want.tobytes()
    pa, hi = pa0.copy(), hi0.copy()
    gc.integrate(scans, lens, np.stack([want["x"], want["y"], want["ang"]], 1), R["cols"], R["rows"], R["resol"], R["range_max"], pa, hi)
    gp, gh = m.counts()
    assert gp.tobytes() == pa.tobytes() and gh.tobytes() == hi.tobytes()
    assert gp.tobytes() == (pa0 // 2 * 3).tobytes()                            # the third entry landed exactly where the first two did
    with pytest.raises(lsdmod.LsdError):
        m.match_device(dev(scans), dev(lens), dev(moved[:1]))


# ---- 6. end to end: the data log's first 20 frames -----------------------------------------------------------------------------------------
FRAMES = 20
RANGE_MAX = 8.0
LOG_SEARCH = gm.search(3, 2, 1, 0.5, min_beams=30, min_num=1, min_den=8)


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


def states_of(lsdmod, out):
    import torch
    torch.cuda.synchronize()
    st = out[0]
    return st.cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(st.shape[:2])


def test_localizer_refines_and_integrates_its_last_tick(lsdmod, ctx, log):
    """The tick's frames entered once at the localiser's poses, then matched on that grid and entered again at the records: planes and
    records equal the restatement fed with the device's own states and the ingested scans."""
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    with pytest.raises(lsdmod.LsdError):
        loc.refine_and_integrate_last_tick(m, LOG_SEARCH)                              # no tick yet
    out = loc.step_device(dev(log.lid[None]), dev(log.odom[None, 1:]))
    loc.integrate_last_tick(m)
    rec = loc.refine_and_integrate_last_tick(m, LOG_SEARCH)
    states = states_of(lsdmod, out)
    poses = np.ascontiguousarray(states["x"][0, :, :3])
    pa, hi = np.zeros((log.rows, log.cols), np.uint32), np.zeros((log.rows, log.cols), np.uint32)
    gc.integrate(log.scans, log.lens, poses, log.cols, log.rows, log.resol, RANGE_MAX, pa, hi)
    r, w = lsdmod.grid_smear_table(lsdmod.grid_smear_default(1.0, 3))
    corr = gm.likelihood(pa, hi, 2, 1, 10, r, w)
    assert m._corr.cpu().numpy().tobytes() == corr.tobytes() and corr.any()
    want = gm.match(log.scans, log.lens, poses, log.resol, RANGE_MAX, corr, LOG_SEARCH)
    got = rec.cpu().numpy().reshape(-1).view(gm.MATCH_DTYPE)
    assert got.tobytes() == want.tobytes()
    assert (want["flags"] & gm.ACCEPTED).any() and want["score"].any()                 # the match took part: not every frame passed through
    gc.integrate(log.scans, log.lens, np.stack([want["x"], want["y"], want["ang"]], 1), log.cols, log.rows, log.resol, RANGE_MAX, pa, hi)
    gp, gh = m.counts()
    assert gp.tobytes() == pa.tobytes() and gh.tobytes() == hi.tobytes()


def test_match_and_integrate_is_match_then_integrate(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    out = loc.step_device(dev(log.lid[None]), dev(log.odom[None, 1:]))
    torch.cuda.synchronize()
    d_sc, d_ln, d_st = dev(log.scans), dev(log.lens), out[0].reshape(-1).view(torch.uint8).clone()
    a, b = log.mapper(lsdmod, ctx), log.mapper(lsdmod, ctx)
    for m in (a, b):
        m.integrate_device(d_sc, d_ln, d_st, 720)
    rec_a = a.match_and_integrate_device(d_sc, d_ln, d_st, 720, LOG_SEARCH)
    b.likelihood_device()
    rec_b = b.match_device(d_sc, d_ln, d_st, 720, LOG_SEARCH)
    b.integrate_device(d_sc, d_ln, rec_b, 56)
    torch.cuda.synchronize()
    assert rec_a.cpu().numpy().tobytes() == rec_b.cpu().numpy().tobytes()
    (pa, ha), (pb, hb) = a.counts(), b.counts()
    assert pa.any() and pa.tobytes() == pb.tobytes() and ha.tobytes() == hb.tobytes()
    # refresh=False keeps the plane: a second pass on `a` is matched against the plane of the first
    plane = a._corr.clone()
    a.match_and_integrate_device(d_sc, d_ln, d_st, 720, LOG_SEARCH, refresh=False)
    torch.cuda.synchronize()
    assert torch.equal(plane, a._corr)


def test_refine_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    d_lid, d_od = dev(log.lid[None, :4]), dev(log.odom[None, 1:5])
    loc.step_device(d_lid, d_od)                                                       # warm: the staging, the workspace and the slots have their size
    loc.refine_and_integrate_last_tick(m, LOG_SEARCH)
    d_sc, d_ln, d_po = dev(log.scans[:4]), dev(log.lens[:4]), dev(np.tile([300.0, 300.0, 0.0], (4, 1)))
    m.match_and_integrate_device(d_sc, d_ln, d_po, 24, LOG_SEARCH)
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
    count = max(10, min(5000, int(math.ceil(0.08 / per))))                             # ~80 ms of work in front of the tick
    done = torch.cuda.Event()
    burn(count)
    done.record()
    if done.query():
        pytest.skip("the stream drained before the calls were made (%d matmuls of %.3f ms): the host was too slow to tell" % (count, per * 1e3))
    loc.step_device(d_lid, d_od)
    rec = loc.refine_and_integrate_last_tick(m, LOG_SEARCH)
    rec2 = m.match_and_integrate_device(d_sc, d_ln, d_po, 24, LOG_SEARCH)
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "refine_and_integrate_last_tick / match_and_integrate_device returned only after the work in front of them had finished"
    assert rec.is_cuda and rec2.is_cuda and m.counts()[0].any()
