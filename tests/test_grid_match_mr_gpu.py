"""Coarse-to-fine correlative matching on the device (csrc/k_gridmatch_mr.hip: lsd_enqueue_grid_coarse_device,
lsd_enqueue_grid_match_mr_device, lsd_grid_match_mr; GridMapper.coarse_device / match*(block=); Localizer.refine_and_integrate_last_tick(block=))
against the restatement of tests/grid_match_mr_cases.py and against the device's own plain entry.  The rule is exact and has no iteration
order, so every comparison is byte equality -- the records' 56 bytes and the statistics' 16."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import grid_match_cases as gm
import grid_match_mr_cases as mr

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
def mr_cases(oracle):
    """(case, records, stats) of the campaign at each case's own block size: the restatement, computed once."""
    return [(c,) + mr.run_mr_case(c)[:2] for c in mr.mr_campaign()]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n_bytes):
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


def device_coarse(cx, corr, b):
    """(the coarse plane the device makes of corr, its guard untouched)."""
    import torch
    rows, cols = corr.shape
    n = (rows + b - 1) * (cols + b - 1)
    d = filled(n)
    assert cx.L.lsd_enqueue_grid_coarse_device(cx.h, dev(corr).data_ptr(), cols, rows, b, d.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    got, ok = back(d, n)
    return got.reshape(rows + b - 1, cols + b - 1), ok


def device_match_mr(lsdmod, cx, case, b, d_out, d_stats, d_poses=None, pitch=24):
    import torch
    d_sc, d_ln, d_co = dev(case["scans"]), dev(case["lens"]), dev(case["corr"])
    d_cs = dev(mr.coarse_plane(case["corr"], b))
    d_po = dev(case["poses"]) if d_poses is None else d_poses
    st = cx.L.lsd_enqueue_grid_match_mr_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), len(case["lens"]), case["scans"].shape[1], d_po.data_ptr(), pitch,
                                               lsdmod.lsd_map_param(*mp_of(case)), case["range_max"], d_co.data_ptr(), d_cs.data_ptr(), b,
                                               lsdmod.grid_search(case["search"]), d_out.data_ptr(), d_stats.data_ptr() if d_stats is not None else None,
                                               stream())
    torch.cuda.synchronize()
    return st


def device_plain(lsdmod, cx, case):
    import torch
    n = len(case["lens"])
    d_out = filled(56 * n)
    d_sc, d_ln, d_co, d_po = dev(case["scans"]), dev(case["lens"]), dev(case["corr"]), dev(case["poses"])
    assert cx.L.lsd_enqueue_grid_match_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, case["scans"].shape[1], d_po.data_ptr(), 24,
                                              lsdmod.lsd_map_param(*mp_of(case)), case["range_max"], d_co.data_ptr(),
                                              lsdmod.grid_search(case["search"]), d_out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    return back(d_out, 56 * n)[0].tobytes()


# ---- 1. the coarse plane -------------------------------------------------------------------------------------------------------------------
def test_coarse_plane_byte_for_byte(lsdmod, ctx):
    rng = np.random.default_rng(11)
    planes = [gm.random_plane(rng, 61, 47, 0.3), gm.random_plane(rng, 1, 1, 1.0), gm.random_plane(rng, 257, 1, 0.5), gm.random_plane(rng, 1, 257, 0.5),
              gm.random_plane(rng, 33, 9, 0.9), gm.random_plane(rng, 95, 40, 0.02), gm.recovery()[0]]       # (33 x 9, 95 x 40: one past the tile)
    for corr in planes:
        for b in (2, 3, 4, 8, 15, 16):
            got, ok = device_coarse(ctx, corr, b)
            assert ok, (corr.shape, b)
            assert got.tobytes() == mr.coarse_plane(corr, b).tobytes(), (corr.shape, b)
            assert lsdmod.load_library().lsd_grid_coarse_bytes(corr.shape[1], corr.shape[0], b) == got.size
    lib = lsdmod.load_library()
    assert [lib.lsd_grid_coarse_bytes(*a) for a in ((0, 5, 4), (5, 65536, 4), (5, 5, 1), (5, 5, 17))] == [0] * 4
    assert lib.lsd_grid_coarse_bytes(65535, 65535, 16) == 65550 * 65550


# ---- 2. the campaign through both entries ------------------------------------------------------------------------------------------------
def test_campaign_device_entry(lsdmod, ctx, ctx_long, mr_cases):
    """Records and statistics equal the restatement; the records equal the device's own plain entry on the same inputs."""
    for case, want, want_stats in mr_cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        n = len(case["lens"])
        d_out, d_stats = filled(56 * n), filled(16 * n)
        assert device_match_mr(lsdmod, cx, case, case["block"], d_out, d_stats) == lsdmod.LSD_OK, case["name"]
        got, ok = back(d_out, 56 * n)
        got_stats, ok_stats = back(d_stats, 16 * n)
        assert ok and ok_stats, case["name"]
        assert got.tobytes() == want.tobytes(), (case["name"], got.view(gm.MATCH_DTYPE), want)
        assert got_stats.tobytes() == want_stats.tobytes(), (case["name"], got_stats.view(mr.STATS_DTYPE), want_stats)
        assert got.tobytes() == device_plain(lsdmod, cx, case), case["name"]


def test_campaign_host_entry(lsdmod, ctx, ctx_long, mr_cases):
    assert lsdmod.GRID_MATCH_MR_STATS_DTYPE == mr.STATS_DTYPE
    for case, want, want_stats in mr_cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        got, stats = cx.grid_match_mr(case["scans"], case["lens"], case["poses"], mp_of(case), case["range_max"], case["corr"], case["block"],
                                      case["search"], stats=True)
        assert got.tobytes() == want.tobytes() and stats.tobytes() == want_stats.tobytes(), case["name"]
        alone = cx.grid_match_mr(case["scans"], case["lens"], case["poses"], mp_of(case), case["range_max"], case["corr"], case["block"], case["search"])
        assert alone.tobytes() == want.tobytes(), case["name"]


def test_every_block_size_gives_the_plain_records(lsdmod, ctx, mr_cases):
    """The hand-made cases, the room and the widest window at b = 2 .. 16 against the device's plain entry; d_stats null."""
    picked = [c for c, _, _ in mr_cases if c["name"].startswith(("equal_peaks", "prior_pruned", "low_rim", "lonely", "other_angle", "room_", "w63_",
                                                                   "peaks_many", "edges_"))]
    assert len(picked) >= 27
    for case in picked:
        plain = device_plain(lsdmod, ctx, case)
        n = len(case["lens"])
        for b in (2, 3, 4, 5, 8, 13, 16):
            d_out = filled(56 * n)
            assert device_match_mr(lsdmod, ctx, case, b, d_out, None) == lsdmod.LSD_OK
            got, ok = back(d_out, 56 * n)
            assert ok and got.tobytes() == plain, (case["name"], b)


def test_no_scans_is_a_no_op(lsdmod, ctx, mr_cases):
    import torch
    case = mr_cases[0][0]
    d_out, d_stats = filled(56), filled(16)
    d = dev(np.zeros(4))
    st = ctx.L.lsd_enqueue_grid_match_mr_device(ctx.h, d.data_ptr(), d.data_ptr(), 0, 4, d.data_ptr(), 24, lsdmod.lsd_map_param(*mp_of(case)), 2.0,
                                                dev(case["corr"]).data_ptr(), dev(mr.coarse_plane(case["corr"], 4)).data_ptr(), 4,
                                                lsdmod.grid_search(case["search"]), d_out.data_ptr(), d_stats.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK and (d_out.cpu().numpy() == FILL).all() and (d_stats.cpu().numpy() == FILL).all()


# ---- 3. poses inside lsd_fa_state and lsd_fa_carry records --------------------------------------------------------------------------------
def test_poses_as_carries_and_states(lsdmod, ctx, mr_cases):
    rng = np.random.default_rng(5)
    picked = [c for c in mr_cases if c[0]["name"] in ("nb65_1_b4", "skipped_scans_0_b2", "edges_1_b3", "room_b8_1")]
    assert len(picked) == 4
    for case, want, want_stats in picked:
        n = len(case["lens"])
        for dtype, pitch in ((lsdmod.FA_CARRY_DTYPE, 768), (lsdmod.FA_STATE_DTYPE, 720)):
            rec = rng.integers(0, 256, n * pitch, dtype=np.uint8).view(dtype)        # everything but the pose is noise
            st = rec["state"] if pitch == 768 else rec
            st["x"][:, :3] = case["poses"]
            d_out, d_stats = filled(56 * n), filled(16 * n)
            assert device_match_mr(lsdmod, ctx, case, case["block"], d_out, d_stats, dev(rec.view(np.uint8)), pitch) == lsdmod.LSD_OK
            got, ok = back(d_out, 56 * n)
            got_stats, ok_stats = back(d_stats, 16 * n)
            assert ok and ok_stats and got.tobytes() == want.tobytes() and got_stats.tobytes() == want_stats.tobytes(), (case["name"], pitch)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, mr_cases):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    mcase = next(c for c, _, _ in mr_cases if c["name"] == "nb65_0_b16")
    n = len(mcase["lens"])
    corr = mcase["corr"]
    d_corr = dev(corr)
    d_coarse = filled(mr.coarse_plane(corr, 4).size)
    co = lambda h=ctx.h, src=d_corr.data_ptr(), cols=mcase["cols"], rows=mcase["rows"], b=4, dst=d_coarse.data_ptr(): \
        ctx.L.lsd_enqueue_grid_coarse_device(h, src, cols, rows, b, dst, stream())
    refused = [co(h=None), co(src=None), co(dst=None), co(cols=0), co(cols=65536), co(rows=0), co(rows=-2), co(rows=65536), co(b=1), co(b=0), co(b=17),
               co(b=-4)]
    assert refused == [INV] * len(refused), refused
    torch.cuda.synchronize()
    assert (d_coarse.cpu().numpy() == FILL).all()

    d_out, d_stats = filled(56 * n), filled(16 * n)
    wide = np.zeros((1, 1025, 2)); wide[..., 0] = 0.5
    d_sc, d_ln, d_po, d_cs = dev(mcase["scans"]), dev(mcase["lens"]), dev(mcase["poses"]), dev(mr.coarse_plane(corr, 4))
    d_wide = dev(wide)
    base = dict(mcase["search"])

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=n, stride=mcase["scans"].shape[1], po=d_po.data_ptr(), pitch=24, cols=mcase["cols"],
             rows=mcase["rows"], resol=0.05, range_max=1.5, co=d_corr.data_ptr(), cs=d_cs.data_ptr(), b=4, out=d_out.data_ptr(),
             stats=d_stats.data_ptr(), **se):
        s = lsdmod.lsd_grid_search(*[dict(base, **se)[k] for k in gm.SEARCH_KEYS])
        return ctx.L.lsd_enqueue_grid_match_mr_device(h, sc, ln, n, stride, po, pitch, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max, co,
                                                      cs, b, s, out, stats, stream())
    assert ctx.scan_capacity == 1024
    refused = [call(h=None), call(sc=None), call(ln=None), call(po=None), call(co=None), call(cs=None), call(out=None), call(n=-1), call(stride=0),
               call(sc=d_wide.data_ptr(), n=1, stride=1025), call(cols=0), call(cols=65536), call(rows=-3), call(rows=65536), call(resol=0.0),
               call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf), call(range_max=32767 * 0.05),
               call(pitch=16), call(pitch=28), call(sc=d_sc.data_ptr() + 8), call(po=d_po.data_ptr() + 4), call(out=d_out.data_ptr() + 4),
               call(wx=-1), call(wx=64), call(wy=-1), call(wy=64), call(na=-1), call(na=64), call(ang_step=math.nan), call(ang_step=math.inf),
               call(ang_step=-0.5), call(na=1, ang_step=0.0), call(min_den=0), call(min_num=5, min_den=4),
               call(b=1), call(b=0), call(b=17), call(b=-2), call(stats=d_stats.data_ptr() + 2), call(stats=d_stats.data_ptr() + 1)]
    assert refused == [INV] * len(refused), refused
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_stats.cpu().numpy() == FILL).all()
    # the host entry refuses the same before anything travels, and a length outside 0..stride
    out = np.full(n, FILL, np.uint8).repeat(56).view(gm.MATCH_DTYPE)
    hstats = np.full(n, FILL, np.uint8).repeat(16).view(mr.STATS_DTYPE)
    keep, keep_stats = out.tobytes(), hstats.tobytes()

    def host(lens=mcase["lens"], cols=mcase["cols"], range_max=1.5, b=4, **se):
        s = lsdmod.lsd_grid_search(*[dict(base, **se)[k] for k in gm.SEARCH_KEYS])
        ln = np.ascontiguousarray(lens, np.int32)
        return ctx.L.lsd_grid_match_mr(ctx.h, mcase["scans"].ctypes.data, ln.ctypes.data, n, mcase["scans"].shape[1], mcase["poses"].ctypes.data,
                                       lsdmod.lsd_map_param(cols, mcase["rows"], 0.05, 0.0, 0.0), range_max, corr.ctypes.data, b, s,
                                       out.ctypes.data, hstats.ctypes.data)
    bad_len = mcase["lens"].copy(); bad_len[0] = mcase["scans"].shape[1] + 1
    refused = [host(lens=bad_len), host(cols=65536), host(range_max=32767 * 0.05), host(wx=64), host(na=2, ang_step=0.0), host(min_den=0), host(b=1),
               host(b=17)]
    assert refused == [INV] * len(refused) and out.tobytes() == keep and hstats.tobytes() == keep_stats
    # a statistics pointer that is 4-byte but not 8-byte aligned is taken
    assert call(stats=d_stats.data_ptr() + 4, n=1) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert back(d_out, 56 * n)[1] and back(d_stats, 16 * n)[1]


# ---- 5. GridMapper -------------------------------------------------------------------------------------------------------------------------
def test_grid_mapper_with_a_block(lsdmod, ctx, oracle):
    """The room at a large displacement: match, match_device and match_and_integrate_device with block= give the block=0 records."""
    import torch
    corr, scans, lens, truth = gm.recovery()
    se, R = mr.ROOM_SEARCH, gm.ROOM
    m = lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx)
    m.integrate(scans, lens, truth)
    m.integrate(scans, lens, truth)
    sm = lsdmod.grid_smear((3, gm.GAUSS))
    m.likelihood_device(sm)
    moved = truth + np.array([-11, 13, 2 * se["ang_step"]])
    want, want_stats = mr.match_mr(scans, lens, moved, R["resol"], R["range_max"], corr, se, 4)
    assert want["di"].tolist() == [11] * 3 and want["dj"].tolist() == [-13] * 3 and want["da"].tolist() == [-2] * 3
    plain = m.match(scans, lens, moved, se)
    assert plain.tobytes() == want.tobytes()
    plane = m.coarse_device(4)
    assert tuple(plane.shape) == (R["rows"] + 3, R["cols"] + 3) and plane.cpu().numpy().tobytes() == mr.coarse_plane(corr, 4).tobytes()
    assert m.match(scans, lens, moved, se, block=4).tobytes() == want.tobytes()
    rec, stats = m.match_device(dev(scans), dev(lens), dev(moved), 24, se, block=4, stats=True)
    assert rec.cpu().numpy().tobytes() == want.tobytes() and stats.cpu().numpy().tobytes() == want_stats.tobytes()
    assert tuple(stats.shape) == (3, 16) and stats.dtype == torch.uint8
    twin = lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx)
    twin._planes.copy_(m._planes)
    rec8, stats8 = m.match_and_integrate_device(dev(scans), dev(lens), dev(moved), 24, se, smear=sm, block=8, stats=True)
    rec0 = twin.match_and_integrate_device(dev(scans), dev(lens), dev(moved), 24, se, smear=sm)
    assert rec8.cpu().numpy().tobytes() == rec0.cpu().numpy().tobytes() == want.tobytes()
    assert stats8.cpu().numpy().tobytes() == mr.match_mr(scans, lens, moved, R["resol"], R["range_max"], corr, se, 8)[1].tobytes()
    assert m._coarse[8].cpu().numpy().tobytes() == mr.coarse_plane(corr, 8).tobytes()          # refreshed with the lookup plane
    (pa, ha), (pb, hb) = m.counts(), twin.counts()
    assert pa.tobytes() == pb.tobytes() and ha.tobytes() == hb.tobytes()
    # a refresh follows the counters: the coarse plane of the next call is the one of the NEW lookup plane
    m.match_and_integrate_device(dev(scans), dev(lens), dev(moved), 24, se, smear=sm, block=8)
    torch.cuda.synchronize()
    assert m._coarse[8].cpu().numpy().tobytes() == mr.coarse_plane(m._corr.cpu().numpy(), 8).tobytes()
    for bad in (1, 17):
        with pytest.raises(lsdmod.LsdError):
            m.coarse_device(bad)
    with pytest.raises(lsdmod.LsdError):
        m.match_device(dev(scans), dev(lens), dev(moved), 24, se, stats=True)                    # statistics belong to the coarse-to-fine search


# ---- 6. end to end: the data log's first 20 frames -----------------------------------------------------------------------------------------
FRAMES = 20
RANGE_MAX = 8.0
LOG_SEARCH = gm.search(9, 7, 1, 0.5, min_beams=30, min_num=1, min_den=8)


class DataLog:
    def __init__(self, lsdmod, ctx):
        m, self.mp, lid, odom = fr.load_log("data")
        self.lid, self.odom = lid[:FRAMES], odom[:FRAMES + 1]
        self.mc = ctx.map_cache(m.copy(), float(self.mp[2]), lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.cols, self.rows, self.resol = int(self.mp[0]), int(self.mp[1]), float(self.mp[2])
        self.scans, self.lens = lsdmod.lidar_frames_batch(self.lid)

    def mapper(self, lsdmod, ctx):
        return lsdmod.GridMapper(self.cols, self.rows, self.resol, float(self.mp[3]), float(self.mp[4]), RANGE_MAX, ctx=ctx)


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    return DataLog(lsdmod, ctx)


def test_localizer_refines_with_a_block(lsdmod, ctx, log):
    """The same tick refined into two mappers, block=4 and block=0: records, lookup planes and counters are equal."""
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    a, b = log.mapper(lsdmod, ctx), log.mapper(lsdmod, ctx)
    loc.step_device(dev(log.lid[None]), dev(log.odom[None, 1:]))
    for m in (a, b):
        loc.integrate_last_tick(m)
    rec_a = loc.refine_and_integrate_last_tick(a, LOG_SEARCH, block=4)
    rec_b = loc.refine_and_integrate_last_tick(b, LOG_SEARCH)
    torch.cuda.synchronize()
    got = rec_a.cpu().numpy().reshape(-1).view(gm.MATCH_DTYPE)
    assert tuple(rec_a.shape) == (FRAMES, 56) and got.tobytes() == rec_b.cpu().numpy().tobytes()
    assert (got["flags"] & gm.ACCEPTED).any() and got["score"].any()                    # the match took part
    assert torch.equal(a._corr, b._corr) and a._corr.any()
    assert a._coarse[4].cpu().numpy().tobytes() == mr.coarse_plane(a._corr.cpu().numpy(), 4).tobytes()
    (pa, ha), (pb, hb) = a.counts(), b.counts()
    assert pa.any() and pa.tobytes() == pb.tobytes() and ha.tobytes() == hb.tobytes()


def test_the_block_path_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    d_lid, d_od = dev(log.lid[None, :4]), dev(log.odom[None, 1:5])
    loc.step_device(d_lid, d_od)                                                       # warm: the staging, the workspace and the planes have their size
    loc.refine_and_integrate_last_tick(m, LOG_SEARCH, block=4)
    d_sc, d_ln, d_po = dev(log.scans[:4]), dev(log.lens[:4]), dev(np.tile([300.0, 300.0, 0.0], (4, 1)))
    m.match_and_integrate_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, block=4, stats=True)
    m.match_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, block=4)
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
    rec = loc.refine_and_integrate_last_tick(m, LOG_SEARCH, block=4)
    rec2, stats2 = m.match_and_integrate_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, block=4, stats=True)
    rec3 = m.match_device(d_sc, d_ln, d_po, 24, LOG_SEARCH, block=4)
    m.coarse_device(4)
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "the block= calls returned only after the work in front of them had finished"
    assert rec.is_cuda and rec2.is_cuda and stats2.is_cuda and rec3.is_cuda and m.counts()[0].any()
