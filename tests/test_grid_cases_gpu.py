"""Mapping with known poses on the device (csrc/k_gridmap.hip: lsd_enqueue_grid_integrate_device, lsd_enqueue_grid_publish_device,
lsd_grid_integrate; GridMapper; Localizer / FleetLocalizer.integrate_last_tick) against the restatement of tests/grid_cases.py.  The rule
is exact and has no iteration order, so every comparison is byte equality."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import grid_cases as gc

pytestmark = pytest.mark.gpu

GUARD = 64                                     # words behind each plane, bytes behind a grid
GUARD_WORD = 0xA5A5A5A5


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
    """(case, pass, hit) of the campaign on zeroed planes: the restatement, computed once."""
    return [(case,) + gc.run_case(case)[:2] for case in gc.campaign()]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pattern(cells, seed):
    """A non-zero starting content of a plane."""
    return ((np.arange(cells, dtype=np.uint64) * 2654435761 + seed) % 1000 + 1).astype(np.uint32)


def guarded(values):
    """A CUDA int32 tensor holding the uint32 `values` and GUARD guard words behind them."""
    return dev(np.concatenate([values.reshape(-1), np.full(GUARD, GUARD_WORD, np.uint32)]).view(np.int32))


def back(t, cells):
    """(the plane, True if the guard is untouched) of a guarded tensor."""
    a = t.cpu().numpy().view(np.uint32)
    return a[:cells], bool((a[cells:] == GUARD_WORD).all())


def map_param(case):
    return (case["cols"], case["rows"], case["resol"], -1.5, 2.25)


def device_integrate(lsdmod, cx, case, d_pass, d_hit, d_poses=None, pitch=24):
    """The device entry through the raw C ABI, then the caller's synchronisation; returns the status."""
    import torch
    d_sc, d_ln = dev(case["scans"]), dev(case["lens"])
    d_po = dev(case["poses"]) if d_poses is None else d_poses
    st = cx.L.lsd_enqueue_grid_integrate_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), len(case["lens"]), case["scans"].shape[1], d_po.data_ptr(),
                                                pitch, lsdmod.lsd_map_param(*map_param(case)), case["range_max"], d_pass.data_ptr(),
                                                d_hit.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


# ---- 1. the campaign through both entries ------------------------------------------------------------------------------------------------
def test_campaign_device_entry(lsdmod, ctx, ctx_long, cases):
    """Planes pre-filled with a pattern (accumulation), a second call on top, guard words behind both planes."""
    for case, pa, hi in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        cells = case["cols"] * case["rows"]
        p0, h0 = pattern(cells, 1), pattern(cells, 2)
        d_pass, d_hit = guarded(p0), guarded(h0)
        for times in (1, 2):
            assert device_integrate(lsdmod, cx, case, d_pass, d_hit) == lsdmod.LSD_OK, case["name"]
            (gp, okp), (gh, okh) = back(d_pass, cells), back(d_hit, cells)
            assert okp and okh, case["name"]
            assert gp.tobytes() == (p0 + times * pa.reshape(-1)).tobytes(), (case["name"], times)
            assert gh.tobytes() == (h0 + times * hi.reshape(-1)).tobytes(), (case["name"], times)


def test_campaign_host_entry(lsdmod, ctx, ctx_long, cases):
    for case, pa, hi in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        cells = case["cols"] * case["rows"]
        p0, h0 = pattern(cells, 3), pattern(cells, 4)
        gp, gh = cx.grid_integrate(case["scans"], case["lens"], case["poses"], map_param(case), case["range_max"], p0, h0)
        assert gp.tobytes() == (p0 + pa.reshape(-1)).tobytes() and gh.tobytes() == (h0 + hi.reshape(-1)).tobytes(), case["name"]
        gp, gh = cx.grid_integrate(case["scans"], case["lens"], case["poses"], map_param(case), case["range_max"], gp, gh)
        assert gp.tobytes() == (p0 + 2 * pa.reshape(-1)).tobytes() and gh.tobytes() == (h0 + 2 * hi.reshape(-1)).tobytes(), case["name"]


def test_no_scans_is_a_no_op(lsdmod, ctx, cases):
    import torch
    case = cases[0][0]
    cells = case["cols"] * case["rows"]
    d_pass, d_hit = guarded(pattern(cells, 5)), guarded(pattern(cells, 6))
    before = (d_pass.cpu().numpy().tobytes(), d_hit.cpu().numpy().tobytes())
    d = dev(np.zeros(4))
    st = ctx.L.lsd_enqueue_grid_integrate_device(ctx.h, d.data_ptr(), d.data_ptr(), 0, 4, d.data_ptr(), 24, lsdmod.lsd_map_param(*map_param(case)), 2.0,
                                                 d_pass.data_ptr(), d_hit.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK and (d_pass.cpu().numpy().tobytes(), d_hit.cpu().numpy().tobytes()) == before


# ---- 2. poses inside lsd_fa_carry records ------------------------------------------------------------------------------------------------
def test_poses_as_carries_and_states(lsdmod, ctx, cases):
    rng = np.random.default_rng(3)
    picked = [c for c in cases if c[0]["name"] in ("octants1", "skipped_scans0", "len65_1", "crossing2")]
    assert len(picked) == 4
    for case, pa, hi in picked:
        cells, n = case["cols"] * case["rows"], len(case["lens"])
        for dtype, pitch in ((lsdmod.FA_CARRY_DTYPE, 768), (lsdmod.FA_STATE_DTYPE, 720)):
            rec = rng.integers(0, 256, n * pitch, dtype=np.uint8).view(dtype)        # everything but the pose is noise
            st = rec["state"] if pitch == 768 else rec
            st["x"][:, :3] = case["poses"]
            d_pass, d_hit = guarded(np.zeros(cells, np.uint32)), guarded(np.zeros(cells, np.uint32))
            assert device_integrate(lsdmod, ctx, case, d_pass, d_hit, dev(rec.view(np.uint8)), pitch) == lsdmod.LSD_OK
            (gp, okp), (gh, okh) = back(d_pass, cells), back(d_hit, cells)
            assert okp and okh and gp.tobytes() == pa.tobytes() and gh.tobytes() == hi.tobytes(), (case["name"], pitch)


# ---- 3. publish --------------------------------------------------------------------------------------------------------------------------
def publish_counters(n, seed):
    """Counters around every threshold of the rule, and beyond 32 bits in the products."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 40, n).astype(np.uint32)
    h = np.minimum(rng.integers(0, 8, n), p).astype(np.uint32)
    big = rng.random(n) < 0.25
    p[big] = rng.integers(1 << 31, 1 << 32, int(big.sum()), dtype=np.uint64).astype(np.uint32)
    h[big] = (p[big].astype(np.int64) // 10 + rng.integers(-1, 2, int(big.sum()))).astype(np.uint32)
    return p, h


@pytest.mark.parametrize("n_cells", [1, 255, 256, 257, 61 * 47])
def test_publish(lsdmod, ctx, n_cells):
    import torch
    p, h = publish_counters(n_cells, n_cells)
    d_p, d_h = dev(p.view(np.int32)), dev(h.view(np.int32))
    for min_pass, num, den in ((2, 1, 10), (0, 1, 1), (5, 3, 4), (1, 0, 7)):
        d_g = torch.full((n_cells + GUARD,), 0x5A, dtype=torch.int8, device="cuda")
        ctx.enqueue_grid_publish_device(d_p.data_ptr(), d_h.data_ptr(), n_cells, d_g.data_ptr(), min_pass, num, den,
                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        g = d_g.cpu().numpy()
        assert (g[n_cells:] == 0x5A).all()
        assert g[:n_cells].tobytes() == gc.publish(p, h, min_pass, num, den).tobytes(), (min_pass, num, den)


def test_publish_hand_made_thresholds(lsdmod, ctx):
    import torch
    p = np.array([1, 2, 20, 20, 20, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 31, 1 << 31], np.uint32)
    h = np.array([1, 2, 1, 2, 3, 429496729, 429496730, 1 << 30, (1 << 30) - 1], np.uint32)
    d_p, d_h = dev(p.view(np.int32)), dev(h.view(np.int32))
    d_g = torch.zeros(len(p), dtype=torch.int8, device="cuda")
    ctx.enqueue_grid_publish_device(d_p.data_ptr(), d_h.data_ptr(), len(p), d_g.data_ptr())
    torch.cuda.synchronize()
    assert d_g.cpu().tolist()[:7] == [-1, 100, 0, 100, 100, 0, 100]
    ctx.enqueue_grid_publish_device(d_p.data_ptr(), d_h.data_ptr(), len(p), d_g.data_ptr(), 2, 1, 2)
    torch.cuda.synchronize()
    assert d_g.cpu().tolist()[7:] == [100, 0]


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, cases):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    case = next(c for c, _, _ in cases if c["name"] == "octants0")
    cells = case["cols"] * case["rows"]
    p0, h0 = pattern(cells, 7), pattern(cells, 8)
    d_pass, d_hit = guarded(p0), guarded(h0)
    wide = np.zeros((1, 1025, 2)); wide[..., 0] = 0.5
    wide[0, :4] = [(5000.0, 0.0), (1e6, 2.0), (1638.0, -1.0), (32766.5 * 0.05, 0.3)]      # rays of up to 32766 cells once the range allows them
    d_sc, d_ln, d_po = dev(wide), dev(np.array([360], np.int32)), dev(np.array([[30.0, 20.0, 0.0]]))
    stream = torch.cuda.current_stream().cuda_stream

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=1, stride=360, po=d_po.data_ptr(), pitch=24, cols=case["cols"], rows=case["rows"],
             resol=0.05, range_max=2.0, pa=d_pass.data_ptr(), hi=d_hit.data_ptr()):
        return ctx.L.lsd_enqueue_grid_integrate_device(h, sc, ln, n, stride, po, pitch, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max,
                                                       pa, hi, stream)
    assert ctx.scan_capacity == 1024
    refused = [call(range_max=32767 * 0.05), call(range_max=1e9), call(resol=2.0 / 40000), call(cols=65536), call(rows=65536), call(stride=1025),
               call(h=None), call(sc=None), call(ln=None), call(po=None), call(pa=None), call(hi=None), call(n=-1), call(stride=0), call(cols=0),
               call(rows=-3), call(resol=0.0), call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf),
               call(pitch=16), call(pitch=28), call(sc=d_sc.data_ptr() + 8), call(po=d_po.data_ptr() + 4)]
    assert refused == [INV] * len(refused), refused
    # the host entry refuses the same, before anything travels
    sc, ln, po = wide[:, :360].copy(), np.array([360], np.int32), np.array([[30.0, 20.0, 0.0]])
    for kw in (dict(range_max=32767 * 0.05), dict(cols=65536), dict(rows=65536), dict(stride=1025)):
        a = dict(cols=case["cols"], rows=case["rows"], range_max=2.0, stride=360)
        a.update(kw)
        hp, hh = p0.copy(), h0.copy()
        src = wide if a["stride"] == 1025 else sc
        st = ctx.L.lsd_grid_integrate(ctx.h, src.ctypes.data, ln.ctypes.data, 1, a["stride"], po.ctypes.data,
                                      lsdmod.lsd_map_param(a["cols"], a["rows"], 0.05, 0.0, 0.0), a["range_max"], hp.ctypes.data, hh.ctypes.data)
        assert st == INV and np.array_equal(hp, p0) and np.array_equal(hh, h0), kw
    bad_len = np.array([361], np.int32)
    assert ctx.L.lsd_grid_integrate(ctx.h, sc.ctypes.data, bad_len.ctypes.data, 1, 360, po.ctypes.data,
                                    lsdmod.lsd_map_param(case["cols"], case["rows"], 0.05, 0.0, 0.0), 2.0, p0.copy().ctypes.data, h0.copy().ctypes.data) == INV
    # publish
    d_g = torch.full((cells + GUARD,), 0x5A, dtype=torch.int8, device="cuda")
    pub = lambda h=ctx.h, pa=d_pass.data_ptr(), hi=d_hit.data_ptr(), n=cells, mn=2, num=1, den=10, g=d_g.data_ptr(): \
        ctx.L.lsd_enqueue_grid_publish_device(h, pa, hi, n, mn, num, den, g, stream)
    refused = [pub(den=0), pub(num=11), pub(num=2, den=1), pub(h=None), pub(pa=None), pub(hi=None), pub(g=None), pub(n=0)]
    assert refused == [INV] * len(refused), refused
    # the accepted edge: just below the limit, on a stride the capacity allows (the long rays leave the grid; their cells outside are skipped)
    assert call(stride=1024, range_max=32766.5 * 0.05) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    (gp, okp), (gh, okh) = back(d_pass, cells), back(d_hit, cells)
    assert okp and okh and (d_g.cpu().numpy() == 0x5A).all()
    edge = dict(case, scans=wide[:, :1024], lens=np.array([360], np.int32), poses=np.array([[30.0, 20.0, 0.0]]), range_max=32766.5 * 0.05)
    wp, wh, _ = gc.run_case(edge, pass_counts=p0.reshape(case["rows"], case["cols"]), hit_counts=h0.reshape(case["rows"], case["cols"]))
    assert gp.tobytes() == wp.tobytes() and gh.tobytes() == wh.tobytes()
    # GridMapper says the same in Python
    for kw in (dict(cols=65536), dict(rows=0), dict(range_max=32767 * 0.05), dict(occ=(1, 0)), dict(occ=(3, 2)), dict(min_pass=-1), dict(mapResol=0.0)):
        a = dict(cols=40, rows=30, mapResol=0.05, mapOriX=0.0, mapOriY=0.0, range_max=2.0, ctx=ctx)
        a.update(kw)
        with pytest.raises(lsdmod.LsdError) as e:
            lsdmod.GridMapper(**a)
        assert e.value.status == INV


# ---- 5. GridMapper ---------------------------------------------------------------------------------------------------------------------
def test_grid_mapper(lsdmod, ctx, cases):
    import torch
    case, pa, hi = next(c for c in cases if c[0]["name"] == "len360_1")
    m = lsdmod.GridMapper(case["cols"], case["rows"], case["resol"], -1.5, 2.25, case["range_max"], ctx=ctx)
    assert m.map_param == (case["cols"], case["rows"], case["resol"], -1.5, 2.25)
    m.integrate(case["scans"], case["lens"], case["poses"])
    m.integrate_device(dev(case["scans"]), dev(case["lens"]), dev(case["poses"]))
    gp, gh = m.counts()
    assert gp.dtype == np.uint32 and gp.shape == (case["rows"], case["cols"])
    assert gp.tobytes() == (2 * pa).tobytes() and gh.tobytes() == (2 * hi).tobytes()
    grid = m.publish_device()
    assert grid.is_cuda and grid.dtype == torch.int8 and tuple(grid.shape) == (case["rows"], case["cols"])
    torch.cuda.synchronize()
    assert grid.cpu().numpy().tobytes() == gc.publish(2 * pa, 2 * hi).tobytes()
    assert set(np.unique(grid.cpu().numpy()).tolist()) == {-1, 0, 100}
    m.clear()
    assert not m.counts()[0].any() and not m.counts()[1].any()
    with pytest.raises(lsdmod.LsdError):
        m.integrate_device(dev(case["scans"]), dev(case["lens"]), dev(case["poses"][:1]))          # fewer poses than scans


# ---- 6. end to end: the data log's first 20 frames -----------------------------------------------------------------------------------------
FRAMES = 20
RANGE_MAX = 8.0


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

    def restated(self, frames, poses):
        pa, hi = np.zeros((self.rows, self.cols), np.uint32), np.zeros((self.rows, self.cols), np.uint32)
        gc.integrate(self.scans[frames], self.lens[frames], poses, self.cols, self.rows, self.resol, RANGE_MAX, pa, hi)
        return pa, hi


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    return DataLog(lsdmod, ctx)


def states_of(lsdmod, out):
    import torch
    torch.cuda.synchronize()
    st = out[0]
    return st.cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(st.shape[:2])


def test_localizer_integrates_its_last_tick(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    with pytest.raises(lsdmod.LsdError):
        loc.integrate_last_tick(m)                                                     # no tick yet
    out = loc.step_device(dev(log.lid[None]), dev(log.odom[None, 1:]))
    loc.integrate_last_tick(m)
    states = states_of(lsdmod, out)
    poses = states["x"][0, :, :3]
    assert (np.abs(poses[:, 0] + 1) >= 1e-4).sum() >= FRAMES // 2                      # most frames have a pose: the map is not empty
    pa, hi = log.restated(np.arange(FRAMES), poses)
    gp, gh = m.counts()
    assert pa.any() and hi.any()
    assert gp.tobytes() == pa.tobytes() and gh.tobytes() == hi.tobytes()
    # the loop closes on the device: the published grid becomes the map, and the next tick runs on it
    grid = m.publish_device()
    loc.set_map_device(grid, *m.map_param)
    out2 = loc.step_device(dev(log.lid[None, :2]), dev(log.odom[None, 1:3]))
    torch.cuda.synchronize()
    assert int(loc.map_counts.item()) >= 0
    assert grid.cpu().numpy().tobytes() == gc.publish(pa, hi).tobytes()
    assert tuple(out2[0].shape[:2]) == (1, 2)


def test_fleet_integrates_only_the_robots_of_a_map(lsdmod, ctx, log):
    S, k = 4, FRAMES // 4
    ids = [0, 1, 0, 1]
    fleet = lsdmod.FleetLocalizer([(log.mc, log.ml, log.mp), (log.mc, log.ml, log.mp)], ids, ctx=ctx)
    od0 = np.stack([log.odom[s * k] for s in range(S)]); od0[:, 0] = 0.0
    fleet.reset(range(S), od0)
    lid = log.lid.reshape(S, k, 360, 2)
    od = np.stack([log.odom[s * k + 1:s * k + 1 + k] for s in range(S)])
    mappers = [log.mapper(lsdmod, ctx), log.mapper(lsdmod, ctx)]
    out = fleet.step_device(dev(lid), dev(od))
    fleet.assign([0], [1])                                                             # after the tick: the tick's ids count
    for i, m in enumerate(mappers):
        fleet.integrate_last_tick(m, map_id=i)
    states = states_of(lsdmod, out)
    for i, m in enumerate(mappers):
        robots = [s for s in range(S) if ids[s] == i]
        frames = np.concatenate([np.arange(s * k, s * k + k) for s in robots])
        poses = np.concatenate([states["x"][s, :, :3] for s in robots])
        pa, hi = log.restated(frames, poses)
        gp, gh = m.counts()
        assert pa.any() and gp.tobytes() == pa.tobytes() and gh.tobytes() == hi.tobytes(), i
    assert not np.array_equal(*[m.counts()[0] for m in mappers])
    with pytest.raises(lsdmod.LsdError):
        fleet.integrate_last_tick(mappers[0], map_id=2)


def test_integrate_last_tick_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    d_lid, d_od = dev(log.lid[None, :4]), dev(log.odom[None, 1:5])
    loc.step_device(d_lid, d_od)                                                       # warm: the staging and the workspace have their size
    loc.integrate_last_tick(m)
    m.publish_device()
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
    loc.integrate_last_tick(m)
    grid = m.publish_device()
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "integrate_last_tick / publish_device returned only after the work in front of them had finished"
    assert grid.is_cuda and m.counts()[0].any()
