"""Ray casting on the grid on the device (csrc/k_gridray.hip: lsd_enqueue_grid_raycast_device, lsd_grid_raycast; GridMapper.raycast_device,
screen_and_integrate_device; Localizer.screen_and_integrate_last_tick) against the restatement of tests/grid_ray_cases.py.  The rule is
exact and has no iteration order, so every comparison is byte equality."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import grid_cases as gc
import grid_ray_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 256                                    # bytes behind each output
GUARD_BYTE = 0xA5


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


def fill(nbytes, seed):
    """The pattern the outputs start from (no byte of it is 0 or the guard's)."""
    return ((np.arange(nbytes, dtype=np.uint64) * 2654435761 + seed) % 160 + 1).astype(np.uint8)


@pytest.fixture(scope="module")
def cases(oracle):
    """(case, out, sums, scans_out) of the campaign on pre-filled outputs: the restatement, computed once."""
    return [(case,) + rc.run_case(case, fill=fill)[:3] for case in rc.campaign()]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes, seed):
    return dev(np.concatenate([fill(nbytes, seed), np.full(GUARD, GUARD_BYTE, np.uint8)]))


def back(t, nbytes):
    """(the bytes, True if the guard is untouched) of a guarded tensor."""
    a = t.cpu().numpy()
    return a[:nbytes].tobytes(), bool((a[nbytes:] == GUARD_BYTE).all())


def map_param(case):
    return (case["cols"], case["rows"], case["resol"], -1.5, 2.25)


def c_par(lsdmod, par):
    return lsdmod.lsd_grid_ray_par(par["tol"], par["drop_mask"], par["min_beams"], par["ok_num"], par["ok_den"], par["gate"])


def device_raycast(lsdmod, cx, case, d_poses=None, pitch=24, in_place=False):
    """The device entry through the raw C ABI on guarded, pre-filled outputs, then the caller's synchronisation.  Returns (status, the
    bytes of out, sums and the screened scans, True if every guard is untouched)."""
    import torch
    n, stride = case["scans"].shape[:2]
    sizes = (n * stride * 32, n * 64, n * stride * 16)
    d_out, d_sum = guarded(sizes[0], 1), guarded(sizes[1], 2)
    d_so = dev(np.concatenate([case["scans"].reshape(-1).view(np.uint8), np.full(GUARD, GUARD_BYTE, np.uint8)])) if in_place else guarded(sizes[2], 3)
    d_sc = d_so if in_place else dev(case["scans"])
    d_ln, d_gr = dev(case["lens"]), dev(case["grid"])
    d_po = dev(case["poses"]) if d_poses is None else d_poses
    st = cx.L.lsd_enqueue_grid_raycast_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, stride, d_po.data_ptr(), pitch,
                                              lsdmod.lsd_map_param(*map_param(case)), case["range_max"], d_gr.data_ptr(), c_par(lsdmod, case["par"]),
                                              d_out.data_ptr(), d_sum.data_ptr(), d_so.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [back(t, nb) for t, nb in zip((d_out, d_sum, d_so), sizes)]
    return st, [g[0] for g in got], all(g[1] for g in got)


# ---- 1. the campaign through both entries ------------------------------------------------------------------------------------------------
def test_campaign_device_entry(lsdmod, ctx, ctx_long, cases):
    """Every byte of every record, summary and screened reading; the slots at i >= len keep the pattern (the restatement starts from the
    same one), the guards behind the three outputs stay."""
    for case, out, sums, so in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        st, got, guards = device_raycast(lsdmod, cx, case)
        assert st == lsdmod.LSD_OK and guards, case["name"]
        assert got[0] == out.tobytes(), case["name"]
        assert got[1] == sums.tobytes(), case["name"]
        assert got[2] == so.tobytes(), case["name"]


def test_campaign_host_entry(lsdmod, ctx, ctx_long, cases):
    for case, out, sums, so in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        n, stride = case["scans"].shape[:2]
        o0 = fill(n * stride * 32, 1).view(lsdmod.GRID_RAY_DTYPE)
        s0 = fill(n * 64, 2).view(lsdmod.GRID_RAY_SUM_DTYPE)
        so0 = fill(n * stride * 16, 3).view(np.float64)
        go, gs, gso = cx.grid_raycast(case["scans"], case["lens"], case["poses"], map_param(case), case["range_max"], case["grid"],
                                      c_par(lsdmod, case["par"]), o0, s0, so0)
        assert go.tobytes() == out.tobytes() and gs.tobytes() == sums.tobytes() and gso.tobytes() == so.tobytes(), case["name"]


def test_no_scans_is_a_no_op(lsdmod, ctx, cases):
    import torch
    case = cases[0][0]
    d_out, d_sum = guarded(64, 1), guarded(64, 2)
    d = dev(np.zeros(8))
    st = ctx.L.lsd_enqueue_grid_raycast_device(ctx.h, d.data_ptr(), d.data_ptr(), 0, 4, d.data_ptr(), 24, lsdmod.lsd_map_param(*map_param(case)), 2.0,
                                               d.data_ptr(), c_par(lsdmod, rc.ray_par()), d_out.data_ptr(), d_sum.data_ptr(), None,
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK and back(d_out, 64) == (fill(64, 1).tobytes(), True) and back(d_sum, 64) == (fill(64, 2).tobytes(), True)


# ---- 2. other inputs ---------------------------------------------------------------------------------------------------------------------
PICKED = ("octants1", "skipped_scans0", "len65_1", "k_hit_strides0", "edges1", "summary_gate1", "len257_2")


def test_screening_in_place(lsdmod, ctx, cases):
    picked = [c for c in cases if c[0]["name"] in PICKED]
    assert len(picked) == len(PICKED)
    for case, out, sums, so in picked:
        st, got, guards = device_raycast(lsdmod, ctx, case, in_place=True)
        live = np.arange(case["scans"].shape[1])[None, :] < case["lens"][:, None]
        want = np.where(live[..., None], so, case["scans"])              # beyond len the input's own readings stay
        assert st == lsdmod.LSD_OK and guards and got[0] == out.tobytes() and got[1] == sums.tobytes(), case["name"]
        assert got[2] == want.tobytes(), case["name"]


def test_poses_as_carries_and_states(lsdmod, ctx, cases):
    rng = np.random.default_rng(3)
    picked = [c for c in cases if c[0]["name"] in PICKED[:4]]
    for case, out, sums, so in picked:
        n = len(case["lens"])
        for dtype, pitch in ((lsdmod.FA_CARRY_DTYPE, 768), (lsdmod.FA_STATE_DTYPE, 720)):
            rec = rng.integers(0, 256, n * pitch, dtype=np.uint8).view(dtype)        # everything but the pose is noise
            st = rec["state"] if pitch == 768 else rec
            st["x"][:, :3] = case["poses"]
            status, got, guards = device_raycast(lsdmod, ctx, case, dev(rec.view(np.uint8)), pitch)
            assert status == lsdmod.LSD_OK and guards, (case["name"], pitch)
            assert got[0] == out.tobytes() and got[1] == sums.tobytes() and got[2] == so.tobytes(), (case["name"], pitch)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, oracle):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    cols, rows, stride = 33000, 3, 1024
    grid = np.zeros((rows, cols), np.int8)
    grid[0, 32800], grid[2, 20000:20003] = 100, -1
    sc = np.zeros((1, 1025, 2)); sc[..., 0] = 0.5
    sc[0, :6] = [(5000.0, 0.0), (math.inf, 0.0), (1638.0, 1e-5), (1.0, math.pi), (1635.0, -3.06e-5), (250.0, 3.0e-5)]
    lens, poses = np.array([360], np.int32), np.array([[100.4, 1.0, 0.0]])
    d_sc, d_ln, d_po, d_gr = dev(sc), dev(lens), dev(poses), dev(grid)
    sizes = (stride * 32, 64, stride * 16)
    d_out, d_sum, d_so = guarded(sizes[0], 1), guarded(sizes[1], 2), guarded(sizes[2], 3)
    stream = torch.cuda.current_stream().cuda_stream
    good = rc.ray_par(tol=0.1)

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=1, stride=360, po=d_po.data_ptr(), pitch=24, cols=61, rows=3, resol=0.05,
             range_max=2.0, gr=d_gr.data_ptr(), out=d_out.data_ptr(), su=d_sum.data_ptr(), so=d_so.data_ptr(), **par):
        return ctx.L.lsd_enqueue_grid_raycast_device(h, sc, ln, n, stride, po, pitch, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max,
                                                     gr, c_par(lsdmod, dict(good, **par)), out, su, so, stream)
    assert ctx.scan_capacity == 1024
    refused = [call(range_max=32767 * 0.05), call(range_max=1e9), call(resol=2.0 / 40000), call(cols=65536), call(rows=65536), call(stride=1025),
               call(h=None), call(sc=None), call(ln=None), call(po=None), call(n=-1), call(stride=0), call(cols=0), call(rows=-3),
               call(resol=0.0), call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf), call(pitch=16),
               call(pitch=28), call(sc=d_sc.data_ptr() + 8), call(po=d_po.data_ptr() + 4),
               call(gr=None), call(out=None), call(su=None), call(tol=math.nan), call(tol=math.inf), call(tol=-0.01), call(drop_mask=128),
               call(ok_den=0), call(ok_num=3, ok_den=2), call(out=d_out.data_ptr() + 4), call(su=d_sum.data_ptr() + 4),
               call(so=d_sc.data_ptr() + 16), call(so=d_sc.data_ptr() + 359 * 16), call(sc=d_sc.data_ptr() + 16, so=d_sc.data_ptr()),
               call(so=d_so.data_ptr() + 8)]
    assert refused == [INV] * len(refused), refused
    torch.cuda.synchronize()
    for t, nb, seed in zip((d_out, d_sum, d_so), sizes, (1, 2, 3)):
        assert back(t, nb) == (fill(nb, seed).tobytes(), True)
    assert d_sc.cpu().numpy().tobytes() == sc.tobytes()
    # the host entry refuses the same, before anything travels
    h_sc, o0, s0, so0 = sc[:, :360].copy(), fill(360 * 32, 1), fill(64, 2), fill(360 * 16, 3)
    small = np.zeros((3, 61), np.int8)

    def host(src=h_sc, ln=lens, stride=360, cols=61, rows=3, range_max=2.0, gr=small, **par):
        o, s, so = o0.copy(), s0.copy(), so0.copy()
        st = ctx.L.lsd_grid_raycast(ctx.h, src.ctypes.data, ln.ctypes.data, 1, stride, poses.ctypes.data, lsdmod.lsd_map_param(cols, rows, 0.05, 0.0, 0.0),
                                    range_max, gr.ctypes.data if gr is not None else None, c_par(lsdmod, dict(good, **par)), o.ctypes.data, s.ctypes.data,
                                    so.ctypes.data)
        return st, np.array_equal(o, o0) and np.array_equal(s, s0) and np.array_equal(so, so0)
    for kw in (dict(range_max=32767 * 0.05), dict(cols=65536), dict(rows=65536), dict(src=sc, stride=1025), dict(ln=np.array([361], np.int32)),
               dict(ln=np.array([-1], np.int32)), dict(gr=None), dict(tol=math.nan), dict(tol=-1.0), dict(drop_mask=128), dict(ok_den=0),
               dict(ok_num=2, ok_den=1)):
        assert host(**kw) == (INV, True), kw
    assert host()[0] == lsdmod.LSD_OK
    # the accepted edge: just below the limit, on a stride the capacity allows -- rays of 32 767 steps through a free strip
    edge = dict(name="edge", cols=cols, rows=rows, resol=0.05, range_max=32766.5 * 0.05, scans=sc[:, :stride], lens=lens, poses=poses, grid=grid,
                par=good)
    out, sums, so, trace = rc.run_case(edge, fill=fill)
    steps = [max(abs(t["x1"] - t["x0"]), abs(t["y1"] - t["y0"])) for t in trace if not t["skip"]]
    assert max(steps) == 32767 and any(t["k_hit"] == 32700 for t in trace) and any(t["k_hit"] < 0 and t["k_unk"] < 0 for t in trace)
    assert call(stride=stride, cols=cols, rows=rows, range_max=edge["range_max"]) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    got = [back(t, nb) for t, nb in zip((d_out, d_sum, d_so), sizes)]
    assert all(g[1] for g in got)
    assert got[0][0] == out.tobytes() and got[1][0] == sums.tobytes() and got[2][0] == so.tobytes()
    # grid_ray says the same in Python
    for kw in (dict(tol=None), dict(tol=0.1, drop=("nothing",)), dict(tol=0.1, drop=(7,)), dict(tol=0.1, min_beams=-1)):
        with pytest.raises(lsdmod.LsdError) as e:
            lsdmod.grid_ray(**kw)
        assert e.value.status == INV
    p = lsdmod.grid_ray(dict(drop=("short", "long", 6), ok=(2, 3), gate=True), mapResol=0.05)
    assert (p.tol, p.drop_mask, p.min_beams, p.ok_num, p.ok_den, p.gate) == (0.1, 16 + 32 + 64, 1, 2, 3, 1)


# ---- 4. chaining -------------------------------------------------------------------------------------------------------------------------
def sum_poses(sums):
    return np.stack([sums["x"], sums["y"], sums["ang"]], 1)


def test_summaries_are_poses_for_the_integration(lsdmod, ctx, cases):
    """The summary array as d_poses at pitch 64, the screened scans as d_scans: the restatement's planes, gated scans adding nothing."""
    import torch
    picked = [c for c in cases if c[0]["name"] in ("summary_gate0", "summary_gate2", "len360_1", "skipped_scans1", "leaves2")]
    assert len(picked) == 5
    gated = 0
    for case, out, sums, so in picked:
        n, stride = case["scans"].shape[:2]
        cells = case["cols"] * case["rows"]
        par = dict(case["par"], gate=1)
        o, s, sc_out = np.zeros((n, stride), rc.RAY_DTYPE), np.zeros(n, rc.SUM_DTYPE), np.zeros((n, stride, 2))
        rc.raycast(case["scans"], case["lens"], case["poses"], case["grid"], case["resol"], case["range_max"], par, o, s, sc_out)
        gated += int(((s["x"] == -1.0) & (case["poses"][:, 0] != -1.0)).sum())
        pa, hi = np.zeros((case["rows"], case["cols"]), np.uint32), np.zeros((case["rows"], case["cols"]), np.uint32)
        gc.integrate(sc_out, case["lens"], sum_poses(s), case["cols"], case["rows"], case["resol"], case["range_max"], pa, hi)
        d_sc, d_ln, d_po, d_gr = dev(case["scans"]), dev(case["lens"]), dev(case["poses"]), dev(case["grid"])
        d_out, d_sum, d_so = dev(np.zeros(n * stride * 32, np.uint8)), dev(np.zeros(n * 64, np.uint8)), dev(np.zeros((n, stride, 2)))
        d_planes = torch.zeros((2, cells), dtype=torch.int32, device="cuda")
        mp = map_param(case)
        ctx.enqueue_grid_raycast_device(d_sc.data_ptr(), d_ln.data_ptr(), n, stride, d_po.data_ptr(), 24, mp, case["range_max"], d_gr.data_ptr(),
                                        c_par(lsdmod, par), d_out.data_ptr(), d_sum.data_ptr(), d_so.data_ptr())
        ctx.enqueue_grid_integrate_device(d_so.data_ptr(), d_ln.data_ptr(), n, stride, d_sum.data_ptr(), 64, mp, case["range_max"],
                                          d_planes[0].data_ptr(), d_planes[1].data_ptr())
        torch.cuda.synchronize()
        got = d_planes.cpu().numpy().view(np.uint32)
        assert d_sum.cpu().numpy().tobytes() == s.tobytes(), case["name"]
        assert got[0].tobytes() == pa.tobytes() and got[1].tobytes() == hi.tobytes(), case["name"]
    assert gated >= 3


def test_screen_and_integrate_device_is_the_chain_by_hand(lsdmod, ctx, cases):
    import torch
    case = next(c for c, *_ in cases if c["name"] == "len360_1")
    n, stride = case["scans"].shape[:2]
    live = np.arange(stride)[None, :] < case["lens"][:, None]
    ray = dict(tol=None, drop=("short", "unexplored"), min_beams=10, ok=(1, 3), gate=True)
    mappers = [lsdmod.GridMapper(case["cols"], case["rows"], case["resol"], -1.5, 2.25, case["range_max"], ctx=ctx) for _ in range(2)]
    d_sc, d_ln, d_po = dev(case["scans"]), dev(case["lens"]), dev(case["poses"])
    for m in mappers:
        m.integrate_device(d_sc, d_ln, d_po)                          # a map to judge against: the scans themselves, entered twice
        m.integrate_device(d_sc, d_ln, d_po)
    rays, sums = mappers[0].screen_and_integrate_device(d_sc, d_ln, d_po, ray=ray)
    grid = mappers[1].publish_device()
    rays2, sums2, so2 = mappers[1].raycast_device(d_sc, d_ln, d_po, ray=ray, d_grid=grid, screened=True)
    mappers[1].integrate_device(so2, d_ln, sums2, 64)
    torch.cuda.synchronize()
    as_rays = lambda t: t.cpu().numpy().reshape(-1).view(lsdmod.GRID_RAY_DTYPE).reshape(n, stride)
    assert tuple(rays.shape) == (n, stride, 32) and tuple(sums.shape) == (n, 64) and tuple(so2.shape) == (n, stride, 2)
    assert as_rays(rays)[live].tobytes() == as_rays(rays2)[live].tobytes() and sums.cpu().numpy().tobytes() == sums2.cpu().numpy().tobytes()
    assert mappers[0].last_screened.cpu().numpy()[live].tobytes() == so2.cpu().numpy()[live].tobytes()
    (p0, h0), (p1, h1) = mappers[0].counts(), mappers[1].counts()
    assert p0.tobytes() == p1.tobytes() and h0.tobytes() == h1.tobytes()
    # ... and the restatement's
    pa, hi, _ = gc.run_case(case)
    pa, hi = 2 * pa, 2 * hi
    grid0 = gc.publish(pa, hi)
    par = rc.ray_par(tol=2 * case["resol"], drop_mask=(1 << rc.SHORT) | (1 << rc.UNEXPLORED), min_beams=10, ok_num=1, ok_den=3, gate=1)
    o, s, so = np.zeros((n, stride), rc.RAY_DTYPE), np.zeros(n, rc.SUM_DTYPE), np.zeros((n, stride, 2))
    rc.raycast(case["scans"], case["lens"], case["poses"], grid0, case["resol"], case["range_max"], par, o, s, so)
    gc.integrate(so, case["lens"], sum_poses(s), case["cols"], case["rows"], case["resol"], case["range_max"], pa, hi)
    assert as_rays(rays)[live].tobytes() == o[live].tobytes() and sums.cpu().numpy().tobytes() == s.tobytes()
    assert p0.tobytes() == pa.tobytes() and h0.tobytes() == hi.tobytes()
    # the host convenience of the mapper: the same records, zeros beyond len
    mr, ms = mappers[1].raycast(case["scans"], case["lens"], case["poses"], ray=ray, grid=grid0)
    assert mr.tobytes() == o.tobytes() and ms.tobytes() == s.tobytes()


# ---- 5. end to end: the data log's first 20 frames -----------------------------------------------------------------------------------------
FRAMES, HALF = 20, 10
RANGE_MAX = 8.0


class Replay:
    """step_device + integrate_last_tick for the first 10 frames, step_device + screen_and_integrate_last_tick for the rest, the published
    grid handed to set_map_device and one more tick: the device's side, run once."""

    def __init__(self, lsdmod, ctx):
        import torch
        m, self.mp, lid, odom = fr.load_log("data")
        lid, odom = lid[:FRAMES], odom[:FRAMES + 1]
        mc = ctx.map_cache(m.copy(), float(self.mp[2]), lsdmod.z_occ_max_dis)
        ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.cols, self.rows, self.resol = int(self.mp[0]), int(self.mp[1]), float(self.mp[2])
        self.scans, self.lens = lsdmod.lidar_frames_batch(lid)                       # what k_ingest writes
        loc = lsdmod.Localizer(mc, ml, self.mp, 1, odom0=odom[0], ctx=ctx)
        mapper = lsdmod.GridMapper(self.cols, self.rows, self.resol, float(self.mp[3]), float(self.mp[4]), RANGE_MAX, ctx=ctx)
        with pytest.raises(lsdmod.LsdError):
            loc.screen_and_integrate_last_tick(mapper)                               # no tick yet
        self.ray = dict(drop=("short", "long"), min_beams=30, ok=(1, 2), gate=True)
        states = lambda out: out[0].cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE)["x"][:, :3].copy()
        out = loc.step_device(dev(lid[None, :HALF]), dev(odom[None, 1:HALF + 1]))
        loc.integrate_last_tick(mapper)
        torch.cuda.synchronize()
        self.poses1 = states(out)
        out = loc.step_device(dev(lid[None, HALF:]), dev(odom[None, HALF + 1:]))
        rays, sums = loc.screen_and_integrate_last_tick(mapper, ray=self.ray)
        torch.cuda.synchronize()
        self.poses2 = states(out)
        self.rays = rays.cpu().numpy().reshape(-1).view(lsdmod.GRID_RAY_DTYPE).reshape(FRAMES - HALF, -1)
        self.sums = sums.cpu().numpy().reshape(-1).view(lsdmod.GRID_RAY_SUM_DTYPE)
        self.screened = mapper.last_screened.cpu().numpy()
        self.counts = mapper.counts()
        # the loop closes on the device: the grid published after screening becomes the map, and the next tick runs on it
        grid = mapper.publish_device()
        loc.set_map_device(grid, *mapper.map_param)
        out2 = loc.step_device(dev(lid[None, :2]), dev(odom[None, 1:3]))
        torch.cuda.synchronize()
        self.grid, self.map_count, self.next_shape = grid.cpu().numpy(), int(loc.map_counts.item()), tuple(out2[0].shape[:2])


@pytest.fixture(scope="module")
def replay(lsdmod, ctx, oracle):
    return Replay(lsdmod, ctx)


@pytest.fixture(scope="module")
def restated(replay):
    r = replay
    pa, hi = np.zeros((r.rows, r.cols), np.uint32), np.zeros((r.rows, r.cols), np.uint32)
    gc.integrate(r.scans[:HALF], r.lens[:HALF], r.poses1, r.cols, r.rows, r.resol, RANGE_MAX, pa, hi)
    grid = gc.publish(pa, hi)
    n, stride = FRAMES - HALF, r.scans.shape[1]
    par = rc.ray_par(tol=2 * r.resol, drop_mask=(1 << rc.SHORT) | (1 << rc.LONG), min_beams=30, ok_num=1, ok_den=2, gate=1)
    out, sums, so = np.zeros((n, stride), rc.RAY_DTYPE), np.zeros(n, rc.SUM_DTYPE), np.zeros((n, stride, 2))
    rc.raycast(r.scans[HALF:], r.lens[HALF:], r.poses2, grid, r.resol, RANGE_MAX, par, out, sums, so)
    gc.integrate(so, r.lens[HALF:], sum_poses(sums), r.cols, r.rows, r.resol, RANGE_MAX, pa, hi)
    return grid, out, sums, so, pa, hi


def test_log_replay_equals_the_restatement(replay, restated):
    r = replay
    grid, out, sums, so, pa, hi = restated
    assert (np.abs(r.poses1[:, 0] + 1) >= 1e-4).sum() >= HALF // 2 and (grid == 100).any()      # there is a map to judge against
    live = np.arange(r.scans.shape[1])[None, :] < r.lens[HALF:, None]
    assert live.sum() > 1000 and (out["cls"][live] >= rc.AGREE_FREE).sum() > 500               # and beams that were judged
    assert r.rays[live].tobytes() == out[live].tobytes()
    assert r.sums.tobytes() == sums.tobytes()
    assert r.screened[live].tobytes() == so[live].tobytes()
    assert r.counts[0].tobytes() == pa.tobytes() and r.counts[1].tobytes() == hi.tobytes()


def test_published_grid_after_screening_is_taken_as_the_map(replay, restated):
    pa, hi = restated[4:]
    assert replay.grid.tobytes() == gc.publish(pa, hi).tobytes()
    assert replay.map_count >= 0 and replay.next_shape == (1, 2)


def test_the_new_calls_do_not_synchronise(lsdmod, ctx, replay):
    import torch
    m, mp, lid, odom = fr.load_log("data")
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsdmod.z_occ_max_dis)
    ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    loc = lsdmod.Localizer(mc, ml, mp, 1, odom0=odom[0], ctx=ctx)
    mapper = lsdmod.GridMapper(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]), RANGE_MAX, ctx=ctx)
    d_lid, d_od = dev(lid[None, :4]), dev(odom[None, 1:5])
    d_sc, d_ln, d_po = dev(replay.scans[:4]), dev(replay.lens[:4]), dev(replay.poses1[:4])
    loc.step_device(d_lid, d_od)                                                       # warm: the staging and the allocator have their sizes
    loc.screen_and_integrate_last_tick(mapper)
    mapper.raycast_device(d_sc, d_ln, d_po, screened=True)
    mapper.screen_and_integrate_device(d_sc, d_ln, d_po)
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
    rays, sums = loc.screen_and_integrate_last_tick(mapper)
    mapper.raycast_device(d_sc, d_ln, d_po, screened=True)
    mapper.screen_and_integrate_device(d_sc, d_ln, d_po)
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "a ray-casting call returned only after the work in front of it had finished"
    assert rays.is_cuda and sums.is_cuda and mapper.counts()[0].any()
