"""The tight global localisation on the device (csrc/k_gridlocate_tight.hip: lsd_enqueue_grid_locate_tight_device, lsd_grid_locate_tight;
GridMapper.locate_device / locate, Localizer / FleetLocalizer .locate_last_tick / .relocate_last_tick with tight=) against the restatement
of tests/grid_locate_tight_cases.py, against the existing entry and against the device's own exhaustive search.  The rule is exact and has
no iteration order, so every comparison is byte equality -- the records' 64 bytes and the statistics' 128."""
import math
import time

import numpy as np
import pytest

import fa_relocate_cases as rc
import grid_locate_cases as lc
import grid_locate_tight_cases as tc
import test_fa_relocate_gpu as chain               # the `data` log chain: its log, its lost tick, its restated frames
from test_fa_relocate_gpu import dev, filled, stream

pytestmark = pytest.mark.gpu

F0 = chain.F0
RANGE_MAX = chain.RANGE_MAX


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
    """(case, {tight: (records, statistics, traces)}) over both campaigns: the restatement, computed once."""
    return list(zip(lc.campaign(), tc.expected_existing())) + [(c, res) for c, (res, _) in zip(tc.campaign(), tc.expected())]


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    return chain.DataLog(lsdmod, ctx)


def mp_of(case):
    return (case["cols"], case["rows"], case["resol"], -1.5, 2.25)


def par_of(lsdmod, p):
    return lsdmod.lsd_grid_locate_par(*[p[k] for k in lc.PAR_KEYS])


class Inputs:
    """A case's scans, lengths and pyramid on the device, uploaded once for every flag word."""

    def __init__(self, lsdmod, case, levels=None):
        self.p = case["par"] if levels is None else dict(case["par"], levels=levels)
        self.case, self.n, self.stride = case, len(case["lens"]), case["scans"].shape[1]
        self.sc, self.ln, self.py = dev(case["scans"]), dev(case["lens"]), dev(lc.pyramid(case["corr"], self.p["levels"]))
        self.mp, self.par = lsdmod.lsd_map_param(*mp_of(case)), par_of(lsdmod, self.p)

    def tight(self, cx, tight, out, stats):
        return cx.L.lsd_enqueue_grid_locate_tight_device(cx.h, self.sc.data_ptr(), self.ln.data_ptr(), self.n, self.stride, self.mp, self.case["range_max"],
                                                         self.py.data_ptr(), self.par, tight, out.ptr, stats.ptr if stats is not None else None, stream())

    def existing(self, cx, out, stats):
        return cx.L.lsd_enqueue_grid_locate_device(cx.h, self.sc.data_ptr(), self.ln.data_ptr(), self.n, self.stride, self.mp, self.case["range_max"],
                                                   self.py.data_ptr(), self.par, out.ptr, stats.ptr, stream())


def but_lower_bound(raw):
    a = np.frombuffer(raw, np.uint8).reshape(-1, 64).copy()
    a[:, lc.LOWER_BOUND_BYTES] = 0
    return a


# ---- 1. both campaigns through both entries, at every flag word ------------------------------------------------------------------------------
def test_campaigns_device_entry(lsdmod, ctx, ctx_long, cases):
    """Every byte of the records and of the 128-byte statistics at tight = 0, 1, 2 and 3: the outputs pre-filled, guard words on both
    sides.  tight = 0 against the existing entry's own output as well."""
    import torch
    for case, res in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        ins = Inputs(lsdmod, case)
        n = ins.n
        outs = {t: (filled(64 * n), filled(128 * n)) for t in tc.TIGHTS}
        own = (filled(64 * n), filled(48 * n))
        for t in tc.TIGHTS:
            assert ins.tight(cx, t, *outs[t]) == lsdmod.LSD_OK, (case["name"], t)
        assert ins.existing(cx, *own) == lsdmod.LSD_OK
        torch.cuda.synchronize()
        for t in tc.TIGHTS:
            (got, ok), (got_st, ok_st) = outs[t][0].back(), outs[t][1].back()
            want, want_st, _ = res[t]
            assert ok and ok_st, (case["name"], t)
            assert got.tobytes() == want.tobytes(), (case["name"], t, got.view(lc.LOCATE_DTYPE), want)
            assert got_st.tobytes() == want_st.tobytes(), (case["name"], t, got_st.view(tc.TIGHT_STATS_DTYPE), want_st)
        (rec0, _), (st0, _) = outs[0][0].back(), outs[0][1].back()
        (rec, ok), (st, ok_st) = own[0].back(), own[1].back()
        assert ok and ok_st and rec0.tobytes() == rec.tobytes() and st0.reshape(n, 128)[:, :48].tobytes() == st.tobytes(), case["name"]


def test_campaigns_host_entry(lsdmod, ctx, ctx_long, cases):
    assert lsdmod.GRID_LOCATE_TIGHT_STATS_DTYPE == tc.TIGHT_STATS_DTYPE
    for case, res in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        for t in tc.TIGHTS:
            got, stats = cx.grid_locate_tight(case["scans"], case["lens"], mp_of(case), case["range_max"], case["corr"], case["par"], t, stats=True)
            assert got.tobytes() == res[t][0].tobytes() and stats.tobytes() == res[t][1].tobytes(), (case["name"], t)
        alone = cx.grid_locate_tight(case["scans"], case["lens"], mp_of(case), case["range_max"], case["corr"], case["par"])
        assert alone.tobytes() == res[3][0].tobytes(), case["name"]


def test_levels_5_against_the_device_at_levels_0(lsdmod, ctx, ctx_long, cases):
    """The device's tight search at levels = 5 against the device's own exhaustive search: all record bytes but lower_bound, wherever the
    restatement at levels = 5 does not overflow."""
    import torch
    compared = 0
    for case, _ in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        deep, flat = Inputs(lsdmod, case, levels=5), Inputs(lsdmod, case, levels=0)
        n = deep.n
        d_deep, d_flat = filled(64 * n), filled(64 * n)
        assert deep.tight(cx, 3, d_deep, None) == lsdmod.LSD_OK and flat.tight(cx, 3, d_flat, None) == lsdmod.LSD_OK, case["name"]
        torch.cuda.synchronize()
        (a, ok_a), (b, ok_b) = d_deep.back(), d_flat.back()
        keep = a.view(lc.LOCATE_DTYPE)["flags"] != lc.OVERFLOW
        assert ok_a and ok_b and but_lower_bound(a.tobytes())[keep].tobytes() == but_lower_bound(b.tobytes())[keep].tobytes(), case["name"]
        compared += int(keep.sum())
    assert compared >= 130


def test_a_deeper_pyramid_and_no_scans(lsdmod, ctx, cases):
    import torch
    case, res = next(c for c in cases if c[0]["name"] == "probe_rescue_1")
    ins = Inputs(lsdmod, case)
    ins.py = dev(lc.pyramid(case["corr"], 8))
    d_out, d_stats = filled(64 * ins.n), filled(128 * ins.n)
    assert ins.tight(ctx, 3, d_out, d_stats) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert d_out.back()[0].tobytes() == res[3][0].tobytes() and d_stats.back()[0].tobytes() == res[3][1].tobytes()
    ins.n = 0
    d_out, d_stats = filled(64), filled(128)
    assert ins.tight(ctx, 3, d_out, d_stats) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert d_out.unchanged() and d_stats.unchanged()


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(lsdmod, ctx, cases):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    case = next(c for c, _ in cases if c["name"] == "nb65_1")
    n, corr, base = len(case["lens"]), case["corr"], dict(case["par"])
    d_out, d_stats = filled(64 * n), filled(128 * n)
    wide = np.zeros((1, 1025, 2)); wide[..., 0] = 0.5
    d_sc, d_ln, d_py, d_wide = dev(case["scans"]), dev(case["lens"]), dev(lc.pyramid(corr, 4)), dev(wide)

    def par(se):
        return lsdmod.lsd_grid_locate_par(*[dict(base, **se)[k] for k in lc.PAR_KEYS])

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=n, stride=case["scans"].shape[1], cols=case["cols"], rows=case["rows"], resol=0.05,
             range_max=1.5, pyr=d_py.data_ptr(), tight=3, out=d_out.ptr, stats=d_stats.ptr, **se):
        return ctx.L.lsd_enqueue_grid_locate_tight_device(h, sc, ln, n, stride, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max, pyr, par(se),
                                                          tight, out, stats, stream())
    assert ctx.scan_capacity == 1024
    bad_par = [dict(x0=-(1 << 20) - 1), dict(x0=(1 << 20) + 1), dict(y0=-(1 << 20) - 1), dict(y0=(1 << 20) + 1), dict(nx=0), dict(nx=65536), dict(ny=0),
               dict(ny=-3), dict(ny=65536), dict(n_ang=0), dict(n_ang=4097), dict(ang0=math.nan), dict(ang0=math.inf), dict(ang_step=math.nan),
               dict(ang_step=math.inf), dict(ang_step=-0.5), dict(n_ang=2, ang_step=0.0), dict(levels=-1), dict(levels=9), dict(max_nodes=0),
               dict(max_nodes=(1 << 24) + 1), dict(min_den=0), dict(min_num=5, min_den=4),
               dict(nx=65535, ny=65535, n_ang=4096, levels=7), dict(nx=65535, ny=65535, n_ang=17, levels=4)]
    assert call(nx=65535, ny=65535, n_ang=4096, levels=8, n=0) == lsdmod.LSD_OK            # (exactly 2^28 top nodes: taken; no scans: nothing runs)
    refused = [call(h=None), call(sc=None), call(ln=None), call(pyr=None), call(out=None), call(n=-1), call(stride=0),
               call(sc=d_wide.data_ptr(), n=1, stride=1025), call(cols=0), call(cols=65536), call(rows=-3), call(rows=65536), call(resol=0.0),
               call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf), call(range_max=32767 * 0.05),
               call(sc=d_sc.data_ptr() + 8), call(out=d_out.ptr + 4), call(stats=d_stats.ptr + 2), call(stats=d_stats.ptr + 1), call(ln=d_ln.data_ptr() + 2),
               call(tight=4), call(tight=7), call(tight=1 << 31), call(tight=8 | 3)] + [call(**se) for se in bad_par]
    assert refused == [INV] * len(refused), refused
    lib = lsdmod.load_library()
    assert [lib.lsd_grid_locate_tight_workspace_bytes(n, 68, par(se)) for se in bad_par] == [0] * len(bad_par)
    assert lib.lsd_grid_locate_tight_workspace_bytes(-1, 68, par({})) == lib.lsd_grid_locate_tight_workspace_bytes(1, 0, par({})) == 0
    assert lib.lsd_grid_locate_tight_workspace_bytes(n, 68, par({})) > lib.lsd_grid_locate_workspace_bytes(n, 68, par({})) > 0
    torch.cuda.synchronize()
    assert d_out.unchanged() and d_stats.unchanged()
    # the host entry refuses the same before anything travels, and a length outside 0..stride
    out = np.full(n, chain.FILL, np.uint8).repeat(64).view(lc.LOCATE_DTYPE)
    hstats = np.full(n, chain.FILL, np.uint8).repeat(128).view(tc.TIGHT_STATS_DTYPE)
    keep, keep_stats = out.tobytes(), hstats.tobytes()

    def host(lens=case["lens"], cols=case["cols"], range_max=1.5, co=corr.ctypes.data, tight=3, **se):
        ln = np.ascontiguousarray(lens, np.int32)
        return ctx.L.lsd_grid_locate_tight(ctx.h, case["scans"].ctypes.data, ln.ctypes.data, n, case["scans"].shape[1],
                                           lsdmod.lsd_map_param(cols, case["rows"], 0.05, 0.0, 0.0), range_max, co, par(se), tight, out.ctypes.data,
                                           hstats.ctypes.data)
    bad_len = case["lens"].copy(); bad_len[0] = case["scans"].shape[1] + 1
    refused = [host(lens=bad_len), host(cols=65536), host(range_max=32767 * 0.05), host(co=None), host(nx=0), host(n_ang=2, ang_step=0.0),
               host(min_den=0), host(levels=9), host(max_nodes=0), host(tight=4), host(tight=0x10003)]
    assert refused == [INV] * len(refused) and out.tobytes() == keep and hstats.tobytes() == keep_stats
    # a statistics pointer that is 4-byte but not 8-byte aligned is taken
    assert call(stats=d_stats.ptr + 4, n=1) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert d_out.back()[1] and d_stats.back()[1]
    for bad in (4, "both", -1):
        with pytest.raises(lsdmod.LsdError):
            ctx.enqueue_grid_locate_tight_device(d_sc.data_ptr(), d_ln.data_ptr(), n, case["scans"].shape[1], (case["cols"], case["rows"], 0.05, 0.0, 0.0),
                                                 1.5, d_py.data_ptr(), base, bad, d_out.ptr, None, stream())


# ---- 3. GridMapper -------------------------------------------------------------------------------------------------------------------------
def mapper_with_plane(lsdmod, ctx, case):
    """A mapper whose lookup plane is the case's (refresh=False keeps it)."""
    m = lsdmod.GridMapper(case["cols"], case["rows"], case["resol"], 0.0, 0.0, case["range_max"], ctx=ctx)
    m._corr.copy_(dev(case["corr"]).reshape(m._corr.shape))
    return m


def test_grid_mapper_rescues(lsdmod, ctx, cases):
    """The rescue cases through GridMapper.locate_device: tight=None overflows as the existing entry does, tight=True finds the pose;
    "probe" rescues the probe's cases and not the retry's; the statistics tensor is [n, 128] under tight and [n, 48] without."""
    import torch
    seen = 0
    for case, res in cases:
        if not case["name"].startswith(("probe_rescue_", "retry_rescue_")):
            continue
        m = mapper_with_plane(lsdmod, ctx, case)
        d_sc, d_ln = dev(case["scans"]), dev(case["lens"])
        plain, plain_st = m.locate_device(d_sc, d_ln, case["par"], refresh=False, stats=True)
        rec, st = m.locate_device(d_sc, d_ln, case["par"], refresh=False, stats=True, tight=True)
        rec1 = m.locate_device(d_sc, d_ln, case["par"], refresh=False, tight="probe")
        rec2, st2 = m.locate_device(d_sc, d_ln, case["par"], refresh=False, stats=True, tight=lsdmod.GRID_LOCATE_TIGHT_RETRY)
        torch.cuda.synchronize()
        assert tuple(plain_st.shape) == (1, 48) and tuple(st.shape) == tuple(st2.shape) == (1, 128) and tuple(rec.shape) == (1, 64)
        assert plain.cpu().numpy().tobytes() == res[0][0].tobytes() and res[0][0][0]["flags"] == lc.OVERFLOW
        assert rec.cpu().numpy().tobytes() == res[3][0].tobytes() and st.cpu().numpy().tobytes() == res[3][1].tobytes()
        assert res[3][0][0]["flags"] == lc.ACCEPTED
        assert rec1.cpu().numpy().tobytes() == res[1][0].tobytes() and rec2.cpu().numpy().tobytes() == res[2][0].tobytes()
        assert (res[1][0][0]["flags"] == lc.OVERFLOW) == case["name"].startswith("retry_rescue_") and st2.cpu().numpy().tobytes() == res[2][1].tobytes()
        got, hst = m.locate(case["scans"], case["lens"], case["par"], refresh=False, stats=True, tight=True)
        assert got.dtype == lsdmod.GRID_LOCATE_DTYPE and hst.dtype == lsdmod.GRID_LOCATE_TIGHT_STATS_DTYPE
        assert got.tobytes() == res[3][0].tobytes() and hst.tobytes() == res[3][1].tobytes()
        assert m.locate(case["scans"], case["lens"], case["par"], refresh=False, tight=0).tobytes() == res[0][0].tobytes()
        seen += 1
    assert seen == 6
    with pytest.raises(lsdmod.LsdError):
        m.locate_device(d_sc, d_ln, case["par"], refresh=False, tight="both")


# ---- 4. the chain on the `data` log -----------------------------------------------------------------------------------------------------------
def small_nodes(log, states, carries, corr, p, max_lost):
    """max_nodes of the chain: the largest at which the existing rule overflows on the gathered scans, from the restatement alone; None if
    that search never holds more than one node at a level."""
    S = len(carries)
    scans, lens = np.repeat(log.scans[None, :F0], S, 0), np.repeat(log.lens[None, :F0], S, 0)
    sc, ln, _, _ = rc.gather(carries, np.ascontiguousarray(states["x"][:, :, :3]), scans, lens, None, 0, max_lost, np.zeros((max_lost, scans.shape[2], 2)))
    _, st = lc.locate(sc, ln, log.resol, RANGE_MAX, corr, dict(p, max_nodes=tc.UNLIMITED))
    return sc, ln, int(st[0]["frontier"][1:].max()) - 1


def test_relocate_chain_under_tight(lsdmod, ctx, log):
    """test_fa_relocate_gpu's chain with tight=True: picks, counts, locate records, the 128-byte statistics, seed reports and carries
    equal the restated chain -- the gather, THIS restatement's search, the seed.  max_nodes sits one below the existing rule's largest
    frontier, so the existing rule overflows on the lost robot's scan; whether the tight one does is the restatement's to say."""
    import torch
    loc, m, states, before, p = chain.lost_tick(lsdmod, ctx, log, 2, [1])
    m.likelihood_device()
    torch.cuda.synchronize()
    corr = m._corr.cpu().numpy()
    sc, ln, nodes = small_nodes(log, states, before, corr, p, 2)
    assert nodes >= 1
    p = dict(p, max_nodes=nodes)
    seed_par = rc.SEED_DEFAULTS[:5] + (1 << 16,)
    pick, n_lost, rec, stats, rep = loc.relocate_last_tick(m, p, chain.SEED_MANY, max_lost=2, stats=True, tight=True)
    torch.cuda.synchronize()
    assert m._corr.cpu().numpy().tobytes() == corr.tobytes()
    want_rec, want_st = tc.locate_tight(sc, ln, log.resol, RANGE_MAX, corr, p, 3)
    old_rec, _ = lc.locate(sc, ln, log.resol, RANGE_MAX, corr, p)
    assert old_rec[0]["flags"] == lc.OVERFLOW
    print("existing:", old_rec[0], "tight:", want_rec[0], want_st[0])
    want_pick = np.array([2 * F0 - 1, -1], np.int32)
    want_cy, want_rp = rc.seed(before, F0, want_pick, want_rec, None, seed_par)
    assert pick.cpu().numpy().tolist() == want_pick.tolist() and n_lost.cpu().numpy().tolist() == [1, 1]
    assert tuple(rec.shape) == (2, 64) and tuple(stats.shape) == (2, 128)
    assert rec.cpu().numpy().tobytes() == want_rec.tobytes() and stats.cpu().numpy().tobytes() == want_st.tobytes()
    assert rep.cpu().numpy().tobytes() == want_rp.tobytes() and loc.carries.tobytes() == want_cy.tobytes()
    assert loc.carries[0].tobytes() == before[0].tobytes()
    # locate_last_tick: every slot, the tight statistics
    rec_all, st_all = loc.locate_last_tick(m, p, refresh=False, stats=True, tight="probe")
    torch.cuda.synchronize()
    scans, lens = np.repeat(log.scans[None, :F0], 2, 0).reshape(2 * F0, -1, 2), np.repeat(log.lens[None, :F0], 2, 0).reshape(-1)
    want_all, want_all_st = tc.locate_tight(scans, lens, log.resol, RANGE_MAX, corr, p, 1)
    assert rec_all.cpu().numpy().tobytes() == want_all.tobytes() and st_all.cpu().numpy().tobytes() == want_all_st.tobytes()


# ---- 5. the fleet --------------------------------------------------------------------------------------------------------------------------
def test_fleet_relocates_both_maps_under_tight(lsdmod, ctx, log):
    """Two maps with a lost robot on each: each map's call gathers, locates under the tight rule and seeds its own lost robot, and every
    other carry keeps every byte."""
    import torch
    import fa_restatement as fr
    MAP_OF = chain.MAP_OF
    mp2 = np.array(log.mp, np.float64)
    mp2[2:5] *= 2.0
    S = len(MAP_OF)
    lid, odom = np.repeat(log.lid[None, :F0], S, 0).copy(), np.repeat(log.odom[None, :F0 + 1], S, 0).copy()
    for s in (1, 3):
        lid[s, ..., 0] = np.where(np.isfinite(lid[s, ..., 0]), lid[s, ..., 0] * 2.0, lid[s, ..., 0])
        odom[s, :, :2] *= 2.0
    mc2 = ctx.map_cache(fr.load_log("data")[0].copy(), float(mp2[2]), lsdmod.z_occ_max_dis)
    fl = lsdmod.FleetLocalizer([(log.mc, log.ml, log.mp), (mc2, log.ml, mp2)], MAP_OF, odom0=odom[:, 0], ctx=ctx)
    out = fl.step_device(dev(lid), dev(odom[:, 1:]))
    mappers = [log.mapper(lsdmod, ctx), lsdmod.GridMapper(log.cols, log.rows, float(mp2[2]), float(mp2[3]), float(mp2[4]), 2.0 * RANGE_MAX, ctx=ctx)]
    for i in (0, 1):
        fl.integrate_last_tick(mappers[i], i)
        mappers[i].likelihood_device()
    chain.reset_robots(lsdmod, fl, out, [1, 4], F0)                           # lost: robot 1 on map 1, robot 4 on map 0
    torch.cuda.synchronize()
    states = out[0].cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(S, F0).copy()
    before = fl.carries
    scans, lens = np.repeat(log.scans[None, :F0], S, 0).copy(), np.repeat(log.lens[None, :F0], S, 0)
    for s in (1, 3):
        scans[s, ..., 0] *= 2.0
    keys = np.array(MAP_OF, np.int32)
    seed_par = rc.SEED_DEFAULTS[:5] + (1 << 16,)
    now = before
    for i, found, lost in ((0, 0, 4), (1, 3, 1)):
        x, y, ang = (float(v) for v in states["x"][found, F0 - 1, :3])
        p = lc.par(int(x) - 11, int(y) - 9, 24, 19, ang0=float(round(ang)) - 4.0, ang_step=2.0, n_ang=5, levels=3, max_nodes=40, min_beams=30, min_num=1,
                   min_den=8)
        pick, n_lost, rec, stats, rep = fl.relocate_last_tick(mappers[i], i, p, chain.SEED_MANY, max_lost=2, refresh=False, stats=True, tight=True)
        torch.cuda.synchronize()
        corr = mappers[i]._corr.cpu().numpy()
        sc, ln, want_pick, want_n = rc.gather(now, np.ascontiguousarray(states["x"][:, :, :3]), scans, lens, keys, i, 2, np.zeros((2, scans.shape[2], 2)))
        want_rec, want_st = tc.locate_tight(sc, ln, (log.resol, float(mp2[2]))[i], (RANGE_MAX, 2.0 * RANGE_MAX)[i], corr, p, 3)
        want_cy, want_rp = rc.seed(now, F0, want_pick, want_rec, None, seed_par)
        assert want_pick.tolist() == [lost * F0 + F0 - 1, -1] == pick.cpu().numpy().tolist() and n_lost.cpu().numpy().tolist() == want_n.tolist() == [1, 1]
        print("map", i, want_rec[0], want_st[0])
        assert rec.cpu().numpy().tobytes() == want_rec.tobytes() and stats.cpu().numpy().tobytes() == want_st.tobytes(), (i, want_rec, want_st)
        assert rep.cpu().numpy().tobytes() == want_rp.tobytes()
        after = fl.carries
        others = [s for s in range(S) if s != lost]
        assert after.tobytes() == want_cy.tobytes() and after[others].tobytes() == now[others].tobytes()
        now = after
    pick, n_lost, rec, stats = fl.locate_last_tick(mappers[0], 0, p, max_lost=1, refresh=False, stats=True, tight="retry")
    torch.cuda.synchronize()
    assert tuple(stats.shape) == (1, 128) and fl.carries.tobytes() == now.tobytes()


# ---- 6. nothing waits ----------------------------------------------------------------------------------------------------------------------
def test_tight_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc, m, states, before, p = chain.lost_tick(lsdmod, ctx, log, 2, [1])
    fl = lsdmod.FleetLocalizer([(log.mc, log.ml, log.mp)], [0, 0], odom0=log.odom[0], ctx=ctx)
    d_lid, d_od = dev(np.repeat(log.lid[None, :F0], 2, 0)), dev(np.repeat(log.odom[None, 1:F0 + 1], 2, 0))
    out = fl.step_device(d_lid, d_od)
    chain.reset_robots(lsdmod, fl, out, [0], F0)
    d_sc, d_ln = dev(log.scans[:F0]), dev(log.lens[:F0])
    d_pyr = m.pyramid_device(p["levels"])
    d_out, d_stats = filled(64 * F0), filled(128 * F0)

    def calls():
        got = loc.relocate_last_tick(m, p, chain.SEED_MANY, max_lost=2, stats=True, tight=True)
        got += fl.locate_last_tick(m, 0, p, max_lost=2, refresh=False, tight=True)
        got += fl.relocate_last_tick(m, 0, p, chain.SEED_MANY, max_lost=2, refresh=False, tight="probe")
        got += (loc.locate_last_tick(m, p, refresh=False, tight=True),)
        got += m.locate_device(d_sc, d_ln, p, stats=True, tight=True)
        ctx.enqueue_grid_locate_tight_device(d_sc.data_ptr(), d_ln.data_ptr(), F0, log.scans.shape[1], m.map_param, m.range_max, d_pyr.data_ptr(), p, 3,
                                             d_out.ptr, d_stats.ptr, stream())
        return got
    for _ in range(2):                                                       # warm: the staging, the workspaces and the pyramid have their size
        calls()
    loc._carry.copy_(dev(before.view(np.uint8).reshape(-1)))
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
    got = calls()
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "the tight locate calls returned only after the work in front of them had finished"
    assert all(t.is_cuda for t in got) and d_out.back()[1] and d_stats.back()[1]
