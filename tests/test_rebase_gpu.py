"""Maps that change under a running fleet, on the device: k_fa_rebase against its restatement (tests/fa_rebase.py) bit for bit, the
opt-in re-base at Localizer's hand-over against the restated loop fed the device's own FeatureScan and candidates, and the per-map
device hand-over of FleetLocalizer against a Localizer on each map alone.  The expectation is the restatement or the single-map
Localizer everywhere, never the code under test.

Fixtures: the first frames of the data log on its map (A); B, that map grown by 96 columns on the left and 80 rows on top
(tests/fa_rebase.py: grow_map / grow_grid), a shift of 125 px, above maxEstiDist; `data2x`, the twin of tests/test_fleet_gpu.py
(mapResol, the origin, the ranges and the odometry's x, y doubled)."""
import numpy as np
import pytest

import fa_rebase as rb
import fa_restatement as fr
from fa_resume import ResumableLoop

pytestmark = pytest.mark.gpu
STATE_B, REPORT_B, CARRY_B = 720, 72, 768
K = 6                                                                          # frames before and after a hand-over
D_COLS, D_ROWS = 96, 80
LINES_CAP = 128


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_state(rec, x, P):
    assert np.array_equal(rec["x"], np.array(x), equal_nan=True), (rec["x"][:3], x[:3])
    assert np.array_equal(rec["P"].reshape(9, 9, order="F"), np.array(P), equal_nan=True)


def same_report(rep, want):
    assert (int(rep["branch"]), int(rep["n_kept"]), int(rep["llt"]), int(rep["n_pairs"])) == (want["branch"], want["n_kept"], want["llt"], want["n_pairs"])
    est = np.array([rep["estimate"]["x"], rep["estimate"]["y"], rep["estimate"]["ang"], rep["score"]])
    assert np.array_equal(est, np.array(list(want["estimate"]) + [want["score"]]), equal_nan=True)
    assert np.array_equal([rep["scan_pose"][k] for k in ("x", "y", "ang")], want["scan_pose"], equal_nan=True)


class Site:
    """The data log, its map as host arrays and as an OccupancyGrid, map B, and the data2x twin."""

    def __init__(self, lsdmod, ctx):
        m, mp, lid, od = fr.load_log("data")
        self.lsdmod, self.ctx = lsdmod, ctx
        self.mp = tuple(float(v) for v in mp)
        self.lid, self.odom = np.array(lid[:40], np.float64), np.array(od[:41], np.float64)
        self.scans, self.lens = lsdmod.lidar_frames(self.lid)
        self.grid = np.where(m == 0, -1, np.where(m == 255, 0, 100)).astype(np.int8)
        self.mc = ctx.map_cache(m.copy(), self.mp[2], lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.mc_b, self.ml_b, self.mp_b = rb.grow_map(self.mc, self.ml, self.mp, D_COLS, D_ROWS, lsdmod.z_occ_max_dis)
        self.grid_b = rb.grow_grid(self.grid, D_COLS, D_ROWS)
        # data2x: the same pixels through a doubled resolution (tests/test_fleet_gpu.py: Fix)
        self.mp2 = self.mp[:2] + tuple(2.0 * v for v in self.mp[2:])
        self.lid2 = self.lid.copy()
        fin = np.isfinite(self.lid2[..., 0])
        self.lid2[..., 0] = np.where(fin, self.lid2[..., 0] * 2.0, self.lid2[..., 0])
        self.odom2 = self.odom.copy()
        self.odom2[:, :2] *= 2.0
        self.scans2, self.lens2 = lsdmod.lidar_frames(self.lid2)
        self.mc2 = ctx.map_cache(m.copy(), self.mp2[2], lsdmod.z_occ_max_dis)
        self._fs = {}

    def triple(self):
        return self.mc, self.ml, self.mp

    def grid_args(self, b=False):
        """set_map_device's arguments for the data map, or for B."""
        import torch
        g, p = (self.grid_b, self.mp_b) if b else (self.grid, self.mp)
        return torch.from_numpy(g).cuda(), g.shape[1], g.shape[0], p[2], p[3], p[4]

    def scanner(self, map_param, twin=False):
        """feature_scan(t) of tests/fa_rebase.py: replay, from the device's FeatureScan in the geometry of map_param."""
        scans, lens = (self.scans2, self.lens2) if twin else (self.scans, self.lens)

        def fs(t):
            key = (tuple(map_param), twin, t)
            if key not in self._fs:
                r = self.ctx.feature_scan_batch(scans[t:t + 1], lens[t:t + 1], map_param, pts_cap=8192)[0]
                self._fs[key] = (r["linesInfo"], r["scanImPoint"], r["lidarPos"])
            return self._fs[key]
        return fs

    def match(self, mc, ml, sl, pts, lp, last, pr):
        d = self.ctx.scan_to_map_match(mc, ml, sl, pts, lp, last, pr).reshape(-1)
        return np.stack([d["x"], d["y"], d["ang"], d["score"]], 1)


@pytest.fixture(scope="module")
def site(lsdmod, ctx):
    return Site(lsdmod, ctx)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
def hand_made_carries(lsdmod):
    """An ordinary tracked state, the sentinel, a NaN state, a frames == 0 carry, a tracked state whose key does not match -- and two
    more tracked ones, so that the launch has more than one workgroup and a last one that is half empty (seven sequences, two each)."""
    rng = np.random.default_rng(29)

    def tracked(seed_x):
        x = [float(v) for v in rng.normal(seed_x, 40, 9)]
        A = rng.normal(size=(9, 9))
        lp = ResumableLoop(0.025, x, (A @ A.T + 9 * np.eye(9)).tolist(), odom0=(0.5, -0.25, 0.125))
        lp.ang_sum, lp.ang_count, lp.frames, lp.is_offset = 12.5, 3.0, 3, True
        return lp.carry(lsdmod.FA_CARRY_DTYPE)
    rx, rP = fr.reset_state()
    reset = ResumableLoop(0.025, rx, rP, odom0=(1.0, 2.0, 3.0))
    reset.ang_sum, reset.ang_count, reset.frames = -7.0, 2.0, 2                 # a robot that has just lost its track
    nan = tracked(250)
    nan["state"]["x"][0] = np.nan
    nan["state"]["P"][4] = np.nan
    recs = [tracked(300), reset.carry(lsdmod.FA_CARRY_DTYPE), nan, lsdmod.Context.fa_carry_init(odom0=(0.0, 1.5, -2.25)), tracked(200), tracked(-50),
            tracked(1e4)]
    return np.array(recs, lsdmod.FA_CARRY_DTYPE), np.array([7, 7, 7, 7, 3, 7, 7], np.int32)


def same_carries(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for s in range(len(got)):
        assert np.array_equal(got[s]["state"]["x"], want[s]["state"]["x"], equal_nan=True), s
        assert np.array_equal(got[s]["state"]["P"], want[s]["state"]["P"], equal_nan=True), s
        for f in ("odom", "ang_sum", "ang_count", "frames", "is_offset"):
            assert got[s][f].tobytes() == want[s][f].tobytes(), (s, f)


@pytest.mark.parametrize("case", ["equal_resolutions", "data_to_data2x"])
def test_kernel_against_the_restatement(case, lsdmod, ctx, site):
    import torch
    recs, keys = hand_made_carries(lsdmod)
    frm = rb.frame_of(site.mp)
    to = rb.frame_of(site.mp_b) if case == "equal_resolutions" else rb.frame_of(site.mp2)
    assert (frm[0] / to[0] == 1.0) if case == "equal_resolutions" else (frm[0] / to[0] == 0.5)
    stream = torch.cuda.current_stream().cuda_stream
    for use_keys in (True, False):
        d = dev(recs.view(np.uint8).copy())
        d_key = dev(keys)
        ctx.enqueue_fa_carry_rebase_device(d.data_ptr(), len(recs), d_key.data_ptr() if use_keys else None, 7, frm, to, stream)
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(lsdmod.FA_CARRY_DTYPE)
        want = np.array([rb.rebase_carry(r, frm, to) if (keys[s] == 7 or not use_keys) else r for s, r in enumerate(recs)], lsdmod.FA_CARRY_DTYPE)
        same_carries(got, want)
        for s in (1, 3) + ((4,) if use_keys else ()):                          # the sentinel, frames == 0, the other key: every byte kept
            assert got[s].tobytes() == recs[s].tobytes(), s
        assert got[0].tobytes() != recs[0].tobytes() and np.isnan(got[2]["state"]["x"][0])
        if case == "equal_resolutions":                                        # s == 1: P and the rates keep their bits
            assert got[0]["state"]["P"].tobytes() == recs[0]["state"]["P"].tobytes()
            assert got[0]["state"]["x"][2:].tobytes() == recs[0]["state"]["x"][2:].tobytes()


def test_kernel_same_frame_writes_nothing_and_refusals(lsdmod, ctx, site):
    import torch
    recs, keys = hand_made_carries(lsdmod)
    d = dev(recs.view(np.uint8).copy())
    f = rb.frame_of(site.mp)
    L, E = ctx.L, lsdmod
    stream = torch.cuda.current_stream().cuda_stream
    fr_c, other = E.map_frame(f), E.map_frame(rb.frame_of(site.mp_b))
    assert L.lsd_enqueue_fa_carry_rebase_device(ctx.h, d.data_ptr(), len(recs), None, 0, fr_c, fr_c, stream) == E.LSD_OK
    mk = lambda r, x, y: E.lsd_map_frame(r, x, y)
    inf, nan = float("inf"), float("nan")
    for args in ((None, 7, fr_c, other), (d.data_ptr(), 0, fr_c, other), (d.data_ptr(), -1, fr_c, other), (d.data_ptr(), 7, mk(0.0, 0, 0), other),
                 (d.data_ptr(), 7, fr_c, mk(-0.025, 0, 0)), (d.data_ptr(), 7, mk(inf, 0, 0), other), (d.data_ptr(), 7, fr_c, mk(nan, 0, 0)),
                 (d.data_ptr(), 7, mk(0.025, inf, 0), other), (d.data_ptr(), 7, fr_c, mk(0.025, 0, nan))):
        assert L.lsd_enqueue_fa_carry_rebase_device(ctx.h, args[0], args[1], None, 0, args[2], args[3], stream) == E.LSD_ERR_INVALID, args[1:]
    torch.cuda.synchronize()
    assert d.cpu().numpy().tobytes() == recs.tobytes()                         # nothing ran


# ---- 2. Localizer: the opt-in re-base at the hand-over ---------------------------------------------------------------------------------------
STARTS = (0, 7, 20)                                                            # three robots on three stretches of the log


def run_localizer(site, loc, swap):
    """K ticks on A, swap(loc), K ticks on B; one frame per robot and tick.  Returns (states, reports) [S, 2K]."""
    S = len(STARTS)
    st, rp = [], []
    for j in range(2 * K):
        if j == K:
            swap(loc)
        lid = np.stack([site.lid[a + j:a + j + 1] for a in STARTS])
        od = np.stack([site.odom[a + j + 1:a + j + 2] for a in STARTS])
        s, r = loc.step(lid, od)
        st.append(s); rp.append(r)
    return np.concatenate(st, 1), np.concatenate(rp, 1)


def restated(site, rebase):
    """Per robot: the restated loop over the same frames, the first K on A, the rest on B -- with or without the restated re-base
    between them -- fed the device's own FeatureScan and candidates."""
    out = []
    for a in STARTS:
        loop = ResumableLoop(site.mp[2], odom0=site.odom[a])
        got = rb.replay(range(a, a + K), site.odom, loop, site.mc, site.ml, site.mp, site.scanner(site.mp), site.match)
        if rebase:
            rb.rebase_loop(loop, rb.frame_of(site.mp), rb.frame_of(site.mp_b))
        got += rb.replay(range(a + K, a + 2 * K), site.odom, loop, site.mc_b, site.ml_b, site.mp_b, site.scanner(site.mp_b), site.match)
        out.append((got, loop))
    return out


@pytest.mark.parametrize("rebase", [True, False], ids=["rebase", "default"])
def test_localizer_set_map_mid_log(rebase, lsdmod, ctx, site):
    od0 = np.stack([site.odom[a] for a in STARTS])
    loc = lsdmod.Localizer(site.mc, site.ml, site.mp, len(STARTS), odom0=od0, ctx=ctx)
    kw = dict(rebase=True) if rebase else {}                                   # the default is today's call, untouched
    st, rp = run_localizer(site, loc, lambda l: l.set_map(site.mc_b, site.ml_b, site.mp_b, **kw))
    want = restated(site, rebase)
    carries = loc.carries
    for s, (frames, loop) in enumerate(want):
        for j, (x, P, rep) in enumerate(frames):
            same_state(st[s, j], x, P)
            same_report(rp[s, j], rep)
        assert frames[K - 1][2]["branch"] == fr.UKF                            # tracking when the map changes
        if rebase:
            assert [f[2]["branch"] for f in frames[K:]] == [fr.UKF] * K        # and afterwards
        else:
            assert frames[K][2]["branch"] == fr.RESET and frames[K][2]["n_kept"] == 0   # today's behaviour: the track is lost
        assert carries[s].tobytes() == loop.carry(lsdmod.FA_CARRY_DTYPE).tobytes()
    assert loc.map_param == site.mp_b


def test_localizer_hand_overs_compose_and_reset_flushes(lsdmod, ctx, site):
    """A -> an intermediate frame -> B without a tick between them is one re-base A -> B; a robot reset while it is pending starts
    over at the sentinel, and a state given to reset is taken in the new map's frame."""
    od0 = np.stack([site.odom[a] for a in STARTS])
    mid = site.mp_b[:3] + (site.mp_b[3] + 0.4, site.mp_b[4] - 0.3)

    def swap(l):
        l.set_map(site.mc_b, site.ml_b, mid, rebase=True)
        l.set_map(site.mc_b, site.ml_b, site.mp_b, rebase=True)
    loc = lsdmod.Localizer(site.mc, site.ml, site.mp, len(STARTS), odom0=od0, ctx=ctx)
    st, rp = run_localizer(site, loc, swap)
    want = restated(site, True)
    for s, (frames, loop) in enumerate(want):
        for j, (x, P, rep) in enumerate(frames):
            same_state(st[s, j], x, P)
            same_report(rp[s, j], rep)
    # reset under a pending re-base
    loc = lsdmod.Localizer(site.mc, site.ml, site.mp, len(STARTS), odom0=od0, ctx=ctx)
    run = run_localizer(site, loc, lambda l: None)                             # 2K ticks on A
    before = loc.carries
    loc.set_map(site.mc_b, site.ml_b, site.mp_b, rebase=True)
    given = lsdmod.fa_state((np.arange(9.0) + 400.0, np.eye(9) * 3.0))
    loc.reset([0], odom0=site.odom[0])
    loc.reset([1], odom0=site.odom[3], state=given[0])
    after = loc.carries
    fa, fb = rb.frame_of(site.mp), rb.frame_of(site.mp_b)
    assert after[0].tobytes() == lsdmod.Context.fa_carry_init(odom0=site.odom[0]).tobytes()
    assert after[1].tobytes() == lsdmod.Context.fa_carry_init(given[0], site.odom[3]).tobytes()    # as given: not shifted
    assert after[2].tobytes() == rb.rebase_carry(before[2], fa, fb).tobytes() != before[2].tobytes()
    assert run[1][2, -1]["branch"] == fr.UKF


# ---- 3. FleetLocalizer: the per-map device hand-over ---------------------------------------------------------------------------------------
MAP_OF = (0, 1, 1, 0)
FSTARTS = (0, 7, 20, 12)


def tick_inputs(site, j):
    return (dev(np.stack([site.lid[a + j:a + j + 1] for a in FSTARTS])), dev(np.stack([site.odom[a + j + 1:a + j + 2] for a in FSTARTS])))


def test_fleet_set_map_device(lsdmod, ctx, site):
    import torch
    S = len(MAP_OF)
    od0 = np.stack([site.odom[a] for a in FSTARTS])
    cols_b, rows_b = site.grid_b.shape[1], site.grid_b.shape[0]
    # each robot alone: a Localizer on its map; those of map 1 do the same set_map_device
    solo_st, solo_rp, solo_count, solo_carry = [], [], None, []
    for s in range(S):
        loc = lsdmod.Localizer(*site.triple(), 1, odom0=od0[s], ctx=ctx)
        loc.reserve_map(cols_b, rows_b, lines_cap=LINES_CAP)
        st, rp = [], []
        for j in range(2 * K):
            if j == K and MAP_OF[s] == 1:
                assert loc.rebase_on_hand_over is False
                loc.rebase_on_hand_over = True                                 # (Localizer.set_map_device has no keyword for it)
                loc.set_map_device(*site.grid_args(b=True))
            a = FSTARTS[s]
            x, r = loc.step(site.lid[None, a + j:a + j + 1], site.odom[None, a + j + 1:a + j + 2])
            st.append(x[0]); rp.append(r[0])
        solo_st.append(np.concatenate(st)); solo_rp.append(np.concatenate(rp)); solo_carry.append(loc.carries[0])
        if MAP_OF[s] == 1:
            solo_count = int(loc.map_counts.cpu()[0])
    assert 0 < solo_count <= LINES_CAP
    for s in range(S):                                                         # the track survives the grown map; map 0 never changed
        assert (solo_rp[s]["branch"][K - 1:] == fr.UKF).all(), (s, solo_rp[s]["branch"])
    # the fleet: map 1 is replaced from the int8 grid on a side stream while the ticks run, nothing synchronises in between
    fl = lsdmod.FleetLocalizer([site.triple(), site.triple()], MAP_OF, odom0=od0, ctx=ctx)
    fl.reserve_map(1, cols_b, rows_b, lines_cap=LINES_CAP)
    side = torch.cuda.Stream()
    ins = [tick_inputs(site, j) for j in range(2 * K)]
    args = site.grid_args(b=True)
    o_st = torch.zeros((2 * K, S, STATE_B), dtype=torch.uint8, device="cuda")
    o_rp = torch.zeros((2 * K, S, REPORT_B), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    stats0 = None
    for j in range(2 * K):
        if j == 1:                                                             # (tick 0 was the warm one: the staging and the tables have their size)
            stats0 = torch.cuda.memory_stats()
        if j == K:
            fl.set_map_device(1, *args, stream=side, rebase=True)
        o = fl.step_device(*ins[j])
        o_st[j].copy_(o[0].view(S, STATE_B)); o_rp[j].copy_(o[1].view(S, REPORT_B))
    stats1 = torch.cuda.memory_stats()
    torch.cuda.synchronize()
    # after reserve_map neither the update nor the ticks allocate, as far as torch's allocator shows (the library's own workspace is
    # not its business: lsd_reserve_map_update and the warm tick size it)
    for key in ("allocation.all.allocated", "segment.all.allocated"):
        assert stats1[key] == stats0[key], (key, stats0[key], stats1[key])
    st = o_st.cpu().numpy().transpose(1, 0, 2)
    rp = o_rp.cpu().numpy().transpose(1, 0, 2)
    got_carry = fl.carries
    for s in range(S):
        assert np.ascontiguousarray(st[s]).tobytes() == solo_st[s].tobytes(), s
        assert np.ascontiguousarray(rp[s]).tobytes() == solo_rp[s].tobytes(), s
        assert got_carry[s].tobytes() == solo_carry[s].tobytes(), s
    counts = fl.map_counts
    assert len(counts) == 2 and all(c.is_cuda and c.dtype == torch.int32 and c.numel() == 1 for c in counts)
    assert int(counts[1].cpu()[0]) == solo_count and int(counts[0].cpu()[0]) == len(site.ml)
    # a host-made map takes the id back: the two kinds alternate on one id
    fl.set_map(1, *site.triple(), rebase=True)
    loc = lsdmod.Localizer(*site.triple(), 1, ctx=ctx)
    loc.carries = np.array([rb.rebase_carry(solo_carry[1], rb.frame_of(site.mp_b), rb.frame_of(site.mp))], lsdmod.FA_CARRY_DTYPE)
    a, j = FSTARTS[1], 2 * K
    lid, od = np.stack([site.lid[b + j:b + j + 1] for b in FSTARTS]), np.stack([site.odom[b + j + 1:b + j + 2] for b in FSTARTS])
    x, r = fl.step(lid, od)
    x1, r1 = loc.step(lid[1:2], od[1:2])
    assert x[1].tobytes() == x1[0].tobytes() and r[1].tobytes() == r1[0].tobytes() and r[1, 0]["branch"] == fr.UKF


def test_fleet_map_overflow_and_given_up(lsdmod, ctx, site, maps):
    """A device-made fleet map with more lines than its slots hold, then one whose count is -1: step() raises as Localizer.step does,
    names the map, fills `partial`, and the robots on the other map get what they get alone."""
    import torch
    m1 = maps["map1"]
    g1 = np.where(m1 == 0, -1, np.where(m1 == 255, 0, 100)).astype(np.int8)
    args = lambda: (torch.from_numpy(g1).cuda(), g1.shape[1], g1.shape[0], site.mp[2], site.mp[3], site.mp[4])
    S = len(MAP_OF)
    od0 = np.stack([site.odom[a] for a in FSTARTS])
    fl = lsdmod.FleetLocalizer([site.triple(), site.triple()], MAP_OF, odom0=od0, ctx=ctx)
    fl.reserve_map(1, g1.shape[1], g1.shape[0], lines_cap=4)
    solo = []
    for s in range(S):
        loc = lsdmod.Localizer(*site.triple(), 1, odom0=od0[s], ctx=ctx)
        if MAP_OF[s] == 1:
            loc.reserve_map(g1.shape[1], g1.shape[0], lines_cap=4)
        solo.append(loc)
    for step in ("overflow", "given_up"):
        if step == "overflow":
            fl.set_map_device(1, *args())
            for s in (1, 2):
                solo[s].set_map_device(*args())
            status = lsdmod.LSD_ERR_CAPACITY
        else:
            torch.cuda.synchronize()
            fl.map_counts[1].fill_(-1)                                         # what the detector writes for a map it gives up
            for s in (1, 2):
                solo[s].map_counts.fill_(-1)
            status = lsdmod.LSD_ERR_INTERNAL
        j = 0 if step == "overflow" else 1
        lid = np.stack([site.lid[a + j:a + j + 1] for a in FSTARTS])
        od = np.stack([site.odom[a + j + 1:a + j + 2] for a in FSTARTS])
        with pytest.raises(lsdmod.LsdError) as e:
            fl.step(lid, od)
        assert e.value.status == status and "map 1" in str(e.value) and e.value.partial is not None
        st, rp = e.value.partial
        assert st.shape == rp.shape == (S, 1)
        for s in range(S):
            if MAP_OF[s] == 1:
                with pytest.raises(lsdmod.LsdError) as e1:
                    solo[s].step(lid[s:s + 1], od[s:s + 1])
                assert e1.value.status == status
                st1, rp1 = e1.value.partial
            else:
                st1, rp1 = solo[s].step(lid[s:s + 1], od[s:s + 1])
            assert st[s].tobytes() == st1[0].tobytes() and rp[s].tobytes() == rp1[0].tobytes(), (step, s)
        if step == "overflow":
            assert int(fl.map_counts[1].cpu()[0]) == 7 > 4
        else:
            assert (rp[[1, 2], 0]["n_pairs"] == 0).all() and (rp[[1, 2], 0]["branch"] == fr.RESET).all()


def test_fleet_assign_and_rebase_between_resolutions(lsdmod, ctx, site):
    """Robots 0 and 1 on `data`, robot 2 on `data2x`; after K ticks robot 0 moves to data2x and its carry is re-based.  The moved robot
    is the restated loop's, bit for bit, and keeps FA_UKF; the others keep their bytes through the re-base."""
    maps = [site.triple(), (site.mc2, site.ml, site.mp2)]
    map_of = [0, 0, 1]
    starts = (0, 7, 20)
    od0 = np.stack([site.odom[starts[0]], site.odom[starts[1]], site.odom2[starts[2]]])
    fl = lsdmod.FleetLocalizer(maps, map_of, odom0=od0, ctx=ctx)

    def inputs(j, twin):
        lid = np.stack([(site.lid2 if twin[s] else site.lid)[a + j:a + j + 1] for s, a in enumerate(starts)])
        od = np.stack([(site.odom2 if twin[s] else site.odom)[a + j + 1:a + j + 2] for s, a in enumerate(starts)])
        return lid, od
    st, rp = [], []
    for j in range(K):
        s, r = fl.step(*inputs(j, (False, False, True)))
        st.append(s); rp.append(r)
    before = fl.carries
    fl.assign([0], [1])
    fl.rebase([0], 0, 1)
    after = fl.carries
    fa, f2 = rb.frame_of(site.mp), rb.frame_of(site.mp2)
    assert after[0].tobytes() == rb.rebase_carry(before[0], fa, f2).tobytes() != before[0].tobytes()
    assert after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    assert fl.map_of.tolist() == [1, 0, 1]
    for j in range(K, 2 * K):
        s, r = fl.step(*inputs(j, (True, False, True)))
        st.append(s); rp.append(r)
    st, rp = np.concatenate(st, 1), np.concatenate(rp, 1)
    a = starts[0]
    loop = ResumableLoop(site.mp[2], odom0=site.odom[a])
    want = rb.replay(range(a, a + K), site.odom, loop, site.mc, site.ml, site.mp, site.scanner(site.mp), site.match)
    rb.rebase_loop(loop, fa, f2)
    want += rb.replay(range(a + K, a + 2 * K), site.odom2, loop, site.mc2, site.ml, site.mp2, site.scanner(site.mp2, twin=True), site.match)
    print("moved robot: branches %s, pose before %s, after the re-base %s" % ([w[2]["branch"] for w in want], before[0]["state"]["x"][:2], after[0]["state"]["x"][:2]))
    for j, (x, P, rep) in enumerate(want):
        same_state(st[0, j], x, P)
        same_report(rp[0, j], rep)
    assert fl.carries[0].tobytes() == loop.carry(lsdmod.FA_CARRY_DTYPE).tobytes()
    assert rp[0, K]["branch"] == fr.UKF                                        # the next frame after the move: still tracking
    # the robots that did not move are what they are alone on their maps
    for s, (trip, lid, od) in ((1, (site.triple(), site.lid, site.odom)), (2, (maps[1], site.lid2, site.odom2))):
        loc = lsdmod.Localizer(*trip, 1, odom0=od[starts[s]], ctx=ctx)
        b = starts[s]
        for j in range(2 * K):
            x, r = loc.step(lid[None, b + j:b + j + 1], od[None, b + j + 1:b + j + 2])
            assert st[s, j].tobytes() == x[0, 0].tobytes() and rp[s, j].tobytes() == r[0, 0].tobytes(), (s, j)
