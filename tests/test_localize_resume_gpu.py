"""The resumable replay loop (lsd_enqueue_localize_resume_device, Localizer) on the device: a sequence cut into calls anywhere -- frame by
frame, in random chunks, ragged across 16 robots in lock-step ticks, through a checkpoint -- gives the states and reports of one
lsd_localize call bit for bit, and its carry holds the restated loop's variables (tests/fa_restatement.py: Loop)."""
import numpy as np
import pytest

import fa_restatement as fr

pytestmark = pytest.mark.gpu
PTS_CAP = 8192
STATE_B, REPORT_B, CARRY_B, LINE_B = 720, 72, 768, 80


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def same_records(a, b):
    """Bitwise equality of structured records field by field (NaN equals NaN)."""
    assert a.dtype == b.dtype and a.shape == b.shape
    for name in a.dtype.names:
        x, y = a[name], b[name]
        if x.dtype.names:
            same_records(x, y)
        elif x.dtype.kind == "f":
            assert np.array_equal(x, y, equal_nan=True), name
        else:
            assert np.array_equal(x, y), name


class Log:
    """One log on the device: the map, FeatureScan of every frame (slot t = frame t), the Odom vector, and its one-call replay."""

    def __init__(self, lsdmod, ctx, name, odom=None):
        import torch
        m, mp, lid, od = fr.load_log(name)
        self.mp, self.lid = mp, lid
        self.odom = np.array(od if odom is None else odom, np.float64)
        self.scans, self.lens = lsdmod.lidar_frames(lid)
        self.n = len(self.scans)
        self.mc = ctx.map_cache(m.copy(), float(mp[2]), lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.states, self.reports = ctx.localize(self.mc, self.ml, self.scans, self.lens, self.odom, mp)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d_mc, self.d_ml, self.d_od = dev(self.mc), dev(np.ascontiguousarray(self.ml).view(np.uint8)), dev(self.odom)
        n = self.n
        z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")
        self.d_lines, self.d_nl, self.d_np = z(n * 360 * LINE_B, torch.uint8), z(n, torch.int32), z(n, torch.int32)
        self.d_pts, self.d_lp, self.d_sz = z(n * PTS_CAP * 3, torch.float64), z(n * 2, torch.float64), z(n * 2, torch.int32)
        d_sc, d_ln = dev(self.scans), dev(self.lens)
        mpar = lsdmod.lsd_map_param(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]))
        ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, 360, mpar, 3, 0.08, 0.5,
                                                             self.d_lines.data_ptr(), self.d_nl.data_ptr(), self.d_pts.data_ptr(), PTS_CAP,
                                                             self.d_np.data_ptr(), self.d_lp.data_ptr(), self.d_sz.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def resume(self, ctx, lsdmod, chunks):
        """Replays the log in calls of chunks[i] frames, the carry in place; returns (states, reports, carry after each call)."""
        import torch
        carry = torch.from_numpy(np.array([lsdmod.Context.fa_carry_init(odom0=self.odom[0])]).view(np.uint8).copy()).cuda()
        d_st = torch.zeros(self.n * STATE_B, dtype=torch.uint8, device="cuda")
        d_rp = torch.zeros(self.n * REPORT_B, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        t0, carries = 0, []
        for k in chunks:
            ctx.enqueue_localize_resume_device(self.d_mc.data_ptr(), self.mc.shape[1], self.mc.shape[0], self.d_ml.data_ptr(), len(self.ml), 1,
                                               k, [k], self.d_lines.data_ptr() + t0 * 360 * LINE_B, self.d_nl.data_ptr() + 4 * t0,
                                               self.d_pts.data_ptr() + t0 * PTS_CAP * 24, PTS_CAP, self.d_np.data_ptr() + 4 * t0,
                                               self.d_lp.data_ptr() + 16 * t0, self.d_od.data_ptr() + 24 * (t0 + 1), float(self.mp[2]),
                                               carry.data_ptr(), d_st.data_ptr() + STATE_B * t0, d_rp.data_ptr() + REPORT_B * t0, stream)
            carries.append(carry.clone())
            t0 += k
        assert t0 == self.n
        torch.cuda.synchronize()
        return (d_st.cpu().numpy().view(lsdmod.FA_STATE_DTYPE), d_rp.cpu().numpy().view(lsdmod.FA_REPORT_DTYPE),
                [c.cpu().numpy().view(lsdmod.FA_CARRY_DTYPE)[0] for c in carries])

    def loop_after(self, k):
        """The restated loop's variables after the first k frames, its states the device's one-call ones (checked against the
        restatement frame by frame in tests/test_localize_gpu.py::test_replay_log)."""
        loop = fr.Loop(self.odom, self.mp[2])
        for t in range(k):
            x = [float(v) for v in self.states[t]["x"]]
            loop.finish(t, x, self.states[t]["P"].reshape(9, 9, order="F").tolist())
        return loop


_logs = {}


def get_log(lsdmod, ctx, name):
    if name not in _logs:
        _logs[name] = Log(lsdmod, ctx, name)
    return _logs[name]


def check_carry(lsdmod, log, rec, k):
    """The carry after k frames against the restated Loop: x, P, the sum and length of angRotate, isOffset, Odom[k]."""
    loop = log.loop_after(k)
    assert np.array_equal(rec["state"]["x"], np.array(loop.x), equal_nan=True)
    assert np.array_equal(rec["state"]["P"].reshape(9, 9, order="F"), np.array(loop.P), equal_nan=True)
    s = 0.0
    for v in loop.ang_rotate:
        s += v
    assert np.array_equal(rec["ang_sum"], s, equal_nan=True) and rec["ang_count"] == len(loop.ang_rotate)
    assert rec["frames"] == k and rec["is_offset"] == int(loop.is_offset)
    assert (rec["odom"]["x"], rec["odom"]["y"], rec["odom"]["ang"]) == tuple(log.odom[k])
    assert rec["state"].tobytes() == log.states[k - 1].tobytes()


@pytest.mark.parametrize("name", fr.LOGS)
def test_frame_by_frame_equals_one_call(name, lsdmod, ctx):
    """n_frames = 1 per call: the fuse kernel reads the previous state from the carry it updates."""
    log = get_log(lsdmod, ctx, name)
    st, rp, carries = log.resume(ctx, lsdmod, [1] * log.n)
    same_records(st, log.states)
    same_records(rp, log.reports)
    for k in (1, 2, log.n // 2, log.n):
        check_carry(lsdmod, log, carries[k - 1], k)
    assert (log.reports["branch"] == fr.UKF).sum() > log.n // 2


@pytest.mark.parametrize("name", fr.LOGS)
def test_random_chunks_equal_one_call(name, lsdmod, ctx):
    log = get_log(lsdmod, ctx, name)
    first_ukf = int(np.argmax(log.reports["branch"] == fr.UKF))
    assert log.reports["branch"][first_ukf] == fr.UKF
    rng = np.random.default_rng(17 + len(name))
    for trial in range(3):
        cuts = {1, first_ukf + 1} | set(int(v) for v in rng.integers(1, log.n, size=int(rng.integers(2, 9))))
        cuts = sorted(c for c in cuts if 0 < c < log.n)
        chunks = np.diff([0] + cuts + [log.n]).tolist()
        st, rp, carries = log.resume(ctx, lsdmod, chunks)
        same_records(st, log.states)
        same_records(rp, log.reports)
        ends = np.cumsum(chunks)
        for i in (0, len(chunks) // 2, len(chunks) - 1):
            check_carry(lsdmod, log, carries[i], int(ends[i]))


def test_ragged_robots_in_lock_step(lsdmod, ctx):
    """16 robots on segments of the data/ log, 4 frame slots per tick, 0..4 frames each per tick: every robot's states and reports are
    its own one-call replay's, and a robot with no frame in a tick keeps its carry byte for byte and gets no slot written."""
    import torch
    log = get_log(lsdmod, ctx, "data")
    S, K = 16, 4
    rng = np.random.default_rng(5)
    starts = [(7 * s) % 50 for s in range(S)]
    lengths = [30 + (s % 5) * 4 for s in range(S)]
    segs = []
    for s in range(S):
        od = log.odom[starts[s]:starts[s] + lengths[s] + 1].copy()
        od[0, 0] = 0.0                                                     # the driver's Odom[0].x = 0
        segs.append(od)
    carry = torch.from_numpy(np.array([lsdmod.Context.fa_carry_init(odom0=segs[s][0]) for s in range(S)]).view(np.uint8).copy()).cuda()
    done = [0] * S
    got_st = [[] for _ in range(S)]
    got_rp = [[] for _ in range(S)]
    stream = torch.cuda.current_stream().cuda_stream
    mpar = lsdmod.lsd_map_param(*[int(v) for v in log.mp[:2]], *[float(v) for v in log.mp[2:]])
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")
    n = S * K
    d_lines, d_nl, d_np = z(n * 360 * LINE_B, torch.uint8), z(n, torch.int32), z(n, torch.int32)
    d_pts, d_lp, d_sz = z(n * PTS_CAP * 3, torch.float64), z(n * 2, torch.float64), z(n * 2, torch.int32)
    idle_seen = 0
    while any(done[s] < lengths[s] for s in range(S)):
        nf = np.array([min(int(rng.integers(0, K + 1)), lengths[s] - done[s]) for s in range(S)], np.int32)
        sc = np.zeros((S, K, 360, 2)); ln = np.zeros((S, K), np.int32); od = np.zeros((S, K, 3))
        for s in range(S):
            a = starts[s] + done[s]
            sc[s, :nf[s]] = log.scans[a:a + nf[s]]; ln[s, :nf[s]] = log.lens[a:a + nf[s]]
            od[s, :nf[s]] = segs[s][done[s] + 1:done[s] + 1 + nf[s]]
        d_sc, d_ln, d_od = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (sc, ln, od))
        d_st, d_rp = z(n * STATE_B, torch.uint8), z(n * REPORT_B, torch.uint8)
        ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, 360, mpar, 3, 0.08, 0.5,
                                                             d_lines.data_ptr(), d_nl.data_ptr(), d_pts.data_ptr(), PTS_CAP, d_np.data_ptr(),
                                                             d_lp.data_ptr(), d_sz.data_ptr(), stream))
        before = carry.cpu().numpy().reshape(S, CARRY_B).copy()
        ctx.enqueue_localize_resume_device(log.d_mc.data_ptr(), log.mc.shape[1], log.mc.shape[0], log.d_ml.data_ptr(), len(log.ml), S, K, nf,
                                           d_lines.data_ptr(), d_nl.data_ptr(), d_pts.data_ptr(), PTS_CAP, d_np.data_ptr(), d_lp.data_ptr(),
                                           d_od.data_ptr(), float(log.mp[2]), carry.data_ptr(), d_st.data_ptr(), d_rp.data_ptr(), stream)
        after = carry.cpu().numpy().reshape(S, CARRY_B)
        st = d_st.cpu().numpy().view(lsdmod.FA_STATE_DTYPE).reshape(S, K)
        rp = d_rp.cpu().numpy().reshape(S, K, REPORT_B)
        for s in range(S):
            if nf[s] == 0:
                idle_seen += 1
                assert after[s].tobytes() == before[s].tobytes(), s
            assert not rp[s, nf[s]:].any() and not st[s, nf[s]:].view(np.uint8).any()   # slots past a robot's frames: not written
            got_st[s].append(st[s, :nf[s]].copy())
            got_rp[s].append(rp[s, :nf[s]].copy().view(lsdmod.FA_REPORT_DTYPE).reshape(-1))
            done[s] += int(nf[s])
    assert idle_seen > 0
    final = carry.cpu().numpy().view(lsdmod.FA_CARRY_DTYPE)
    for s in range(S):
        a = starts[s]
        alone, arep = ctx.localize(log.mc, log.ml, log.scans[a:a + lengths[s]], log.lens[a:a + lengths[s]], segs[s], log.mp)
        same_records(np.concatenate(got_st[s]), alone)
        same_records(np.concatenate(got_rp[s]), arep)
        assert final[s]["state"].tobytes() == alone[-1].tobytes() and final[s]["frames"] == lengths[s]


def test_is_offset_across_a_call_boundary(lsdmod, ctx):
    """The first frame sets isOffset (|angDiff| > 90 at cnt_frame == 1); a frame with a negative angDiff in a later call must still get
    the + 360.  The odometry angle of Odom[1] is pushed to +-1e6 (atand -> -+90) where a log does not set the flag by itself; the first
    frame's pose does not depend on the odometry (lastPose = -1: ScanPose 0, the FIRST branch)."""
    found = None
    for name in fr.LOGS:
        base = get_log(lsdmod, ctx, name)
        for push in (False, True):
            od = base.odom.copy()
            if push:
                od[1, 2] = -1e6 if base.states[0]["x"][2] > 0 else 1e6
            log = base if push is None else Log(lsdmod, ctx, name, odom=od)
            loop = fr.Loop(log.odom, log.mp[2])
            raw = []
            for t in range(log.n):
                x = [float(v) for v in log.states[t]["x"]]
                raw.append(x[2] - fr.atand(log.odom[t + 1][2]))
                loop.finish(t, x, log.states[t]["P"].reshape(9, 9, order="F").tolist())
            neg = [t for t in range(2, log.n) if raw[t] < 0 and loop.is_offset]
            if loop.is_offset and abs(raw[0]) > 90 and neg:
                found = (log, neg[0])
                break
        if found:
            break
    assert found, "no log sets isOffset on its first frame and has a later negative angDiff"
    log, t_neg = found
    split = t_neg - 1                                                      # the negative frame lies in the second call (not its first frame)
    st, rp, carries = log.resume(ctx, lsdmod, [split, log.n - split])
    same_records(st, log.states)
    same_records(rp, log.reports)
    assert carries[0]["is_offset"] == 1
    check_carry(lsdmod, log, carries[0], split)
    check_carry(lsdmod, log, carries[1], log.n)


def test_localizer_staggered_robots_and_checkpoint(lsdmod, ctx):
    """Localizer.step for 6 robots that start on different ticks (one frame per tick), against each robot's one-call replay; a
    checkpoint of the carries restored into a new Localizer continues identically."""
    log = get_log(lsdmod, ctx, "data")
    S, T = 6, 40
    first_tick = [0, 0, 3, 5, 9, 14]
    starts = [0, 11, 20, 7, 33, 50]
    segs = []
    for s in range(S):
        n_s = T - first_tick[s]
        od = log.odom[starts[s]:starts[s] + n_s + 1].copy()
        od[0, 0] = 0.0
        segs.append(od)

    def run(loc, ticks, out):
        for tick in ticks:
            lid = np.zeros((S, 1, 360, 2)); od = np.zeros((S, 1, 3)); nf = np.zeros(S, np.int32)
            for s in range(S):
                t = tick - first_tick[s]
                if t >= 0:
                    lid[s, 0] = log.lid[starts[s] + t]; od[s, 0] = segs[s][t + 1]; nf[s] = 1
            st, rp = loc.step(lid, od, nf)
            assert st.shape == (S, 1) and rp.shape == (S, 1)
            for s in range(S):
                if nf[s]:
                    out[s][0].append(st[s, :1].copy()); out[s][1].append(rp[s, :1].copy())
                else:
                    assert not st[s].view(np.uint8).any() and not rp[s].view(np.uint8).any()

    odom0 = np.stack([segs[s][0] for s in range(S)])
    whole = [([], []) for _ in range(S)]
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, S, odom0=odom0, ctx=ctx)
    run(loc, range(T), whole)
    final = loc.carries
    part = [([], []) for _ in range(S)]
    loc1 = lsdmod.Localizer(log.mc, log.ml, log.mp, S, odom0=odom0, ctx=ctx)
    run(loc1, range(17), part)
    saved = loc1.carries
    assert saved.dtype == lsdmod.FA_CARRY_DTYPE and (saved["frames"] == [17 - f for f in first_tick]).all()
    loc2 = lsdmod.Localizer(log.mc, log.ml, log.mp, S, ctx=ctx)
    loc2.carries = saved
    run(loc2, range(17, T), part)
    assert loc2.carries.tobytes() == final.tobytes()
    for s in range(S):
        n_s = T - first_tick[s]
        alone, arep = ctx.localize(log.mc, log.ml, log.scans[starts[s]:starts[s] + n_s], log.lens[starts[s]:starts[s] + n_s], segs[s], log.mp)
        for got in (whole[s], part[s]):
            same_records(np.concatenate(got[0]), alone)
            same_records(np.concatenate(got[1]), arep)
        assert final[s]["frames"] == n_s and final[s]["state"].tobytes() == alone[-1].tobytes()
    loc2.reset([1], odom0=segs[1][0])
    c = loc2.carries
    assert c[1].tobytes() == lsdmod.Context.fa_carry_init(odom0=segs[1][0]).tobytes() and c[0].tobytes() == final[0].tobytes()


def test_argument_errors(lsdmod, ctx):
    import torch
    log = get_log(lsdmod, ctx, "data")
    carry = torch.from_numpy(np.array([lsdmod.Context.fa_carry_init(odom0=log.odom[0])] * 2).view(np.uint8).copy()).cuda()
    before = carry.cpu().numpy().tobytes()
    d_st, d_rp = torch.zeros(4 * STATE_B, dtype=torch.uint8, device="cuda"), torch.zeros(4 * REPORT_B, dtype=torch.uint8, device="cuda")
    L = ctx.L

    def call(n_seq=2, pitch=2, nf=(1, 2), d_carry="c", d_odom="o", resol=0.025):
        nfa = None if nf is None else np.ascontiguousarray(nf, np.int32)
        return L.lsd_enqueue_localize_resume_device(ctx.h, log.d_mc.data_ptr(), log.mc.shape[1], log.mc.shape[0], log.d_ml.data_ptr(),
                                                    len(log.ml), n_seq, pitch, None if nfa is None else nfa.ctypes.data,
                                                    log.d_lines.data_ptr(), log.d_nl.data_ptr(), log.d_pts.data_ptr(), PTS_CAP,
                                                    log.d_np.data_ptr(), log.d_lp.data_ptr(), log.d_od.data_ptr() if d_odom else None, resol,
                                                    carry.data_ptr() if d_carry else None, d_st.data_ptr(), d_rp.data_ptr(), None)
    assert call(d_carry=None) == lsdmod.LSD_ERR_INVALID
    assert call(nf=(1, 3)) == lsdmod.LSD_ERR_INVALID                       # n_frames[s] > frames_pitch
    assert call(nf=(-1, 1)) == lsdmod.LSD_ERR_INVALID
    assert call(nf=None) == lsdmod.LSD_ERR_INVALID
    assert call(n_seq=0) == lsdmod.LSD_ERR_INVALID
    assert call(pitch=0, nf=(0, 0)) == lsdmod.LSD_ERR_INVALID
    assert call(d_odom=None) == lsdmod.LSD_ERR_INVALID
    assert call(resol=0.0) == lsdmod.LSD_ERR_INVALID
    torch.cuda.synchronize()
    assert carry.cpu().numpy().tobytes() == before                         # nothing ran
    with pytest.raises(lsdmod.LsdError):
        lsdmod.Localizer(log.mc, log.ml, log.mp, 2, ctx=ctx).step(np.zeros((3, 1, 360, 2)), np.zeros((3, 1, 3)))
    with pytest.raises(lsdmod.LsdError):
        lsdmod.Localizer(log.mc, log.ml, log.mp, 2, ctx=ctx).step(np.zeros((2, 1, 360, 2)), np.zeros((2, 1, 3)), n_frames=[2, 0])


def test_localizer_from_occupancy_grid(lsdmod, ctx):
    """The constructor on an OccupancyGrid takes mapCallback's map (z_occ_max_dis = 2) and steps like a Localizer built on it."""
    log = get_log(lsdmod, ctx, "data")
    m, mp, _, _ = fr.load_log("data")
    grid = np.where(m == 0, -1, np.where(m == 255, 0, 100)).astype(np.int8)          # unknown / free / occupied cells
    _, mc, LSD = lsdmod.mapCallback(grid.reshape(-1), m.shape[1], m.shape[0], float(mp[2]), ctx=ctx)
    a = lsdmod.Localizer.from_occupancy_grid(grid.reshape(-1), m.shape[1], m.shape[0], float(mp[2]), float(mp[3]), float(mp[4]), 1,
                                             odom0=log.odom[0], ctx=ctx)
    b = lsdmod.Localizer(mc, LSD.linesInfo, mp, 1, odom0=log.odom[0], ctx=ctx)
    for t in range(3):
        ra, rb = a.step(log.lid[t][None, None], log.odom[t + 1][None, None]), b.step(log.lid[t][None, None], log.odom[t + 1][None, None])
        same_records(ra[0], rb[0]); same_records(ra[1], rb[1])
    assert a.carries.tobytes() == b.carries.tobytes() and a.carries["frames"][0] == 3
