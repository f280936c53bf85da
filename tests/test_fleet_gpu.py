"""A fleet on several maps in one tick (lsd_enqueue_feature_scan_maps_device, lsd_enqueue_localize_maps_device,
lsd_enqueue_localize_resume_maps_device, FleetLocalizer): every robot gets, byte for byte (NaN equal to NaN), what it gets alone on its
map through the single-map entries -- ctx.localize, lsd_enqueue_feature_scan_batch_device, lsd_enqueue_localize_resume_device,
Localizer -- which are the expectation everywhere; the code under test never is.

Fixtures: the first 12 frames of the three replay logs (three different maps, all at mapResol 0.025) and `data2x`: the data map with
mapResol, mapOriX, mapOriY, every finite range and every odometry x, y multiplied by 2 (exact in binary), so that the scan pixels land
where data's do while line_dist_thre_m / mapResol and the odometry division differ -- the per-map resolution is exercised."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr

pytestmark = pytest.mark.gpu
PTS_CAP = 8192
STATE_B, REPORT_B, CARRY_B, LINE_B = 720, 72, 768, 80
N = 12                                                                         # frames per fixture
NAMES = fr.LOGS + ("data2x",)


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def zeros(count, dt):
    import torch
    return torch.zeros(count, dtype=dt, device="cuda")


def filled(count, dt):
    """A device buffer whose every byte is 0xFF."""
    import torch
    return torch.full((count * torch.empty(0, dtype=dt).element_size(),), 0xFF, dtype=torch.uint8, device="cuda").view(dt)


def cur_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def map_param_c(lsdmod, mp):
    return lsdmod.lsd_map_param(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]))


class Fix:
    """One fixture: the map on the device, the single-map FeatureScan of its 12 frames (slot t = frame t, outputs pre-filled with
    0xFF) and its one-call single-map replay."""

    def __init__(self, lsdmod, ctx, name):
        import torch
        m, mp, lid, od = fr.load_log("data" if name == "data2x" else name)
        mp, lid, od = np.array(mp, np.float64), np.array(lid[:N], np.float64), np.array(od[:N + 1], np.float64)
        if name == "data2x":
            mp[2:5] *= 2.0
            fin = np.isfinite(lid[..., 0])
            lid[..., 0] = np.where(fin, lid[..., 0] * 2.0, lid[..., 0])
            od[:, :2] *= 2.0
        self.name, self.mp, self.lid, self.odom = name, mp, lid, od
        self.scans, self.lens = lsdmod.lidar_frames(lid)
        self.mc = ctx.map_cache(m.copy(), float(mp[2]), lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.states, self.reports = ctx.localize(self.mc, self.ml, self.scans, self.lens, self.odom, mp)
        self.d_mc, self.d_ml, self.d_od = dev(self.mc), dev(np.ascontiguousarray(self.ml).view(np.uint8)), dev(self.odom)
        self.d_sc, self.d_ln = dev(self.scans), dev(self.lens)
        self.fs = self.feature_scan(lsdmod, ctx, N)
        torch.cuda.synchronize()

    def feature_scan(self, lsdmod, ctx, n):
        """The single-map FeatureScan of the first n frames into 0xFF-filled outputs: (lines, n_lines, pts, n_pts, lidar_pos, size)."""
        import torch
        out = (filled(n * 360 * LINE_B, torch.uint8), filled(n, torch.int32), filled(n * PTS_CAP * 3, torch.float64), filled(n, torch.int32),
               filled(n * 2, torch.float64), filled(n * 2, torch.int32))
        ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, self.d_sc.data_ptr(), self.d_ln.data_ptr(), n, 360, map_param_c(lsdmod, self.mp),
                                                             3, 0.08, 0.5, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), PTS_CAP,
                                                             out[3].data_ptr(), out[4].data_ptr(), out[5].data_ptr(), cur_stream()))
        return out

    def ref(self, lsdmod, n_map=None, d_n_map=0, lines=None):
        """This map's record of a table."""
        return lsdmod.map_ref(self.d_mc.data_ptr(), self.mc.shape[1], self.mc.shape[0], (self.d_ml if lines is None else lines).data_ptr(),
                              len(self.ml) if n_map is None else n_map, self.mp, d_n_map)

    def triple(self):
        return self.mc, self.ml, self.mp

    def alone(self, ctx, frames):
        """The single-map replay of a robot that saw only `frames` of this fixture (in that order)."""
        frames = list(frames)
        od = self.odom[[0] + [t + 1 for t in frames]]
        return ctx.localize(self.mc, self.ml, self.scans[frames], self.lens[frames], od, self.mp)


@pytest.fixture(scope="module")
def fixes(lsdmod, ctx):
    f = {name: Fix(lsdmod, ctx, name) for name in NAMES}
    for name, x in f.items():                                                  # the expectation exercises the filter on every map
        ukf = (x.reports["branch"] == fr.UKF) & (x.reports["n_kept"] > 0)
        print("fixture %s: %d map lines, branches %s, n_kept %s" % (name, len(x.ml), x.reports["branch"].tolist(), x.reports["n_kept"].tolist()))
        assert ukf.any(), "the 12-frame replay of %s has no FA_UKF frame with n_kept > 0" % name
    return [f[name] for name in NAMES]                                         # map id = position in NAMES


class Slots:
    """FeatureScan results of S sequences x K frame slots, as the loops read them, filled from the fixtures' single-map FeatureScan."""

    def __init__(self, S, K):
        import torch
        self.S, self.K = S, K
        n = S * K
        self.lines, self.nl, self.np_ = zeros(n * 360 * LINE_B, torch.uint8), zeros(n, torch.int32), zeros(n, torch.int32)
        self.pts, self.lp = zeros(n * PTS_CAP * 3, torch.float64), zeros(n * 2, torch.float64)

    def put(self, s, j, fix, t):
        """Slot (s, j) = frame t of `fix`."""
        q = s * self.K + j
        li, nl, pt, npt, lp, _ = fix.fs
        self.lines[q * 360 * LINE_B:(q + 1) * 360 * LINE_B] = li[t * 360 * LINE_B:(t + 1) * 360 * LINE_B]
        self.pts[q * PTS_CAP * 3:(q + 1) * PTS_CAP * 3] = pt[t * PTS_CAP * 3:(t + 1) * PTS_CAP * 3]
        self.nl[q], self.np_[q] = nl[t], npt[t]
        self.lp[2 * q:2 * q + 2] = lp[2 * t:2 * t + 2]

    def args(self):
        return self.lines.data_ptr(), self.nl.data_ptr(), self.pts.data_ptr(), PTS_CAP, self.np_.data_ptr(), self.lp.data_ptr()


def init_carries(lsdmod, odoms):
    return dev(np.array([lsdmod.Context.fa_carry_init(odom0=o) for o in odoms]).view(np.uint8).copy())


# ---- 1. FeatureScan per scan -------------------------------------------------------------------------------------------------------------
def test_feature_scan_per_scan(lsdmod, ctx, fixes):
    import torch
    order, k = [2, 0, 3, 1, -1, len(fixes)], 3                               # sequences 4 and 5 sit out; their scans are fixture 0's
    S = len(order)
    n = S * k
    src = [fixes[m] if 0 <= m < len(fixes) else fixes[0] for m in order]
    d_sc = torch.cat([f.d_sc[:k].reshape(-1) for f in src])
    d_ln = torch.cat([f.d_ln[:k] for f in src])
    out = (filled(n * 360 * LINE_B, torch.uint8), filled(n, torch.int32), filled(n * PTS_CAP * 3, torch.float64), filled(n, torch.int32),
           filled(n * 2, torch.float64), filled(n * 2, torch.int32))
    ctx.enqueue_feature_scan_maps_device(d_sc.data_ptr(), d_ln.data_ptr(), n, 360, [f.ref(lsdmod) for f in fixes], dev(np.array(order, np.int32)).data_ptr(),
                                         k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), PTS_CAP, out[3].data_ptr(), out[4].data_ptr(),
                                         out[5].data_ptr(), stream=cur_stream())
    torch.cuda.synchronize()
    li, nl, pt, npt, lp, sz = (t.cpu().numpy() for t in out)
    li, pt = li.reshape(n, 360 * LINE_B), pt.view(np.uint8).reshape(n, PTS_CAP * 24)
    lp, sz = lp.view(np.uint8).reshape(n, 16), sz.view(np.uint8).reshape(n, 8)
    for s, m in enumerate(order):
        for j in range(k):
            q = s * k + j
            if not 0 <= m < len(fixes):                                        # counts 0, everything else keeps its fill
                assert nl[q] == 0 and npt[q] == 0
                assert (li[q] == 0xFF).all() and (pt[q] == 0xFF).all() and (lp[q] == 0xFF).all() and (sz[q] == 0xFF).all()
                continue
            e_li, e_nl, e_pt, e_np, e_lp, e_sz = (t.cpu().numpy() for t in fixes[m].fs)
            assert nl[q] == e_nl[j] and npt[q] == e_np[j] and 0 < nl[q] <= 360 and 0 < npt[q] <= PTS_CAP
            assert li[q].tobytes() == e_li.reshape(N, -1)[j].tobytes()        # the records, and the fill behind them
            assert pt[q].tobytes() == e_pt.view(np.uint8).reshape(N, -1)[j].tobytes()
            assert lp[q].tobytes() == e_lp.view(np.uint8).reshape(N, 16)[j].tobytes()
            assert sz[q].tobytes() == e_sz.view(np.uint8).reshape(N, 8)[j].tobytes()
    # data2x is told apart from data: the same pixels through another resolution (the line threshold in pixels differs)
    assert fixes[3].mp[2] == 2 * fixes[0].mp[2]


# ---- 2. one robot per map, one call ------------------------------------------------------------------------------------------------------
def one_call(lsdmod, ctx, table, map_of, fix_of, n_frames=None):
    """lsd_enqueue_localize_maps_device over the whole prefix of fix_of[s] for each sequence; outputs pre-filled with 0xFF.  Returns
    (states uint8 [S, N, 720], reports uint8 [S, N, 72])."""
    import torch
    S = len(map_of)
    sl = Slots(S, N)
    for s, f in enumerate(fix_of):
        for t in range(N):
            sl.put(s, t, f, t)
    d_od = torch.cat([f.d_od.reshape(-1) for f in fix_of])
    d_init = dev(np.array([lsdmod.Context.fa_initial_state()] * S).view(np.uint8).copy())
    d_st, d_rp = filled(S * N * STATE_B, torch.uint8), filled(S * N * REPORT_B, torch.uint8)
    ctx.enqueue_localize_maps_device(table, dev(np.array(map_of, np.int32)).data_ptr(), S, N, [N] * S if n_frames is None else n_frames,
                                     *sl.args(), d_od.data_ptr(), d_init.data_ptr(), d_st.data_ptr(), d_rp.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    return d_st.cpu().numpy().reshape(S, N, STATE_B), d_rp.cpu().numpy().reshape(S, N, REPORT_B)


def test_one_robot_per_map_in_one_call(lsdmod, ctx, fixes):
    map_of = [0, 1, 2, 3, -1, len(fixes)]
    st, rp = one_call(lsdmod, ctx, [f.ref(lsdmod) for f in fixes], map_of, fixes + [fixes[1], fixes[2]])
    for s, f in enumerate(fixes):
        same_records(st[s].reshape(-1).view(lsdmod.FA_STATE_DTYPE), f.states)
        same_records(rp[s].reshape(-1).view(lsdmod.FA_REPORT_DTYPE), f.reports)
    assert (st[4:] == 0xFF).all() and (rp[4:] == 0xFF).all()                   # the two that sit out: no slot written


# ---- 3. resumable, interleaved and ragged --------------------------------------------------------------------------------------------------
def run_ticks(lsdmod, ctx, fixes, map_of, delays, chunks):
    """The resume entry, tick after tick: robot s, on map map_of[s], takes chunks[g - delays[s]] frames in global tick g.  Returns the
    robots' states and reports (records, N each) and the final carries."""
    import torch
    S, K = len(map_of), max(chunks)
    table = [f.ref(lsdmod) for f in fixes]
    d_of = dev(np.array(map_of, np.int32))
    carry = init_carries(lsdmod, [fixes[m].odom[0] for m in map_of])
    done = [0] * S
    got_st, got_rp = [[] for _ in range(S)], [[] for _ in range(S)]
    for g in range(len(chunks) + max(delays)):
        nf = [chunks[g - d] if 0 <= g - d < len(chunks) else 0 for d in delays]
        sl = Slots(S, K)
        od = np.zeros((S, K, 3))
        for s in range(S):
            f = fixes[map_of[s]]
            for j in range(nf[s]):
                sl.put(s, j, f, done[s] + j)
            od[s, :nf[s]] = f.odom[done[s] + 1:done[s] + 1 + nf[s]]
        d_od = dev(od)
        d_st, d_rp = filled(S * K * STATE_B, torch.uint8), filled(S * K * REPORT_B, torch.uint8)
        ctx.enqueue_localize_resume_maps_device(table, d_of.data_ptr(), S, K, nf, *sl.args(), d_od.data_ptr(), carry.data_ptr(), d_st.data_ptr(),
                                                d_rp.data_ptr(), cur_stream())
        st, rp = d_st.cpu().numpy().reshape(S, K, STATE_B), d_rp.cpu().numpy().reshape(S, K, REPORT_B)
        for s in range(S):
            assert (st[s, nf[s]:] == 0xFF).all() and (rp[s, nf[s]:] == 0xFF).all()     # slots past a robot's frames: not written
            got_st[s].append(st[s, :nf[s]].copy().reshape(-1).view(lsdmod.FA_STATE_DTYPE))
            got_rp[s].append(rp[s, :nf[s]].copy().reshape(-1).view(lsdmod.FA_REPORT_DTYPE))
            done[s] += nf[s]
    assert done == [N] * S
    return [np.concatenate(v) for v in got_st], [np.concatenate(v) for v in got_rp], carry.cpu().numpy().reshape(S, CARRY_B)


def single_map_carry(lsdmod, ctx, f, chunks):
    """The carry the single-map resume entry leaves after the prefix of `f` in the same chunks."""
    import torch
    carry = init_carries(lsdmod, [f.odom[0]])
    d_st, d_rp = zeros(N * STATE_B, torch.uint8), zeros(N * REPORT_B, torch.uint8)
    li, nl, pt, npt, lp, _ = f.fs
    t0 = 0
    for k in chunks:
        ctx.enqueue_localize_resume_device(f.d_mc.data_ptr(), f.mc.shape[1], f.mc.shape[0], f.d_ml.data_ptr(), len(f.ml), 1, k, [k],
                                           li.data_ptr() + t0 * 360 * LINE_B, nl.data_ptr() + 4 * t0, pt.data_ptr() + t0 * PTS_CAP * 24, PTS_CAP,
                                           npt.data_ptr() + 4 * t0, lp.data_ptr() + 16 * t0, f.d_od.data_ptr() + 24 * (t0 + 1), float(f.mp[2]),
                                           carry.data_ptr(), d_st.data_ptr() + STATE_B * t0, d_rp.data_ptr() + REPORT_B * t0, cur_stream())
        t0 += k
    torch.cuda.synchronize()
    return (carry.cpu().numpy().reshape(CARRY_B), d_st.cpu().numpy().view(lsdmod.FA_STATE_DTYPE), d_rp.cpu().numpy().view(lsdmod.FA_REPORT_DTYPE))


@pytest.mark.parametrize("chunks", [[1] * N, [1, 1, 3, 7]], ids=["frame_by_frame", "chunks_1_1_3_7"])
def test_resumable_interleaved_and_ragged(chunks, lsdmod, ctx, fixes):
    map_of = [2, 0, 1, 0, 3, 2]
    delays = [0, 0, 0, 1, 0, 2]                                                # the second robot of map 0 one tick late, of map 2 two
    st, rp, carries = run_ticks(lsdmod, ctx, fixes, map_of, delays, chunks)
    for s, m in enumerate(map_of):
        same_records(st[s], fixes[m].states)
        same_records(rp[s], fixes[m].reports)
        want, _, _ = single_map_carry(lsdmod, ctx, fixes[m], chunks)
        assert carries[s].tobytes() == want.tobytes(), s


# ---- 4. sitting out ----------------------------------------------------------------------------------------------------------------------
def test_sitting_out(lsdmod, ctx, fixes):
    """Every robot is offered frame t in tick t; robot 4 (on f3key, next to robot 1) has id -1 in ticks 4-6."""
    import torch
    map_of = [0, 1, 2, 3, 1]
    fl = lsdmod.FleetLocalizer([f.triple() for f in fixes], map_of, odom0=np.stack([fixes[m].odom[0] for m in map_of]), ctx=ctx)
    S = len(map_of)
    got_st, got_rp = [[] for _ in range(S)], [[] for _ in range(S)]
    out_ticks = (4, 5, 6)
    before = None
    for t in range(N):
        if t == out_ticks[0]:
            fl.assign([4], -1)
            before = fl.carries
        if t == out_ticks[-1] + 1:
            assert fl.carries[4].tobytes() == before[4].tobytes()              # the carry kept its bytes through the three ticks
            assert fl.carries[1].tobytes() != before[1].tobytes()
            fl.assign([4], [1])
        lid = np.stack([fixes[m].lid[t:t + 1] for m in map_of])
        od = np.stack([fixes[m].odom[t + 1:t + 2] for m in map_of])
        st, rp, cn = fl.step_device(dev(lid), dev(od))
        torch.cuda.synchronize()
        st, rp, cn = st.cpu().numpy(), rp.cpu().numpy(), cn.cpu().numpy()
        for s in range(S):
            if s == 4 and t in out_ticks:
                assert not st[s].any() and not rp[s].any() and cn[0, s] == 0 and cn[1, s] == 0   # its slots: as the tick found them
                continue
            got_st[s].append(st[s].reshape(-1).view(lsdmod.FA_STATE_DTYPE))
            got_rp[s].append(rp[s].reshape(-1).view(lsdmod.FA_REPORT_DTYPE))
    assert fl.map_of.tolist() == map_of
    for s in range(4):                                                         # the others: unaffected
        same_records(np.concatenate(got_st[s]), fixes[s].states)
        same_records(np.concatenate(got_rp[s]), fixes[s].reports)
    want_st, want_rp = fixes[1].alone(ctx, [t for t in range(N) if t not in out_ticks])
    same_records(np.concatenate(got_st[4]), want_st)
    same_records(np.concatenate(got_rp[4]), want_rp)
    assert fl.carries[4]["frames"] == N - len(out_ticks) and fl.carries[4]["state"].tobytes() == want_st[-1].tobytes()


# ---- 5. re-assignment --------------------------------------------------------------------------------------------------------------------
def test_reassignment_without_synchronisation(lsdmod, ctx, fixes):
    import torch
    a, b = fixes[0], fixes[1]                                                  # data, then f3key
    fl = lsdmod.FleetLocalizer([a.triple(), b.triple()], [0], odom0=a.odom[0], ctx=ctx)
    d_la, d_oa, d_lb, d_ob = dev(a.lid[None, :4]), dev(a.odom[None, 1:5]), dev(b.lid[None, :4]), dev(b.odom[None, 1:5])
    torch.cuda.synchronize()
    outs = []
    for t in (0, 2):
        st, rp, _ = fl.step_device(d_la[:, t:t + 2], d_oa[:, t:t + 2])
        outs.append((st.clone(), rp.clone()))                                  # (the views are valid until the next tick)
    fl.assign([0], [1])
    fl.reset([0], b.odom[0])
    for t in (0, 2):
        st, rp, _ = fl.step_device(d_lb[:, t:t + 2], d_ob[:, t:t + 2])
        outs.append((st.clone(), rp.clone()))
    torch.cuda.synchronize()
    st = np.concatenate([o[0].cpu().numpy().reshape(-1) for o in outs]).view(lsdmod.FA_STATE_DTYPE)
    rp = np.concatenate([o[1].cpu().numpy().reshape(-1) for o in outs]).view(lsdmod.FA_REPORT_DTYPE)
    same_records(st[:4], a.states[:4])
    same_records(rp[:4], a.reports[:4])
    same_records(st[4:], b.states[:4])
    same_records(rp[4:], b.reports[:4])


# ---- 6. counts on the device ---------------------------------------------------------------------------------------------------------------
def test_counts_on_the_device(lsdmod, ctx, fixes):
    import torch
    a, b = fixes[0], fixes[1]
    n = len(a.ml)
    assert 16 < n <= 512
    lines512 = zeros(512 * LINE_B, torch.uint8)
    lines512[:n * LINE_B] = a.d_ml.reshape(-1)
    d_cnt = dev(np.array([n, 0, -1], np.int32))
    empty = np.zeros(0, lsdmod.LINE_DTYPE)
    cases = [(512, 0, a.ml), (16, 0, a.ml[:16]), (512, 1, empty), (512, 2, empty)]   # (capacity, which count, the old entry's map lines)
    for cap, which, ml in cases:
        table = [a.ref(lsdmod, n_map=cap, d_n_map=d_cnt.data_ptr() + 4 * which, lines=lines512), b.ref(lsdmod)]
        st, rp = one_call(lsdmod, ctx, table, [0, 1], [a, b])
        want_st, want_rp = ctx.localize(a.mc, ml, a.scans, a.lens, a.odom, a.mp)
        same_records(st[0].reshape(-1).view(lsdmod.FA_STATE_DTYPE), want_st)
        same_records(rp[0].reshape(-1).view(lsdmod.FA_REPORT_DTYPE), want_rp)
        if not len(ml):
            assert (want_rp["n_pairs"] == 0).all() and (want_rp["branch"] == fr.RESET).all()
        same_records(st[1].reshape(-1).view(lsdmod.FA_STATE_DTYPE), b.states)   # the map whose count is the host's: unaffected
        same_records(rp[1].reshape(-1).view(lsdmod.FA_REPORT_DTYPE), b.reports)


# ---- 7. n_maps = 1 -----------------------------------------------------------------------------------------------------------------------
def test_one_map_equals_the_resume_entry(lsdmod, ctx, fixes):
    chunks = [5, 7]
    want_carry, want_st, want_rp = single_map_carry(lsdmod, ctx, fixes[0], chunks)
    st, rp, carries = run_ticks(lsdmod, ctx, fixes[:1], [0], [0], chunks)
    assert st[0].tobytes() == want_st.tobytes() and rp[0].tobytes() == want_rp.tobytes() and carries[0].tobytes() == want_carry.tobytes()
    same_records(want_st, fixes[0].states)


# ---- 8. FleetLocalizer.step ----------------------------------------------------------------------------------------------------------------
def test_fleet_step_equals_localizer_step_per_map(lsdmod, ctx, fixes):
    map_of, k = [3, 1, 0, 2], 3
    od0 = np.stack([fixes[m].odom[0] for m in map_of])
    ami = np.tile(np.array([-3.12414, 0.0174533], np.float32), (len(map_of), k, 1))
    for laser in (False, True):
        fl = lsdmod.FleetLocalizer([f.triple() for f in fixes], map_of, odom0=od0, ctx=ctx)
        solo = [lsdmod.Localizer(*fixes[m].triple(), 1, odom0=fixes[m].odom[0], ctx=ctx) for m in map_of]
        for t in (0, 3):
            lid = np.stack([fixes[m].lid[t:t + k] for m in map_of])
            od = np.stack([fixes[m].odom[t + 1:t + 1 + k] for m in map_of])
            nf = np.array([3, 2, 3, 1], np.int32) if t else None
            kw = dict(ranges=lid[..., 0].astype(np.float32), angle_min_inc=ami) if laser else {}
            st, rp = fl.step(None if laser else lid, od, nf, **kw)
            assert st.shape == rp.shape == (len(map_of), k)
            for s, loc in enumerate(solo):
                kw1 = {key: v[s:s + 1] for key, v in kw.items()}
                st1, rp1 = loc.step(None if laser else lid[s:s + 1], od[s:s + 1], None if nf is None else nf[s:s + 1], **kw1)
                assert st[s].tobytes() == st1[0].tobytes() and rp[s].tobytes() == rp1[0].tobytes(), (laser, t, s)
        got = fl.carries
        for s, loc in enumerate(solo):
            assert got[s].tobytes() == loc.carries[0].tobytes()


def test_fleet_step_capacity_error(lsdmod, ctx, fixes):
    """More pixels than pts_cap: LSD_ERR_CAPACITY with the records computed from the stored part in `partial`, as Localizer.step."""
    f = fixes[1]
    fl = lsdmod.FleetLocalizer([fixes[0].triple(), f.triple()], [1], odom0=f.odom[0], ctx=ctx, pts_cap=64)
    loc = lsdmod.Localizer(*f.triple(), 1, odom0=f.odom[0], ctx=ctx, pts_cap=64)
    with pytest.raises(lsdmod.LsdError) as e:
        fl.step(f.lid[None, :2], f.odom[None, 1:3])
    with pytest.raises(lsdmod.LsdError) as e1:
        loc.step(f.lid[None, :2], f.odom[None, 1:3])
    assert e.value.status == e1.value.status == lsdmod.LSD_ERR_CAPACITY
    assert e.value.partial[0].tobytes() == e1.value.partial[0].tobytes() and e.value.partial[1].tobytes() == e1.value.partial[1].tobytes()


# ---- 9. no host wait ---------------------------------------------------------------------------------------------------------------------
def test_assign_and_step_device_do_not_synchronise(lsdmod, ctx, fixes):
    import torch
    map_of = [0, 1, 2, 3]
    od0 = np.stack([fixes[m].odom[0] for m in map_of])
    fl = lsdmod.FleetLocalizer([f.triple() for f in fixes], map_of, odom0=od0, ctx=ctx)
    d_lid = dev(np.stack([fixes[m].lid[:2] for m in map_of]))
    d_od = dev(np.stack([fixes[m].odom[1:3] for m in map_of]))
    fl.assign([3], [3])
    fl.step_device(d_lid[:, :1], d_od[:, :1])                                  # warm: the staging, the workspace and the table have their size
    a = torch.randn(4096, 4096, device="cuda")

    def burn(count):
        for _ in range(count):
            a @ a
    burn(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    burn(10)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 10                                      # the trial run: seconds per matmul
    count = max(10, min(5000, int(math.ceil(0.08 / per))))                     # ~80 ms of work in front of the tick
    done = torch.cuda.Event()
    burn(count)
    done.record()
    if done.query():
        pytest.skip("the stream drained before assign was called (%d matmuls of %.3f ms): the host was too slow to tell" % (count, per * 1e3))
    fl.assign([2], -1)
    out = fl.step_device(d_lid[:, 1:2], d_od[:, 1:2])
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "assign + step_device returned only after the work in front of them had finished: they synchronised"
    st = out[0].cpu().numpy()
    rp = out[1].cpu().numpy()
    for s in (0, 1, 3):
        assert st[s, 0].tobytes() == fixes[s].states[1].tobytes() and rp[s, 0].tobytes() == fixes[s].reports[1].tobytes()
    assert not st[2].any() and not rp[2].any()


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(lsdmod, ctx, fixes):
    import torch
    L, E = ctx.L, lsdmod
    a, b = fixes[0], fixes[1]
    good = lsdmod.map_table([a.ref(lsdmod), b.ref(lsdmod)])

    def broken(**kw):
        t = good.copy()
        for key, v in kw.items():
            t[1][key] = v
        return t
    big = lsdmod.map_table([a.ref(lsdmod)] * (lsdmod.LSD_MAX_MAPS + 1))
    d_of = dev(np.array([0, 1], np.int32))
    # (table, n_maps, d_map_of, status); None for the table: a null pointer
    cases = [(good, 0, d_of, E.LSD_ERR_INVALID), (good, -1, d_of, E.LSD_ERR_INVALID), (None, 2, d_of, E.LSD_ERR_INVALID),
             (good, 2, None, E.LSD_ERR_INVALID), (big, len(big), d_of, E.LSD_ERR_UNSUPPORTED),
             (broken(cols=0), 2, d_of, E.LSD_ERR_INVALID), (broken(rows=-3), 2, d_of, E.LSD_ERR_INVALID),
             (broken(n_map=-1), 2, d_of, E.LSD_ERR_INVALID), (broken(d_map_cache=0), 2, d_of, E.LSD_ERR_INVALID),
             (broken(d_map_lines=0), 2, d_of, E.LSD_ERR_INVALID), (broken(mapResol=0.0), 2, d_of, E.LSD_ERR_INVALID),
             (broken(mapResol=-0.025), 2, d_of, E.LSD_ERR_INVALID), (broken(mapResol=float("nan")), 2, d_of, E.LSD_ERR_INVALID),
             (broken(n_map=(1 << 26) // 360 + 1), 2, d_of, E.LSD_ERR_UNSUPPORTED)]
    S, K = 2, 2
    sl = Slots(S, K)
    for s, f in enumerate((a, b)):
        for j in range(K):
            sl.put(s, j, f, j)
    d_od = dev(np.stack([a.odom[:K + 1], b.odom[:K + 1]]))
    d_init = dev(np.array([lsdmod.Context.fa_initial_state()] * S).view(np.uint8).copy())
    carry0 = init_carries(lsdmod, [a.odom[0], b.odom[0]])
    carry = carry0.clone()
    n = S * K
    d_sc = torch.cat([a.d_sc[:K].reshape(-1), b.d_sc[:K].reshape(-1)])
    d_ln = torch.cat([a.d_ln[:K], b.d_ln[:K]])
    outs = [filled(n * STATE_B, torch.uint8), filled(n * REPORT_B, torch.uint8), filled(n * 360 * LINE_B, torch.uint8), filled(n, torch.int32),
            filled(n * PTS_CAP * 3, torch.float64), filled(n, torch.int32), filled(n * 2, torch.float64), filled(n * 2, torch.int32)]
    d_st, d_rp, o_li, o_nl, o_pt, o_np, o_lp, o_sz = outs
    p = lambda t: None if t is None else t.data_ptr()
    stream = cur_stream()

    def feature_scan(tab, n_maps, of, per_seq=K):
        return L.lsd_enqueue_feature_scan_maps_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, 360, None if tab is None else tab.ctypes.data, n_maps,
                                                      p(of), per_seq, 3, 0.08, 0.5, o_li.data_ptr(), o_nl.data_ptr(), o_pt.data_ptr(), PTS_CAP,
                                                      o_np.data_ptr(), o_lp.data_ptr(), o_sz.data_ptr(), stream)

    def loops(tab, n_maps, of):
        nf = np.array([K] * S, np.int32)
        t = None if tab is None else tab.ctypes.data
        tail = (S, K, nf.ctypes.data, *sl.args(), d_od.data_ptr())
        return (L.lsd_enqueue_localize_maps_device(ctx.h, t, n_maps, p(of), *tail, d_init.data_ptr(), d_st.data_ptr(), d_rp.data_ptr(), stream),
                L.lsd_enqueue_localize_resume_maps_device(ctx.h, t, n_maps, p(of), *tail, carry.data_ptr(), d_st.data_ptr(), d_rp.data_ptr(), stream))
    for tab, n_maps, of, status in cases:
        pair_limit = tab is not None and tab is not big and tab[1]["n_map"] > 1 << 17
        if not pair_limit:                                                     # (the pair limit is the loops': FeatureScan reads no map line)
            assert feature_scan(tab, n_maps, of) == status, (n_maps, status)
        assert loops(tab, n_maps, of) == (status, status), (n_maps, status)
    assert feature_scan(good, 2, d_of, per_seq=0) == E.LSD_ERR_INVALID and feature_scan(good, 2, d_of, per_seq=-1) == E.LSD_ERR_INVALID
    torch.cuda.synchronize()
    for o in outs:
        assert (o.view(torch.uint8) == 0xFF).all()
    assert carry.cpu().numpy().tobytes() == carry0.cpu().numpy().tobytes()
    # and the same arguments with the table as it should be are taken
    nf = np.array([K] * S, np.int32)
    assert feature_scan(good, 2, d_of) == E.LSD_OK
    assert L.lsd_enqueue_localize_maps_device(ctx.h, good.ctypes.data, 2, d_of.data_ptr(), S, K, nf.ctypes.data, *sl.args(), d_od.data_ptr(),
                                              d_init.data_ptr(), d_st.data_ptr(), d_rp.data_ptr(), stream) == E.LSD_OK
    torch.cuda.synchronize()
    same_records(d_st.cpu().numpy().view(lsdmod.FA_STATE_DTYPE).reshape(S, K)[1], b.states[:K])
