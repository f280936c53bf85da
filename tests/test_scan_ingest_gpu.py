"""Scan ingestion on the device (k_ingest.hip: lsd_enqueue_scan_ingest_device, lsd_enqueue_laserscan_ingest_device) and the Localizer's
device tick (Localizer.step_device).  Every comparison is byte equality: the kernel moves values and does two single-precision
operations that numpy float32 reproduces exactly (tests/scan_ingest.py)."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import scan_ingest as si
from test_localize_resume_gpu import same_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_ingest(ctx, n, stride, take, enqueue):
    """One launch into buffers pre-filled with 0xFF (an unwritten byte shows); returns (scans float64 [n, stride, 2], lens int32 [n])."""
    import torch
    d_sc = torch.full((n * stride * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_ln = torch.full((n * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    d_tk = None if take is None else dev(np.asarray(take, np.int32))
    enqueue(None if d_tk is None else d_tk.data_ptr(), d_sc.data_ptr(), d_ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_sc.cpu().numpy().view(np.float64).reshape(n, stride, 2), d_ln.cpu().numpy().view(np.int32)


def ingest_pairs(ctx, raw, stride=None, take=None):
    raw = np.ascontiguousarray(raw, np.float64)
    n, n_beams = raw.shape[:2]
    stride = stride or n_beams
    d_raw = dev(raw)
    return run_ingest(ctx, n, stride, take,
                      lambda tk, sc, ln, st: ctx.enqueue_scan_ingest_device(d_raw.data_ptr(), n, n_beams, tk, sc, ln, stride, st))


def ingest_laserscan(ctx, ranges, ami, stride=None, take=None):
    ranges, ami = np.ascontiguousarray(ranges, np.float32), np.ascontiguousarray(ami, np.float32)
    n, n_beams = ranges.shape
    stride = stride or n_beams
    d_rg, d_ami = dev(ranges), dev(ami)
    return run_ingest(ctx, n, stride, take, lambda tk, sc, ln, st: ctx.enqueue_laserscan_ingest_device(d_rg.data_ptr(), d_ami.data_ptr(), n,
                                                                                                         n_beams, tk, sc, ln, stride, st))


def same_bytes(got, want):
    assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes()
    assert np.array_equal(got[1], want[1])


# ---- 1. the logs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["data", "f3key", "f4key"])
def test_pairs_on_every_log_frame(lsdmod, ctx, name):
    lid = fr.load_log(name)[2]
    same_bytes(ingest_pairs(ctx, lid), lsdmod.lidar_frames_batch(lid))


# ---- 2. hand-made scans ----------------------------------------------------------------------------------------------------------------
def handmade(n_beams, seed):
    """Scans of n_beams pairs: all finite, all +inf, +inf at beam 0 only, at the last beam only, -inf and NaN in place, random mixes."""
    rng = np.random.default_rng(seed)
    raw = np.empty((10, n_beams, 2))
    raw[..., 0] = rng.uniform(0.1, 12.0, (10, n_beams))
    raw[..., 1] = rng.uniform(-math.pi, math.pi, (10, n_beams))
    raw[1, :, 0] = np.inf
    raw[2, 0, 0] = np.inf
    raw[3, -1, 0] = np.inf
    raw[4, ::3, 0] = -np.inf
    raw[4, 1::3, 0] = np.nan
    raw[5, ::2, 0] = np.inf
    raw[5, 1::4, 0] = np.nan
    for s in range(6, 10):
        raw[s, rng.random(n_beams) < rng.uniform(0.05, 0.9), 0] = np.inf
    return raw


@pytest.mark.parametrize("n_beams", [1, 63, 64, 65, 359, 360, 1024])
def test_handmade_scans(ctx, n_beams):
    raw = handmade(n_beams, n_beams)
    strides = [n_beams] + ([min(1024, n_beams + 37)] if n_beams < 1024 else [])
    for stride in strides:
        for take in (None, [1, 0] * 5, [0, 1, 1, 1, 1, 1, 0, 0, 1, 0]):
            got = ingest_pairs(ctx, raw, stride, take)
            same_bytes(got, si.ingest_pairs(raw, stride, take))
            if take is None:
                assert got[1][0] == n_beams and got[1][1] == 0 and not got[0][1].view(np.uint8).any()
                assert got[1][4] == n_beams                                    # -inf and NaN are kept


# ---- 3. LaserScan ------------------------------------------------------------------------------------------------------------------------
def test_laserscan_random(ctx):
    rng = np.random.default_rng(7)
    n, n_beams = 64, 360
    ranges = rng.uniform(0.1, 12.0, (n, n_beams)).astype(np.float32)
    for s in range(n):
        ranges[s, rng.random(n_beams) < rng.uniform(0.0, 0.4)] = np.inf
    ami = np.stack([rng.uniform(-math.pi, 0.0, n), rng.uniform(0.005, 0.02, n)], 1).astype(np.float32)
    ami[0] = (-3.12414, 0.0174533)
    assert len({tuple(r) for r in ami.tolist()}) == n
    take = (rng.random(n) < 0.8).astype(np.int32)
    for stride, tk in ((360, None), (360, take), (401, take)):
        same_bytes(ingest_laserscan(ctx, ranges, ami, stride, tk), si.ingest_laserscan(ranges, ami, stride, tk))
    got = ingest_laserscan(ctx, ranges, ami)[0]
    widened = ami[0, 0].astype(np.float64) + np.arange(360) * ami[0, 1].astype(np.float64)
    keep = ranges[0] != np.inf
    assert (got[0, :keep.sum(), 1] != widened[keep]).any()                     # the angle is the single-precision one


def test_laserscan_on_the_data_log(lsdmod, ctx):
    lid = fr.load_log("data")[2]
    ranges = lid[..., 0].astype(np.float32)
    ami = np.tile(np.array([[-3.12414, 0.0174533]], np.float32), (len(lid), 1))
    got = ingest_laserscan(ctx, ranges, ami)
    same_bytes(got, si.ingest_laserscan(ranges, ami))
    assert np.array_equal(got[1], lsdmod.lidar_frames_batch(lid)[1])           # the kept set is the float64 log's


# ---- 4. / 5. the Localizer ------------------------------------------------------------------------------------------------------------------
class DataLog:
    def __init__(self, lsdmod, ctx):
        m, self.mp, self.lid, self.odom = fr.load_log("data")
        self.n = len(self.lid)
        self.mc = ctx.map_cache(m.copy(), float(self.mp[2]), lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo

    def localizer(self, lsdmod, ctx, S=1, odom0=None):
        return lsdmod.Localizer(self.mc, self.ml, self.mp, S, odom0=self.odom[0] if odom0 is None else odom0, ctx=ctx)


@pytest.fixture(scope="module")
def log(lsdmod, ctx):
    return DataLog(lsdmod, ctx)


def read_back(lsdmod, out):
    """step_device's tensors on the host, after the caller's own synchronisation."""
    import torch
    torch.cuda.synchronize()
    st, rp, cn = out
    assert st.is_cuda and rp.is_cuda and cn.is_cuda and cn.dtype == torch.int32
    S, k = st.shape[:2]
    assert cn.shape == (2, S * k)
    return (st.cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(S, k),
            rp.cpu().numpy().reshape(-1).view(lsdmod.FA_REPORT_DTYPE).reshape(S, k), cn.cpu().numpy())


def scan_counts(lsdmod, ctx, log, lid, taken):
    """FeatureScan's line and pixel counts of raw frames [n, 360, 2] through the host entry; slots not taken are empty scans."""
    scans, lens = lsdmod.lidar_frames_batch(lid)
    lens = np.where(taken, lens, 0).astype(np.int32)
    fs = ctx.feature_scan_batch(scans, lens, log.mp, pts_cap=8192)
    return np.array([[f["len_linesInfo"] for f in fs], [len(f["scanImPoint"]) for f in fs]], np.int32)


def test_step_device_frame_by_frame(lsdmod, ctx, log):
    host, devl = log.localizer(lsdmod, ctx), log.localizer(lsdmod, ctx)
    d_lid, d_od = dev(log.lid), dev(log.odom)
    want_counts = scan_counts(lsdmod, ctx, log, log.lid, np.ones(log.n, bool))
    states, reports = [], []
    for t in range(log.n):
        st_h, rp_h = host.step(log.lid[None, t:t + 1], log.odom[None, t + 1:t + 2])
        st_d, rp_d, cn = read_back(lsdmod, devl.step_device(d_lid[None, t:t + 1], d_od[None, t + 1:t + 2]))
        assert st_d.tobytes() == st_h.tobytes() and rp_d.tobytes() == rp_h.tobytes()
        assert np.array_equal(cn[:, 0], want_counts[:, t])
        states.append(st_d[0]); reports.append(rp_d[0])
    assert host.carries.tobytes() == devl.carries.tobytes()
    scans, lens = lsdmod.lidar_frames(log.lid)
    whole_st, whole_rp = ctx.localize(log.mc, log.ml, scans, lens, log.odom, log.mp)          # the one-call replay
    same_records(np.concatenate(states), whole_st)
    same_records(np.concatenate(reports), whole_rp)


def ragged_tick(log):
    S, k = 5, 3
    starts, nf = [0, 11, 20, 7, 33], np.array([3, 0, 2, 1, 0], np.int32)
    lid = np.stack([log.lid[s:s + k] for s in starts])
    od = np.stack([log.odom[s + 1:s + 1 + k] for s in starts])
    od0 = np.stack([log.odom[s] for s in starts]); od0[:, 0] = 0.0
    return S, k, starts, nf, lid, od, od0


def test_step_device_ragged_tick(lsdmod, ctx, log):
    S, k, starts, nf, lid, od, od0 = ragged_tick(log)
    host, devl = log.localizer(lsdmod, ctx, S, od0), log.localizer(lsdmod, ctx, S, od0)
    st_h, rp_h = host.step(lid, od, nf)
    st_d, rp_d, cn = read_back(lsdmod, devl.step_device(dev(lid), dev(od), nf))
    assert st_d.tobytes() == st_h.tobytes() and rp_d.tobytes() == rp_h.tobytes()
    taken = (np.arange(k)[None, :] < nf[:, None]).reshape(-1)
    assert np.array_equal(cn, scan_counts(lsdmod, ctx, log, lid.reshape(-1, 360, 2), taken))
    assert host.carries.tobytes() == devl.carries.tobytes()
    for s in range(S):                                                         # each robot: the one-call replay of its frames
        if nf[s] == 0:
            assert not st_d[s].view(np.uint8).any() and not rp_d[s].view(np.uint8).any()
            continue
        seg = np.concatenate([od0[s:s + 1], od[s, :nf[s]]])
        scans, lens = lsdmod.lidar_frames(lid[s, :nf[s]])
        alone_st, alone_rp = ctx.localize(log.mc, log.ml, scans, lens, seg, log.mp)
        same_records(st_d[s, :nf[s]], alone_st)
        same_records(rp_d[s, :nf[s]], alone_rp)
        assert not st_d[s, nf[s]:].view(np.uint8).any() and not rp_d[s, nf[s]:].view(np.uint8).any()


def test_laserscan_step_equals_pairs_step(lsdmod, ctx, log):
    """Localizer.step / step_device on LaserScan fields against step on the pairs the restatement builds from the same float32 message."""
    S, k, starts, nf, lid, od, od0 = ragged_tick(log)
    B = 353                                                                    # fewer beams than the staging's 360
    ranges = lid[:, :, :B, 0].astype(np.float32)
    rng = np.random.default_rng(3)
    ami = np.stack([rng.uniform(-3.2, -3.0, (S, k)), rng.uniform(0.0174, 0.0176, (S, k))], -1).astype(np.float32)
    pairs = np.full((S, k, 360, 2), np.inf)                                    # the beams a 353-beam message lacks: dropped like +inf ones
    for s in range(S):
        for t in range(k):
            for i in range(B):
                pairs[s, t, i] = (float(ranges[s, t, i]), si.laserscan_angle(ami[s, t, 0], ami[s, t, 1], i))
    a, b, c = (log.localizer(lsdmod, ctx, S, od0) for _ in range(3))
    st_p, rp_p = a.step(pairs, od, nf)
    st_l, rp_l = b.step(None, od, nf, ranges=ranges, angle_min_inc=ami)
    assert st_l.tobytes() == st_p.tobytes() and rp_l.tobytes() == rp_p.tobytes()
    st_d, rp_d, _ = read_back(lsdmod, c.step_device(None, dev(od), nf, ranges=dev(ranges), angle_min_inc=dev(ami)))
    assert st_d.tobytes() == st_p.tobytes() and rp_d.tobytes() == rp_p.tobytes()
    assert a.carries.tobytes() == b.carries.tobytes() == c.carries.tobytes()


# ---- 6. no hidden synchronisation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_step_device_does_not_synchronise(lsdmod, ctx, log, ragged):
    import torch
    S, k, starts, nf, lid, od, od0 = ragged_tick(log)
    nf = nf if ragged else None
    loc = log.localizer(lsdmod, ctx, S, od0)
    d_lid, d_od = dev(lid), dev(od)
    loc.step_device(d_lid, d_od, nf)                                           # warm: the staging and the workspace have their size
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
        pytest.skip("the stream drained before step_device was called (%d matmuls of %.3f ms): the host was too slow to tell" % (count, per * 1e3))
    out = loc.step_device(d_lid, d_od, nf)
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "step_device returned only after the work in front of it had finished: it synchronised"
    ref = log.localizer(lsdmod, ctx, S, od0)
    ref.step(lid, od, nf)
    st_h, rp_h = ref.step(lid, od, nf)                                         # the second tick on the same inputs, as loc's
    st_d, rp_d, _ = read_back(lsdmod, out)
    assert st_d.tobytes() == st_h.tobytes() and rp_d.tobytes() == rp_h.tobytes()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors(lsdmod, ctx, log):
    import torch
    L, INV, UNS = ctx.L, lsdmod.LSD_ERR_INVALID, lsdmod.LSD_ERR_UNSUPPORTED
    d_raw = torch.zeros(2 * 1100 * 2, dtype=torch.float64, device="cuda")
    d_rg, d_ami = torch.zeros(2 * 1100, dtype=torch.float32, device="cuda"), torch.zeros(4, dtype=torch.float32, device="cuda")
    d_sc = torch.full((2 * 1100 * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_ln = torch.full((8,), 0xFF, dtype=torch.uint8, device="cuda")

    def pairs(h=ctx.h, raw=d_raw.data_ptr(), n=2, beams=360, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), stride=360):
        return L.lsd_enqueue_scan_ingest_device(h, raw, n, beams, None, sc, ln, stride, None)

    def laser(h=ctx.h, rg=d_rg.data_ptr(), ami=d_ami.data_ptr(), n=2, beams=360, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), stride=360):
        return L.lsd_enqueue_laserscan_ingest_device(h, rg, ami, n, beams, None, sc, ln, stride, None)
    for call in (pairs, laser):
        assert call(h=None) == INV and call(n=0) == INV and call(n=-1) == INV and call(beams=0) == INV and call(stride=0) == INV
        assert call(sc=None) == INV and call(ln=None) == INV
        assert call(beams=361) == INV                                          # n_beams > stride
        assert call(beams=1025, stride=1025) == UNS and call(stride=1025) == UNS
        assert call(sc=d_sc.data_ptr() + 8) == INV                             # a pair moves as one 16-byte access
    assert pairs(raw=None) == INV and pairs(raw=d_raw.data_ptr() + 8) == INV
    assert laser(rg=None) == INV and laser(ami=None) == INV
    torch.cuda.synchronize()
    assert (d_sc.cpu().numpy() == 0xFF).all() and (d_ln.cpu().numpy() == 0xFF).all()      # nothing ran
    assert pairs(beams=1024, stride=1024) == lsdmod.LSD_OK and laser(beams=1024, stride=1024) == lsdmod.LSD_OK
    torch.cuda.synchronize()

    S, k, starts, nf, lid, od, od0 = ragged_tick(log)
    loc = log.localizer(lsdmod, ctx, S, od0)
    before = loc.carries.tobytes()
    d_lid, d_od = dev(lid), dev(od)
    d_rgs, d_amis = dev(lid[..., 0].astype(np.float32)), torch.zeros(S, k, 2, dtype=torch.float32, device="cuda")
    bad = [dict(lidar=lid, odom=d_od),                                         # a host array
           dict(lidar=torch.from_numpy(lid), odom=d_od),                       # a host tensor
           dict(lidar=d_lid, odom=torch.from_numpy(od)),
           dict(lidar=d_lid.float(), odom=d_od),                               # the wrong type
           dict(lidar=d_lid[:, :, :359], odom=d_od),                           # the wrong shape
           dict(lidar=d_lid[:4], odom=d_od[:4]),
           dict(lidar=d_lid, odom=d_od[:, :2]),
           dict(lidar=d_lid, odom=d_od, ranges=d_rgs, angle_min_inc=d_amis),   # both
           dict(odom=d_od),                                                    # neither
           dict(odom=d_od, ranges=d_rgs),                                      # no angle_min_inc
           dict(odom=d_od, ranges=d_rgs, angle_min_inc=d_amis[:, :1]),
           dict(odom=d_od, ranges=torch.zeros(S, k, 361, dtype=torch.float32, device="cuda"), angle_min_inc=d_amis),      # B > 360
           dict(lidar=d_lid, odom=d_od, n_frames=[4, 0, 0, 0, 0]),
           dict(lidar=d_lid, odom=d_od, n_frames=[1, -1, 0, 0, 0])]
    for kw in bad:
        with pytest.raises(lsdmod.LsdError) as e:
            loc.step_device(**kw)
        assert e.value.status == INV
    with pytest.raises(lsdmod.LsdError):
        loc.step(lid, od, ranges=lid[..., 0].astype(np.float32), angle_min_inc=np.zeros((S, k, 2), np.float32))
    with pytest.raises(lsdmod.LsdError):
        loc.step(None, od, ranges=np.zeros((S, k, 361), np.float32), angle_min_inc=np.zeros((S, k, 2), np.float32))
    assert loc.carries.tobytes() == before                                     # nothing ran
