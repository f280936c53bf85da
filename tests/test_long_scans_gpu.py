"""Lidars beyond 1024 readings on the device: the scan capacity of a context (lsd_set_scan_capacity), k_rdp_long.hip against the
oracle's correctly rounded build over the campaign of tests/scan_cases_long.py -- bit for bit, as tests/test_feature_scan_gpu.py
holds k_rdp (its helpers and its NaN rule are used here) --, the ingest at the full capacity, and n_beams through Localizer and
FleetLocalizer.  tests/test_long_scans_cpu.py shows on the CPU what the campaign reaches."""
import numpy as np
import pytest

import scan_cases as sc
import scan_cases_long as scl
import scan_ingest as si
from test_feature_scan_gpu import GUARD, diffs, run_fs, run_fs_device
from test_scan_ingest_gpu import DataLog, dev, ingest_laserscan, ingest_pairs, read_back, same_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    c.set_scan_capacity(lsdmod.LSD_SCAN_MAX_LEN)
    yield c
    c.close()


@pytest.fixture(scope="module")
def campaign():
    return {g["name"]: g for g in scl.campaign()}


@pytest.fixture(scope="module")
def log(lsdmod, ctx):
    return DataLog(lsdmod, ctx)


# ---- 1. the capacity ---------------------------------------------------------------------------------------------------------------------
def test_scan_capacity_of_a_fresh_context(lsdmod, campaign):
    g = campaign["log_defaults"]
    c = lsdmod.Context(0)
    try:
        assert c.scan_capacity == 1024 and c.L.lsd_scan_capacity(None) == lsdmod.LSD_ERR_INVALID
        assert c.L.lsd_set_scan_capacity(c.h, 1023) == lsdmod.LSD_ERR_INVALID
        assert c.L.lsd_set_scan_capacity(c.h, 4097) == lsdmod.LSD_ERR_UNSUPPORTED
        assert c.L.lsd_set_scan_capacity(None, 2048) == lsdmod.LSD_ERR_INVALID
        assert c.scan_capacity == 1024
        s = next(s for s in g["scans"] if len(s) == 1025)

        def refused(stride):
            wide = np.zeros((1, stride, 2)); wide[0, :1025] = s
            st, out = run_fs(c, lsdmod, wide, [1025], g, pts_cap=64)
            assert st == lsdmod.LSD_ERR_UNSUPPORTED
            assert all((a.view(np.uint8) == 0xA5).all() for a in out.values())   # nothing ran
            import torch
            d_raw = dev(wide)
            d_sc = torch.full((stride * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            d_ln = torch.full((4 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            assert c.L.lsd_enqueue_scan_ingest_device(c.h, d_raw.data_ptr(), 1, stride, None, d_sc.data_ptr(), d_ln.data_ptr(), stride,
                                                      None) == lsdmod.LSD_ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert (d_sc.cpu().numpy() == 0xA5).all() and (d_ln.cpu().numpy() == 0xA5).all()

        refused(1025)                                                          # the default: as before
        c.set_scan_capacity(2048)
        assert c.scan_capacity == 2048
        refused(2049)
        st, _ = run_fs(c, lsdmod, np.ascontiguousarray(s[None]), [1025], g, pts_cap=scl.PTS_CAP_LONG)
        assert st in (lsdmod.LSD_OK, lsdmod.LSD_ERR_CAPACITY)
        c.set_scan_capacity(4096)
        assert c.scan_capacity == 4096
        refused(4097)
        c.set_scan_capacity(1024)                                              # back down: the wall is back
        refused(1025)
    finally:
        c.close()


# ---- 2. the campaign -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [g[0] for g in sc.GROUPS])
def test_long_campaign_group_equals_the_correctly_rounded_oracle(name, campaign, lsdmod, ctx, oracle):
    """Per stride of the group one launch through the device entry and one through the host entry; every field of every scan, with
    room for every pixel and again truncated at PTS_CAP_SMALL; guards behind every array (run_fs / run_fs_device assert them)."""
    g = campaign[name]
    refs = sc.reference(oracle, g, oracle.lib_cr())
    scl.check_bounds(refs)
    bad, nan_only, n = [], 0, 0
    for stride, idx in scl.by_stride(g).items():
        packed, lens = sc.pack([g["scans"][i] for i in idx], stride=stride)
        rs = [refs[i] for i in idx]
        want = lsdmod.LSD_ERR_CAPACITY if any(r["n_lines"] > 360 for r in rs) else lsdmod.LSD_OK
        for cap in (scl.PTS_CAP_LONG, sc.PTS_CAP_SMALL):
            st, host = run_fs(ctx, lsdmod, packed, lens, g, pts_cap=cap)
            assert st == want, (stride, cap, st)
            devo = run_fs_device(ctx, lsdmod, packed, lens, g, pts_cap=cap)
            for which, out in (("host", host), ("device", devo)):
                for j, (i, r) in enumerate(zip(idx, rs)):
                    n += 1
                    d = diffs(out, j, r, cap)
                    if d:
                        bad.append((which, cap, i, g["tags"][i], len(g["scans"][i]), d))
                    elif out["lines"][j, :len(r["lines"])].tobytes() != r["lines"].tobytes():
                        nan_only += 1
            for j, r in enumerate(rs):                                         # behind what a scan stores: untouched
                assert (devo["pts"][j, min(len(r["pts"]), cap):].view(np.uint8) == 0xA5).all(), (stride, j)
                assert (devo["lines"][j, min(r["n_lines"], 360):].view(np.uint8) == 0xA5).all(), (stride, j)
    print("%s: %d comparisons, %d differ, %d equal but for the sign / payload of a NaN" % (name, n, len(bad), nan_only))
    assert not bad, bad[:10]


# ---- 3. short scans: the long kernel against the short one ---------------------------------------------------------------------------------
def test_short_scans_on_the_long_kernel_equal_the_short_kernel(lsdmod, ctx):
    bytes_of = lambda o: b"".join(o[k].tobytes() for k in ("lines", "n_lines", "pts", "n_pts", "lidar_pos", "im_size"))
    most = 0
    for g in sc.campaign(reps=4):
        scans = g["scans"]                                                     # every length of scan_cases.LENGTHS, up to 1024
        assert len(scans) >= 40
        a, la = sc.pack(scans, stride=1024)
        b, lb = sc.pack(scans, stride=1025)
        old, new = run_fs_device(ctx, lsdmod, a, la, g), run_fs_device(ctx, lsdmod, b, lb, g)
        assert bytes_of(old) == bytes_of(new), g["name"]                       # the 0xA5 fill where nothing is stored included
        most = max(most, int(old["n_lines"].max()))
    assert most > 3


# ---- 4. the fleet's form ----------------------------------------------------------------------------------------------------------------------
def test_maps_entry_at_stride_1081(campaign, lsdmod, ctx):
    import torch
    ga, gb = campaign["log_defaults"], campaign["res05"]                       # two maps of different resolution and origin
    scans = [s for s in ga["scans"] if len(s) == 1081][:2] + [s for s in gb["scans"] if len(s) == 1081][:2]
    k, ids = 2, np.array([1, -1, 0], np.int32)                                 # robot 0 on map 1, robot 1 parked, robot 2 on map 0
    per_robot = [scans[2:4], scans[0:2], scans[0:2]]
    packed, lens = sc.pack([s for r in per_robot for s in r], stride=1081)
    n, cap = len(lens), sc.PTS_CAP
    dummy = torch.zeros(16, dtype=torch.float64, device="cuda")
    tab = [lsdmod.map_ref(dummy.data_ptr(), 4, 4, 0, 0, g["map_param"]) for g in (ga, gb)]
    size = dict(lines=n * 360 * 80, n_lines=n * 4, pts=n * cap * 24, n_pts=n * 4, lidar_pos=n * 16, im_size=n * 8)
    d = {key: torch.full((b + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for key, b in size.items()}
    d_sc, d_len, d_ids = dev(packed), dev(lens), dev(ids)
    ctx.enqueue_feature_scan_maps_device(d_sc.data_ptr(), d_len.data_ptr(), n, 1081, tab, d_ids.data_ptr(), k, d["lines"].data_ptr(),
                                         d["n_lines"].data_ptr(), d["pts"].data_ptr(), cap, d["n_pts"].data_ptr(), d["lidar_pos"].data_ptr(),
                                         d["im_size"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = {key: v.cpu().numpy() for key, v in d.items()}
    for key, raw in h.items():
        assert (raw[-GUARD:] == 0xA5).all(), key
    nl, npt = h["n_lines"][:n * 4].view(np.int32), h["n_pts"][:n * 4].view(np.int32)
    lines, pts = h["lines"][:size["lines"]].reshape(n, -1), h["pts"][:size["pts"]].reshape(n, -1)
    lp, sz = h["lidar_pos"][:n * 16].reshape(n, 16), h["im_size"][:n * 8].reshape(n, 8)
    assert nl.max() > 0 and npt.max() > 0
    for robot, g in ((0, gb), (2, ga)):                                        # each scan: as alone on its map
        for t in range(k):
            j = robot * k + t
            one = run_fs_device(ctx, lsdmod, np.ascontiguousarray(packed[j:j + 1]), lens[j:j + 1], dict(g, limit=3, thre_line=0.08, line_dist=0.5))
            assert nl[j] == one["n_lines"][0] and npt[j] == one["n_pts"][0]
            assert lines[j].tobytes() == one["lines"][0].tobytes() and pts[j].tobytes() == one["pts"][0].tobytes()
            assert lp[j].tobytes() == one["lidar_pos"][0].tobytes() and sz[j].tobytes() == one["im_size"][0].tobytes()
    for j in (2, 3):                                                           # the parked robot: counts 0 and nothing else
        assert nl[j] == 0 and npt[j] == 0
        assert (lines[j] == 0xA5).all() and (pts[j] == 0xA5).all() and (lp[j] == 0xA5).all() and (sz[j] == 0xA5).all()


# ---- 5. the ingest at the capacity --------------------------------------------------------------------------------------------------------------
def test_ingest_at_4096_beams(ctx):
    rng = np.random.default_rng(4096)
    n, B = 6, 4096
    raw = np.stack([rng.uniform(0.1, 30.0, (n, B)), rng.uniform(-np.pi, np.pi, (n, B))], -1)
    raw[1, :, 0] = np.inf
    raw[2, ::2, 0] = np.inf
    raw[3, [0, 63, 64, 4095], 0] = np.inf
    raw[4, rng.random(B) < 0.7, 0] = np.inf
    raw[5, 1::3, 0] = np.nan
    take = [1, 1, 1, 0, 1, 1]
    for tk in (None, take):
        same_bytes(ingest_pairs(ctx, raw, B, tk), si.ingest_pairs(raw, B, tk))
    ranges = raw[..., 0].astype(np.float32)
    ami = np.stack([rng.uniform(-3.2, -3.0, n), rng.uniform(0.0015, 0.0016, n)], -1).astype(np.float32)
    for tk in (None, take):
        same_bytes(ingest_laserscan(ctx, ranges, ami, B, tk), si.ingest_laserscan(ranges, ami, B, tk))


# ---- 6. n_beams is plumbing: padded frames give the 360-reading results ------------------------------------------------------------------------
FRAMES = 20


def _padded(lid):
    """[n, 360, 2] -> [n, 1080, 2]: two +inf readings behind every beam."""
    out = np.full((len(lid), 1080, 2), np.inf)
    out[:, ::3] = lid
    out[:, 1::3, 1] = out[:, 2::3, 1] = 0.0
    return out


def test_localizer_n_beams_1080_equals_the_default_on_the_data_log(lsdmod, ctx, log):
    lid, od = log.lid[:FRAMES], log.odom[1:FRAMES + 1]
    ranges = lid[..., 0].astype(np.float32)
    ami = np.tile(np.array([-3.12414, 0.0174533], np.float32), (1, FRAMES, 1))
    tail = np.full((FRAMES, 1080), np.inf, np.float32); tail[:, :360] = ranges
    mk = lambda **kw: lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx, **kw)
    base, wide, base_ls, wide_ls, wide_dev = mk(), mk(n_beams=1080), mk(), mk(n_beams=1080), mk(n_beams=1080)
    assert base.n_beams == 360 and base._IN_B == 5788 and wide._IN_B == 16 * 1080 + 28
    st0, rp0 = base.step(lid[None], od[None])
    st1, rp1 = wide.step(_padded(lid)[None], od[None])
    assert st0["x"][0, -1, 0] != -1 and st1.tobytes() == st0.tobytes() and rp1.tobytes() == rp0.tobytes()
    st2, rp2 = base_ls.step(None, od[None], ranges=ranges[None], angle_min_inc=ami)
    st3, rp3 = wide_ls.step(None, od[None], ranges=tail[None], angle_min_inc=ami)
    assert st3.tobytes() == st2.tobytes() and rp3.tobytes() == rp2.tobytes()
    st4, rp4, _ = read_back(lsdmod, wide_dev.step_device(dev(_padded(lid)[None]), dev(od[None])))
    assert st4.tobytes() == st0.tobytes() and rp4.tobytes() == rp0.tobytes()
    assert base.carries.tobytes() == wide.carries.tobytes() == wide_dev.carries.tobytes()
    assert base_ls.carries.tobytes() == wide_ls.carries.tobytes()
    for bad in (lid[None], _padded(lid)[None, :, :1079]):                      # the shape check follows n_beams
        with pytest.raises(lsdmod.LsdError):
            wide.step(bad, od[None])


def test_fleet_n_beams_1080_equals_the_default_on_the_data_log(lsdmod, ctx, log):
    starts = [0, 15]
    lid = np.stack([log.lid[s:s + FRAMES] for s in starts])
    od = np.stack([log.odom[s + 1:s + 1 + FRAMES] for s in starts])
    od0 = np.stack([log.odom[s] for s in starts]); od0[:, 0] = 0.0
    mk = lambda **kw: lsdmod.FleetLocalizer([(log.mc, log.ml, log.mp)], [0, 0], odom0=od0, ctx=ctx, **kw)
    base, wide = mk(), mk(n_beams=1080)
    st0, rp0 = base.step(lid, od)
    st1, rp1 = wide.step(np.stack([_padded(l) for l in lid]), od)
    assert st0["x"][1, -1, 0] != -1 and st1.tobytes() == st0.tobytes() and rp1.tobytes() == rp0.tobytes()
    assert base.carries.tobytes() == wide.carries.tobytes()


def test_n_beams_raises_the_capacity_of_the_context(lsdmod, log):
    c = lsdmod.Context(0)
    try:
        mk = lambda n: lsdmod.Localizer(log.mc, log.ml, log.mp, 1, ctx=c, n_beams=n)
        mk(1000)
        assert c.scan_capacity == 1024
        mk(1081)
        assert c.scan_capacity == 1081
        mk(360); mk(1025)
        assert c.scan_capacity == 1081                                         # never lowered
        for n, code in ((0, lsdmod.LSD_ERR_INVALID), (4097, lsdmod.LSD_ERR_UNSUPPORTED)):
            with pytest.raises(lsdmod.LsdError) as e:
                mk(n)
            assert e.value.status == code
    finally:
        c.close()


# ---- 7. dense scans: the tick is the three calls ---------------------------------------------------------------------------------------------
def test_dense_tick_equals_the_context_calls(lsdmod, ctx, log):
    import torch
    B, k = 2160, 4
    g = sc.GROUPS[0]
    assert g[1] == sc.LOG_MAP_PARAM
    lid = np.stack([sc.fam_room(np.random.default_rng((2160, t)), B, g, True, 0.0) for t in (0, 4, 8, 9)])   # (rooms with furniture: a bare room has no gap, so no cluster)
    lid[:, 5::97, 0] = np.inf                                                  # holes for the ingest
    od = np.cumsum(np.tile([0.01, 0.002, 0.001], (k, 1)), 0)
    od0 = (0.0, 0.0, 0.0)
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=od0, ctx=ctx, n_beams=B)
    d_lid, d_od = dev(lid), dev(od)
    st, rp, cn = read_back(lsdmod, loc.step_device(d_lid[None], d_od[None]))
    assert cn[0].min() > 3 and cn[0].max() <= 360 and cn[1].max() <= loc.pts_cap
    # by hand
    cap = loc.pts_cap
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_sc, d_ln, d_lines, d_pts = z(k * B * 16), z(k * 4), z(k * 360 * 80), z(k * cap * 24)
    d_nl, d_np, d_lp, d_sz = z(k * 4), z(k * 4), z(k * 16), z(k * 8)
    d_st, d_rp = z(k * lsdmod.FA_STATE_DTYPE.itemsize), z(k * lsdmod.FA_REPORT_DTYPE.itemsize)
    d_carry = dev(np.array([lsdmod.Context.fa_carry_init(None, od0)]).view(np.uint8))
    d_mc, d_ml = dev(np.ascontiguousarray(log.mc, np.float64)), dev(np.ascontiguousarray(log.ml).view(np.uint8))
    s = torch.cuda.current_stream().cuda_stream
    ctx.enqueue_scan_ingest_device(d_lid.data_ptr(), k, B, None, d_sc.data_ptr(), d_ln.data_ptr(), B, s)
    mp = log.mp
    ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), k, B,
                                                         lsdmod.lsd_map_param(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4])),
                                                         3, 0.08, 0.5, d_lines.data_ptr(), d_nl.data_ptr(), d_pts.data_ptr(), cap, d_np.data_ptr(),
                                                         d_lp.data_ptr(), d_sz.data_ptr(), s))
    rows, cols = log.mc.shape
    ctx.enqueue_localize_resume_device(d_mc.data_ptr(), cols, rows, d_ml.data_ptr(), len(log.ml), 1, k, [k], d_lines.data_ptr(), d_nl.data_ptr(),
                                       d_pts.data_ptr(), cap, d_np.data_ptr(), d_lp.data_ptr(), d_od.data_ptr(), float(mp[2]), d_carry.data_ptr(),
                                       d_st.data_ptr(), d_rp.data_ptr(), s)
    torch.cuda.synchronize()
    assert d_st.cpu().numpy().tobytes() == st.tobytes() and d_rp.cpu().numpy().tobytes() == rp.tobytes()
    assert np.array_equal(d_nl.cpu().numpy().view(np.int32), cn[0]) and np.array_equal(d_np.cpu().numpy().view(np.int32), cn[1])
    assert np.array_equal(d_ln.cpu().numpy().view(np.int32), (lid[..., 0] != np.inf).sum(1))
    assert d_carry.cpu().numpy().tobytes() == loc.carries.tobytes()
