"""Global scan-to-grid localisation on the device (csrc/k_gridlocate.hip: lsd_enqueue_grid_pyramid_device, lsd_enqueue_grid_locate_device,
lsd_grid_locate; GridMapper.pyramid_device / locate_device / locate; Localizer.locate_last_tick) against the restatement of
tests/grid_locate_cases.py and against the device's own exhaustive search (levels = 0).  The rule is exact and has no iteration order, so
every comparison is byte equality -- the records' 64 bytes and the statistics' 48."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
import grid_cases as gc
import grid_locate_cases as lc
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
def cases(oracle):
    """(case, records, stats) of the campaign at each case's own levels: the restatement, computed once."""
    return [(c, rec, st) for c, (rec, st, _) in zip(lc.campaign(), lc.expected())]


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


def par_of(lsdmod, p):
    return lsdmod.lsd_grid_locate_par(*[p[k] for k in lc.PAR_KEYS])


def device_pyramid(lsdmod, cx, corr, levels):
    """(the buffer the device makes of corr, its guard untouched)."""
    import torch
    rows, cols = corr.shape
    n = lsdmod.grid_pyramid_bytes(cols, rows, levels)
    d = filled(n)
    assert cx.L.lsd_enqueue_grid_pyramid_device(cx.h, dev(corr).data_ptr(), cols, rows, levels, d.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    return back(d, n)


def device_locate(lsdmod, cx, case, d_out, d_stats, levels=None):
    import torch
    p = case["par"] if levels is None else dict(case["par"], levels=levels)
    d_sc, d_ln, d_py = dev(case["scans"]), dev(case["lens"]), dev(lc.pyramid(case["corr"], p["levels"]))
    st = cx.L.lsd_enqueue_grid_locate_device(cx.h, d_sc.data_ptr(), d_ln.data_ptr(), len(case["lens"]), case["scans"].shape[1],
                                             lsdmod.lsd_map_param(*mp_of(case)), case["range_max"], d_py.data_ptr(), par_of(lsdmod, p),
                                             d_out.data_ptr(), d_stats.data_ptr() if d_stats is not None else None, stream())
    torch.cuda.synchronize()
    return st


def but_lower_bound(raw):
    a = np.frombuffer(raw, np.uint8).reshape(-1, 64).copy()
    a[:, lc.LOWER_BOUND_BYTES] = 0
    return a.tobytes()


# ---- 1. the pyramid ------------------------------------------------------------------------------------------------------------------------
def test_pyramid_byte_for_byte(lsdmod, ctx, oracle):
    """Every level equals the numpy plane; levels 1..4 equal the device's own coarse plane at b = 2, 4, 8, 16; guards untouched."""
    import torch
    rng = np.random.default_rng(12)
    planes = [gm.random_plane(rng, 61, 47, 0.3), gm.random_plane(rng, 1, 1, 1.0), gm.random_plane(rng, 257, 1, 0.5), gm.random_plane(rng, 1, 257, 0.5),
              gm.random_plane(rng, 65, 5, 0.9), gm.random_plane(rng, 130, 9, 0.05), lc.recovery()[0]["corr"]]     # (65 x 5, 130 x 9: one past the tile)
    lib = lsdmod.load_library()
    for corr in planes:
        rows, cols = corr.shape
        for levels in (0, 3, 8):
            got, ok = device_pyramid(lsdmod, ctx, corr, levels)
            assert ok, (corr.shape, levels)
            assert got.tobytes() == lc.pyramid(corr, levels).tobytes(), (corr.shape, levels)
            assert len(got) == lib.lsd_grid_pyramid_bytes(cols, rows, levels) == lc.pyramid_offset(cols, rows, levels + 1)
        for h in range(9):
            assert lib.lsd_grid_pyramid_offset(cols, rows, h) == lc.pyramid_offset(cols, rows, h)
        for h in (1, 2, 3, 4):
            b = 1 << h
            d = filled((rows + b - 1) * (cols + b - 1))
            assert ctx.L.lsd_enqueue_grid_coarse_device(ctx.h, dev(corr).data_ptr(), cols, rows, b, d.data_ptr(), stream()) == 0
            torch.cuda.synchronize()
            own = back(d, (rows + b - 1) * (cols + b - 1))[0]
            assert got[lc.pyramid_offset(cols, rows, h):lc.pyramid_offset(cols, rows, h + 1)].tobytes() == own.tobytes(), (corr.shape, h)
    assert [lib.lsd_grid_pyramid_bytes(*a) for a in ((0, 5, 4), (5, 65536, 4), (5, 5, -1), (5, 5, 9))] == [0] * 4
    assert lib.lsd_grid_pyramid_offset(5, 5, 9) == lib.lsd_grid_pyramid_offset(0, 5, 1) == 2 ** 64 - 1


# ---- 2. the campaign through both entries ------------------------------------------------------------------------------------------------
def test_campaign_device_entry(lsdmod, ctx, ctx_long, cases):
    """Records and statistics equal the restatement; the device's records at levels = 0 agree with them on everything but lower_bound
    (a scan that overflows has no counterpart there)."""
    for case, want, want_stats in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        n = len(case["lens"])
        d_out, d_stats = filled(64 * n), filled(48 * n)
        assert device_locate(lsdmod, cx, case, d_out, d_stats) == lsdmod.LSD_OK, case["name"]
        got, ok = back(d_out, 64 * n)
        got_stats, ok_stats = back(d_stats, 48 * n)
        assert ok and ok_stats, case["name"]
        assert got.tobytes() == want.tobytes(), (case["name"], got.view(lc.LOCATE_DTYPE), want)
        assert got_stats.tobytes() == want_stats.tobytes(), (case["name"], got_stats.view(lc.STATS_DTYPE), want_stats)
        d_flat = filled(64 * n)
        assert device_locate(lsdmod, cx, case, d_flat, None, levels=0) == lsdmod.LSD_OK, case["name"]
        flat, ok = back(d_flat, 64 * n)
        keep = want["flags"] != lc.OVERFLOW
        a = np.frombuffer(but_lower_bound(got.tobytes()), np.uint8).reshape(n, 64)[keep]
        b = np.frombuffer(but_lower_bound(flat.tobytes()), np.uint8).reshape(n, 64)[keep]
        assert ok and a.tobytes() == b.tobytes(), (case["name"], got.view(lc.LOCATE_DTYPE), flat.view(lc.LOCATE_DTYPE))


def test_campaign_host_entry(lsdmod, ctx, ctx_long, cases):
    assert lsdmod.GRID_LOCATE_DTYPE == lc.LOCATE_DTYPE and lsdmod.GRID_LOCATE_STATS_DTYPE == lc.STATS_DTYPE
    assert lsdmod.GRID_LOCATE_KEYS == lc.PAR_KEYS
    for case, want, want_stats in cases:
        cx = ctx if case["capacity"] <= 1024 else ctx_long
        got, stats = cx.grid_locate(case["scans"], case["lens"], mp_of(case), case["range_max"], case["corr"], case["par"], stats=True)
        assert got.tobytes() == want.tobytes() and stats.tobytes() == want_stats.tobytes(), case["name"]
        alone = cx.grid_locate(case["scans"], case["lens"], mp_of(case), case["range_max"], case["corr"], case["par"])
        assert alone.tobytes() == want.tobytes(), case["name"]


def test_a_deeper_pyramid_serves_a_shallower_search(lsdmod, ctx, cases):
    import torch
    case, want, want_stats = next(c for c in cases if c[0]["name"] == "levels1_1")
    n = len(case["lens"])
    d_out, d_stats = filled(64 * n), filled(48 * n)
    d_sc, d_ln, d_py = dev(case["scans"]), dev(case["lens"]), dev(lc.pyramid(case["corr"], 8))
    assert ctx.L.lsd_enqueue_grid_locate_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, case["scans"].shape[1], lsdmod.lsd_map_param(*mp_of(case)),
                                                case["range_max"], d_py.data_ptr(), par_of(lsdmod, case["par"]), d_out.data_ptr(),
                                                d_stats.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert back(d_out, 64 * n)[0].tobytes() == want.tobytes() and back(d_stats, 48 * n)[0].tobytes() == want_stats.tobytes()


def test_recovery_on_the_device(lsdmod, ctx, oracle):
    """The asymmetric room over the whole grid and 360 degrees: the true cells and headings, the restatement's bytes, both entries."""
    case, truth = lc.recovery()
    want, want_stats, _ = lc.run_case(case)
    n = len(truth)
    d_out, d_stats = filled(64 * n), filled(48 * n)
    assert device_locate(lsdmod, ctx, case, d_out, d_stats) == lsdmod.LSD_OK
    got = back(d_out, 64 * n)[0]
    rec = got.view(lc.LOCATE_DTYPE)
    assert [(int(r["cx"]), int(r["cy"]), int(r["a"])) for r in rec] == truth and (rec["n_best"] == 1).all() and (rec["flags"] == lc.ACCEPTED).all()
    assert got.tobytes() == want.tobytes() and back(d_stats, 48 * n)[0].tobytes() == want_stats.tobytes()
    d_flat = filled(64 * n)
    assert device_locate(lsdmod, ctx, case, d_flat, None, levels=0) == lsdmod.LSD_OK
    assert but_lower_bound(back(d_flat, 64 * n)[0].tobytes()) == but_lower_bound(want.tobytes())
    host = ctx.grid_locate(case["scans"], case["lens"], mp_of(case), case["range_max"], case["corr"], case["par"])
    assert host.tobytes() == want.tobytes()


def test_no_scans_is_a_no_op(lsdmod, ctx, cases):
    import torch
    case = cases[0][0]
    d_out, d_stats = filled(64), filled(48)
    d = dev(np.zeros(4))
    st = ctx.L.lsd_enqueue_grid_locate_device(ctx.h, d.data_ptr(), d.data_ptr(), 0, 4, lsdmod.lsd_map_param(*mp_of(case)), 2.0,
                                              dev(lc.pyramid(case["corr"], 1)).data_ptr(), par_of(lsdmod, case["par"]), d_out.data_ptr(),
                                              d_stats.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK and (d_out.cpu().numpy() == FILL).all() and (d_stats.cpu().numpy() == FILL).all()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, cases):
    import torch
    INV = lsdmod.LSD_ERR_INVALID
    case = next(c for c, _, _ in cases if c["name"] == "nb65_1")
    n, corr, base = len(case["lens"]), case["corr"], dict(case["par"])
    d_corr = dev(corr)
    d_pyr = filled(lsdmod.grid_pyramid_bytes(case["cols"], case["rows"], 4))
    py = lambda h=ctx.h, src=d_corr.data_ptr(), cols=case["cols"], rows=case["rows"], levels=4, dst=d_pyr.data_ptr(): \
        ctx.L.lsd_enqueue_grid_pyramid_device(h, src, cols, rows, levels, dst, stream())
    refused = [py(h=None), py(src=None), py(dst=None), py(cols=0), py(cols=65536), py(rows=0), py(rows=-2), py(rows=65536), py(levels=-1), py(levels=9)]
    assert refused == [INV] * len(refused), refused
    torch.cuda.synchronize()
    assert (d_pyr.cpu().numpy() == FILL).all()

    d_out, d_stats = filled(64 * n), filled(48 * n)
    wide = np.zeros((1, 1025, 2)); wide[..., 0] = 0.5
    d_sc, d_ln, d_py, d_wide = dev(case["scans"]), dev(case["lens"]), dev(lc.pyramid(corr, 4)), dev(wide)

    def par(se):
        return lsdmod.lsd_grid_locate_par(*[dict(base, **se)[k] for k in lc.PAR_KEYS])

    def call(h=ctx.h, sc=d_sc.data_ptr(), ln=d_ln.data_ptr(), n=n, stride=case["scans"].shape[1], cols=case["cols"], rows=case["rows"], resol=0.05,
             range_max=1.5, pyr=d_py.data_ptr(), out=d_out.data_ptr(), stats=d_stats.data_ptr(), **se):
        return ctx.L.lsd_enqueue_grid_locate_device(h, sc, ln, n, stride, lsdmod.lsd_map_param(cols, rows, resol, 0.0, 0.0), range_max, pyr, par(se), out,
                                                    stats, stream())
    assert ctx.scan_capacity == 1024
    bad_par = [dict(x0=-(1 << 20) - 1), dict(x0=(1 << 20) + 1), dict(y0=-(1 << 20) - 1), dict(y0=(1 << 20) + 1), dict(nx=0), dict(nx=65536), dict(ny=0),
               dict(ny=-3), dict(ny=65536), dict(n_ang=0), dict(n_ang=4097), dict(ang0=math.nan), dict(ang0=math.inf), dict(ang_step=math.nan),
               dict(ang_step=math.inf), dict(ang_step=-0.5), dict(n_ang=2, ang_step=0.0), dict(levels=-1), dict(levels=9), dict(max_nodes=0),
               dict(max_nodes=(1 << 24) + 1), dict(min_den=0), dict(min_num=5, min_den=4),
               dict(nx=65535, ny=65535, n_ang=4096, levels=7),                             # 4096 * 512 * 512 top nodes
               dict(nx=65535, ny=65535, n_ang=17, levels=4)]                               # 17 * 4096 * 4096: one heading beyond 2^28
    assert call(nx=65535, ny=65535, n_ang=4096, levels=8, n=0) == lsdmod.LSD_OK            # (exactly 2^28: taken; no scans: nothing runs)
    refused = [call(h=None), call(sc=None), call(ln=None), call(pyr=None), call(out=None), call(n=-1), call(stride=0),
               call(sc=d_wide.data_ptr(), n=1, stride=1025), call(cols=0), call(cols=65536), call(rows=-3), call(rows=65536), call(resol=0.0),
               call(resol=math.nan), call(range_max=0.0), call(range_max=math.nan), call(range_max=math.inf), call(range_max=32767 * 0.05),
               call(sc=d_sc.data_ptr() + 8), call(out=d_out.data_ptr() + 4), call(stats=d_stats.data_ptr() + 2), call(stats=d_stats.data_ptr() + 1),
               call(ln=d_ln.data_ptr() + 2)] + [call(**se) for se in bad_par]
    assert refused == [INV] * len(refused), refused
    lib = lsdmod.load_library()
    assert [lib.lsd_grid_locate_workspace_bytes(n, 68, par(se)) for se in bad_par] == [0] * len(bad_par)
    assert lib.lsd_grid_locate_workspace_bytes(-1, 68, par({})) == lib.lsd_grid_locate_workspace_bytes(1, 0, par({})) == 0
    assert lib.lsd_grid_locate_workspace_bytes(n, 68, par({})) > 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_stats.cpu().numpy() == FILL).all()
    # the host entry refuses the same before anything travels, and a length outside 0..stride
    out = np.full(n, FILL, np.uint8).repeat(64).view(lc.LOCATE_DTYPE)
    hstats = np.full(n, FILL, np.uint8).repeat(48).view(lc.STATS_DTYPE)
    keep, keep_stats = out.tobytes(), hstats.tobytes()

    def host(lens=case["lens"], cols=case["cols"], range_max=1.5, co=corr.ctypes.data, **se):
        ln = np.ascontiguousarray(lens, np.int32)
        return ctx.L.lsd_grid_locate(ctx.h, case["scans"].ctypes.data, ln.ctypes.data, n, case["scans"].shape[1],
                                     lsdmod.lsd_map_param(cols, case["rows"], 0.05, 0.0, 0.0), range_max, co, par(se), out.ctypes.data, hstats.ctypes.data)
    bad_len = case["lens"].copy(); bad_len[0] = case["scans"].shape[1] + 1
    refused = [host(lens=bad_len), host(cols=65536), host(range_max=32767 * 0.05), host(co=None), host(nx=0), host(n_ang=2, ang_step=0.0),
               host(min_den=0), host(levels=9), host(max_nodes=0)]
    assert refused == [INV] * len(refused) and out.tobytes() == keep and hstats.tobytes() == keep_stats
    # a statistics pointer that is 4-byte but not 8-byte aligned is taken
    assert call(stats=d_stats.data_ptr() + 4, n=1) == lsdmod.LSD_OK
    torch.cuda.synchronize()
    assert back(d_out, 64 * n)[1] and back(d_stats, 48 * n)[1]


# ---- 4. composition: the records are poses ------------------------------------------------------------------------------------------------
def test_records_are_a_poses_argument(lsdmod, ctx, cases):
    """The locate records at pitch 64 as d_poses of the match and of the integration: the restatements' bytes for the poses at the
    records' heads, and the scans whose record carries the sentinel are skipped."""
    import torch
    picked = [c for c in cases if c[0]["name"] in ("empty_middle_0", "min_beams_1", "accept-1_0", "accept+0_0", "floor_above_1", "nb65_1")]
    assert len(picked) == 6
    se = gm.search(2, 1, 1, 1.0, min_beams=1, min_num=1, min_den=8)
    skipped = taken = 0
    for case, want, _ in picked:
        n, stride = len(case["lens"]), case["scans"].shape[1]
        d_rec = filled(64 * n)
        assert device_locate(lsdmod, ctx, case, d_rec, None) == lsdmod.LSD_OK
        assert back(d_rec, 64 * n)[0].tobytes() == want.tobytes()
        poses = np.ascontiguousarray(np.stack([want["x"], want["y"], want["ang"]], 1))
        d_sc, d_ln, d_co = dev(case["scans"]), dev(case["lens"]), dev(case["corr"])
        mp = lsdmod.lsd_map_param(*mp_of(case))
        d_out = filled(56 * n)
        assert ctx.L.lsd_enqueue_grid_match_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, stride, d_rec.data_ptr(), 64, mp, case["range_max"],
                                                   d_co.data_ptr(), lsdmod.grid_search(se), d_out.data_ptr(), stream()) == 0
        planes = torch.zeros((2, case["rows"] * case["cols"]), dtype=torch.int32, device="cuda")
        assert ctx.L.lsd_enqueue_grid_integrate_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, stride, d_rec.data_ptr(), 64, mp, case["range_max"],
                                                       planes[0].data_ptr(), planes[1].data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        got, ok = back(d_out, 56 * n)
        want_match = gm.match(case["scans"], case["lens"], poses, case["resol"], case["range_max"], case["corr"], se)
        assert ok and got.tobytes() == want_match.tobytes(), case["name"]
        sentinel = want["flags"] != lc.ACCEPTED
        assert ((want_match["flags"] == gm.SKIPPED) == sentinel).all()
        pa, hi = np.zeros((case["rows"], case["cols"]), np.uint32), np.zeros((case["rows"], case["cols"]), np.uint32)
        gc.integrate(case["scans"], case["lens"], poses, case["cols"], case["rows"], case["resol"], case["range_max"], pa, hi)
        both = planes.cpu().numpy().view(np.uint32)
        assert both[0].tobytes() == pa.tobytes() and both[1].tobytes() == hi.tobytes(), case["name"]
        skipped, taken = skipped + int(sentinel.sum()), taken + int((~sentinel).sum())
    assert skipped >= 4 and taken >= 4


# ---- 5. GridMapper -------------------------------------------------------------------------------------------------------------------------
def test_grid_mapper_locates(lsdmod, ctx, oracle):
    """locate_device is likelihood + pyramid + locate called by hand; locate reads the records back; the default box is the whole grid."""
    import torch
    case, truth = lc.recovery()
    corr, scans, lens, p = case["corr"], case["scans"], case["lens"], case["par"]
    m = lsdmod.GridMapper(case["cols"], case["rows"], case["resol"], 0.0, 0.0, case["range_max"], ctx=ctx)
    mapped = np.array([(14.0, 11.0, 0.0), (44.0, 14.0, 90.0), (26.0, 30.0, 180.0), (14.0, 34.0, 270.0), (28.0, 12.0, 45.0)])
    sc = np.stack([lc.room_scan(q, 360) for q in mapped])
    for _ in range(2):
        m.integrate(sc, np.full(len(mapped), 360, np.int32), mapped)
    sm = lsdmod.grid_smear((3, gm.GAUSS))
    want, want_stats, _ = lc.run_case(case)
    rec, stats = m.locate_device(dev(scans), dev(lens), p, smear=sm, stats=True)
    torch.cuda.synchronize()
    assert tuple(rec.shape) == (3, 64) and tuple(stats.shape) == (3, 48) and rec.dtype == stats.dtype == torch.uint8
    assert m._corr.cpu().numpy().tobytes() == corr.tobytes()
    assert rec.cpu().numpy().tobytes() == want.tobytes() and stats.cpu().numpy().tobytes() == want_stats.tobytes()
    # by hand, on the mapper's own counters
    d_corr = filled(corr.size)
    ctx.enqueue_grid_likelihood_device(m.d_pass, m.d_hit, m.cols, m.rows, d_corr.data_ptr(), smear=sm, stream=stream())
    d_pyr = filled(lsdmod.grid_pyramid_bytes(m.cols, m.rows, p["levels"]))
    ctx.enqueue_grid_pyramid_device(d_corr.data_ptr(), m.cols, m.rows, p["levels"], d_pyr.data_ptr(), stream())
    d_out, d_stats = filled(64 * 3), filled(48 * 3)
    d_sc, d_ln = dev(scans), dev(lens)
    ctx.enqueue_grid_locate_device(d_sc.data_ptr(), d_ln.data_ptr(), 3, scans.shape[1], m.map_param, m.range_max, d_pyr.data_ptr(), p, d_out.data_ptr(),
                                   d_stats.data_ptr(), stream())
    torch.cuda.synchronize()
    assert back(d_out, 192)[0].tobytes() == rec.cpu().numpy().tobytes() and back(d_stats, 144)[0].tobytes() == stats.cpu().numpy().tobytes()
    assert back(d_pyr, len(d_pyr) - GUARD)[0].tobytes() == m.pyramid_device(p["levels"]).cpu().numpy().tobytes() == lc.pyramid(corr, p["levels"]).tobytes()
    # host arrays; keywords over the default box
    got = m.locate(scans, lens, p, refresh=False)
    assert got.dtype == lsdmod.GRID_LOCATE_DTYPE and got.tobytes() == want.tobytes()
    kw = {k: p[k] for k in ("ang_step", "n_ang", "levels", "max_nodes", "min_beams", "min_num", "min_den")}
    got, st = m.locate(scans, lens, kw, smear=sm, stats=True)
    assert got.tobytes() == want.tobytes() and st.tobytes() == want_stats.tobytes()
    q = lsdmod.grid_locate(cols=61, rows=47)
    assert (q.x0, q.y0, q.nx, q.ny) == (0, 0, 61, 47)
    for bad in (dict(levels=9), dict(nx=0), dict(min_den=0)):
        with pytest.raises(lsdmod.LsdError):
            m.locate_device(dev(scans), dev(lens), dict(p, **bad))
    with pytest.raises(lsdmod.LsdError):
        lsdmod.grid_locate()                                                           # no grid known: no default box
    with pytest.raises(lsdmod.LsdError):
        m.pyramid_device(9)


# ---- 6. end to end: the data log's first frames --------------------------------------------------------------------------------------------
FRAMES = 8
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


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    return DataLog(lsdmod, ctx)


def log_box(lsdmod, out):
    """The parameters of a small box and a few headings around the first state of a tick: a search the restatement can follow."""
    import torch
    torch.cuda.synchronize()
    st = out[0].cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE)
    x, y, ang = (float(v) for v in st["x"][0, :3])
    return lc.par(int(x) - 11, int(y) - 9, 24, 19, ang0=float(round(ang)) - 4.0, ang_step=2.0, n_ang=5, levels=3, min_beams=30, min_num=1, min_den=8)


def test_localizer_locates_its_last_tick(lsdmod, ctx, log):
    """The tick's frames entered at the localiser's poses, then located on that grid from the scans alone: the records equal the
    restatement fed with the ingested scans and the lookup plane the mapper made."""
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    with pytest.raises(lsdmod.LsdError):
        loc.locate_last_tick(m)                                                        # no tick yet
    out = loc.step_device(dev(log.lid[None]), dev(log.odom[None, 1:]))
    loc.integrate_last_tick(m)
    p = log_box(lsdmod, out)
    rec, stats = loc.locate_last_tick(m, p, stats=True)
    corr = m._corr.cpu().numpy()
    assert corr.any()
    want, want_stats = lc.locate(log.scans, log.lens, log.resol, RANGE_MAX, corr, p)
    assert tuple(rec.shape) == (FRAMES, 64) and rec.cpu().numpy().tobytes() == want.tobytes()
    assert stats.cpu().numpy().tobytes() == want_stats.tobytes()
    assert (want["flags"] == lc.ACCEPTED).any() and want["score"].any()                # the search took part


def test_locate_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    d_lid, d_od = dev(log.lid[None]), dev(log.odom[None, 1:])
    out = loc.step_device(d_lid, d_od)                                                 # warm: the staging, the workspace and the planes have their size
    loc.integrate_last_tick(m)
    p = log_box(lsdmod, out)
    loc.locate_last_tick(m, p, stats=True)
    d_sc, d_ln = dev(log.scans), dev(log.lens)
    m.locate_device(d_sc, d_ln, p, stats=True)
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
    rec = loc.locate_last_tick(m, p)
    rec2, stats2 = m.locate_device(d_sc, d_ln, p, stats=True)
    m.pyramid_device(3)
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "the locate calls returned only after the work in front of them had finished"
    assert rec.is_cuda and rec2.is_cuda and stats2.is_cuda and rec.cpu().numpy().tobytes() == rec2.cpu().numpy().tobytes()
