"""The grid match response fused into the carry, on the device (csrc/k_facorrect.hip: lsd_enqueue_fa_carry_correct_device,
lsd_fa_carry_correct; Localizer / FleetLocalizer .correct_last_tick and correct= of refine_and_integrate_last_tick) against the restatement of
tests/fa_correct_cases.py.  The rule fixes the order of every sum, so every comparison is byte equality."""
import math
import time

import numpy as np
import pytest

import fa_correct_cases as fc
import fa_restatement as fr
import grid_cases as gc
import grid_match_cases as gm
import grid_response_cases as gr
from fa_resume import ResumableLoop

pytestmark = pytest.mark.gpu

GUARD = 256                                    # bytes behind every buffer
FILL = 0x5A
FRAMES = 20                                    # of the `data` log: one tick
NEXT = 4                                       # frames of the tick after it
RANGE_MAX = 8.0
LOG_SEARCH = gm.search(3, 2, 1, 0.5, min_beams=30, min_num=1, min_den=8)
LOG_RESPONSE = gr.params(2, 2, 1)


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a):
    """The bytes of `a` on the device with GUARD bytes of the fill pattern behind them."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return dev(np.concatenate([b, np.full(GUARD, FILL, np.uint8)]))


def back(t, n_bytes):
    """(the first n_bytes, True if the guard is untouched)."""
    a = t.cpu().numpy()
    return a[:n_bytes], bool((a[n_bytes:] == FILL).all())


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class DataLog:
    def __init__(self, lsdmod, ctx):
        m, self.mp, lid, odom = fr.load_log("data")
        self.lid, self.odom = lid[:FRAMES + NEXT], odom[:FRAMES + NEXT + 1]
        self.mc = ctx.map_cache(m.copy(), float(self.mp[2]), lsdmod.z_occ_max_dis)
        self.ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
        self.cols, self.rows, self.resol = int(self.mp[0]), int(self.mp[1]), float(self.mp[2])
        self.scans, self.lens = lsdmod.lidar_frames_batch(self.lid)                  # what k_ingest writes (tests/test_scan_ingest_gpu.py)
        self.states, self.reports = ctx.localize(self.mc, self.ml, self.scans[:FRAMES], self.lens[:FRAMES], self.odom[:FRAMES + 1], self.mp)

    def mapper(self, lsdmod, ctx):
        return lsdmod.GridMapper(self.cols, self.rows, self.resol, float(self.mp[3]), float(self.mp[4]), RANGE_MAX, ctx=ctx)


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    return DataLog(lsdmod, ctx)


@pytest.fixture(scope="module")
def cases(log):
    """(batch, carries after, reports) of every launch of the campaign: the restatement, computed once.  The campaign's log states are
    the device's own replay of the data log."""
    ukf = [t for t in range(FRAMES) if log.reports[t]["branch"] == fr.UKF][:8]
    assert len(ukf) >= 3
    units = fc.campaign([fc.rows_of(log.states[t]) for t in ukf])
    return [(b,) + fc.run_batch(b) for b in fc.batches(units)]


def pose_records(b, pitch, seed):
    """The original poses of a batch at the head of records of `pitch` bytes of noise."""
    n = len(b["units"]) * b["frames_pitch"]
    rec = np.random.default_rng(seed).integers(0, 256, (n, pitch), dtype=np.uint8)
    rec[:, :24] = np.concatenate([u["poses"] for u in b["units"]]).view(np.uint8).reshape(n, 24)
    return rec


def device_correct(lsdmod, cx, b, pitch=24, with_rep=True, seed=0, **kw):
    """One launch of a batch through the raw entry: (status, carry bytes, report bytes or None, every guard and input untouched)."""
    import torch
    n = len(b["units"])
    carries = np.array([u["carry"] for u in b["units"]], fc.CARRY_DTYPE)
    poses, resp = pose_records(b, pitch, seed), np.concatenate([u["resp"] for u in b["units"]])
    d_cy, d_po, d_re = guarded(carries), guarded(poses), guarded(resp)
    d_rp = guarded(np.full(n * 48, FILL, np.uint8))
    d_key = dev(b["keys"]) if b["keys"] is not None else None
    a = dict(h=cx.h, cy=d_cy.data_ptr(), n=n, fp=b["frames_pitch"], po=d_po.data_ptr(), pp=pitch, re=d_re.data_ptr(),
             key=d_key.data_ptr() if d_key is not None else None, k=b["key"], par=lsdmod.lsd_fa_correct(*b["par"]),
             rp=d_rp.data_ptr() if with_rep else None)
    a.update(kw)
    st = cx.L.lsd_enqueue_fa_carry_correct_device(a["h"], a["cy"], a["n"], a["fp"], a["po"], a["pp"], a["re"], a["key"], a["k"], a["par"], a["rp"],
                                                  stream())
    torch.cuda.synchronize()
    got_cy, ok1 = back(d_cy, carries.nbytes)
    got_rp, ok2 = back(d_rp, n * 48)
    got_po, ok3 = back(d_po, poses.nbytes)
    got_re, ok4 = back(d_re, resp.nbytes)
    clean = ok1 and ok2 and ok3 and ok4 and got_po.tobytes() == poses.tobytes() and got_re.tobytes() == resp.tobytes()
    return st, got_cy, got_rp, clean


def want_reports(reps):
    """The report bytes after a launch into a buffer of the fill pattern: a sequence the key leaves out keeps the pattern."""
    return b"".join(bytes([FILL]) * 48 if r is None else r.tobytes() for r in reps)


# ---- 1. the campaign, bit for bit ----------------------------------------------------------------------------------------------------------
def test_campaign_device_entry(lsdmod, ctx, cases):
    """Every launch of the campaign at pose pitches 24, 720 and 768, with reports and without: all 768 bytes of every carry and all 48 of
    every report are the restatement's; a sequence the key leaves out keeps its carry and its report bytes; no guard is touched."""
    assert {len(b["units"]) for b, _, _ in cases} >= {1, 2, 3, 65} and {b["frames_pitch"] for b, _, _ in cases} == {1, 3, 64, 65}
    for n, (b, want_cy, want_rp) in enumerate(cases):
        for pitch in (24, 720, 768):
            st, cy, rp, clean = device_correct(lsdmod, ctx, b, pitch, seed=n)
            assert st == lsdmod.LSD_OK and clean, (b["name"], pitch)
            bad = [u["name"] for s, u in enumerate(b["units"]) if cy[768 * s:768 * s + 768].tobytes() != want_cy[s].tobytes()]
            assert not bad, (b["name"], pitch, bad)
            assert rp.tobytes() == want_reports(want_rp), (b["name"], pitch)
        st, cy, rp, clean = device_correct(lsdmod, ctx, b, 24, with_rep=False, seed=n)
        assert st == lsdmod.LSD_OK and clean and cy.tobytes() == want_cy.tobytes(), b["name"]
        assert rp.tobytes() == bytes([FILL]) * len(rp), b["name"]                      # d_rep = NULL: nothing of it is written


def test_campaign_host_entry(lsdmod, ctx, cases):
    """lsd_fa_carry_correct from host arrays (no key: the batches without the units a key leaves out)."""
    for b, want_cy, want_rp in cases:
        keep = [s for s, u in enumerate(b["units"]) if not u["skip"]]
        if not keep:
            continue
        us = [b["units"][s] for s in keep]
        carries = np.array([u["carry"] for u in us], lsdmod.FA_CARRY_DTYPE)
        before = carries.tobytes()
        cy, rp = ctx.fa_carry_correct(carries, np.stack([u["poses"] for u in us]), np.stack([u["resp"] for u in us]), b["par"])
        assert carries.tobytes() == before
        assert cy.tobytes() == want_cy[keep].tobytes(), b["name"]
        assert rp.tobytes() == b"".join(want_rp[s].tobytes() for s in keep), b["name"]
    b = cases[0][0]
    u = b["units"][0]
    L, par = ctx.L, lsdmod.lsd_fa_correct(*b["par"])
    cy, po, re_ = np.array([u["carry"]]), np.ascontiguousarray(u["poses"]), np.ascontiguousarray(u["resp"])
    rep = np.full(48, FILL, np.uint8)
    before = cy.tobytes()
    good = (ctx.h, cy.ctypes.data, 1, len(po), po.ctypes.data, re_.ctypes.data, par, rep.ctypes.data)
    for i, v in ((0, None), (1, None), (2, 0), (3, 0), (3, 4097), (4, None), (5, None), (6, lsdmod.lsd_fa_correct(1.0, -1.0, 1.0, 0.0)),
                 (7, rep.ctypes.data + 4)):
        args = list(good)
        args[i] = v
        assert L.lsd_fa_carry_correct(*args) == lsdmod.LSD_ERR_INVALID, i
        assert cy.tobytes() == before and (rep == FILL).all(), i


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(lsdmod, ctx, cases):
    """LSD_ERR_INVALID before anything is enqueued: the carries and the reports keep every byte."""
    b = next(b for b, _, _ in cases if len(b["units"]) >= 3 and b["frames_pitch"] == 3 and b["par"] == fc.DEFAULTS)
    carries = np.array([u["carry"] for u in b["units"]], fc.CARRY_DTYPE).tobytes()
    par = lambda *v: lsdmod.lsd_fa_correct(*v)
    bad = [dict(h=None), dict(cy=None), dict(po=None), dict(re=None), dict(n=0), dict(n=-1), dict(fp=0), dict(fp=-3), dict(fp=4097),
           dict(pp=0), dict(pp=16), dict(pp=28), dict(pp=25), dict(par=par(-1.0, 1.0, 1.0, 0.0)), dict(par=par(1.0, -0.5, 1.0, 0.0)),
           dict(par=par(1.0, 1.0, -1.0, 0.0)), dict(par=par(1.0, 1.0, 1.0, -2.0)), dict(par=par(math.nan, 1.0, 1.0, 0.0)),
           dict(par=par(1.0, math.inf, 1.0, 0.0)), dict(par=par(1.0, 1.0, math.nan, 0.0)), dict(par=par(1.0, 1.0, 1.0, math.inf))]
    for kw in bad:
        st, cy, rp, clean = device_correct(lsdmod, ctx, b, **kw)
        assert st == lsdmod.LSD_ERR_INVALID, kw
        assert clean and cy.tobytes() == carries and (rp == FILL).all(), kw
    for name in ("cy", "po", "re", "rp"):                                              # a pointer that is not 8-byte aligned
        import torch
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        st, cy, rp, clean = device_correct(lsdmod, ctx, dict(b, units=b["units"][:1], keys=None), **{name: buf.data_ptr() + 4})
        assert st == lsdmod.LSD_ERR_INVALID and clean and cy.tobytes() == carries[:768] and (rp == FILL).all(), name
        assert not buf.any()
    with pytest.raises(lsdmod.LsdError):
        ctx.enqueue_fa_carry_correct_device(0, 1, 1, 0, 24, 0)
    with pytest.raises(lsdmod.LsdError):
        ctx.fa_carry_correct(np.zeros(2, lsdmod.FA_CARRY_DTYPE), np.zeros((2, 1, 3)), np.zeros((2, 2), lsdmod.GRID_RESPONSE_DTYPE))


# ---- 3. end to end: the data log's first 20 frames, and the tick after them -----------------------------------------------------------------
def tick(lsdmod, ctx, log, n_robots=1):
    """A localiser after its first tick of FRAMES frames, integrated into a fresh mapper: (loc, mapper, states, carries before)."""
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, n_robots, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    out = loc.step_device(dev(np.repeat(log.lid[None, :FRAMES], n_robots, 0)), dev(np.repeat(log.odom[None, 1:FRAMES + 1], n_robots, 0)))
    loc.integrate_last_tick(m)
    torch.cuda.synchronize()
    states = out[0].cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(n_robots, FRAMES).copy()
    return loc, m, states, loc.carries


def restated_tick(lsdmod, log, poses, carry):
    """Match, response and correction restated on the device's own states, the ingested scans and the carry from before."""
    pa, hi = np.zeros((log.rows, log.cols), np.uint32), np.zeros((log.rows, log.cols), np.uint32)
    sc, ln = log.scans[:FRAMES], log.lens[:FRAMES]
    gc.integrate(sc, ln, poses, log.cols, log.rows, log.resol, RANGE_MAX, pa, hi)
    r, w = lsdmod.grid_smear_table(lsdmod.grid_smear_default(1.0, 3))
    corr = gm.likelihood(pa, hi, 2, 1, 10, r, w)
    rec = gm.match(sc, ln, poses, log.resol, RANGE_MAX, corr, LOG_SEARCH)
    resp, _ = gr.response(sc, ln, poses, rec, log.resol, RANGE_MAX, corr, LOG_SEARCH["ang_step"], LOG_RESPONSE)
    after, rep = fc.correct_carry(carry, poses, resp, fc.DEFAULTS)
    return rec, resp, after, rep


def test_localizer_corrects_and_the_next_tick_resumes_from_it(lsdmod, ctx, log):
    """step_device + refine_and_integrate_last_tick(..., correct=True), whichever search wrote the records: the carry afterwards is the
    restatement's, and the NEXT step_device is the restated resume loop (tests/fa_resume.py) from the corrected carry, frame for frame."""
    import torch
    want = None
    for block in (0, 4):
        loc, m, states, before = tick(lsdmod, ctx, log)
        rec, resp, rep = loc.refine_and_integrate_last_tick(m, LOG_SEARCH, block=block, response=LOG_RESPONSE, correct=True)
        after = loc.carries
        poses = np.ascontiguousarray(states["x"][0, :, :3])
        if want is None:
            want = restated_tick(lsdmod, log, poses, before[0])
            assert want[3]["flags"] == fc.APPLIED and want[3]["slot"] == FRAMES - 1 and np.any(want[3]["innov"])     # the correction took part
            assert want[2].tobytes() != before[0].tobytes()
        assert rec.cpu().numpy().tobytes() == want[0].tobytes() and resp.cpu().numpy().tobytes() == want[1].tobytes(), block
        assert tuple(rep.shape) == (1, 48) and rep.cpu().numpy().tobytes() == want[3].tobytes(), block
        assert after[0].tobytes() == want[2].tobytes(), block
        # the tick after: the restated resume from the corrected carry, on the device's FeatureScan and scores
        out = loc.step_device(dev(log.lid[None, FRAMES:]), dev(log.odom[None, FRAMES + 1:]))
        torch.cuda.synchronize()
        got = out[0].cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE)
        fs = ctx.feature_scan_batch(log.scans[FRAMES:], log.lens[FRAMES:], log.mp, pts_cap=8192)
        res = ResumableLoop.from_carry(want[2], log.resol)
        for t in range(NEXT):
            od = tuple(float(v) for v in log.odom[FRAMES + t + 1])
            sp, last = res.scan_pose(od), res.last_pose()
            lp = (fr.c_round(fs[t]["lidarPos"][0]), fr.c_round(fs[t]["lidarPos"][1]), 0.0)
            sl = fs[t]["linesInfo"]
            pr = np.array(fr.pairs(log.ml["len"], sl["len"]), np.int32).reshape(-1, 2)
            d = ctx.scan_to_map_match(log.mc, log.ml, sl, fs[t]["scanImPoint"], lp, last, pr).reshape(-1) if len(pr) else np.zeros(0, lsdmod.SCORE_DTYPE)
            x, P, _ = fr.feature_association(np.stack([d["x"], d["y"], d["ang"], d["score"]], 1), last, sp, res.x, res.P, len(pr))
            res.finish(od, x, P)
            assert got[t]["x"].tobytes() == np.array(x).tobytes(), (block, t)
            assert got[t]["P"].tobytes() == np.array(P).ravel(order="F").tobytes(), (block, t)
        assert loc.carries[0].tobytes() == res.carry(lsdmod.FA_CARRY_DTYPE).tobytes(), block


def test_correct_none_is_the_call_of_before(lsdmod, ctx, log):
    """correct=None: the carries keep every byte, and planes and records are those of a localiser that is never asked for a correction."""
    a, ma, _, before = tick(lsdmod, ctx, log)
    b, mb, _, _ = tick(lsdmod, ctx, log)
    got_a = a.refine_and_integrate_last_tick(ma, LOG_SEARCH, response=LOG_RESPONSE, correct=None)
    got_b = b.refine_and_integrate_last_tick(mb, LOG_SEARCH, response=LOG_RESPONSE)
    assert len(got_a) == len(got_b) == 2
    for x, y in zip(got_a, got_b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a.carries.tobytes() == b.carries.tobytes() == before.tobytes()
    for x, y in zip(ma.counts(), mb.counts()):
        assert x.tobytes() == y.tobytes()
    rec = a.refine_and_integrate_last_tick(ma, LOG_SEARCH, refresh=False)               # and without a response: the records alone
    assert tuple(rec.shape) == (FRAMES, 56)
    with pytest.raises(lsdmod.LsdError) as err:
        a.refine_and_integrate_last_tick(ma, LOG_SEARCH, correct=True)                  # correct needs response
    assert err.value.status == lsdmod.LSD_ERR_INVALID
    assert a.carries.tobytes() == before.tobytes()


def test_correct_last_tick_composes(lsdmod, ctx, log):
    """correct_last_tick(resp) behind refine_and_integrate_last_tick(response=...) is the one call with correct=; a second correction on
    the same tick finds the carry moved on: STALE, and nothing changes."""
    a, ma, _, before = tick(lsdmod, ctx, log, 2)
    b, mb, _, _ = tick(lsdmod, ctx, log, 2)
    rec_a, resp_a, rep_a = a.refine_and_integrate_last_tick(ma, LOG_SEARCH, response=LOG_RESPONSE, correct=dict(floor_ang=0.5))
    rec_b, resp_b = b.refine_and_integrate_last_tick(mb, LOG_SEARCH, response=LOG_RESPONSE)
    rep_b = b.correct_last_tick(resp_b, lsdmod.fa_correct(floor_ang=0.5))
    assert resp_a.cpu().numpy().tobytes() == resp_b.cpu().numpy().tobytes()
    assert rep_a.cpu().numpy().tobytes() == rep_b.cpu().numpy().tobytes()
    after = b.carries
    assert a.carries.tobytes() == after.tobytes() != before.tobytes()
    reps = rep_b.cpu().numpy().reshape(-1).view(lsdmod.FA_CORRECT_DTYPE)
    assert (reps["flags"] == lsdmod.FA_CORRECT_APPLIED).all() and tuple(rep_b.shape) == (2, 48)
    again = b.correct_last_tick(resp_b, lsdmod.fa_correct(floor_ang=0.5)).cpu().numpy().reshape(-1).view(lsdmod.FA_CORRECT_DTYPE)
    assert (again["flags"] == lsdmod.FA_CORRECT_STALE).all() and (again["slot"] == -1).all()
    assert b.carries.tobytes() == after.tobytes()
    with pytest.raises(lsdmod.LsdError):
        b.correct_last_tick(resp_b[:1])


# ---- 4. the fleet --------------------------------------------------------------------------------------------------------------------------
K = 8                                          # frames of the fleet's tick
MAP_OF = [0, 1, -1, 0, 0]                      # robots 0, 3 and 4 on map 0 (two runs of neighbours), one on map 1, one parked
NF = [K, K, K, K - 2, K]


def fleet_site(lsdmod, ctx, log):
    """Map 0 the data log's, map 1 the same map at twice the resolution; every robot replays the log's first K frames in its map's units."""
    mp2 = np.array(log.mp, np.float64)
    mp2[2:5] *= 2.0
    lid = np.repeat(log.lid[None, :K], len(MAP_OF), 0).copy()
    odom = np.repeat(log.odom[None, :K + 1], len(MAP_OF), 0).copy()
    lid[1, ..., 0] = np.where(np.isfinite(lid[1, ..., 0]), lid[1, ..., 0] * 2.0, lid[1, ..., 0])
    odom[1, :, :2] *= 2.0
    mc2 = ctx.map_cache(fr.load_log("data")[0].copy(), float(mp2[2]), lsdmod.z_occ_max_dis)
    return [(log.mc, log.ml, log.mp), (mc2, log.ml, mp2)], lid, odom


def fleet_tick(lsdmod, ctx, log):
    import torch
    maps, lid, odom = fleet_site(lsdmod, ctx, log)
    fl = lsdmod.FleetLocalizer(maps, MAP_OF, odom0=odom[:, 0], ctx=ctx)
    fl.step_device(dev(lid), dev(odom[:, 1:]), NF)
    m0 = log.mapper(lsdmod, ctx)
    fl.integrate_last_tick(m0, 0)
    torch.cuda.synchronize()
    return fl, m0, fl.carries, lid, odom


def test_fleet_refines_and_corrects_one_map(lsdmod, ctx, log):
    """Two maps, robots on map 0 (in two runs), on map 1 and parked: refine_and_integrate_last_tick(m0, 0, ..., correct=True) gives the
    robots on map 0 what a Localizer alone on that map gives them, bit for bit -- records, responses, reports, carries and the mapper's
    planes --; the other robots' slots are zero bytes and their carries keep every byte; a robot an assign() moved off the map before
    the call keeps its carry through the device key."""
    import torch
    fl, m0, before, lid, odom = fleet_tick(lsdmod, ctx, log)
    on0 = [s for s, i in enumerate(MAP_OF) if i == 0]
    rec, resp, rep = fl.refine_and_integrate_last_tick(m0, 0, LOG_SEARCH, response=LOG_RESPONSE, correct=True)
    after = fl.carries
    assert tuple(rec.shape) == (len(MAP_OF) * K, 56) and tuple(resp.shape) == (len(MAP_OF) * K, 192) and tuple(rep.shape) == (len(MAP_OF), 48)
    # the Localizer alone on map 0, with the same three robots
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, len(on0), odom0=odom[on0, 0], ctx=ctx)
    m1 = log.mapper(lsdmod, ctx)
    loc.step_device(dev(lid[on0]), dev(odom[on0, 1:]), [NF[s] for s in on0])
    loc.integrate_last_tick(m1)
    assert loc.carries.tobytes() == before[on0].tobytes()
    rec1, resp1, rep1 = loc.refine_and_integrate_last_tick(m1, LOG_SEARCH, response=LOG_RESPONSE, correct=True)
    torch.cuda.synchronize()
    rows = lambda t, per: t.cpu().numpy().reshape(len(MAP_OF), per, -1)
    for got, alone, per in ((rec, rec1, K), (resp, resp1, K), (rep, rep1, 1)):
        g = rows(got, per)
        assert g[on0].tobytes() == alone.cpu().numpy().tobytes()
        assert not g[[s for s in range(len(MAP_OF)) if s not in on0]].any()
    assert after[on0].tobytes() == loc.carries.tobytes() != before[on0].tobytes()
    reps = rep1.cpu().numpy().reshape(-1).view(lsdmod.FA_CORRECT_DTYPE)
    assert (reps["flags"] == lsdmod.FA_CORRECT_APPLIED).all() and reps["slot"].tolist() == [NF[s] - 1 for s in on0]
    for s in (1, 2):
        assert after[s].tobytes() == before[s].tobytes()
    for x, y in zip(m0.counts(), m1.counts()):
        assert x.tobytes() == y.tobytes()
    # the same with robot 4 moved to map 1 in front of the call: matched and integrated by the host's record of the tick, not corrected
    fl2, m2, before2, _, _ = fleet_tick(lsdmod, ctx, log)
    assert before2.tobytes() == before.tobytes()
    fl2.assign([4], [1])
    rec2, resp2, rep2 = fl2.refine_and_integrate_last_tick(m2, 0, LOG_SEARCH, response=LOG_RESPONSE, correct=True)
    after2 = fl2.carries
    assert resp2.cpu().numpy().tobytes() == resp.cpu().numpy().tobytes()
    assert after2[[0, 3]].tobytes() == after[[0, 3]].tobytes() and after2[[1, 2, 4]].tobytes() == before[[1, 2, 4]].tobytes()
    r2 = rows(rep2, 1)
    assert r2[[0, 3]].tobytes() == rows(rep, 1)[[0, 3]].tobytes() and not r2[[1, 2, 4]].any()
    # correct_last_tick on its own, with the key of map 0: robot 4, back on the map, is corrected now; the others have moved on
    fl2.assign([4], [0])
    rep3 = rows(fl2.correct_last_tick(resp2, 0), 1).reshape(-1).view(lsdmod.FA_CORRECT_DTYPE)
    assert rep3["flags"].tolist() == [lsdmod.FA_CORRECT_STALE, 0, 0, lsdmod.FA_CORRECT_STALE, lsdmod.FA_CORRECT_APPLIED]
    assert fl2.carries.tobytes() == after.tobytes()


# ---- 5. nothing waits ------------------------------------------------------------------------------------------------------------------------
def test_correct_does_not_synchronise(lsdmod, ctx, log):
    import torch
    loc = lsdmod.Localizer(log.mc, log.ml, log.mp, 1, odom0=log.odom[0], ctx=ctx)
    m = log.mapper(lsdmod, ctx)
    maps, lid, odom = fleet_site(lsdmod, ctx, log)
    fl = lsdmod.FleetLocalizer(maps, MAP_OF, odom0=odom[:, 0], ctx=ctx)
    d_lid, d_od, d_fl, d_fo = dev(log.lid[None, :4]), dev(log.odom[None, 1:5]), dev(lid[:, :4]), dev(odom[:, 1:5])
    kw = dict(response=LOG_RESPONSE, correct=True)
    d_cy, d_rp = dev(np.zeros(768, np.uint8)), dev(np.zeros(48, np.uint8))
    d_po, d_re = dev(np.zeros(24, np.uint8)), dev(np.zeros(192, np.uint8))
    raw = lambda: ctx.enqueue_fa_carry_correct_device(d_cy.data_ptr(), 1, 1, d_po.data_ptr(), 24, d_re.data_ptr(), None, 0, None, d_rp.data_ptr(), stream())
    loc.step_device(d_lid, d_od)                                                       # warm: every staging and workspace has its size
    _, resp, _ = loc.refine_and_integrate_last_tick(m, LOG_SEARCH, **kw)
    loc.correct_last_tick(resp)
    fl.step_device(d_fl, d_fo)
    _, resp, _ = fl.refine_and_integrate_last_tick(m, 0, LOG_SEARCH, **kw)
    fl.correct_last_tick(resp, 0)
    raw()
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
    _, resp, rep = loc.refine_and_integrate_last_tick(m, LOG_SEARCH, **kw)
    rep2 = loc.correct_last_tick(resp)
    fl.step_device(d_fl, d_fo)
    _, resp3, rep3 = fl.refine_and_integrate_last_tick(m, 0, LOG_SEARCH, **kw)
    rep4 = fl.correct_last_tick(resp3, 0)
    raw()
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "a call of the correction returned only after the work in front of it had finished"
