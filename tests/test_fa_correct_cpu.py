"""The grid match response fused into the carry, without a GPU: the restatement (tests/fa_correct_cases.py) on its own -- the campaign
reaches every class, the closed form, what an update must do to a covariance, a second formulation in exact arithmetic, the recovery of
displaced poses on the room of tests/grid_match_cases.py -- and the ABI's names and sizes."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import fa_correct_cases as fc
import fa_restatement as fr
import grid_match_cases as gm

LOG_FRAMES = 12                                 # of the `data` log, replayed with the oracle


@pytest.fixture(scope="module")
def log_states(oracle, lsdmod):
    """(x, P rows) after each of the data log's first frames that holds a pose: the oracle's FeatureScan and scores, then the restatement."""
    m, mp, lid, odom = fr.load_log("data")
    mc = oracle.map_cache(m.copy(), mp[2])
    ml = oracle.lsd(m.copy())["lines"]
    scans, lens = lsdmod.lidar_frames(lid[:LOG_FRAMES])
    loop, out = fr.Loop(odom, mp[2]), []
    for t in range(LOG_FRAMES):
        fs = oracle.feature_scan(scans[t, :lens[t]], mp)
        sp, lp, last = loop.scan_pose(t), loop.lidar_pose(fs["lidar_pos"]), loop.last_pose()
        pr = np.array(fr.pairs(ml["len"], fs["lines"]["len"]), np.int32).reshape(-1, 2)
        cands = oracle.scan_to_map_match(mc, ml, fs["lines"], fs["pts"], lp, last, pr).reshape(-1, 4) if len(pr) else np.zeros((0, 4))
        x, P, rep = fr.feature_association(cands, last, sp, loop.x, loop.P, len(pr))
        loop.finish(t, x, P)
        if rep["branch"] == fr.UKF:
            out.append((x, P))
    assert len(out) >= 3
    return out


@pytest.fixture(scope="module")
def runs(log_states):
    """(unit, trace, carry after, report) of every unit of the campaign: the restatement, computed once."""
    out = []
    for u in fc.campaign(log_states):
        tr = {}
        after, rep = fc.run_unit(u, tr)
        out.append((u, tr, after, rep))
    return out


def applied(runs):
    return [(u, tr, after, rep) for u, tr, after, rep in runs if rep is not None and rep["flags"] == fc.APPLIED]


def test_campaign_reaches_every_class(runs):
    count = {c: 0 for c in fc.CLASSES}
    for u, tr, _, rep in runs:
        for c in fc.classes_of(u, tr, rep):
            count[c] += 1
    assert {c: n for c, n in count.items() if n < 3} == {}
    assert len({u["name"] for u, _, _, _ in runs}) == len(runs)
    sizes = sorted({len(b["units"]) for b in fc.batches([u for u, _, _, _ in runs])})
    assert {1, 2, 3, 65} <= set(sizes)


def test_one_flag_and_untouched_bytes(runs):
    """Each outcome is exactly one flag; the carry keeps every byte unless it is APPLIED, and then everything but the state does; report
    fields that were not computed are +0.0 and the slot -1."""
    zero = np.zeros(1).tobytes()
    for u, tr, after, rep in runs:
        if rep is None:
            assert after.tobytes() == u["carry"].tobytes()
            continue
        fl = int(rep["flags"])
        assert fl in fc.FLAG_NAMES, u["name"]
        assert after.tobytes()[720:] == u["carry"].tobytes()[720:]
        assert (after.tobytes() == u["carry"].tobytes()) == (fl != fc.APPLIED), u["name"]
        if fl in (fc.NO_POSE, fc.STALE) or (fl == fc.NOT_FINITE and tr["resp_flags"] is None):
            assert rep["slot"] == -1 and rep.tobytes()[:40] == zero * 5, u["name"]
        else:
            assert 0 <= rep["slot"] < len(u["poses"]) and rep["slot"] == tr["hits"][-1]
        if fl in (fc.NO_RESPONSE, fc.NOT_FINITE):
            assert rep.tobytes()[:40] == zero * 5
        if fl == fc.SINGULAR:
            assert rep.tobytes()[:32] == zero * 4 and not rep["det"] > 0
        if fl == fc.GATED:
            assert not rep["d2"] <= u["par"][3] and u["par"][3] > 0


def test_sentinel_and_gate_edges(runs):
    by = {u["name"]: rep for u, _, _, rep in runs}
    for k in range(3):
        assert by["sentinel_in_lo_%d" % k]["flags"] == by["sentinel_in_hi_%d" % k]["flags"] == fc.NO_POSE
        assert by["sentinel_out_lo_%d" % k]["flags"] == by["sentinel_out_hi_%d" % k]["flags"] == fc.APPLIED
        assert [int(by["gate_%s_%d" % (t, k)]["flags"]) for t in ("eq", "below", "above", "wide", "tight")] == \
            [fc.APPLIED, fc.GATED, fc.APPLIED, fc.APPLIED, fc.GATED]
        assert by["zero_sign_%d" % k]["flags"] == fc.STALE and by["zero_sign_match_%d" % k]["flags"] == fc.APPLIED
        assert by["nf_cov4_other_slot_%d" % k]["flags"] == fc.APPLIED
        assert by["twice_65_%d" % k]["slot"] == (64 if k == 2 else 32)


def test_closed_form(runs):
    """P = p I, R = r I (cov 0, floors r), p = r a power of two and a dyadic pose and measurement (fa_correct_cases.POW2 says why): nothing
    rounds, so x'[q] - x[q] == innov[q] * p / (p + r) and P'(q,q) == p - p * p / (p + r) exactly, and x[3..8] are unchanged."""
    seen = 0
    for u, tr, after, rep in runs:
        if u["origin"] != "closed_form":
            continue
        seen += 1
        assert rep["flags"] == fc.APPLIED
        p, r = float(u["carry"]["state"]["P"][0]), u["par"][1]
        x, x1 = u["carry"]["state"]["x"], after["state"]["x"]
        P1 = after["state"]["P"].reshape(9, 9, order="F")
        for q in range(3):
            assert rep["innov"][q] != 0
            assert x1[q] - x[q] == rep["innov"][q] * p / (p + r)
            assert P1[q, q] == p - p * p / (p + r)
        assert x1[3:].tobytes() == x[3:].tobytes()
        off = P1 - np.diag(np.diag(P1))
        assert not off.any() and (np.diag(P1)[3:] == p).all()
    assert seen == 3


def test_covariance_stays_a_covariance(runs):
    """Every applied case whose input P passes llt and whose floors are positive: P' passes llt, and the pose variances do not grow."""
    seen = 0
    for u, tr, after, rep in applied(runs):
        _, P = fc.rows_of(u["carry"])
        if fr.llt(P)[1] != -1 or not (u["par"][1] > 0 and u["par"][2] > 0):
            continue
        seen += 1
        _, P1 = fc.rows_of(after)
        assert fr.llt(P1)[1] == -1, u["name"]
        for q in range(3):
            assert P1[q][q] <= P[q][q], (u["name"], q)
    assert seen >= 30


def test_second_formulation_in_exact_arithmetic(runs):
    """K, x' and P' once more in fractions.Fraction from the same rounded Sinv and innovation: the restatement's floats agree within the
    bound the roundings give (fa_correct_cases.exact_update states it: three rounded products and their sum per dot product, twice, and
    the last addition)."""
    seen = 0
    for u, tr, after, rep in applied(runs):
        x, P = fc.rows_of(u["carry"])
        x1, P1 = fc.rows_of(after)
        xe, Pe, bx, bP = fc.exact_update(x, P, tr["Sinv"], [float(v) for v in rep["innov"]])
        for i in range(9):
            assert abs(Fraction(x1[i]) - xe[i]) <= bx[i], (u["name"], i)
            for j in range(9):
                assert abs(Fraction(P1[i][j]) - Pe[i][j]) <= bP[i][j], (u["name"], i, j)
        seen += 1
    assert seen >= 30


def test_recovery_on_the_room(oracle):
    """Carries at the reset covariance around each of the room's three true poses, every component displaced by 1..3 (cells, cells,
    degrees; 40 draws of default_rng(1)): match, response and correction in sequence bring each of x, y and ang closer to the truth, in
    every draw."""
    corr, scans, lens, truth = gm.recovery()
    worst = 0.0
    for n, off in enumerate(fc.recovery_draws()):
        got, reps = fc.recover(corr, scans, lens, truth, off)
        assert all(o["flags"] == fc.APPLIED for o in reps), n
        before, after = np.abs(off), np.abs(got - truth)
        print("draw %d: before %s after %s" % (n, before.round(3).tolist(), after.round(3).tolist()))
        worst = max(worst, float((after / before).max()))
        assert (after < before).all(), (n, before.tolist(), after.tolist())
    print("largest after / before: %.3f" % worst)


def test_abi_names_and_sizes(lsdmod):
    assert {"lsd_enqueue_fa_carry_correct_device", "lsd_fa_carry_correct"} <= set(lsdmod.EXPORTED_SYMBOLS)
    assert C.sizeof(lsdmod.lsd_fa_correct) == 32 and lsdmod.FA_CORRECT_DTYPE.itemsize == 48 == fc.REP_DTYPE.itemsize
    assert lsdmod.FA_CORRECT_DTYPE == fc.REP_DTYPE and lsdmod.FA_CARRY_DTYPE == fc.CARRY_DTYPE
    assert [getattr(lsdmod, "FA_CORRECT_" + n.upper()) for n in ("applied", "no_pose", "not_finite", "stale", "no_response", "singular", "gated")] == \
        [1, 2, 4, 8, 16, 32, 64]
    assert (fc.APPLIED, fc.NO_POSE, fc.NOT_FINITE, fc.STALE, fc.NO_RESPONSE, fc.SINGULAR, fc.GATED) == (1, 2, 4, 8, 16, 32, 64)
    d = lsdmod.fa_correct()
    assert (d.cov_scale, d.floor_xy, d.floor_ang, d.gate) == fc.DEFAULTS == (1.0, 1.0, 1.0, 0.0)
    assert lsdmod.fa_correct(True).floor_xy == 1.0 and lsdmod.fa_correct(d) is d
    e = lsdmod.fa_correct(dict(gate=9.0, cov_scale=2.0))
    assert (e.cov_scale, e.floor_xy, e.floor_ang, e.gate) == (2.0, 1.0, 1.0, 9.0)
    assert lsdmod.fa_correct((0.0, 0.5, 0.25, 3.0)).floor_ang == 0.25 and lsdmod.fa_correct(gate=2.5).gate == 2.5
    for bad in (dict(gate=-1.0), dict(cov_scale=math.nan), dict(floor_xy=math.inf), (1.0, 1.0, -0.5, 0.0)):
        with pytest.raises(lsdmod.LsdError) as err:
            lsdmod.fa_correct(bad)
        assert err.value.status == lsdmod.LSD_ERR_INVALID
    for cls in (lsdmod.Localizer, lsdmod.FleetLocalizer):
        assert callable(cls.correct_last_tick) and callable(cls.refine_and_integrate_last_tick)
    assert callable(lsdmod.Context.enqueue_fa_carry_correct_device) and callable(lsdmod.Context.fa_carry_correct)
