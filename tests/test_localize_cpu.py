"""FeatureAssociation's restatement (tests/fa_restatement.py) on its own, without a GPU: the branches on hand-made candidate lists,
the sigma points against an independent numpy form, the LLT's failure path, the odometry fixture, and a replay of the data/ log
with the oracle's glibc scores against its correctly rounded ones."""
import math
import os

import numpy as np
import pytest

import fa_restatement as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def spd(seed=5):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(9, 9))
    return A @ A.T + 9 * np.eye(9)


def test_reset_branch():
    x, P, rep = fr.feature_association([(1.0, 2.0, 3.0, 3.0), (1.0, 2.0, 3.0, INF)], (10.0, 10.0, 0.0), (0, 0, 0), [5.0] * 9, spd().tolist())
    rx, rP = fr.reset_state()
    assert rep["branch"] == fr.RESET and rep["n_kept"] == 0 and x == rx and P == rP and rep["score"] == INF


INF = float("inf")


def test_first_frame_branch_takes_the_best_candidate_and_keeps_P():
    P = spd().tolist()
    cands = [(1.0, 1.0, 1.0, 2.5), (7.0, 8.0, 9.0, 0.5), (3.0, 3.0, 3.0, 0.5)]
    x, Po, rep = fr.feature_association(cands, (-1.0, -1.0, 0.0), (4.0, 4.0, 4.0), list(range(9)), P)
    assert rep["branch"] == fr.FIRST and x[:3] == [7.0, 8.0, 9.0] and x[3:] == list(range(3, 9)) and Po == P
    assert rep["score"] == 0.5                           # the first of two equal scores: stable order


def test_fusion_in_stable_sorted_order():
    cands = [(5.0, 0.0, 10.0, 2.0), (1e16, 3.0, 1.0, 1.0), (7.0, 0.0, 2.0, 3.0), (1.0, 5.0, 3.0, 1.0), (-1e16, 1.0, 4.0, 1.0)]
    kept = fr.keep_sorted(cands)
    assert kept == [cands[1], cands[3], cands[4], cands[0]]              # ties in input order, score 3 dropped
    sx = sw = 0.0
    for c in kept:
        w = 1 / (c[3] * c[3]); sx += c[0] * w; sw += w
    x, P, rep = fr.feature_association(cands, (5.0, 5.0, 0.0), (0, 0, 0), [0.0] * 9, spd().tolist())
    assert rep["branch"] == fr.UKF and rep["estimate"][0] == sx / sw and rep["n_kept"] == 4
    alt = 0.0                                                             # another order of the ties gives another sum
    for c in [cands[1], cands[4], cands[3], cands[0]]:
        alt += c[0] * (1 / (c[3] * c[3]))
    assert alt != sx


def test_angles_are_averaged_without_wrapping():
    x, P, rep = fr.feature_association([(0.0, 0.0, 179.0, 1.0), (0.0, 0.0, -179.0, 1.0)], (3.0, 3.0, 0.0), (0, 0, 0), [0.0] * 9,
                                       fr.reset_state()[1])
    assert rep["estimate"][2] == 0.0


def test_score_zero_makes_the_state_nan():
    x, P, rep = fr.feature_association([(2.0, 2.0, 1.0, 0.0)], (3.0, 3.0, 0.0), (0, 0, 0), [0.0] * 9, fr.reset_state()[1])
    assert math.isnan(rep["estimate"][0]) and all(math.isnan(v) for v in x[:3])


def test_sigma_points_are_rows_of_L():
    P = spd(7)
    x = np.arange(9, dtype=float) * 0.5
    X, k = fr.sigma_points(list(x), P.tolist())
    assert k == -1
    L = np.linalg.cholesky(P)
    c = math.sqrt(9 + (1e-2 * 1e-2 * 9 - 9))
    X = np.array(X)
    for j in range(9):
        np.testing.assert_allclose(X[:, j + 1], x + c * L[j, :], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(X[:, j + 10], x - c * L[j, :], rtol=1e-12, atol=1e-12)
    assert not np.allclose(X[:, 1], x + c * L[:, 0])     # (columns would be the textbook form)


def test_llt_stops_at_the_first_non_positive_pivot():
    P = spd(3)
    P[4, :] *= 1e-9; P[:, 4] *= 1e-9
    P[4, 4] = -1.0
    m, k = fr.llt(P.tolist())
    assert k == 4
    Lk = np.tril(np.array(m))[:, :4]                                       # columns < 4 factored: L[:, :4] L[:4, :4]^T = P[:, :4]
    np.testing.assert_allclose(Lk @ Lk[:4].T, P[:, :4], rtol=1e-12, atol=1e-12)
    assert np.array_equal(np.triu(np.array(m), 1), np.triu(P, 1))            # the upper triangle is never touched
    assert np.array_equal(np.tril(np.array(m)[:, 4:]), np.tril(P[:, 4:]))
    x, Po, kk = fr.ukf([0.0] * 9, P.tolist(), (0, 0, 0), (1.0, 1.0, 1.0))
    assert kk == 4


@pytest.mark.parametrize("name", fr.LOGS)
def test_log_fixtures(name):
    m, mp, lid, odom = fr.load_log(name)
    n = fr.LOG_FRAMES[name]
    z = np.load(os.path.join(GOLDEN, "localize_%s.npz" % name))
    assert int(z["n_frames"]) == n and lid.shape == (n, 360, 2) and odom.shape == (n + 1, 3)
    assert odom[0, 0] == 0 and np.array_equal(odom[-1], odom[-2]) and np.array_equal(odom[1:n], z["odom_raw"][1:])
    assert m.shape == (int(mp[1]), int(mp[0])) and mp[2] == 0.025
    if name != "data":
        assert fr.log_lidar(z).shape[0] == n + 1               # one lidar frame more than the driver replays (:183)


def replay(oracle, lsdmod, name, _lib):
    m, mp, lid, odom = fr.load_log(name)
    mc = oracle.map_cache(m.copy(), mp[2])
    ml = oracle.lsd(m.copy())["lines"]
    scans, lens = lsdmod.lidar_frames(lid)
    loop = fr.Loop(odom, mp[2])
    out = []
    for t in range(len(scans)):
        fs = oracle.feature_scan(scans[t, :lens[t]], mp)
        sp = loop.scan_pose(t)
        lp = loop.lidar_pose(fs["lidar_pos"])
        last = loop.last_pose()
        pr = np.array(fr.pairs(ml["len"], fs["lines"]["len"]), np.int32).reshape(-1, 2)
        cands = oracle.scan_to_map_match(mc, ml, fs["lines"], fs["pts"], lp, last, pr, _lib=_lib).reshape(-1, 4) if len(pr) else np.zeros((0, 4))
        x, P, rep = fr.feature_association(cands, last, sp, loop.x, loop.P, len(pr))
        loop.finish(t, x, P)
        out.append((x, rep, fr.keep_sorted(cands)))
    return out


@pytest.mark.parametrize("name", fr.LOGS)
def test_replay_glibc_scores_against_correctly_rounded_ones(name, oracle, lsdmod):
    a = replay(oracle, lsdmod, name, None)
    b = replay(oracle, lsdmod, name, oracle.lib_cr())
    branches = [r["branch"] for _, r, _ in a]
    assert branches.count(fr.UKF) > len(a) // 2
    for t, ((xa, ra, ka), (xb, rb, kb)) in enumerate(zip(a, b)):
        assert ra["branch"] == rb["branch"] and ra["n_kept"] == rb["n_kept"], t
        ka, kb = np.array(ka).reshape(-1, 4), np.array(kb).reshape(-1, 4)
        assert np.allclose(ka, kb, rtol=0, atol=1e-9), t          # the same kept candidates, in the same sorted order
        assert np.allclose(xa, xb, rtol=0, atol=1e-6, equal_nan=True), (t, xa[:3], xb[:3])
