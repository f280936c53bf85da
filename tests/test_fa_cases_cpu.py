"""The fusion campaign (tests/fa_cases.py) under the restatement alone: every group reaches the boundary it was built for.  This is the
guard against a campaign that silently tests nothing; tests/test_fa_cases_gpu.py runs the same cases on the device."""
import math

import numpy as np
import pytest

import fa_cases as fc
import fa_restatement as fr


def run(c):
    cands, last, sp, x, P = c
    return fr.feature_association(cands.tolist(), last, sp, list(x), P.tolist())


@pytest.fixture(scope="module")
def results():
    return {g: {name: (c, run(c)) for name, c in fc.cases(g)} for g in fc.GROUPS}


def isnan_state(x):
    return any(math.isnan(v) for v in x)


def test_campaign_is_small_and_deterministic():
    total = sum(len(fc.cases(g)) for g in fc.GROUPS)
    assert 80 <= total <= 400
    for g in fc.GROUPS:
        for (na, a), (nb, b) in zip(fc.cases(g), fc.cases(g)):
            assert na == nb and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def test_counts_reach_every_pair(results):
    want = {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1300}
    assert set(fc.BOUNDARY) == want
    seen = set()
    for name, (c, (x, P, rep)) in results["counts"].items():
        n, k = len(c[0]), rep["n_kept"]
        seen.add((n, k))
        assert rep["branch"] == fr.UKF and rep["llt"] == -1 and not isnan_state(x), name
        if n > k:
            sc = c[0][:, 3]
            dropped = sc[~(sc < 3)]
            if n - k >= 4:
                assert (dropped == 3.0).any() and (dropped == 3.5).any() and np.isinf(dropped).any() and np.isnan(dropped).any(), name
            pos = np.flatnonzero(sc < 3)
            if k >= 256:                                     # kept and dropped positions in every whole wavefront of every round
                full = set(range(n // 64))
                assert full <= set(pos // 64) and full <= set(np.flatnonzero(~(sc < 3)) // 64), name
                assert (pos != np.arange(k)).any()
    assert {(n, n) for n in want} <= seen
    assert {k for n, k in seen if n > k} == want and all(abs(n - 1.5 * k) <= 1 for n, k in seen if n > k)
    assert set(fc.LDS_RERUNS) == {257, 1024} and all(v == (k, k - 1) for k, v in fc.LDS_RERUNS.items())
    assert all(sum(1 for n, kk in seen if kk == k) == 2 for k in fc.LDS_RERUNS)


def test_ties_cross_rounds_and_their_order_shows(results):
    assert set(results["ties"]) == {"one_score", "two_scores", "round_apart"}
    for name, (c, (x, P, rep)) in results["ties"].items():
        assert rep["n_kept"] == 700 and rep["branch"] == fr.UKF, name
        assert fc.order_matters(c), name                     # another order of the equal scores gives another sum
    sc = results["ties"]["one_score"][0][0][:, 3]
    assert len(set(sc)) == 1
    sc = results["ties"]["two_scores"][0][0][:, 3]
    assert len(set(sc)) == 2 and (sc[::2] == sc[0]).all() and (sc[1::2] == sc[1]).all()
    sc = results["ties"]["round_apart"][0][0][:, 3]
    assert len(set(sc[:256])) == 256 and np.array_equal(sc[256:512], sc[:256]) and np.array_equal(sc[512:], sc[:700 - 512])


KEPT = {"below3": True, "3": False, "above3": False, "nan": False, "neg0": True, "neg1": True, "neginf": True, "denorm": True,
        "1e-200": True, "1e200": False, "neg1e200": True}
NAN_ALONE = {"neg0", "neginf", "denorm", "1e-200", "neg1e200"}         # 1 / (s * s) is inf or 0: the weighted mean is inf / inf or 0 / 0


def test_keep_edges(results):
    assert math.nextafter(3.0, 0.0) < 3.0 < math.nextafter(3.0, math.inf) and 5e-324 * 5e-324 == 0 and 5e-324 > 0
    assert {n for n, _ in fc.KEEP_EDGES} == set(KEPT)
    for name, kept in KEPT.items():
        c, (x, P, rep) = results["keep_edges"][name + "_alone"]
        assert rep["n_kept"] == int(kept) and rep["branch"] == (fr.UKF if kept else fr.RESET), name
        if kept:
            assert isnan_state(x) == (name in NAN_ALONE), name
        c, (x, P, rep) = results["keep_edges"][name + "_mixed"]
        assert len(c[0]) == 9 and rep["n_kept"] == 8 + int(kept) and rep["branch"] == fr.UKF, name
    x = results["keep_edges"]["neg1e200_mixed"][1][0]
    assert not isnan_state(x)                                # a weight of 0 among ordinary ones
    x = results["keep_edges"]["denorm_mixed"][1][0]
    assert isnan_state(x)                                    # a weight of inf


def test_first_edges_take_both_branches_on_either_side(results):
    (hi_in, hi_out), (lo_in, lo_out) = fc.first_thresholds()
    assert lo_out < lo_in < -1.0 < hi_in < hi_out
    assert math.nextafter(hi_in, math.inf) == hi_out and math.nextafter(lo_in, -math.inf) == lo_out
    assert abs(hi_in + 1) < 0.0001 and abs(lo_in + 1) < 0.0001 and not abs(hi_out + 1) < 0.0001 and not abs(lo_out + 1) < 0.0001
    want = dict(minus1=fr.FIRST, hi_inner=fr.FIRST, hi_outer=fr.UKF, lo_inner=fr.FIRST, lo_outer=fr.UKF, nan=fr.UKF)
    for name, branch in want.items():
        c, (x, P, rep) = results["first_edges"][name]
        assert rep["branch"] == branch and rep["n_kept"] == 2, name
        assert math.isnan(c[1][0]) == (name == "nan")
        if branch == fr.FIRST:
            assert x[:3] == [11.0, 19.0, 29.0] and rep["score"] == 1.25       # the better candidate is the second


def test_llt_fails_at_every_column_and_through_a_zero_pivot(results):
    seen = set()
    for k in range(9):
        for kind in ("negative", "zero"):
            c, (x, P, rep) = results["llt"]["%s_%d" % (kind, k)]
            assert rep["llt"] == k, (kind, k)
            m, kk = fr.llt(c[4].tolist())
            pivot = m[k][k] - math.fsum(m[k][j] * m[k][j] for j in range(k))
            assert kk == k and (pivot == 0 if kind == "zero" else pivot < 0), (kind, k, pivot)
            seen.add(k)
    for k in (0, 4, 8):
        c, (x, P, rep) = results["llt"]["nan_%d" % k]
        assert rep["llt"] == -1 and isnan_state(x) and math.isnan(c[4][k, k])          # a NaN pivot is not <= 0: "success"
    for name in ("reset_P", "exact_P", "garbage_upper", "scaled_1e-300", "scaled_1e300"):
        assert results["llt"][name][1][2]["llt"] == -1, name
        seen.add(-1)
    assert seen == set(range(-1, 9))
    c, (x, P, rep) = results["llt"]["garbage_upper"]
    assert np.isnan(c[4][0, 8]) and not np.array_equal(np.triu(c[4], 1), np.tril(c[4], -1).T)
    clean = np.tril(c[4]) + np.tril(c[4], -1).T
    x2, P2, _ = run((c[0], c[1], c[2], c[3], clean))
    assert x == x2 and P == P2 and not isnan_state(x)        # only the lower triangle is read
    assert not isnan_state(results["llt"]["scaled_1e-300"][1][0])


def test_state_edges(results):
    r = results["state_edges"]
    assert not isnan_state(r["x_1e6"][1][0]) and max(abs(v) for v in r["x_1e6"][1][0]) > 1e5
    assert not isnan_state(r["angles"][1][0]) and abs(r["angles"][1][2]["estimate"][2]) > 360
    assert isnan_state(r["nan_scan_pose"][1][0]) and r["nan_scan_pose"][1][2]["branch"] == fr.UKF
    assert r["inf_pose"][1][2]["estimate"][0] == math.inf
    assert math.isnan(r["inf_both_signs"][1][2]["estimate"][0]) and r["inf_both_signs"][1][2]["estimate"][2] == -math.inf
