"""The matching campaign (tests/grid_match_cases.py) under the restatement alone: every class of both rules is reached by at least three
cases, the lookup plane against a second, gathering formulation, the winner's order on hand-made score tables, and the recovery of known
displacements in a room the restatement integrated itself.  No GPU."""
import numpy as np
import pytest

import grid_cases as gc
import grid_match_cases as gm


PINNED_PRIOR = [9160, 9471, 8673]          # S at the zero offset of the three room scans displaced by (2, -1) cells and one step


@pytest.fixture(scope="module")
def like_traced():
    out = []
    for case in gm.like_campaign():
        corr = gm.likelihood(case["pass"], case["hit"], case["min_pass"], case["occ_num"], case["occ_den"], case["radius"], case["w"])
        out.append((case, corr, gm.like_classes_of(case)))
    return out


@pytest.fixture(scope="module")
def match_traced(oracle):
    out = []
    for case in gm.match_campaign():
        rec, trace = gm.run_match_case(case)
        out.append((case, rec, trace, gm.match_classes_of(case, trace) | gm.window_classes(case, trace)))
    return out


def test_every_likelihood_class_is_reached(like_traced):
    count = {c: 0 for c in gm.LIKE_CLASSES}
    for case, corr, classes in like_traced:
        assert classes <= set(gm.LIKE_CLASSES)
        assert (case["cols"] <= gc.MAX_COLS and case["rows"] <= gc.MAX_ROWS) or "grid_1x257" in classes
        for c in classes:
            count[c] += 1
    for c, n in count.items():
        assert n >= 3, (c, n)


def test_likelihood_is_the_gathered_maximum(like_traced):
    """The definition read the other way round: every cell gathers over its own window; and occupied() is the publish rule's 100."""
    for case, corr, _ in like_traced:
        occ = gm.occupied(case["pass"], case["hit"], case["min_pass"], case["occ_num"], case["occ_den"])
        assert np.array_equal(occ, gc.publish(case["pass"], case["hit"], case["min_pass"], case["occ_num"], case["occ_den"]) == 100), case["name"]
        r, w = case["radius"], case["w"]
        rows, cols = occ.shape
        want = np.zeros_like(corr)
        for y in range(rows):
            for x in range(cols):
                best = 0
                for v in range(-r, r + 1):
                    for u in range(-r, r + 1):
                        if 0 <= y + v < rows and 0 <= x + u < cols and occ[y + v, x + u]:
                            best = max(best, int(w[abs(v), abs(u)]))
                want[y, x] = best
        assert np.array_equal(corr, want), case["name"]
        assert corr.dtype == np.uint8 and (corr[occ] == w[0, 0]).sum() >= 0


def test_likelihood_radius_zero_and_products_beyond_32_bits():
    u = lambda *v: np.array([v], np.uint32)
    w = gm.table(0, lambda a, b: 77)
    assert gm.likelihood(u(1, 2, 20, 20), u(1, 2, 1, 2), 2, 1, 10, 0, w).tolist() == [[0, 77, 0, 77]]
    big = 0xFFFFFFFF
    assert gm.likelihood(u(big, big, 1 << 31, 1 << 31), u(429496729, 429496730, 1 << 30, (1 << 30) - 1), 2, 1, 10, 0, w).tolist() == [[0, 77, 77, 77]]
    assert gm.likelihood(u(1 << 31, 1 << 31), u(1 << 30, (1 << 30) - 1), 2, 1, 2, 0, w).tolist() == [[77, 0]]


def test_every_match_class_is_reached(match_traced):
    count = {c: 0 for c in gm.MATCH_CLASSES}
    for case, rec, trace, classes in match_traced:
        assert classes <= set(gm.MATCH_CLASSES), classes - set(gm.MATCH_CLASSES)
        assert case["cols"] <= gc.MAX_COLS and case["rows"] <= gc.MAX_ROWS
        for c in classes:
            count[c] += 1
    for c, n in count.items():
        assert n >= (1 if c == "nb_1025" else 3), (c, n)
    assert sum(1 for case, _, _, _ in match_traced if case["capacity"] > 1024) == 1          # the 1025 case runs once, at a raised capacity


def test_records_are_what_the_rule_says(match_traced):
    """Every record against its trace, field by field; a skipped scan's record is its pose and the flag."""
    for case, rec, trace, _ in match_traced:
        se = case["search"]
        for t in trace:
            r, pose = rec[t["scan"]], case["poses"][t["scan"]]
            if t["skip"]:
                assert r["flags"] == gm.SKIPPED and r.tobytes()[:24] == pose.tobytes() and r.tobytes()[24:44] == bytes(20) and r.tobytes()[48:] == bytes(8)
                continue
            a, j, i = t["winner"]
            S = t["S"][a][j + se["wy"], i + se["wx"]]
            assert (r["score"], r["n_beams"], r["di"], r["dj"], r["da"], r["reserved"]) == (S, t["nb"][a], i, j, a, 0)
            assert r["score"] == max(s.max() for s in t["S"].values()) and r["score_prior"] == t["S"][0][se["wy"], se["wx"]]
            assert r["score"] <= 255 * r["n_beams"] and r["score_prior"] <= r["score"]
            ok = r["n_beams"] >= se["min_beams"] and int(r["score"]) * se["min_den"] >= 255 * int(r["n_beams"]) * se["min_num"]
            assert r["flags"] == (gm.ACCEPTED if ok else 0)
            if ok:
                assert (r["x"], r["y"], r["ang"]) == (pose[0] + i, pose[1] + j, pose[2] + a * se["ang_step"])
            else:
                assert r.tobytes()[:24] == pose.tobytes()


def test_the_order_of_the_winner(match_traced):
    by = {case["name"]: rec for case, rec, _, _ in match_traced}
    for v in range(3):
        assert tuple(by["uniform_%d" % v][0][["di", "dj", "da"]]) == (0, 0, 0)
        assert tuple(by["mirror_%d" % v][0][["di", "dj", "da"]]) == (-2, 0, 0)             # i = -2 and i = +2 tie: the smaller index
        assert tuple(by["nearer_%d" % v][0][["di", "dj", "da"]])[2] == 0 and by["nearer_%d" % v][0]["di"] ** 2 + by["nearer_%d" % v][0]["dj"] ** 2 == (1, 1, 4)[v]
        assert tuple(by["angle_tie_%d" % v][0][["di", "dj", "da"]]) == (0, 0, 0)           # a = -1, 0, +1 tie: |a| = 0
        assert tuple(by["angle_mirror_%d" % v][0][["di", "dj", "da"]]) == (0, 0, -1)       # a = -1 and a = +1 tie: the smaller index
        assert [int(by["accept%+d_%d" % (d, v)][0]["flags"]) for d in (-1, 0, 1)] == [0, 1, 1]
        assert by["min_beams_%d" % v]["flags"].tolist() == [1, 0] and by["min_beams_%d" % v]["n_beams"].tolist() == [3, 2]


def test_recovery_of_known_displacements(oracle):
    """A room integrated by the restatement at the true poses; poses displaced by whole cells and whole angle steps come back exactly."""
    corr, scans, lens, truth = gm.recovery()
    se = gm.RECOVERY_SEARCH
    assert (corr == 255).sum() > 100
    for dx, dy, k in gm.RECOVERY_OFFSETS:
        moved = truth + np.array([dx, dy, k * se["ang_step"]])
        rec = gm.match(scans, lens, moved, gm.ROOM["resol"], gm.ROOM["range_max"], corr, se)
        for n in range(len(truth)):
            assert (rec[n]["di"], rec[n]["dj"], rec[n]["da"], rec[n]["flags"]) == (-dx, -dy, -k, gm.ACCEPTED), (dx, dy, k, n, rec[n])
            assert rec[n]["score"] == 255 * rec[n]["n_beams"] and rec[n]["n_beams"] == scans.shape[1]
            assert (rec[n]["x"], rec[n]["y"], rec[n]["ang"]) == tuple(truth[n])
            assert rec[n]["score_prior"] < rec[n]["score"] or (dx, dy, k) == (0, 0, 0)
    # pinned: what the restatement gives for the first displacement
    rec = gm.match(scans, lens, truth + np.array([2, -1, 2.0]), gm.ROOM["resol"], gm.ROOM["range_max"], corr, se)
    assert rec["score"].tolist() == [22950, 22950, 22950] and rec["n_beams"].tolist() == [90, 90, 90]
    assert rec["score_prior"].tolist() == PINNED_PRIOR
