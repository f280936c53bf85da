"""The reduce of the pose graph (include/lsd_hip.h: lsd_enqueue_pg_reduce_device) on its restatement,
tests/pose_graph_reduce_cases.py: the campaign reaches its classes, what is retired leaves the marginal of what stays, a second reduce
retires nothing, and the two laps of 8.1.18 lose their redundant keyframes without losing accuracy.  No GPU."""
import math
import os
import re

import numpy as np

import pose_graph_cases as pg
import pose_graph_loops_cases as pl
import pose_graph_marginal_cases as mc
import pose_graph_reduce_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Property (a), measured on the campaign's well-posed class (test_marginal_is_kept prints both): the largest difference between a surviving
# node's marginal covariance in the reduced and in the full graph (numpy's dense inverse), relative to the block's largest entry, was
# 1.63e-14 (run_11_1); the largest move of a surviving node under the relaxation of the reduced graph was 1.42e-14 pixels / degrees
# (beams_360_0).  Ten times that, as DESIGN.md 8.1.15 did for the relaxation.
COV_MEASURED, MOVE_MEASURED = 1.63e-14, 1.42e-14
COV_BOUND, MOVE_BOUND = 10 * COV_MEASURED, 10 * MOVE_MEASURED
# Property (c), measured on the restatement: the mean keyframe error of the surviving nodes against the ground truth is 0.656769 pixels in
# the full graph and 0.656509 after reduce + relaxation, a difference of -2.6e-4; the margin is ten times its size.
E2E_FULL, E2E_REDUCED = 0.656769, 0.656509
E2E_MARGIN = 10 * abs(E2E_REDUCED - E2E_FULL)


def same(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def counts(g):
    return int(g["head"][0]["n_nodes"]), int(g["head"][0]["n_edges"])


# ---- 1. the campaign ---------------------------------------------------------------------------------------------------------------------
def test_campaign_reaches_every_class_three_times():
    seen = {c: 0 for c in rc.CLASSES}
    cases = rc.campaign()
    assert 90 <= len(cases) <= 130 and len(set(c["name"] for c in cases)) == len(cases)
    for case in cases:
        tr = rc.run_case(case)[4]
        got = rc.classes_of(case, tr)
        assert got <= set(rc.CLASSES), got - set(rc.CLASSES)
        for c in got:
            seen[c] += 1
    assert not {c: n for c, n in seen.items() if n < 3}, seen


def test_records_have_the_headers_sizes():
    text = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name, dtype in (("lsd_pg_reduce_par", rc.PAR_DTYPE), ("lsd_pg_reduce_rep", rc.REP_DTYPE)):
        assert dtype.itemsize == rc.SIZES[name]
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, dtype.itemsize), text) or re.search(
            r"typedef struct %s \{\s*/\* %d bytes \*/" % (name, dtype.itemsize), text), name
    assert re.search(r"#define LSD_PG_EDGE_CONTRACTED %du" % rc.EDGE_CONTRACTED, text)


def test_outputs_hold_together():
    """What the rule promises about its own outputs, on every case: the map is a monotone injection onto 0..n-1, records move whole, what
    lies behind the counts keeps its bytes, lengths and descriptors behind the new count are empty, no surviving edge names a retired
    node, and a case that retires nothing changes no byte but the map and the report."""
    for case in rc.campaign():
        g0, d0 = case["g"], case["desc"]
        g, d, new, rep, tr = rc.run_case(case)
        N, E = tr["N"], tr["E"]
        n, e = counts(g)
        kept = [k for k in range(N) if new[k] >= 0]
        assert [int(new[k]) for k in kept] == list(range(n)) and (new[N:] == -1).all() and n == N - int(rep["retired"]), case["name"]
        for k in kept:
            q = int(new[k])
            assert same(g["nodes"][q], g0["nodes"][k]) and same(g["store"][q], g0["store"][k]) and g["store_lens"][q] == g0["store_lens"][k]
            assert d is None or same(d[q], d0[k])
        assert same(g["nodes"][n:], g0["nodes"][n:]) and same(g["store"][n:], g0["store"][n:]) and same(g["edges"][e:], g0["edges"][e:])
        assert not g["store_lens"][n:N].any() and same(g["store_lens"][N:], g0["store_lens"][N:])
        assert d is None or (not d[n:N].view(np.uint8).any() and same(d[N:], d0[N:]))
        for ed in g["edges"][:e]:
            i, j = int(ed["i"]), int(ed["j"])
            if int(ed["flags"]) == rc.EDGE_CONTRACTED:
                assert 0 <= i < n and 0 <= j < n and i != j and float(ed["chi2"]) == 0.0
        assert e == E - int(rep["retired"]) - int(rep["dropped_edges"]), case["name"]
        for t0, t1 in zip(g0["tracks"], g["tracks"]):
            last = int(t0["last"])
            assert int(t1["last"]) == (int(new[last]) if 0 <= last < N else last) and int(t1["last"]) != -1 or last == -1
            assert same(t1["raw"], t0["raw"]) and t1["reserved"] == t0["reserved"]
        if not int(rep["retired"]):
            assert all(same(g[key], g0[key]) for key in g0) and (d is None or same(d, d0)), case["name"]
            assert int(rep["flags"]) & rc.RETIRED == 0


def test_runs_respect_max_run_and_the_anchors():
    for case in rc.campaign():
        g, d, new, rep, tr = rc.run_case(case)
        assert all(r["len"] <= case["par"]["max_run"] for r in tr["runs"])
        assert int(rep["longest_run"]) <= case["par"]["max_run"]
        nd, lasts = case["g"]["nodes"], set(int(t["last"]) for t in case["g"]["tracks"])
        for k in range(tr["N"]):
            if tr["retired"][k]:
                assert not int(nd[k]["flags"]) & pg.NODE_FIXED and k not in lasts and tr["redundant"][k]


# ---- 2. (a) the marginal is kept -------------------------------------------------------------------------------------------------------------
def test_marginal_is_kept():
    worst_cov, worst_move, retired = (0.0, ""), (0.0, ""), 0
    for case in rc.campaign():
        if not case["well_posed"]:
            continue
        g0 = case["g"]
        N, E = counts(g0)
        g, _, new, rep, _ = rc.run_case(case)
        n, e = counts(g)
        retired += int(rep["retired"])
        full, _ = mc.dense_inverse(g0["nodes"][:N], g0["edges"][:E])
        red, _ = mc.dense_inverse(g["nodes"][:n], g["edges"][:e])
        for k in range(N):
            q = int(new[k])
            if q < 0:
                continue
            A, B = full[3 * k:3 * k + 3, 3 * k:3 * k + 3], red[3 * q:3 * q + 3, 3 * q:3 * q + 3]
            if np.abs(A).max() > 0:
                worst_cov = max(worst_cov, (float(np.abs(A - B).max() / np.abs(A).max()), case["name"]))
        nodes, _, rrep = pg.relax(g["nodes"][:n], g["edges"][:e], dict(pg.RELAX_DEFAULTS))
        assert float(rrep["chi2_before"]) < 1e-20, case["name"]                 # consistent: nothing to redistribute
        for k in range(n):
            move = max(abs(float(nodes[k][f]) - float(g["nodes"][k][f])) for f in ("x", "y", "ang"))
            worst_move = max(worst_move, (move, case["name"]))
    print("marginal kept: covariance %.3g (%s), move %.3g (%s), %d nodes retired" % (worst_cov + worst_move + (retired,)))
    assert retired >= 100
    assert worst_cov[0] <= COV_BOUND, worst_cov
    assert worst_move[0] <= MOVE_BOUND, worst_move


# ---- 3. (b) stable ---------------------------------------------------------------------------------------------------------------------------
def test_second_reduce_retires_nothing():
    """A second reduce with the same parameters changes no byte.  The one exception follows from the rule itself: a node that max_run
    un-marked (the report says SPLIT) is still redundant and removable, so the next call retires it -- it, and nothing else --, and the
    calls reach a fixed point."""
    split = 0
    for case in rc.campaign():
        g, d, new, rep, tr = rc.run_case(case)
        tr2 = {}
        g2, d2, new2, rep2 = rc.reduce(g, d, case["par"], tr2)
        n = counts(g)[0]
        if not int(rep["flags"]) & rc.SPLIT:
            assert int(rep2["retired"]) == 0 and int(rep2["runs"]) == 0 and int(rep2["flags"]) == 0, case["name"]
            assert all(same(g2[key], g[key]) for key in g) and (d is None or same(d2, d)), case["name"]
            assert [int(v) for v in new2[:n]] == list(range(n))
            continue
        split += 1
        deferred = set(int(new[r["b"]]) for r in tr["runs"] if r["forced"])
        assert set(k for k in range(n) if tr2["retired"][k]) <= deferred, case["name"]
        for _ in range(12):
            g, d, new, rep = rc.reduce(g, d, case["par"])
            if not int(rep["retired"]):
                break
        assert not int(rep["retired"]) and not int(rep["flags"]), case["name"]
    assert split >= 3


# ---- 4. (c) end to end on the two laps of 8.1.18 -----------------------------------------------------------------------------------------------
def test_end_to_end_two_laps():
    E = rc.end_to_end()
    L, tr, new, rep = E["loops"], E["trace"], E["map"], E["rep"]
    N = L["n_nodes"]
    g3 = L["g3"]
    closure_ends = set()
    for ed in g3["edges"][:L["n_edges"]]:
        if int(ed["flags"]) & pg.EDGE_CLOSURE:
            closure_ends.update((int(ed["i"]), int(ed["j"])))
    retired = [k for k in range(N) if new[k] < 0]
    assert len(closure_ends) == 12 and len(retired) >= 8 and not closure_ends & set(retired)
    assert sum(k >= 24 for k in retired) >= 8                                   # second-lap keyframes
    assert int(rep["nodes_after"]) == N - len(retired) and int(rep["runs_kept"]) == 0
    truth = L["truth"]

    def mean_error(nodes, index):
        d = [math.hypot(float(nodes[index(k)]["x"]) - truth[k][0], float(nodes[index(k)]["y"]) - truth[k][1]) for k in range(N) if new[k] >= 0]
        return sum(d) / len(d)
    full = mean_error(g3["nodes"], lambda k: k)
    relaxed, rrep = pl.relaxed(E["g4"])
    reduced = mean_error(relaxed["nodes"], lambda k: int(new[k]))
    print("end to end: mean error of the surviving keyframes %.6f full, %.6f reduced and relaxed" % (full, reduced))
    assert abs(full - E2E_FULL) < 1e-5
    assert reduced <= full + E2E_MARGIN
    # driven on: the appended keyframes follow the compacted ones, and only they are described
    n4, n5 = counts(E["g4"])[0], counts(E["g5"])[0]
    assert n5 == n4 + int(E["append_rep"]["nodes"]) and int(E["append_rep"]["nodes"]) >= 3 and int(E["append_rep"]["flags"]) == 0
    assert same(E["desc5"][:n4], E["desc4"][:n4]) and all(int(v) for v in E["desc5"]["valid"][n4:n5]) and not E["desc5"][n5:].view(np.uint8).any()
    assert int(E["place_rep"]["query"]) == n5 - 1
    assert float(E["relax_rep"]["chi2_after"]) <= float(E["relax_rep"]["chi2_before"])
