"""The robust relaxation and the rejection of closures, the restatement alone (tests/pose_graph_robust_cases.py; include/lsd_hip.h, "pose
graph"): the campaigns reach every class, kernel NONE is the plain relaxation byte for byte, the chain robust -> prune ->
refit rejects exactly the closures that are false and ends at the minimum of the graph without them, and the records have the header's
sizes.  No GPU."""
import collections
import os
import re

import numpy as np
import pytest

import pose_graph_cases as pg
import pose_graph_robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest pose difference (pixels / degrees) between the chain's refit and the dense Gauss-Newton of the graph WITHOUT the false
# closures, measured on the four cases below, was 1.6e-11 (drifted_100_3_1); ten times that covers the libm of another
# host and CG stopping by cg_tol, as WELL_POSED_BOUND does for the plain relaxation.
CHAIN_BOUND = 10 * 1.6e-11


def same(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def poses(nodes):
    return np.stack([nodes["x"], nodes["y"], nodes["ang"]], axis=1)


def pose_diff(a, b):
    d = np.abs(a - b)
    d[:, 2] = np.abs([pg.wrap(v) for v in a[:, 2] - b[:, 2]])
    return float(d.max())


def test_relax_campaign_reaches_every_class():
    count = collections.Counter()
    campaign = rc.relax_campaign()
    assert len({c["name"] for c in campaign}) == len(campaign) and max(len(c["edges"]) for c in campaign) <= 1025
    for case in campaign:
        count.update(rc.relax_classes_of(case, rc.run_relax_case(case)[4]))
    short = {c: count[c] for c in rc.RELAX_CLASSES if count[c] < 3}
    assert not short, short
    assert sum(1 for c in campaign if "plain" in c) >= 10


def test_prune_campaign_reaches_every_class():
    count = collections.Counter()
    for case in rc.prune_campaign():
        count.update(rc.prune_classes_of(case, rc.run_prune_case(case)[2]))
    short = {c: count[c] for c in rc.PRUNE_CLASSES if count[c] < 3}
    assert not short, short


def test_none_is_the_plain_relaxation_byte_for_byte():
    """Multiplying by 1.0 is exact: kernel NONE on every case of the plain campaign gives pose_graph_cases.relax's bytes, and the robust
    report says that nothing was weighted."""
    for k, case in enumerate(pg.relax_campaign()):
        n, e, rep, _ = pg.run_relax_case(case)
        gn, ge, grep, rr = rc.relax_robust(case["nodes"], case["edges"], case["par"], rc.rob(rc.NONE, 0.0, k % 2))
        assert same(gn, n) and same(ge, e) and same(grep, rep), case["name"]
        assert int(rr["downweighted"]) == 0 and float(rr["w_min"]) == 1.0 and same(rr["chi2_plain"], rep["chi2_after"]), case["name"]


def test_a_delta_nothing_reaches_is_the_plain_relaxation_too():
    by_name = {c["name"]: c for c in pg.relax_campaign()}
    seen = 0
    for case in rc.relax_campaign():
        if "plain" not in case:
            continue
        n, e, rep, _ = pg.run_relax_case(by_name[case["plain"]])
        gn, ge, grep, rr, _ = rc.run_relax_case(case)
        assert same(gn, n) and same(ge, e) and same(grep, rep) and int(rr["downweighted"]) == 0, case["name"]
        seen += 1
    assert seen >= 10


def test_weight_and_cost_at_the_threshold():
    h, g = rc.rob(rc.HUBER, 3.0), rc.rob(rc.GM, 3.0)
    above = np.nextafter(9.0, np.inf)
    assert rc.weight(h, True, 9.0) == (1.0, 9.0) and rc.weight(h, False, 1e6) == (1.0, 1e6) and rc.weight(rc.rob(rc.NONE, 3.0), True, 1e6) == (1.0, 1e6)
    w, rho = rc.weight(h, True, float(above))
    assert w < 1.0 and abs(rho - 9.0) < 1e-14
    assert rc.weight(h, True, 36.0) == (0.5, 27.0)                                     # r = 6: w = 3 / 6, rho = 2 * 3 * 6 - 9
    assert rc.weight(g, True, 9.0) == (0.25, 4.5) and rc.weight(g, True, 0.0) == (1.0, 0.0)
    assert rc.weight(h, True, pg.INF) == (0.0, pg.INF)
    w, rho = rc.weight(g, True, pg.INF)
    assert w == 0.0 and rho != rho


def test_prune_on_a_small_graph():
    rows = [(pg.EDGE_CLOSURE, 50.0), (0, 1e6), (pg.EDGE_CLOSURE, 70.0), (pg.EDGE_CLOSURE, 50.0), (pg.EDGE_CLOSURE | pg.EDGE_DISABLED, 99.0),
            (pg.EDGE_CLOSURE, rc.GATE)]
    case = rc.pcase("t", np.random.default_rng(0), rows, max_reject=2)
    edges, rep = rc.prune(case["n_edges"], case["edges"], rc.GATE, 2)
    hit = pg.EDGE_CLOSURE | pg.EDGE_DISABLED | rc.EDGE_REJECTED
    assert [int(f) for f in edges["flags"][:6]] == [hit, 0, hit, pg.EDGE_CLOSURE, pg.EDGE_CLOSURE | pg.EDGE_DISABLED, pg.EDGE_CLOSURE]
    assert tuple(rep) == (3, 2, 2, 2, 70.0)
    assert same(edges[6:], case["edges"][6:]) and same(edges["chi2"], case["edges"]["chi2"])


CHAIN_CASES = [dict(d, rob=rc.rob(rc.HUBER, 1.0)) for d in rc.DRIFTED] + [dict(name="relaxed_end_to_end", rob=rc.rob(rc.GM, 3.0))]
_chain = {}


def chain_of(case):
    """(nodes, clean edges, edges, false indices, the chain's result), computed once: Huber / Geman-McClure on the closures, 20 outer
    iterations of at most 3 N CG steps, the gate of 11.345."""
    if case["name"] not in _chain:
        if "seed" in case:
            nodes, clean, edges, bad = rc.drifted(case["n"], case["seed"], case["closures"], case["falses"])
        else:
            nodes, clean, edges, bad = rc.relaxed_with_false_closure()
        par = dict(iters=20, cg_iters=3 * len(nodes))
        _chain[case["name"]] = (nodes, clean, edges, bad, rc.optimize(nodes, edges, case["rob"], rc.GATE, 8, par))
    return _chain[case["name"]]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: c["name"])
def test_chain_rejects_exactly_the_false_closures(case):
    nodes, clean, edges, bad, out = chain_of(case)
    flags = out["edges"]["flags"].astype(np.int64)
    rejected = [e for e in range(len(edges)) if flags[e] & rc.EDGE_REJECTED]
    true_closures = [e for e in range(len(clean)) if int(clean["flags"][e]) & pg.EDGE_CLOSURE]
    ref = pg.dense_gauss_newton(nodes, clean)
    diff = pose_diff(poses(out["nodes"]), ref)
    print("%s: rejected %s, worst chi2 %.4g, %d closures left; refit against the dense minimum without the false edges: %.3g"
          % (case["name"], rejected, out["prune"]["worst_chi2"], out["prune"]["closures_left"], diff))
    assert rejected == bad
    assert true_closures and not any(flags[e] & pg.EDGE_DISABLED for e in true_closures)
    assert int(out["prune"]["rejected"]) == len(bad) and int(out["prune"]["closures_left"]) == len(true_closures)
    assert int(out["refit"]["skipped_edges"]) == len(bad)
    assert diff <= CHAIN_BOUND


@pytest.mark.parametrize("case", CHAIN_CASES[:3], ids=lambda c: c["name"])
def test_plain_relaxation_is_bent_by_the_false_closures(case):
    """The false closures do damage: the plain relaxation of the same graph ends farther from the clean minimum than the chain does."""
    nodes, clean, edges, bad, out = chain_of(case)
    plain, _, _ = pg.relax(nodes, edges, dict(pg.RELAX_DEFAULTS, iters=20, cg_iters=3 * len(nodes)))
    ref = pg.dense_gauss_newton(nodes, clean)
    d_plain, d_chain = pose_diff(poses(plain), ref), pose_diff(poses(out["nodes"]), ref)
    print("%s: plain %.3g, chain %.3g pixels / degrees from the clean minimum" % (case["name"], d_plain, d_chain))
    assert d_plain > 1.0 > d_chain and d_plain > d_chain


def test_struct_sizes_and_offsets_match_the_header():
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name, size in rc.SIZES.items():
        m = re.search(r"typedef struct %s \{.*?\} %s;[^\n]*" % (name, name), src, re.S)
        assert m, name
        assert int(re.search(r"/\* (\d+) bytes", m.group(0)).group(1)) == size, name
    for name, dt in (("lsd_pg_robust_rep", rc.ROBUST_REP_DTYPE), ("lsd_pg_prune_rep", rc.PRUNE_REP_DTYPE)):
        assert dt.itemsize == rc.SIZES[name], name
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == list(dt.names), (name, fields)
    assert rc.ROBUST_REP_DTYPE.fields["downweighted"][1] == 16 and rc.PRUNE_REP_DTYPE.fields["worst_chi2"][1] == 16
    assert re.search(r"#define LSD_PG_EDGE_REJECTED %du" % rc.EDGE_REJECTED, src)
    assert re.search(r"enum \{ LSD_PG_KERNEL_NONE = %d, LSD_PG_KERNEL_HUBER = %d, LSD_PG_KERNEL_GM = %d \}" % (rc.NONE, rc.HUBER, rc.GM), src)
    assert re.search(r"enum \{ LSD_PG_ROBUST_CLOSURES = %d, LSD_PG_ROBUST_ALL = %d \}" % (rc.CLOSURES, rc.ALL), src)


def test_python_mirror_has_the_same_records(lsdmod):
    import ctypes as C
    assert rc.ROBUST_REP_DTYPE == lsdmod.PG_ROBUST_REP_DTYPE and rc.PRUNE_REP_DTYPE == lsdmod.PG_PRUNE_REP_DTYPE
    assert lsdmod.PG_EDGE_REJECTED == rc.EDGE_REJECTED and lsdmod.PG_MAX_REJECT == rc.MAX_REJECT
    assert (C.sizeof(lsdmod.lsd_pg_robust), lsdmod.lsd_pg_robust.delta.offset) == (16, 8)
    assert (C.sizeof(lsdmod.lsd_pg_prune), lsdmod.lsd_pg_prune.max_reject.offset) == (16, 8)
    for name in ("lsd_enqueue_pg_relax_robust_device", "lsd_enqueue_pg_prune_device", "lsd_pg_relax_robust"):
        assert name in lsdmod.EXPORTED_SYMBOLS
    r = lsdmod.pg_robust(kernel="gm", delta=3.0, scope="all")
    assert (r.kernel, r.scope, r.delta) == (rc.GM, rc.ALL, 3.0)
    r = lsdmod.pg_robust(dict(kernel=rc.HUBER))
    assert (r.kernel, r.scope, r.delta) == (rc.HUBER, rc.CLOSURES, 1.0)
    assert lsdmod.pg_robust(kernel="none").kernel == rc.NONE and lsdmod.pg_robust(r) is r
    with pytest.raises(lsdmod.LsdError):
        lsdmod.pg_robust(kernel="cauchy")
    with pytest.raises(lsdmod.LsdError):
        lsdmod.pg_robust(dict(width=2.0))
