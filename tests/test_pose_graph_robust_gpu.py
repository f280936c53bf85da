"""The robust relaxation and the rejection of closures on the device (csrc/k_posegraph.hip, csrc/k_pgprune.hip:
lsd_enqueue_pg_relax_robust_device, lsd_enqueue_pg_prune_device, lsd_pg_relax_robust; PoseGraph.optimize_device) against the restatement of
tests/pose_graph_robust_cases.py.  The rule fixes every operation and every order, so every comparison is byte equality."""
import collections
import math

import numpy as np
import pytest

import grid_cases as gc
import grid_match_cases as gm
import pose_graph_cases as pg
import pose_graph_robust_cases as rc
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream
from test_pose_graph_gpu import laid_out, room_objects, run_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def differing(got, want):
    g = got.view(want.dtype).reshape(want.shape)
    return [(i, g[i], want[i]) for i in np.ndindex(want.shape) if g[i].tobytes() != want[i].tobytes()][:3]


def check(name, buf, want):
    got, ok = buf.back()
    assert ok, name + ": a guard was written"
    if not same(got, want):
        pytest.fail("%s differ from the restatement: %r" % (name, differing(got, want)))


# ---- 1. the relaxation campaign in launches of 1, 2 and 5 cases, an empty graph among those of several --------------------------------
def empty_like(case):
    return dict(name="empty_for_" + case["name"], nodes=case["nodes"][:0], edges=case["edges"][:0], par=case["par"], rob=case["rob"])


def relax_batches():
    """The campaign's cases grouped by their parameters (a launch has one set -- most cases have their own, the campaign gives two groups
    five graphs), each group cut into launches of 5 cases while it has five, then of 2, then of 1; a launch of more than one case gets an
    empty graph as its second, so the launches hold 1, 3 and 6 graphs."""
    groups = {}
    for c in rc.relax_campaign():
        groups.setdefault(tuple(c["par"][k] for k in pg.RELAX_KEYS) + tuple(c["rob"][k] for k in rc.ROBUST_KEYS), []).append(c)
    out = []
    for cases in groups.values():
        while cases:
            size = 5 if len(cases) >= 5 else 2 if len(cases) >= 2 else 1
            batch = cases[:size]
            out.append(batch if size == 1 else batch[:1] + [empty_like(batch[0])] + batch[1:])
            cases = cases[size:]
    return out


def test_relax_launches_hold_one_two_and_five_cases():
    sizes = collections.Counter(len(b) - (len(b) > 1) for b in relax_batches())
    assert sizes[1] >= 3 and sizes[2] >= 3 and sizes[5] >= 2, sizes
    assert all(b[1]["name"].startswith("empty_for_") and len(b[1]["nodes"]) == 0 for b in relax_batches() if len(b) > 1)
    assert max(len(b) for b in prune_batches()) >= 5 and any(len(b) == 1 for b in prune_batches())


def robust_expected(batch, nodes, edges):
    want_n, want_e = nodes.copy(), edges.copy()
    want_r, want_rr = np.zeros(len(batch), pg.RELAX_REP_DTYPE), np.zeros(len(batch), rc.ROBUST_REP_DTYPE)
    for g, c in enumerate(batch):
        n, e, rep, rr, _ = rc.run_relax_case(c)
        want_n[g, :len(n)], want_e[g, :len(e)], want_r[g], want_rr[g] = n, e, rep, rr
    return want_n, want_e, want_r, want_rr


@pytest.mark.parametrize("batch", relax_batches(), ids=lambda b: "%s_x%d" % (b[0]["name"], len(b)))
def test_robust_relax_campaign_byte_for_byte(lsdmod, ctx, batch):
    import torch
    rng = np.random.default_rng(len(batch[0]["name"]))
    heads, nodes, edges, nc, ec = laid_out(batch, rng)
    want_n, want_e, want_r, want_rr = robust_expected(batch, nodes, edges)
    ws_bytes = lsdmod.pg_workspace_bytes(nc, ec)
    d_h, d_n, d_e = Guarded(heads), Guarded(nodes), Guarded(edges)
    d_ws, d_r, d_rr = filled(ws_bytes * len(batch)), filled(56 * len(batch)), filled(24 * len(batch))
    ctx.enqueue_pg_relax_robust_device(len(batch), d_h.ptr, d_n.ptr, nc, d_e.ptr, ec, d_ws.ptr, d_r.ptr, lsdmod.pg_robust(batch[0]["rob"]), d_rr.ptr,
                                       lsdmod.pg_relax(batch[0]["par"]), stream())
    torch.cuda.synchronize()
    assert d_h.unchanged() and d_ws.back()[1]
    for name, d, want in (("nodes", d_n, want_n), ("edges", d_e, want_e), ("reports", d_r, want_r), ("robust reports", d_rr, want_rr)):
        check(name, d, want)


def test_none_through_the_robust_entry_is_the_plain_entry(lsdmod, ctx):
    """The same buffers through both entries on the device: kernel NONE, and a delta nothing reaches, give the plain entry's bytes; and
    without a robust report (NULL) nothing else changes."""
    import torch
    for k, c in enumerate(pg.relax_campaign()[::4]):
        heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(k))
        ws = lsdmod.pg_workspace_bytes(nc, ec)
        plain = [Guarded(heads), Guarded(nodes), Guarded(edges), filled(ws), filled(56)]
        ctx.enqueue_pg_relax_device(1, plain[0].ptr, plain[1].ptr, nc, plain[2].ptr, ec, plain[3].ptr, plain[4].ptr, lsdmod.pg_relax(c["par"]), stream())
        r = (rc.rob(rc.NONE, -1.0, k % 2), rc.rob(rc.HUBER, rc.HUGE, rc.ALL))[k % 2]
        if c["name"].startswith("not_finite"):
            r = rc.rob(rc.NONE, math.nan)
        robust = [Guarded(heads), Guarded(nodes), Guarded(edges), filled(ws), filled(56)]
        ctx.enqueue_pg_relax_robust_device(1, robust[0].ptr, robust[1].ptr, nc, robust[2].ptr, ec, robust[3].ptr, robust[4].ptr, lsdmod.pg_robust(r),
                                           None, lsdmod.pg_relax(c["par"]), stream())
        torch.cuda.synchronize()
        for name, a, b in zip(("head", "nodes", "edges", "workspace", "report"), plain, robust):
            (ga, oka), (gb, okb) = a.back(), b.back()
            assert oka and okb, (c["name"], name)
            if name != "workspace":
                assert same(ga, gb), (c["name"], name)


def test_robust_host_entry(lsdmod, ctx):
    for c in rc.relax_campaign()[::6]:
        n, e, rep, rr, _ = rc.run_relax_case(c)
        got_n, got_e, got_r, got_rr = ctx.pg_relax_robust(c["nodes"], c["edges"], c["rob"], c["par"])
        assert same(got_n, n) and same(got_e, e) and same(got_r, rep) and same(got_rr, rr), c["name"]


# ---- 2. the prune campaign ---------------------------------------------------------------------------------------------------------------
def prune_batches():
    """The cases grouped by (gate, max_reject) and cut into launches of 1, 2, 5, ..; a case whose head is beyond its own capacity is a launch
    of its own at that capacity, so that the device clamps it."""
    groups = {}
    for k, c in enumerate(rc.prune_campaign()):
        above = c["n_edges"] > len(c["edges"])
        groups.setdefault((c["gate"], c["max_reject"], k if above else -1), []).append(c)
    out, sizes, k = [], (1, 2, 5), 0
    for cases in groups.values():
        while cases:
            out.append(cases[:sizes[k % 3]])
            cases = cases[sizes[k % 3]:]
            k += 1
    return out


def test_prune_campaign_byte_for_byte(lsdmod, ctx):
    """Every launch lays its graphs out at one capacity with noise behind each, an empty graph as the second of a launch of several; the
    restatement runs on the rows as they are laid out.  A case whose head is beyond its capacity is laid out alone at exactly that capacity
    (prune_batches), so all three of them reach the device's clamp."""
    import torch
    launches = []
    for k, batch in enumerate(prune_batches()):
        rng = np.random.default_rng(1000 + k)
        graphs = len(batch) + (len(batch) > 1)
        above = [c for c in batch if c["n_edges"] > len(c["edges"])]
        assert not above or len(batch) == 1
        ec = max(len(c["edges"]) for c in batch) + (0 if above else k % 3)
        heads = np.zeros(graphs, pg.HEAD_DTYPE)
        edges = rng.integers(0, 256, (graphs, ec * 96), dtype=np.uint8).view(pg.EDGE_DTYPE).reshape(graphs, ec).copy()
        heads["n_nodes"] = rng.integers(-5, 50, graphs)
        slots = [0] + list(range(2, graphs)) if graphs > 1 else [0]
        for g, c in zip(slots, batch):
            heads[g]["n_edges"] = c["n_edges"]
            edges[g, :len(c["edges"])] = c["edges"]
        want_e, want_r = edges.copy(), np.zeros(graphs, rc.PRUNE_REP_DTYPE)
        for g in range(graphs):
            want_e[g], want_r[g] = rc.prune(int(heads[g]["n_edges"]), edges[g], batch[0]["gate"], batch[0]["max_reject"])
        d_h, d_e, d_r = Guarded(heads), Guarded(edges), filled(24 * graphs)
        ctx.enqueue_pg_prune_device(graphs, d_h.ptr, d_e.ptr, ec, d_r.ptr, batch[0]["gate"], batch[0]["max_reject"], stream())
        launches.append((batch[0]["name"], d_h, d_e, d_r, want_e, want_r))
    assert sum(1 for b in prune_batches() for c in b if c["n_edges"] > len(c["edges"])) >= 3
    torch.cuda.synchronize()
    for name, d_h, d_e, d_r, want_e, want_r in launches:
        assert d_h.unchanged(), name
        check(name + ": edges", d_e, want_e)
        check(name + ": reports", d_r, want_r)


# ---- 3. every refusal leaves the outputs unchanged ---------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    c = next(c for c in rc.relax_campaign() if c["name"] == "huber_closures_0")
    heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(1))
    d_h, d_n, d_e, d_ws, d_r, d_rr = Guarded(heads), Guarded(nodes), Guarded(edges), filled(lsdmod.pg_workspace_bytes(nc, ec)), filled(56), filled(24)
    d_p = filled(24)
    par, good_rob = dict(pg.RELAX_DEFAULTS), rc.rob(rc.HUBER, 1.0)

    def robust(rob=good_rob, relax=par, **kw):
        a = dict(g=1, h=d_h.ptr, n=d_n.ptr, nc=nc, e=d_e.ptr, ec=ec, ws=d_ws.ptr, r=d_r.ptr, rr=d_rr.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_relax_robust_device(h, a["g"], a["h"], a["n"], a["nc"], a["e"], a["ec"], lsdmod.pg_relax(relax),
                                                    lsdmod.lsd_pg_robust(rob["kernel"], rob["scope"], rob["delta"]), a["ws"], a["r"], a["rr"], stream())
    for kw in (dict(g=-1), dict(h=None), dict(n=None), dict(e=None), dict(ws=None), dict(r=None), dict(nc=0), dict(nc=16385), dict(ec=0), dict(ec=65537),
               dict(n=d_n.ptr + 4), dict(r=d_r.ptr + 4), dict(ws=d_ws.ptr + 1), dict(rr=d_rr.ptr + 4)):
        assert robust(**kw) == INV, kw
    for kw in (dict(lambda0=-1.0), dict(lambda_min=math.inf), dict(up=1.0), dict(down=0.5), dict(cg_tol=-1e-3), dict(eps=math.nan), dict(iters=-1),
               dict(iters=65536), dict(cg_iters=-1), dict(cg_iters=65536)):
        assert robust(relax=dict(par, **kw)) == INV, kw
    for bad in (dict(kernel=-1), dict(kernel=3), dict(scope=2), dict(scope=0xFFFFFFFF), dict(delta=0.0), dict(delta=-1.0), dict(delta=math.nan),
                dict(delta=math.inf), dict(kernel=rc.GM, delta=0.0), dict(kernel=rc.GM, delta=math.nan)):
        assert robust(rob=dict(good_rob, **bad)) == INV, bad
    assert robust(g=0) == 0
    rep, rr = np.zeros(1, pg.RELAX_REP_DTYPE), np.zeros(1, rc.ROBUST_REP_DTYPE)
    keep_n, keep_e = c["nodes"].copy(), c["edges"].copy()

    def host(rob=good_rob, relax=par, rr_ptr=rr.ctypes.data):
        return L.lsd_pg_relax_robust(h, keep_n.ctypes.data, len(keep_n), keep_e.ctypes.data, len(keep_e), lsdmod.pg_relax(relax),
                                     lsdmod.lsd_pg_robust(rob["kernel"], rob["scope"], rob["delta"]), rep.ctypes.data, rr_ptr)
    assert host(rob=dict(good_rob, kernel=7)) == INV and host(rob=dict(good_rob, delta=0.0)) == INV and host(relax=dict(par, up=0.5)) == INV
    assert host(rr_ptr=None) == INV
    assert same(keep_n, c["nodes"]) and same(keep_e, c["edges"]) and not rep.view(np.uint8).any() and not rr.view(np.uint8).any()

    def prune(**kw):
        a = dict(g=1, h=d_h.ptr, e=d_e.ptr, ec=ec, gate=rc.GATE, mr=8, r=d_p.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_prune_device(h, a["g"], a["h"], a["e"], a["ec"], lsdmod.lsd_pg_prune(a["gate"], a["mr"], 0), a["r"], stream())
    for kw in (dict(g=-1), dict(h=None), dict(e=None), dict(r=None), dict(ec=0), dict(ec=65537), dict(gate=-1.0), dict(gate=math.nan), dict(gate=math.inf),
               dict(mr=-1), dict(mr=65), dict(h=d_h.ptr + 4), dict(e=d_e.ptr + 4), dict(r=d_p.ptr + 4)):
        assert prune(**kw) == INV, kw
    assert prune(g=0) == 0
    torch.cuda.synchronize()
    for buf in (d_h, d_n, d_e, d_ws, d_r, d_rr, d_p):
        assert buf.unchanged()


# ---- 4. PoseGraph.optimize_device on the end-to-end graph with a false closure ------------------------------------------------------------
def test_optimize_device_equals_the_restated_chain(lsdmod, ctx):
    """The chain of pose_graph_cases.end_to_end() on the device, then a false closure 5 -> 17 written into the edge tensor, then
    optimize_device (Geman-McClure, delta 3, the gate of 11.345) and rerender_device: equal to the restated chain byte for byte -- graph,
    the three reports, the planes.  (That nothing waits is the next test.)"""
    import torch
    E = pg.end_to_end()
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    run_chain(lsdmod, graph, scratch, mapper, E, d_in)
    nn, ne = E["n_nodes"], E["n_edges"]
    nodes, clean, edges, bad = rc.relaxed_with_false_closure()
    assert bad == [ne] and same(graph.nodes(), nodes)
    relax = dict(pg.E2E["relax"], iters=20)
    want = rc.optimize(nodes, edges, rc.rob(rc.GM, 3.0), rc.GATE, 8, relax)
    g4 = pg.copy_graph(E["g3"])
    g4["nodes"][:nn] = want["nodes"]
    R = gm.ROOM
    pa, hi = np.zeros((R["rows"], R["cols"]), np.uint32), np.zeros((R["rows"], R["cols"]), np.uint32)
    gc.integrate(g4["store"], g4["store_lens"], np.stack([g4["nodes"]["x"], g4["nodes"]["y"], g4["nodes"]["ang"]], axis=1), R["cols"], R["rows"], R["resol"],
                 R["range_max"], pa, hi)
    d_edge = dev(edges[ne:ne + 1].view(np.uint8).reshape(1, -1))
    d_head = dev(np.array([(nn, ne + 1)], pg.HEAD_DTYPE).view(np.uint8).reshape(-1))
    graph._edges[ne:ne + 1].copy_(d_edge)
    graph._head.copy_(d_head)
    graph.optimize_device(dict(kernel="gm", delta=3.0), rc.GATE, relax=relax)
    mapper.rerender_device(graph)
    assert graph.head() == (nn, ne + 1)
    assert same(graph.nodes(), want["nodes"]) and same(graph.edges(), want["edges"])
    assert same(graph.robust_report(), want["robust"]) and same(graph.prune_report(), want["prune"]) and same(graph.report(), want["refit"])
    flags = graph.edges()["flags"]
    assert [e for e in range(ne + 1) if flags[e] & lsdmod.PG_EDGE_REJECTED] == bad
    gp, gh = mapper.counts()
    assert same(gp, pa) and same(gh, hi)
    # relax_device(robust=) alone is the first link, and robust=None the call it always made
    graph2, _ = room_objects(lsdmod, ctx, E)
    graph2._nodes.copy_(dev(E["g3"]["nodes"].view(np.uint8).reshape(len(E["g3"]["nodes"]), -1)))
    graph2._edges[:ne + 1].copy_(dev(edges.view(np.uint8).reshape(ne + 1, -1)))
    graph2._head.copy_(d_head)
    graph2.relax_device(relax, robust=lsdmod.pg_robust(kernel="gm", delta=3.0))
    n1, e1, rep1, rr1 = rc.relax_robust(nodes, edges, relax, rc.rob(rc.GM, 3.0))
    assert same(graph2.nodes(), n1) and same(graph2.edges(), e1) and same(graph2.report(), rep1) and same(graph2.robust_report(), rr1)
    graph2.prune_device(rc.GATE, max_reject=0)
    assert int(graph2.prune_report()["candidates"]) == 1 and int(graph2.prune_report()["rejected"]) == 0 and same(graph2.edges(), e1)


def test_optimize_device_does_not_synchronise(lsdmod, ctx):
    """The robust relaxation, prune_device, the refit and rerender_device return while work enqueued in front of them is still running
    (as tests/test_pose_graph_gpu.py holds the chain of 8.1.15 to it: the work in front is sized on this device, ~80 ms), and the result
    behind that work is still the restated chain's."""
    E = pg.end_to_end()
    nn, ne = E["n_nodes"], E["n_edges"]
    nodes, clean, edges, bad = rc.relaxed_with_false_closure()
    relax = dict(pg.E2E["relax"], iters=20)
    want = rc.optimize(nodes, edges, rc.rob(rc.GM, 3.0), rc.GATE, 8, relax)
    d_nodes = dev(E["g3"]["nodes"].view(np.uint8).reshape(len(E["g3"]["nodes"]), -1))
    d_edges = dev(edges.view(np.uint8).reshape(ne + 1, -1))
    d_head = dev(np.array([(nn, ne + 1)], pg.HEAD_DTYPE).view(np.uint8).reshape(-1))

    def loaded():
        graph, (_, mapper) = room_objects(lsdmod, ctx, E)
        graph._nodes.copy_(d_nodes)
        graph._edges[:ne + 1].copy_(d_edges)
        graph._head.copy_(d_head)
        return graph, mapper

    def chain(graph, mapper):
        graph.optimize_device(dict(kernel="gm", delta=3.0), rc.GATE, relax=relax)
        mapper.rerender_device(graph)
    chain(*loaded())                                                                    # warm: every workspace has its size
    graph, mapper = loaded()
    returns_in_front_of_the_device(lambda: chain(graph, mapper), "optimize_device / rerender_device")
    assert same(graph.nodes(), want["nodes"]) and same(graph.edges(), want["edges"]) and same(graph.prune_report(), want["prune"])
