"""The relaxation with the block-tridiagonal preconditioner on the device (csrc/k_pgchain.hip, csrc/pgrelax_dev.h:
lsd_enqueue_pg_relax_pc_device, lsd_pg_relax_pc; PoseGraph.relax_device / optimize_device with precond=) against the restatement of
tests/pose_graph_chain_cases.py.  The rule fixes every operation and every order, so every comparison is byte equality."""
import collections
import math

import numpy as np
import pytest

import pose_graph_cases as pg
import pose_graph_chain_cases as cc
import pose_graph_loops_cases as pl
import pose_graph_robust_cases as rc
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream
from test_pose_graph_gpu import laid_out

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


# ---- 1. the campaign in launches of 1, 2 and 5 graphs of different sizes, an empty graph among those of several ---------------------------
def empty_like(case):
    return dict(case, name="empty_for_" + case["name"], nodes=case["nodes"][:0], edges=case["edges"][:0])


def batches():
    """The campaign's cases grouped by their parameters (a launch has one set), each group cut into launches of 5 cases while it has five,
    then of 2, then of 1; a launch of more than one case gets an empty graph as its second.  The large graphs are launches of their own."""
    groups = {}
    for c in cc.campaign():
        big = c["name"] if len(c["nodes"]) >= 1023 else None
        groups.setdefault(tuple(c["par"][k] for k in pg.RELAX_KEYS) + tuple(c["rob"][k] for k in rc.ROBUST_KEYS) + (c["kind"], big), []).append(c)
    out = []
    for cases in groups.values():
        while cases:
            size = 5 if len(cases) >= 5 else 2 if len(cases) >= 2 else 1
            batch = cases[:size]
            out.append(batch if size == 1 else batch[:1] + [empty_like(batch[0])] + batch[1:])
            cases = cases[size:]
    return out


def test_launches_hold_one_two_and_five_graphs_of_different_sizes():
    sizes = collections.Counter(len(b) - (len(b) > 1) for b in batches())
    assert sizes[1] >= 3 and sizes[2] >= 3 and sizes[5] >= 2, sizes
    assert all(b[1]["name"].startswith("empty_for_") and len(b[1]["nodes"]) == 0 for b in batches() if len(b) > 1)
    assert any(len({len(c["nodes"]) for c in b}) >= 4 for b in batches())
    assert sorted(c["name"] for b in batches() for c in b if not c["name"].startswith("empty_for_")) == sorted(c["name"] for c in cc.campaign())


def expected(batch, nodes, edges):
    want_n, want_e = nodes.copy(), edges.copy()
    want_r, want_rr = np.zeros(len(batch), pg.RELAX_REP_DTYPE), np.zeros(len(batch), rc.ROBUST_REP_DTYPE)
    want_pc = np.zeros(len(batch), cc.PRECOND_REP_DTYPE)
    for g, c in enumerate(batch):
        n, e, rep, rr, pc, _ = cc.run_case(c)
        want_n[g, :len(n)], want_e[g, :len(e)], want_r[g], want_rr[g], want_pc[g] = n, e, rep, rr, pc
    return want_n, want_e, want_r, want_rr, want_pc


@pytest.mark.parametrize("batch", batches(), ids=lambda b: "%s_x%d" % (b[0]["name"], len(b)))
def test_campaign_byte_for_byte_through_the_device_entry(lsdmod, ctx, batch):
    import torch
    rng = np.random.default_rng(len(batch[0]["name"]))
    heads, nodes, edges, nc, ec = laid_out(batch, rng)
    want_n, want_e, want_r, want_rr, want_pc = expected(batch, nodes, edges)
    kind = batch[0]["kind"]
    ws_bytes = lsdmod.pg_workspace_pc_bytes(nc, ec, kind)
    assert ws_bytes > lsdmod.pg_workspace_bytes(nc, ec)
    d_h, d_n, d_e = Guarded(heads), Guarded(nodes), Guarded(edges)
    d_ws, d_r, d_rr, d_pc = filled(ws_bytes * len(batch)), filled(56 * len(batch)), filled(24 * len(batch)), filled(16 * len(batch))
    ctx.enqueue_pg_relax_pc_device(len(batch), d_h.ptr, d_n.ptr, nc, d_e.ptr, ec, d_ws.ptr, d_r.ptr, kind, batch[0]["rob"], d_rr.ptr, d_pc.ptr,
                                   lsdmod.pg_relax(batch[0]["par"]), stream())
    torch.cuda.synchronize()
    assert d_h.unchanged() and d_ws.back()[1]
    for name, d, want in (("nodes", d_n, want_n), ("edges", d_e, want_e), ("reports", d_r, want_r), ("robust reports", d_rr, want_rr),
                          ("preconditioner's reports", d_pc, want_pc)):
        check(name, d, want)


def test_campaign_byte_for_byte_through_the_host_entry(lsdmod, ctx):
    for c in cc.campaign():
        n, e, rep, rr, pc, _ = cc.run_case(c)
        got = ctx.pg_relax_pc(c["nodes"], c["edges"], c["kind"], c["rob"], c["par"])
        for name, g, w in zip(("nodes", "edges", "report", "robust report", "preconditioner's report"), got, (n, e, rep, rr, pc)):
            assert same(g, w), (c["name"], name, g, w)


def test_without_the_optional_reports_nothing_else_changes(lsdmod, ctx):
    import torch
    c = next(c for c in cc.campaign() if c["name"] == "interleaved_2_1")
    n, e, rep, _, _, _ = cc.run_case(c)
    heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(5))
    d_h, d_n, d_e, d_ws, d_r = Guarded(heads), Guarded(nodes), Guarded(edges), filled(lsdmod.pg_workspace_pc_bytes(nc, ec, "chain")), filled(56)
    ctx.enqueue_pg_relax_pc_device(1, d_h.ptr, d_n.ptr, nc, d_e.ptr, ec, d_ws.ptr, d_r.ptr, "chain", c["rob"], None, None, lsdmod.pg_relax(c["par"]), stream())
    torch.cuda.synchronize()
    want_n, want_e = nodes.copy(), edges.copy()
    want_n[0, :len(n)], want_e[0, :len(e)] = n, e
    check("nodes", d_n, want_n), check("edges", d_e, want_e), check("report", d_r, np.array([rep]))


# ---- 2. kind BLOCK is the existing entries, byte for byte --------------------------------------------------------------------------------
def test_block_is_the_existing_entries(lsdmod, ctx):
    """The same buffers through lsd_enqueue_pg_relax_device / lsd_enqueue_pg_relax_robust_device and through the new entry with kind BLOCK,
    on the plain and the robust campaigns' graphs of at most 257 nodes; the preconditioner's report is zeros."""
    import torch
    plain = [dict(c, rob=None) for c in pg.relax_campaign() if len(c["nodes"]) <= 257]
    robust = [c for c in rc.relax_campaign() if len(c["nodes"]) <= 257]
    assert len(plain) >= 40 and len(robust) >= 40
    runs = []
    for k, c in enumerate(plain + robust):
        heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(k))
        ws = lsdmod.pg_workspace_pc_bytes(nc, ec, "block")
        assert ws == lsdmod.pg_workspace_bytes(nc, ec)
        old = [Guarded(heads), Guarded(nodes), Guarded(edges), filled(ws), filled(56), filled(24)]
        new = [Guarded(heads), Guarded(nodes), Guarded(edges), filled(ws), filled(56), filled(24)]
        d_pc = filled(16)
        if c["rob"] is None:
            ctx.enqueue_pg_relax_device(1, old[0].ptr, old[1].ptr, nc, old[2].ptr, ec, old[3].ptr, old[4].ptr, lsdmod.pg_relax(c["par"]), stream())
            ctx.enqueue_pg_relax_pc_device(1, new[0].ptr, new[1].ptr, nc, new[2].ptr, ec, new[3].ptr, new[4].ptr, "block", None, None, d_pc.ptr,
                                           lsdmod.pg_relax(c["par"]), stream())
        else:
            ctx.enqueue_pg_relax_robust_device(1, old[0].ptr, old[1].ptr, nc, old[2].ptr, ec, old[3].ptr, old[4].ptr, lsdmod.pg_robust(c["rob"]),
                                               old[5].ptr, lsdmod.pg_relax(c["par"]), stream())
            ctx.enqueue_pg_relax_pc_device(1, new[0].ptr, new[1].ptr, nc, new[2].ptr, ec, new[3].ptr, new[4].ptr, "block", c["rob"], new[5].ptr, d_pc.ptr,
                                           lsdmod.pg_relax(c["par"]), stream())
        runs.append((c["name"], old, new, d_pc))
    torch.cuda.synchronize()
    for cname, old, new, d_pc in runs:
        for name, a, b in zip(("head", "nodes", "edges", "workspace", "report", "robust report"), old, new):
            (ga, oka), (gb, okb) = a.back(), b.back()
            assert oka and okb, (cname, name)
            if name != "workspace":
                assert same(ga, gb), (cname, name)
        got, ok = d_pc.back()
        assert ok and not got.any(), cname


# ---- 3. every refusal leaves the outputs unchanged ---------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    c = next(c for c in cc.campaign() if c["name"] == "huber_closures_0")
    heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(1))
    d_h, d_n, d_e, d_ws = Guarded(heads), Guarded(nodes), Guarded(edges), filled(lsdmod.pg_workspace_pc_bytes(nc, ec, "chain"))
    d_r, d_rr, d_pc = filled(56), filled(24), filled(16)
    par, good_rob = dict(pg.RELAX_DEFAULTS), rc.rob(rc.HUBER, 1.0)

    def entry(rob=good_rob, relax=par, kind=cc.CHAIN, reserved=0, **kw):
        a = dict(g=1, h=d_h.ptr, n=d_n.ptr, nc=nc, e=d_e.ptr, ec=ec, ws=d_ws.ptr, r=d_r.ptr, rr=d_rr.ptr, pc=d_pc.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_relax_pc_device(h, a["g"], a["h"], a["n"], a["nc"], a["e"], a["ec"], lsdmod.pg_relax(relax),
                                                lsdmod.lsd_pg_robust(rob["kernel"], rob["scope"], rob["delta"]), lsdmod.lsd_pg_precond(kind, reserved),
                                                a["ws"], a["r"], a["rr"], a["pc"], stream())
    for kind in (cc.BLOCK, cc.CHAIN):
        for kw in (dict(kind=-1), dict(kind=2), dict(kind=2 ** 31 - 1), dict(reserved=1), dict(reserved=-1), dict(pc=d_pc.ptr + 4)):
            assert entry(**dict(dict(kind=kind), **kw)) == INV, kw
        # everything the robust entry refuses
        for kw in (dict(g=-1), dict(h=None), dict(n=None), dict(e=None), dict(ws=None), dict(r=None), dict(nc=0), dict(nc=16385), dict(ec=0), dict(ec=65537),
                   dict(n=d_n.ptr + 4), dict(r=d_r.ptr + 4), dict(ws=d_ws.ptr + 1), dict(rr=d_rr.ptr + 4)):
            assert entry(kind=kind, **kw) == INV, kw
        for kw in (dict(lambda0=-1.0), dict(lambda_min=math.inf), dict(up=1.0), dict(down=0.5), dict(cg_tol=-1e-3), dict(eps=math.nan), dict(iters=-1),
                   dict(iters=65536), dict(cg_iters=-1), dict(cg_iters=65536)):
            assert entry(kind=kind, relax=dict(par, **kw)) == INV, kw
        for bad in (dict(kernel=-1), dict(kernel=3), dict(scope=2), dict(scope=0xFFFFFFFF), dict(delta=0.0), dict(delta=-1.0), dict(delta=math.nan),
                    dict(delta=math.inf), dict(kernel=rc.GM, delta=0.0), dict(kernel=rc.GM, delta=math.nan)):
            assert entry(kind=kind, rob=dict(good_rob, **bad)) == INV, bad
        assert entry(kind=kind, g=0) == 0
    rep, rr, pc = np.zeros(1, pg.RELAX_REP_DTYPE), np.zeros(1, rc.ROBUST_REP_DTYPE), np.zeros(1, cc.PRECOND_REP_DTYPE)
    keep_n, keep_e = c["nodes"].copy(), c["edges"].copy()

    def host(rob=good_rob, relax=par, kind=cc.CHAIN, reserved=0, rr_ptr=rr.ctypes.data, pc_ptr=pc.ctypes.data):
        return L.lsd_pg_relax_pc(h, keep_n.ctypes.data, len(keep_n), keep_e.ctypes.data, len(keep_e), lsdmod.pg_relax(relax),
                                 lsdmod.lsd_pg_robust(rob["kernel"], rob["scope"], rob["delta"]), lsdmod.lsd_pg_precond(kind, reserved), rep.ctypes.data,
                                 rr_ptr, pc_ptr)
    assert host(kind=2) == INV and host(kind=-1) == INV and host(reserved=3) == INV and host(rob=dict(good_rob, kernel=7)) == INV
    assert host(relax=dict(par, up=0.5)) == INV and host(rr_ptr=None) == INV and host(pc_ptr=None) == INV
    assert same(keep_n, c["nodes"]) and same(keep_e, c["edges"])
    assert not rep.view(np.uint8).any() and not rr.view(np.uint8).any() and not pc.view(np.uint8).any()
    assert lsdmod.pg_workspace_pc_bytes(nc, ec, 2) == 0 and lsdmod.pg_workspace_pc_bytes(0, ec, "chain") == 0
    torch.cuda.synchronize()
    for buf in (d_h, d_n, d_e, d_ws, d_r, d_rr, d_pc):
        assert buf.unchanged()


# ---- 4. PoseGraph on the graph of two laps with every loop closed -------------------------------------------------------------------------
ROBUST = dict(kernel="huber", delta=2.0, scope="closures")
RELAX = dict(pl.E2E["relax"], iters=6)


def loaded(lsdmod, ctx, E):
    g = E["g2"]
    graph = lsdmod.PoseGraph(len(g["nodes"]), len(g["edges"]), pl.E2E["n_beams"], ctx=ctx)
    graph._nodes.copy_(dev(g["nodes"].view(np.uint8).reshape(len(g["nodes"]), -1)))
    graph._edges.copy_(dev(g["edges"].view(np.uint8).reshape(len(g["edges"]), -1)))
    graph._head.copy_(dev(g["head"].view(np.uint8).reshape(-1)))
    return graph


def test_pose_graph_relax_and_optimize_with_the_chain(lsdmod, ctx):
    E = pl.end_to_end()
    nn, ne = E["n_nodes"], E["n_edges"]
    nodes, edges = E["g2"]["nodes"][:nn], E["g2"]["edges"][:ne]
    n1, e1, rep1, _, pc1 = cc.relax_pc(nodes, edges, RELAX, rc.rob(rc.NONE, 0.0), cc.CHAIN)
    assert int(pc1["chain_edges"]) == nn - 1 and int(pc1["paths"]) == 1 and int(pc1["fallbacks"]) == 0
    graph = loaded(lsdmod, ctx, E)
    before = graph.robust_report().copy()
    graph.relax_device(RELAX, precond="chain")
    assert graph.head() == (nn, ne)
    assert same(graph.nodes(), n1) and same(graph.edges(), e1) and same(graph.report(), rep1) and same(graph.precond_report(), pc1)
    assert same(graph.robust_report(), before)                              # (robust=None leaves the robust report as it was)
    want = cc.optimize_pc(nodes, edges, rc.rob(rc.HUBER, 2.0), rc.GATE, cc.CHAIN, 8, RELAX)
    graph = loaded(lsdmod, ctx, E)
    graph.optimize_device(ROBUST, rc.GATE, relax=RELAX, precond="chain")
    assert same(graph.nodes(), want["nodes"]) and same(graph.edges(), want["edges"])
    assert same(graph.robust_report(), want["robust"]) and same(graph.prune_report(), want["prune"]) and same(graph.report(), want["refit"])
    assert same(graph.precond_report(), want["precond"])
    # precond="block" is the call path of precond=None, byte for byte
    a, b = loaded(lsdmod, ctx, E), loaded(lsdmod, ctx, E)
    a.optimize_device(ROBUST, rc.GATE, relax=RELAX)
    b.optimize_device(ROBUST, rc.GATE, relax=RELAX, precond="block")
    assert same(a.nodes(), b.nodes()) and same(a.edges(), b.edges()) and same(a.report(), b.report()) and same(a.robust_report(), b.robust_report())
    assert not b.precond_report().tobytes().strip(b"\0")
    with pytest.raises(lsdmod.LsdError):
        graph.relax_device(RELAX, precond="tridiagonal")


def test_the_chain_call_does_not_synchronise(lsdmod, ctx):
    """relax_device(precond="chain") and optimize_device(.., precond="chain") return while ~80 ms of work enqueued in front of them is still
    running, and what they leave behind that work is the restated chain's."""
    E = pl.end_to_end()
    nn, ne = E["n_nodes"], E["n_edges"]
    want = cc.optimize_pc(E["g2"]["nodes"][:nn], E["g2"]["edges"][:ne], rc.rob(rc.HUBER, 2.0), rc.GATE, cc.CHAIN, 8, RELAX)

    def chain(graph):
        graph.optimize_device(ROBUST, rc.GATE, relax=RELAX, precond="chain")
    chain(loaded(lsdmod, ctx, E))                                                        # warm
    graph = loaded(lsdmod, ctx, E)
    returns_in_front_of_the_device(lambda: chain(graph), 'optimize_device(precond="chain")')
    assert same(graph.nodes(), want["nodes"]) and same(graph.precond_report(), want["precond"])
