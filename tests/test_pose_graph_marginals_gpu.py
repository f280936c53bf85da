"""Marginal covariances and the gate on new closures on the device (csrc/k_pgmarg.hip: lsd_enqueue_pg_marginals_device,
lsd_enqueue_pg_vet_device, lsd_pg_marginals, lsd_pg_vet; PoseGraph.marginals_device / vet_device / close_all_device(vet=)) against the
restatement of tests/pose_graph_marginal_cases.py.  The rule fixes every operation and every order, so every comparison is byte equality."""
import math

import numpy as np
import pytest

import grid_match_cases as gm
import pose_graph_cases as pg
import pose_graph_loops_cases as pl
import pose_graph_marginal_cases as mc
import pose_graph_place_cases as pp
import pose_graph_robust_cases as rc
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream
from test_pose_graph_gpu import laid_out
from test_pose_graph_loops_gpu import CLOSURE

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


def marg_par(lsdmod, par):
    return lsdmod.lsd_pg_marg(float(par["cg_tol"]), int(par["cg_iters"]), int(par["precond"]), int(par["slots"]), 0)


class Launch:
    """One marginals call on a campaign case between guards: noise behind the graph's records and in every record to be overwritten."""

    def __init__(self, lsdmod, ctx, case, seed, qu=None, slots=None):
        rng = np.random.default_rng(seed)
        heads, nodes, edges, self.nc, _ = laid_out([case], rng)
        self.ec = case["edges_cap"]
        e2 = rng.integers(0, 256, self.ec * 96, dtype=np.uint8).view(pg.EDGE_DTYPE).copy()
        e2[:len(case["edges"])] = case["edges"]
        self.qu = case["queries"] if qu is None else qu
        self.par = dict(case["par"], slots=case["par"]["slots"] if slots is None else slots)
        ws = lsdmod.pg_marginals_workspace_bytes(self.nc, self.ec, self.par["precond"], self.par["slots"])
        assert ws > 0
        self.h, self.n, self.e, self.q = Guarded(heads), Guarded(nodes), Guarded(e2), Guarded(self.qu)
        self.prior = None if case["prior"] is None else Guarded(np.array([(7, case["prior"])], pg.HEAD_DTYPE))
        self.ws, self.recs, self.rep = filled(ws), filled(104 * len(self.qu)), filled(32)
        ctx.enqueue_pg_marginals_device(self.h.ptr, self.n.ptr, self.nc, self.e.ptr, self.ec, self.q.ptr, len(self.qu), self.ws.ptr, self.recs.ptr, self.rep.ptr,
                                        marg_par(lsdmod, self.par), None if self.prior is None else self.prior.ptr, stream())

    def inputs_unchanged(self):
        return all(b.unchanged() for b in (self.h, self.n, self.e, self.q) + (() if self.prior is None else (self.prior,))) and self.ws.back()[1]


# ---- 1. the campaigns through the device entries -------------------------------------------------------------------------------------------
def test_campaign_byte_for_byte_through_the_device_entry(lsdmod, ctx):
    import torch
    runs = [(c, Launch(lsdmod, ctx, c, k)) for k, c in enumerate(mc.campaign())]
    torch.cuda.synchronize()
    for c, L in runs:
        recs, rep, _ = mc.run_case(c)
        assert L.inputs_unchanged(), c["name"] + ": the graph, the queries or a guard changed"
        check(c["name"] + " records", L.recs, recs)
        check(c["name"] + " report", L.rep, np.array([rep]))


def test_vet_campaign_byte_for_byte_through_the_device_entry(lsdmod, ctx):
    import torch
    runs = []
    for k, c in enumerate(mc.vet_campaign()):
        rng = np.random.default_rng(100 + k)
        heads, nodes, edges, nc, ec = laid_out([c], rng)
        d = [Guarded(heads), Guarded(nodes), Guarded(edges), Guarded(c["queries"]), Guarded(c["recs"]), filled(24 * len(c["queries"]))]
        ctx.enqueue_pg_vet_device(d[0].ptr, d[1].ptr, nc, d[2].ptr, ec, d[3].ptr, d[4].ptr, len(c["queries"]), c["gate"], d[5].ptr, stream())
        twin = Guarded(edges)                                                # the same call without the optional reports
        ctx.enqueue_pg_vet_device(d[0].ptr, d[1].ptr, nc, twin.ptr, ec, d[3].ptr, d[4].ptr, len(c["queries"]), c["gate"], None, stream())
        runs.append((c, d, twin, edges))
    torch.cuda.synchronize()
    for c, d, twin, edges in runs:
        want_e, want_r, _ = mc.run_vet_case(c)
        full = edges.copy()
        full[0, :len(want_e)] = want_e
        assert all(b.unchanged() for b in (d[0], d[1], d[3], d[4])), c["name"]
        check(c["name"] + " edges", d[2], full), check(c["name"] + " edges (no reports)", twin, full), check(c["name"] + " reports", d[5], want_r)
        changed = np.flatnonzero(full[0]["flags"] != edges[0]["flags"])
        assert all(int(full[0]["flags"][e]) == int(edges[0]["flags"][e]) | 5 for e in changed)


# ---- 2. a record depends on the graph and the query alone ----------------------------------------------------------------------------------
def test_records_do_not_depend_on_slots_or_order(lsdmod, ctx):
    import torch
    names = ("nodes_chain_0", "nodes_block_1", "new_edges_0", "floating_chain_1", "n_257_2", "joined_2", "fallback_1")
    cases = [c for c in mc.campaign() if c["name"] in names]
    assert len(cases) == len(names)
    runs = []
    for k, c in enumerate(cases):
        n_q = len(c["queries"])
        back = c["queries"][::-1].copy()
        runs.append((c, [Launch(lsdmod, ctx, c, 50 + k, slots=s) for s in (1, 2, n_q + 3, 1024)], Launch(lsdmod, ctx, c, 60 + k, qu=back, slots=2)))
    torch.cuda.synchronize()
    for c, by_slots, reversed_ in runs:
        recs = mc.run_case(c)[0]
        for L in by_slots:
            check("%s at %d slots" % (c["name"], L.par["slots"]), L.recs, recs)
        check(c["name"] + " reversed", reversed_.recs, recs[::-1].copy())


# ---- 3. the host entries -------------------------------------------------------------------------------------------------------------------
def test_host_entries(lsdmod, ctx):
    for c in mc.campaign():
        if len(c["nodes"]) > 257:
            continue
        recs, rep, _ = mc.run_case(c)
        prior = -1 if c["prior"] is None else c["prior"]
        if c["prior"] is not None and not 0 <= c["prior"] <= len(c["edges"]):
            continue                                                         # (the host entry has no capacity beyond the edges: its clamp differs)
        got, grep = ctx.pg_marginals(c["nodes"], c["edges"], c["queries"], marg_par(lsdmod, c["par"]), prior)
        assert same(got, recs) and same(grep, rep), c["name"]
    for c in mc.vet_campaign():
        want_e, want_r, _ = mc.run_vet_case(c)
        ed, reps = ctx.pg_vet(c["nodes"], c["edges"], c["queries"], c["recs"], c["gate"])
        assert same(ed, want_e) and same(reps, want_r), c["name"]
    none, rep = ctx.pg_marginals(mc.campaign()[0]["nodes"], mc.campaign()[0]["edges"], np.zeros(0, mc.QUERY_DTYPE))
    assert len(none) == 0 and not rep.tobytes().strip(b"\0")


# ---- 4. every refusal leaves the outputs unchanged -----------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    c = next(c for c in mc.campaign() if c["name"] == "new_edges_1")
    heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(1))
    qu = c["queries"]
    d_h, d_n, d_e, d_q, d_p = Guarded(heads), Guarded(nodes), Guarded(edges), Guarded(qu), Guarded(np.array([(1, 2)], pg.HEAD_DTYPE))
    d_ws, d_recs, d_rep, d_vrep = filled(lsdmod.pg_marginals_workspace_bytes(nc, ec, "chain", 4)), filled(104 * len(qu)), filled(32), filled(24 * len(qu))
    good = dict(cg_tol=1e-8, cg_iters=10, precond=1, slots=4, reserved=0)

    def marg(par=good, **kw):
        a = dict(h=d_h.ptr, n=d_n.ptr, nc=nc, e=d_e.ptr, ec=ec, p=d_p.ptr, q=d_q.ptr, nq=len(qu), ws=d_ws.ptr, recs=d_recs.ptr, rep=d_rep.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_marginals_device(h, a["h"], a["n"], a["nc"], a["e"], a["ec"], a["p"], a["q"], a["nq"],
                                                 lsdmod.lsd_pg_marg(par["cg_tol"], par["cg_iters"], par["precond"], par["slots"], par["reserved"]),
                                                 a["ws"], a["recs"], a["rep"], stream())

    def vet(gate=16.27, **kw):
        a = dict(h=d_h.ptr, n=d_n.ptr, nc=nc, e=d_e.ptr, ec=ec, q=d_q.ptr, recs=d_recs.ptr, nq=len(qu), rep=d_vrep.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_vet_device(h, a["h"], a["n"], a["nc"], a["e"], a["ec"], a["q"], a["recs"], a["nq"], gate, a["rep"], stream())
    for kw in (dict(h=None), dict(n=None), dict(e=None), dict(q=None), dict(ws=None), dict(recs=None), dict(rep=None), dict(nc=0), dict(nc=16385),
               dict(ec=0), dict(ec=65537), dict(nq=-1), dict(nq=65537), dict(h=d_h.ptr + 4), dict(n=d_n.ptr + 4), dict(e=d_e.ptr + 4), dict(p=d_p.ptr + 4),
               dict(q=d_q.ptr + 4), dict(ws=d_ws.ptr + 1), dict(recs=d_recs.ptr + 4), dict(rep=d_rep.ptr + 4)):
        assert marg(**kw) == INV, kw
    for bad in (dict(cg_tol=-1e-3), dict(cg_tol=math.nan), dict(cg_tol=math.inf), dict(cg_iters=-1), dict(cg_iters=65536), dict(precond=-1), dict(precond=2),
                dict(slots=0), dict(slots=1025), dict(slots=-1), dict(reserved=1)):
        assert marg(dict(good, **bad)) == INV, bad
    assert marg(nq=0) == 0 and marg(nq=0, q=None, recs=None) == 0
    for kw in (dict(h=None), dict(n=None), dict(e=None), dict(q=None), dict(recs=None), dict(nc=0), dict(nc=16385), dict(ec=0), dict(ec=65537), dict(nq=-1),
               dict(nq=65537), dict(gate=-1.0), dict(gate=math.nan), dict(gate=math.inf), dict(h=d_h.ptr + 4), dict(n=d_n.ptr + 4), dict(e=d_e.ptr + 4),
               dict(q=d_q.ptr + 4), dict(recs=d_recs.ptr + 4), dict(rep=d_vrep.ptr + 4)):
        assert vet(**kw) == INV, kw
    assert vet(nq=0) == 0
    # the host entries
    recs, rep, vreps = np.zeros(len(qu), mc.REC_DTYPE), np.zeros(1, mc.REP_DTYPE), np.zeros(len(qu), mc.VET_REP_DTYPE)
    keep_n, keep_e = c["nodes"].copy(), c["edges"].copy()

    def host(par=good, nq=len(qu), n_nodes=len(keep_n), recs_ptr=recs.ctypes.data, rep_ptr=rep.ctypes.data):
        return L.lsd_pg_marginals(h, keep_n.ctypes.data, n_nodes, keep_e.ctypes.data, len(keep_e), 3, qu.ctypes.data, nq,
                                  lsdmod.lsd_pg_marg(par["cg_tol"], par["cg_iters"], par["precond"], par["slots"], par["reserved"]), recs_ptr, rep_ptr)
    assert host(dict(good, slots=0)) == INV and host(dict(good, precond=5)) == INV and host(nq=65537) == INV and host(n_nodes=16385) == INV
    assert host(recs_ptr=None) == INV and host(rep_ptr=None) == INV and host(dict(good, cg_tol=-1.0)) == INV
    assert L.lsd_pg_vet(h, keep_n.ctypes.data, len(keep_n), keep_e.ctypes.data, len(keep_e), qu.ctypes.data, recs.ctypes.data, len(qu), -1.0,
                        vreps.ctypes.data) == INV
    assert L.lsd_pg_vet(h, keep_n.ctypes.data, len(keep_n), keep_e.ctypes.data, len(keep_e), qu.ctypes.data, None, len(qu), 1.0, vreps.ctypes.data) == INV
    assert same(keep_n, c["nodes"]) and same(keep_e, c["edges"])
    assert not recs.view(np.uint8).any() and not rep.view(np.uint8).any() and not vreps.view(np.uint8).any()
    torch.cuda.synchronize()
    for buf in (d_h, d_n, d_e, d_q, d_p, d_ws, d_recs, d_rep, d_vrep):
        assert buf.unchanged()


# ---- 5. PoseGraph --------------------------------------------------------------------------------------------------------------------------
def loaded(lsdmod, ctx, nodes, edges, extra=4):
    graph = lsdmod.PoseGraph(len(nodes) + extra, len(edges) + extra, 8, ctx=ctx)
    graph._nodes[:len(nodes)].copy_(dev(nodes.view(np.uint8).reshape(len(nodes), -1)))
    graph._edges[:len(edges)].copy_(dev(edges.view(np.uint8).reshape(len(edges), -1)))
    graph._head.copy_(dev(np.array([(len(nodes), len(edges))], pg.HEAD_DTYPE).view(np.uint8).reshape(-1)))
    return graph


def test_gate_fixture_on_the_device(lsdmod, ctx):
    """The fixture of the CPU test through PoseGraph: the snapshot in front of the closures, the NEW_EDGE queries, the gate, the refit."""
    nodes, edges, prior, false_idx, true_idx = mc.gate_fixture()
    n_new = len(edges) - prior
    vet_par = dict(gate=mc.GATE_999, marg=mc.FIXTURE["marg"])
    graph = loaded(lsdmod, ctx, nodes, edges[:prior], extra=9)
    graph.snapshot_device()
    graph._edges[prior:len(edges)].copy_(dev(edges[prior:].view(np.uint8).reshape(n_new, -1)))      # the closures arrive
    graph._head.copy_(dev(np.array([(len(nodes), len(edges))], pg.HEAD_DTYPE).view(np.uint8).reshape(-1)))
    graph._vetted(lsdmod.pg_vet(dict(gate=mc.GATE_999, marg=dict(mc.FIXTURE["marg"], precond="chain"))), 8, stream_of(lsdmod))
    want_e, want_recs, want_rep, want_v = mc.vetted_closures(nodes, edges, prior, 8, vet_par, graph.edges_cap)
    assert same(graph.marginal_records(), want_recs) and same(graph.marginals_report(), want_rep) and same(graph.vet_reports(), want_v)
    assert same(graph.edges(), want_e) and same(graph.nodes(), nodes)
    assert [int(f) for f in want_v["flags"]] == [mc.VET_REJECTED if prior + k == false_idx else mc.VET_PASSED for k in range(n_new)] + \
        [mc.VET_NO_EDGE] * (8 - n_new)
    par = dict(pg.RELAX_DEFAULTS, iters=10)
    graph.relax_device(par)
    n1, e1, rep1 = pg.relax(nodes, want_e, par)[:3]
    assert same(graph.nodes(), n1) and same(graph.edges(), e1) and same(graph.report(), rep1)
    # every node's marginal, the tracks' last nodes, and a list of the caller's
    graph = loaded(lsdmod, ctx, nodes, want_e)
    marg = dict(mc.FIXTURE["marg"], precond="chain", slots=16)
    graph.marginals_device(None, marg)
    every, _ = mc.marginals(nodes, want_e, mc.queries(*[(mc.NODE, n, 0) for n in range(len(nodes))]), dict(mc.FIXTURE["marg"], slots=16))
    assert same(graph.marginal_records(), every)
    rows = [(mc.PAIR, 3, 40), (mc.NODE, 49, 0)]
    graph.marginals_device(rows, marg)
    assert same(graph.marginal_records(), mc.marginals(nodes, want_e, mc.queries(*rows), dict(mc.FIXTURE["marg"], slots=2))[0])
    graph.marginals_device("tracks", marg)                                   # (the track record of a loaded graph is empty: last = -1)
    assert int(graph.marginal_records()[0]["flags"]) == mc.BAD_QUERY


def stream_of(lsdmod):
    import torch
    return torch.cuda.current_stream()


VET = dict(gate=mc.VET_E2E["vet"]["gate"], marg=dict(mc.VET_E2E["vet"]["marg"], precond="chain"))
ROBUST = dict(kernel="huber", delta=mc.VET_E2E["robust"]["delta"], scope="closures")


def run_vetted_chain(lsdmod, graph, scratch, mapper, d_in, vet=VET):
    graph.append_device(*d_in, append=pl.E2E["append"])
    graph.close_all_device(scratch, place=pl.E2E["place"], loops=pl.E2E["loops"], search=pl.E2E["search"], response=pl.E2E["response"],
                           smear=(3, gm.GAUSS), closure=CLOSURE, vet=vet)


def vet_room_objects(lsdmod, ctx, V):
    R = pp.PLACE_ROOM
    graph = lsdmod.PoseGraph(V["cap"], V["edges_cap"], pl.E2E["n_beams"], ctx=ctx)
    mappers = [lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx) for _ in range(2)]
    return graph, mappers


def test_close_all_with_vet_equals_the_restated_chain(lsdmod, ctx):
    """append -> close_all_device(vet=) -> optimize_device -> rerender on the gate's fixture WITH scans (two laps round the off-centre box,
    odometry errors drawn at the stated information, one keyframe whose scan is another place's): the chain appends six true closures and
    the false one, the gate passes the six and rejects the one, and the records, the vet's reports, the graph behind the gate and behind
    the optimisation and the re-rendered planes are the restated chain's, byte for byte."""
    V = mc.vet_end_to_end()
    names = [mc.VET_NAMES[int(f)] for f in V["vet_reps"]["flags"]]
    assert names.count("passed") == 6 and names.count("rejected") == 1 and names.count("no_edge") == 1
    graph, (scratch, mapper) = vet_room_objects(lsdmod, ctx, V)
    d_in = (dev(V["scans"]), dev(V["lens"]), dev(V["odom"]))
    run_vetted_chain(lsdmod, graph, scratch, mapper, d_in)
    nears, creps = graph.closure_reports()
    assert same(nears, V["nears"]) and same(creps, V["closure_reps"]) and graph.head() == (V["n_nodes"], V["n_edges"])
    assert same(graph.marginal_records(), V["recs"]) and same(graph.marginals_report(), V["rep"]) and same(graph.vet_reports(), V["vet_reps"])
    assert same(graph.edges(), V["vetted"]) and same(graph.nodes(), V["nodes"])
    graph.optimize_device(ROBUST, rc.GATE, relax=pl.E2E["relax"])
    opt = V["opt"]
    assert same(graph.nodes(), opt["nodes"]) and same(graph.edges(), opt["edges"]) and same(graph.report(), opt["refit"])
    assert same(graph.robust_report(), opt["robust"]) and same(graph.prune_report(), opt["prune"])
    mapper.rerender_device(graph)
    gp, gh = mapper.counts()
    assert same(gp, V["planes"][0]) and same(gh, V["planes"][1])
    # vet=None is the chain as it was: the same closures, no flag set, nothing of the marginals touched
    plain, _ = vet_room_objects(lsdmod, ctx, V)
    run_vetted_chain(lsdmod, plain, scratch, mapper, d_in, vet=None)
    assert same(plain.edges(), V["edges"]) and same(plain.nodes(), V["nodes"]) and plain._marg_q is None


def test_the_vetted_chain_does_not_synchronise(lsdmod, ctx):
    V = mc.vet_end_to_end()

    def chain(graph, scratch, mapper, d_in):
        run_vetted_chain(lsdmod, graph, scratch, mapper, d_in)
        graph.optimize_device(ROBUST, rc.GATE, relax=pl.E2E["relax"])
        mapper.rerender_device(graph)
    graph, (scratch, mapper) = vet_room_objects(lsdmod, ctx, V)
    d_in = (dev(V["scans"]), dev(V["lens"]), dev(V["odom"]))
    chain(graph, scratch, mapper, d_in)                                                 # warm: every workspace has its size
    graph2, _ = vet_room_objects(lsdmod, ctx, V)
    graph2.marginals_device("new", VET["marg"], prior=True)                             # (its records and workspace too)
    returns_in_front_of_the_device(lambda: chain(graph2, scratch, mapper, d_in), "append / close_all(vet=) / optimize / rerender")
    assert same(graph2.nodes(), V["opt"]["nodes"]) and same(graph2.vet_reports(), V["vet_reps"])
    gp, gh = mapper.counts()
    assert same(gp, V["planes"][0]) and same(gh, V["planes"][1])
