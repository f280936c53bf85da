"""Every loop of a track in one pass, on the device (csrc/k_pgloops.hip: lsd_enqueue_pg_recognize_all_device, lsd_enqueue_pg_loops_device,
lsd_enqueue_pg_loop_select_device, lsd_pg_recognize_all, lsd_pg_loops; PoseGraph.recognize_all_device, find_loops_device,
close_all_device) against the restatement of tests/pose_graph_loops_cases.py.  Integers but for one turned pose: every comparison is byte
equality."""
import numpy as np
import pytest

import grid_match_cases as gm
import pose_graph_cases as pg
import pose_graph_loops_cases as pl
import pose_graph_place_cases as pp
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream

pytestmark = pytest.mark.gpu

GRAPH_PARTS = ("head", "nodes", "tracks", "store", "store_lens")


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


# ---- 1. the batch ----------------------------------------------------------------------------------------------------------------------
def run_batch(lsdmod, c, case):
    """(recs, reps) the device leaves for a batch case, the inputs and the guards checked."""
    import torch
    g = case["graph"]
    head, d_desc = Guarded(g["head"]), Guarded(case["desc"])
    d_recs, d_reps = Guarded(case["recs"]), Guarded(case["reps"])
    c.enqueue_pg_recognize_all_device(head.ptr, len(g["nodes"]), d_desc.ptr, lsdmod.pg_place(case["par"]), case["q_lo"], case["n_q"], d_recs.ptr,
                                      d_reps.ptr, stream())
    torch.cuda.synchronize()
    assert head.unchanged() and d_desc.unchanged(), case["name"]
    (recs, ok1), (reps, ok2) = d_recs.back(), d_reps.back()
    assert ok1 and ok2, (case["name"], "a guard was written")
    return recs.view(pp.PLACE_REC_DTYPE).reshape(case["recs"].shape), reps.view(pp.PLACE_REP_DTYPE)


def check_batch(lsdmod, c, case):
    (recs, reps), _ = pl.run_batch_case(case)
    got_recs, got_reps = run_batch(lsdmod, c, case)
    if not (same(got_recs, recs) and same(got_reps, reps)):
        bad = [q for q in range(len(reps)) if not (same(got_recs[q], recs[q]) and same(got_reps[q], reps[q]))][:3]
        pytest.fail("%s: rows %r differ from the restatement: %r %r != %r %r" % (case["name"], bad, got_recs[bad[0]], got_reps[bad[0]], recs[bad[0]],
                                                                                 reps[bad[0]]))


def test_batch_campaign_byte_for_byte(lsdmod, ctx):
    for case in pl.batch_campaign():
        check_batch(lsdmod, ctx, case)


def test_batch_16384_nodes(lsdmod, ctx):
    for case in pl.batch_campaign(big=True):
        check_batch(lsdmod, ctx, case)


def test_batch_against_the_single_device_entry(lsdmod, ctx):
    """Query by query on the same descriptors, on the graphs of at most 257 nodes: the bytes of lsd_enqueue_pg_recognize_device."""
    import torch
    seen = 0
    for case in pl.batch_campaign():
        g = case["graph"]
        cap, stride, k = len(g["nodes"]), g["store"].shape[1], case["par"]["k"]
        if cap > 260 or case["n_q"] == 0:
            continue
        got_recs, got_reps = run_batch(lsdmod, ctx, case)
        ins = {n: dev(g[n].view(np.uint8) if g[n].dtype.names else g[n]) for n in GRAPH_PARTS}
        d_desc = dev(case["desc"].view(np.uint8))
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
        nq = case["n_q"]
        work, recs, reps = z(4 * cap), z(16 * k * nq), z(16 * nq)
        near, sel, row, q_len, pose = z(24), z(24 * cap), z(16 * stride), z(4), z(24)
        par = lsdmod.pg_place(case["par"])
        last = ins["tracks"].view(torch.int32)
        for q in range(nq):
            last[0] = case["q_lo"] + q                                        # (in stream order, in front of the launch that reads it)
            ctx.enqueue_pg_recognize_device(ins["head"].data_ptr(), ins["nodes"].data_ptr(), cap, ins["tracks"].data_ptr(), ins["store"].data_ptr(),
                                            ins["store_lens"].data_ptr(), stride, d_desc.data_ptr(), par, work.data_ptr(),
                                            recs.data_ptr() + 16 * k * q, reps.data_ptr() + 16 * q, near.data_ptr(), sel.data_ptr(), row.data_ptr(),
                                            q_len.data_ptr(), pose.data_ptr(), stream())
        torch.cuda.synchronize()
        assert same(recs.cpu().numpy(), got_recs[:nq]) and same(reps.cpu().numpy(), got_reps[:nq]), case["name"]
        seen += 1
    assert seen > 40


def test_batch_host_entry(lsdmod, ctx):
    for case in pl.batch_campaign()[::5]:
        (recs, reps), _ = pl.run_batch_case(case)
        g = case["graph"]
        n = pg.clamp(g["head"][0]["n_nodes"], len(g["nodes"]))
        lo, nq = case["q_lo"], max(0, min(case["n_q"], n - case["q_lo"]))     # (the host entry's capacity is n_nodes itself)
        if n < 1 or lo > n:
            continue
        got_recs, got_reps = ctx.pg_recognize_all(case["desc"][:n], lo, nq, case["par"])
        assert same(got_recs, recs[:nq]) and same(got_reps, reps[:nq]), case["name"]
    d = pp.random_desc(9, np.random.default_rng(3))
    recs, reps = ctx.pg_recognize_all(d, place=dict(gap=2, k=2))              # n_q None: every node
    assert recs.shape == (9, 2) and [int(v) for v in reps["query"]] == list(range(9))


# ---- 2. the loops ----------------------------------------------------------------------------------------------------------------------
def run_loops(lsdmod, c, case):
    import torch
    head = np.zeros(1, pg.HEAD_DTYPE)
    head[0]["n_nodes"], head[0]["n_edges"] = 54321, case["head_edges"]
    ecap, k = len(case["edges"]), case["k"]
    ins = [Guarded(case["recs"]), Guarded(case["reps"]), Guarded(head), Guarded(case["edges"])]
    ws = filled(lsdmod.pg_loops_workspace_bytes(case["n_q"], k, ecap))
    d_loops, d_rep = filled(16 * case["par"]["max_loops"]), filled(16)
    c.enqueue_pg_loops_device(ins[0].ptr, ins[1].ptr, case["q_lo"], case["n_q"], k, ins[2].ptr, case["nodes_cap"], ins[3].ptr, ecap, case["par"], ws.ptr,
                              d_loops.ptr, d_rep.ptr, stream())
    torch.cuda.synchronize()
    assert all(i.unchanged() for i in ins) and ws.back()[1], case["name"]
    (loops, ok1), (rep, ok2) = d_loops.back(), d_rep.back()
    assert ok1 and ok2, (case["name"], "a guard was written")
    return loops.view(pl.LOOP_REC_DTYPE), rep.view(pl.LOOPS_REP_DTYPE)[0]


def test_loops_campaign_byte_for_byte(lsdmod, ctx):
    for case in pl.loops_campaign():
        (loops, rep), _ = pl.run_loops_case(case)
        got_loops, got_rep = run_loops(lsdmod, ctx, case)
        assert same(got_rep, rep), (case["name"], got_rep, rep)
        assert same(got_loops, loops), (case["name"], got_loops[:8], loops[:8])


def test_loops_host_entry(lsdmod, ctx):
    for case in pl.loops_campaign()[::4]:
        E = pg.clamp(case["head_edges"], len(case["edges"]))
        nq = case["n_q"]
        loops, rep = pl.find_loops(case["recs"], case["reps"], nq, E, case["edges"][:max(E, 1)], case["par"])
        got_loops, got_rep = ctx.pg_loops(case["recs"][:nq], case["reps"][:nq], case["edges"][:E], case["par"])
        assert same(got_loops, loops) and same(got_rep, rep), case["name"]


# ---- 3. the selection ------------------------------------------------------------------------------------------------------------------
def test_select_campaign_byte_for_byte(lsdmod, ctx):
    import torch
    for case in pl.select_campaign():
        g = case["graph"]
        cap, stride = len(g["nodes"]), g["store"].shape[1]
        ins = {n: Guarded(g[n]) for n in GRAPH_PARTS}
        d_loops, d_lrep = Guarded(case["loops"]), Guarded(case["loops_rep"])
        for m in case["ms"]:
            want = pl.run_select_case(case, m)
            outs = [filled(24), filled(24 * cap), Guarded(np.full((stride, 2), 0.125)), filled(4), filled(24)]
            ctx.enqueue_pg_loop_select_device(ins["head"].ptr, ins["nodes"].ptr, cap, ins["store"].ptr, ins["store_lens"].ptr, stride, case["gap"],
                                              case["window"], d_loops.ptr, d_lrep.ptr, m, *[o.ptr for o in outs], stream())
            torch.cuda.synchronize()
            for name, o, w in zip(("near", "sel", "row", "len", "pose"), outs, (want[0], want[1], want[2], np.int32(want[3]), want[4])):
                got, ok = o.back()
                assert ok, (case["name"], m, name, "a guard was written")
                assert same(got, w), (case["name"], m, name)
        assert all(i.unchanged() for i in ins.values()) and d_loops.unchanged() and d_lrep.unchanged(), case["name"]


# ---- 4. every refusal leaves the outputs unchanged -------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    case = next(c for c in pl.batch_campaign() if c["name"] == "q_lo_0")
    g = case["graph"]
    cap, stride, k = len(g["nodes"]), g["store"].shape[1], case["par"]["k"]
    ins = {n: Guarded(g[n]) for n in GRAPH_PARTS}
    d_desc, d_edges = Guarded(case["desc"]), Guarded(np.zeros(8, pg.EDGE_DTYPE))
    outs = dict(recs=Guarded(case["recs"]), reps=Guarded(case["reps"]), ws=filled(lsdmod.pg_loops_workspace_bytes(case["n_q"], k, 8)), loops=filled(16 * 64),
                lrep=filled(16), near=filled(24), sel=filled(24 * cap), row=filled(16 * stride), len=filled(4), pose=filled(24))

    def batch(par=None, **kw):
        a = dict(head=ins["head"].ptr, cap=cap, desc=d_desc.ptr, lo=case["q_lo"], nq=case["n_q"], recs=outs["recs"].ptr, reps=outs["reps"].ptr)
        a.update(kw)
        p = lsdmod.pg_place(dict(case["par"], **(par or {})))
        return L.lsd_enqueue_pg_recognize_all_device(h, a["head"], a["cap"], a["desc"], p, a["lo"], a["nq"], a["recs"], a["reps"], stream())
    for name in ("head", "desc", "recs", "reps"):
        assert batch(**{name: None}) == INV, name
    for kw in (dict(cap=0), dict(cap=16385), dict(lo=-1), dict(nq=-1), dict(lo=cap, nq=1), dict(lo=0, nq=cap + 1), dict(lo=2 ** 31 - 1, nq=2 ** 31 - 1),
               dict(head=ins["head"].ptr + 4), dict(desc=d_desc.ptr + 4), dict(recs=outs["recs"].ptr + 4), dict(reps=outs["reps"].ptr + 4)):
        assert batch(**kw) == INV, kw
    for par in (dict(gap=0), dict(gap=-3), dict(window=-1), dict(spread=-1), dict(k=0), dict(k=9), dict(k=2, pick=2), dict(pick=-1), dict(max_dist=16321),
                dict(min_sectors=0), dict(min_sectors=65)):
        assert batch(par=par) == INV, par
    assert batch(nq=0) == 0 and batch(lo=cap, nq=0) == 0                       # nothing launched

    def loops(par=None, **kw):
        a = dict(recs=outs["recs"].ptr, reps=outs["reps"].ptr, lo=case["q_lo"], nq=case["n_q"], k=k, head=ins["head"].ptr, cap=cap, edges=d_edges.ptr, ecap=8,
                 ws=outs["ws"].ptr, loops=outs["loops"].ptr, lrep=outs["lrep"].ptr)
        a.update(kw)
        p = lsdmod.pg_loops(dict(dict(max_loops=8, spread=2), **(par or {})))
        return L.lsd_enqueue_pg_loops_device(h, a["recs"], a["reps"], a["lo"], a["nq"], a["k"], a["head"], a["cap"], a["edges"], a["ecap"], p, a["ws"],
                                             a["loops"], a["lrep"], stream())
    for name in ("recs", "reps", "head", "edges", "ws", "loops", "lrep"):
        assert loops(**{name: None}) == INV, name
    for kw in (dict(cap=0), dict(cap=16385), dict(ecap=0), dict(ecap=65537), dict(k=0), dict(k=9), dict(lo=-1), dict(nq=-1), dict(lo=cap, nq=1),
               dict(lo=0, nq=cap + 1), dict(recs=outs["recs"].ptr + 4), dict(reps=outs["reps"].ptr + 4), dict(head=ins["head"].ptr + 4),
               dict(edges=d_edges.ptr + 4), dict(ws=outs["ws"].ptr + 4), dict(loops=outs["loops"].ptr + 4), dict(lrep=outs["lrep"].ptr + 4)):
        assert loops(**kw) == INV, kw
    for par in (dict(max_loops=0), dict(max_loops=65), dict(max_loops=-1), dict(spread=-1)):
        assert loops(par=par) == INV, par
    assert lsdmod.pg_loops_workspace_bytes(-1, 1, 8) == 0 and lsdmod.pg_loops_workspace_bytes(4, 9, 8) == 0
    assert lsdmod.pg_loops_workspace_bytes(4, 1, 0) == 0 and lsdmod.pg_loops_workspace_bytes(16385, 1, 8) == 0

    def select(**kw):
        a = dict(head=ins["head"].ptr, nodes=ins["nodes"].ptr, cap=cap, store=ins["store"].ptr, lens=ins["store_lens"].ptr, ss=stride, gap=5, window=2,
                 loops=outs["loops"].ptr, lrep=outs["lrep"].ptr, m=0)
        a.update({n: outs[n].ptr for n in ("near", "sel", "row", "len", "pose")})
        a.update(kw)
        return L.lsd_enqueue_pg_loop_select_device(h, a["head"], a["nodes"], a["cap"], a["store"], a["lens"], a["ss"], a["gap"], a["window"], a["loops"],
                                                   a["lrep"], a["m"], a["near"], a["sel"], a["row"], a["len"], a["pose"], stream())
    for name in ("head", "nodes", "store", "lens", "loops", "lrep", "near", "sel", "row", "len", "pose"):
        assert select(**{name: None}) == INV, name
    for kw in (dict(cap=0), dict(cap=16385), dict(ss=0), dict(ss=1 << 20), dict(gap=0), dict(window=-1), dict(m=-1), dict(m=64),
               dict(store=ins["store"].ptr + 8), dict(row=outs["row"].ptr + 8), dict(head=ins["head"].ptr + 4), dict(nodes=ins["nodes"].ptr + 4),
               dict(loops=outs["loops"].ptr + 4), dict(lrep=outs["lrep"].ptr + 4), dict(near=outs["near"].ptr + 4), dict(sel=outs["sel"].ptr + 4),
               dict(pose=outs["pose"].ptr + 4), dict(lens=ins["store_lens"].ptr + 2), dict(len=outs["len"].ptr + 2)):
        assert select(**kw) == INV, kw
    # the host entries
    desc = case["desc"][:16].copy()
    recs, reps = np.zeros((16, 3), pp.PLACE_REC_DTYPE), np.zeros(16, pp.PLACE_REP_DTYPE)
    lp, lr = np.zeros(8, pl.LOOP_REC_DTYPE), np.zeros(1, pl.LOOPS_REP_DTYPE)
    ok, okl = lsdmod.pg_place(case["par"]), lsdmod.pg_loops()
    for n_nodes, lo, nq in ((0, 0, 0), (16385, 0, 4), (16, -1, 4), (16, 0, -1), (16, 14, 3)):
        assert L.lsd_pg_recognize_all(h, desc.ctypes.data, n_nodes, lo, nq, ok, recs.ctypes.data, reps.ctypes.data) == INV, (n_nodes, lo, nq)
    assert L.lsd_pg_recognize_all(h, None, 16, 0, 4, ok, recs.ctypes.data, reps.ctypes.data) == INV
    assert L.lsd_pg_recognize_all(h, desc.ctypes.data, 16, 0, 4, lsdmod.pg_place(dict(case["par"], k=9)), recs.ctypes.data, reps.ctypes.data) == INV
    ed = np.zeros(4, pg.EDGE_DTYPE)
    for nq, kk, ne, par in ((-1, 3, 4, okl), (16385, 3, 4, okl), (16, 0, 4, okl), (16, 9, 4, okl), (16, 3, -1, okl), (16, 3, 65537, okl),
                            (16, 3, 4, lsdmod.pg_loops(max_loops=65)), (16, 3, 4, lsdmod.pg_loops(spread=-1))):
        assert L.lsd_pg_loops(h, recs.ctypes.data, reps.ctypes.data, nq, kk, ed.ctypes.data, ne, par, lp.ctypes.data, lr.ctypes.data) == INV, (nq, kk, ne)
    assert L.lsd_pg_loops(h, None, reps.ctypes.data, 16, 3, ed.ctypes.data, 4, okl, lp.ctypes.data, lr.ctypes.data) == INV
    assert not any(a.view(np.uint8).any() for a in (recs, reps, lp, lr))
    torch.cuda.synchronize()
    for buf in list(ins.values()) + [d_desc, d_edges] + list(outs.values()):
        assert buf.unchanged()


# ---- 5. PoseGraph: every loop of two laps closed in one pass ---------------------------------------------------------------------------
def room_objects(lsdmod, ctx, E):
    R = pp.PLACE_ROOM
    graph = lsdmod.PoseGraph(len(E["g0"]["nodes"]), len(E["g0"]["edges"]), pl.E2E["n_beams"], ctx=ctx)
    mappers = [lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx) for _ in range(2)]
    return graph, mappers


CLOSURE = dict(zip(("cov_scale", "floor_xy", "floor_ang"), pl.E2E["closure"]))
ROBUST = dict(kernel="huber", delta=1e6, scope="closures")                   # (a delta above every sqrt(chi2) met: the plain relaxation's bytes)


def run_chain(lsdmod, graph, scratch, mapper, d_in):
    graph.append_device(*d_in, append=pl.E2E["append"])
    resp = graph.close_all_device(scratch, place=pl.E2E["place"], loops=pl.E2E["loops"], search=pl.E2E["search"], response=pl.E2E["response"],
                                  smear=(3, gm.GAUSS), closure=CLOSURE)
    graph.optimize_device(ROBUST, gate=1e12, max_reject=0, relax=pl.E2E["relax"], refit=pl.E2E["relax"])
    mapper.rerender_device(graph)
    return resp


def test_chain_equals_the_restatement(lsdmod, ctx):
    E = pl.end_to_end()
    # close_place_device at the end of the track: the one closure of the fixture's condition 1
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    graph.append_device(*d_in, append=pl.E2E["append"])
    graph.close_place_device(scratch, place=pl.E2E["place"], search=pl.E2E["search"], response=pl.E2E["response"], smear=(3, gm.GAUSS), closure=CLOSURE)
    near_rec, crep = graph.closure_report()
    assert same(near_rec, E["single_near"]) and same(crep, E["single_closure_rep"])
    assert same(graph.edges(), E["single"]["edges"][:graph.head()[1]]) and graph.head()[1] == int(E["g1"]["head"][0]["n_edges"]) + 1
    # every loop, on a fresh graph
    graph, _ = room_objects(lsdmod, ctx, E)
    resp = run_chain(lsdmod, graph, scratch, mapper, d_in)
    assert tuple(resp.shape) == (pl.E2E["loops"]["max_loops"], 192)
    cap, k = graph.nodes_cap, pl.E2E["place"]["k"]
    assert same(graph.append_report(), E["append_rep"]) and same(graph._desc.cpu().numpy(), E["desc"])
    assert same(graph._all_recs.cpu().numpy()[:cap * k], E["recs"]) and same(graph._all_reps.cpu().numpy()[:cap], E["reps"])
    assert same(graph.loop_records(), E["loops"]) and same(graph.loops_report(), E["loops_rep"])
    nears, creps = graph.closure_reports()
    assert same(nears, E["nears"]) and same(creps, E["closure_reps"])
    assert same(resp.cpu().numpy(), E["resps"])
    n_loops = int(E["loops_rep"]["n_loops"])
    assert [int(f) for f in creps["flags"]] == [lsdmod.PG_CLOSURE_APPENDED] * n_loops + [lsdmod.PG_CLOSURE_NO_ANCHOR] * (8 - n_loops)
    assert graph.head() == (E["n_nodes"], E["n_edges"])
    assert same(graph.report(), E["relax_rep"])
    assert same(graph.nodes(), E["g3"]["nodes"][:E["n_nodes"]]) and same(graph.edges(), E["g3"]["edges"][:E["n_edges"]])
    gp, gh = mapper.counts()
    assert same(gp, E["planes"][0]) and same(gh, E["planes"][1])
    # a second pass finds every loop known and closes nothing
    graph.close_all_device(scratch, place=pl.E2E["place"], loops=pl.E2E["loops"], search=pl.E2E["search"], response=pl.E2E["response"],
                           smear=(3, gm.GAUSS), closure=CLOSURE)
    rep = graph.loops_report()
    assert int(rep["n_known"]) >= n_loops and graph.head()[1] >= E["n_edges"]
    assert not any((int(L["query"]), int(L["anchor"])) in {(int(o["query"]), int(o["anchor"])) for o in E["loops"][:n_loops]} for L in graph.loop_records())
    with pytest.raises(lsdmod.LsdError):
        lsdmod.PoseGraph(8, 8, 4, ctx=ctx).find_loops_device()                # nothing to choose from yet


def test_chain_does_not_synchronise(lsdmod, ctx):
    E = pl.end_to_end()
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    run_chain(lsdmod, graph, scratch, mapper, d_in)                                     # warm: every workspace has its size
    graph2, _ = room_objects(lsdmod, ctx, E)
    returns_in_front_of_the_device(lambda: run_chain(lsdmod, graph2, scratch, mapper, d_in), "append / close_all / optimize / rerender")
    assert same(graph2.nodes(), E["g3"]["nodes"][:E["n_nodes"]])
