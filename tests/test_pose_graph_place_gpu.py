"""Place recognition on the device (csrc/k_pgplace.hip: lsd_enqueue_pg_describe_device, lsd_enqueue_pg_recognize_device, lsd_pg_describe,
lsd_pg_recognize; PoseGraph.describe_device, recognize_device, close_place_device) against the restatement of
tests/pose_graph_place_cases.py.  One quantisation in fp64, integers after it: every comparison is byte equality."""
import math

import numpy as np
import pytest

import grid_match_cases as gm
import pose_graph_cases as pg
import pose_graph_place_cases as pp
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream

pytestmark = pytest.mark.gpu

GRAPH_PARTS = ("head", "nodes", "tracks", "store", "store_lens")


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


# ---- 1. describe -----------------------------------------------------------------------------------------------------------------------
def check_describe(c, case):
    import torch
    want, _ = pp.run_describe_case(case)
    cap, stride = len(case["desc"]), case["store"].shape[1]
    head = np.zeros(1, pg.HEAD_DTYPE)
    head[0]["n_nodes"], head[0]["n_edges"] = case["head"], 12345
    ins = [Guarded(head), Guarded(case["store"]), Guarded(case["store_lens"])]
    d_desc = Guarded(case["desc"])
    for again in range(2):                                                    # a second launch finds every row valid: the same bytes
        c.enqueue_pg_describe_device(ins[0].ptr, cap, ins[1].ptr, ins[2].ptr, stride, case["range_max"], d_desc.ptr, stream())
        torch.cuda.synchronize()
        got, ok = d_desc.back()
        assert ok and all(i.unchanged() for i in ins), (case["name"], again)
        if not same(got, want):
            g = got.view(pp.DESC_DTYPE)
            bad = [(k, g[k], want[k]) for k in range(cap) if g[k].tobytes() != want[k].tobytes()][:2]
            pytest.fail("%s (launch %d): descriptors differ from the restatement: %r" % (case["name"], again, bad))


def test_describe_campaign_byte_for_byte(lsdmod, ctx):
    for case in pp.describe_campaign():
        check_describe(ctx, case)


def test_describe_a_row_beyond_1024_readings(lsdmod):
    c = lsdmod.Context(0)
    try:
        case = pp.describe_campaign(long_row=True)[0]
        head, store, lens, d_desc = (Guarded(np.zeros(1, pg.HEAD_DTYPE)), Guarded(case["store"]), Guarded(case["store_lens"]), Guarded(case["desc"]))
        assert c.L.lsd_enqueue_pg_describe_device(c.h, head.ptr, len(case["desc"]), store.ptr, lens.ptr, 1025, 4.0, d_desc.ptr, stream()) == INV
        c.set_scan_capacity(1025)
        check_describe(c, case)
    finally:
        c.close()


def test_describe_host_entry(lsdmod, ctx):
    for case in pp.describe_campaign()[::4]:
        n = pg.clamp(case["head"], len(case["desc"]))
        want = pp.describe(n, case["store"], case["store_lens"], case["range_max"], np.zeros(len(case["desc"]), pp.DESC_DTYPE))[:n]
        got = ctx.pg_describe(case["store"][:n], case["store_lens"][:n], case["range_max"])
        assert same(got, want), case["name"]
    assert len(ctx.pg_describe(np.zeros((0, 4, 2)), np.zeros(0, np.int32), 4.0)) == 0


# ---- 2. recognize ----------------------------------------------------------------------------------------------------------------------
OUT_NAMES = ("work", "recs", "rep", "near", "sel", "row", "len", "pose")


def check_recognize(lsdmod, c, case):
    import torch
    work, recs, rep, near, sel, row, q_len, q_pose = pp.run_recognize_case(case)[0]
    g = case["graph"]
    cap, stride, k = len(g["nodes"]), g["store"].shape[1], case["par"]["k"]
    ins = {n: Guarded(g[n]) for n in GRAPH_PARTS}
    d_desc = Guarded(case["desc"])
    outs = [Guarded(case["work"]), filled(16 * k), filled(16), filled(24), filled(24 * cap), Guarded(np.full((stride, 2), 0.125)), filled(4), filled(24)]
    c.enqueue_pg_recognize_device(ins["head"].ptr, ins["nodes"].ptr, cap, ins["tracks"].ptr, ins["store"].ptr, ins["store_lens"].ptr, stride, d_desc.ptr,
                                  lsdmod.pg_place(case["par"]), *[o.ptr for o in outs], stream())
    torch.cuda.synchronize()
    assert all(i.unchanged() for i in ins.values()) and d_desc.unchanged(), case["name"]
    for name, o, want in zip(OUT_NAMES, outs, (work, recs, rep, near, sel, row, np.int32(q_len), q_pose)):
        got, ok = o.back()
        assert ok, (case["name"], name, "a guard was written")
        if not same(got, want):
            w = np.ascontiguousarray(want)
            pytest.fail("%s: %s differs from the restatement: %r != %r" % (case["name"], name, got.view(w.dtype).reshape(w.shape)[:8], w[:8]))


def test_recognize_campaign_byte_for_byte(lsdmod, ctx):
    for case in pp.recognize_campaign():
        check_recognize(lsdmod, ctx, case)


def test_recognize_16384_nodes(lsdmod, ctx):
    import torch
    case = pp.recognize_campaign(big=True)[0]
    check_recognize(lsdmod, ctx, case)
    # and the descriptors of those 16384 rows of 8 readings, through the device
    g = case["graph"]
    d_desc = dev(np.zeros(len(g["nodes"]) * 72, np.uint8))
    ins = [dev(g["head"].view(np.uint8)), dev(g["store"]), dev(g["store_lens"])]
    ctx.enqueue_pg_describe_device(ins[0].data_ptr(), len(g["nodes"]), ins[1].data_ptr(), ins[2].data_ptr(), 8, pp.RANGE_MAX, d_desc.data_ptr(), stream())
    torch.cuda.synchronize()
    assert same(d_desc.cpu().numpy(), case["desc"])


def test_recognize_host_entry(lsdmod, ctx):
    for case in pp.recognize_campaign()[::3]:
        _, recs, rep, _, _, _, _, _ = pp.run_recognize_case(case)[0]
        g = case["graph"]
        n, j = pg.clamp(g["head"][0]["n_nodes"], len(g["nodes"])), int(g["tracks"][0]["last"])
        got_recs, got_rep = ctx.pg_recognize(case["desc"][:n], j, case["par"])
        assert same(got_recs, recs) and same(got_rep, rep), case["name"]


# ---- 3. every refusal leaves the outputs unchanged -------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    case = next(c for c in pp.recognize_campaign() if c["name"] == "tie_dist_0")
    g = case["graph"]
    cap, stride = len(g["nodes"]), g["store"].shape[1]
    ins = {n: Guarded(g[n]) for n in GRAPH_PARTS}
    d_desc = Guarded(case["desc"])
    outs = dict(work=Guarded(case["work"]), recs=filled(16 * 8), rep=filled(16), near=filled(24), sel=filled(24 * cap), row=filled(16 * stride),
                len=filled(4), pose=filled(24))

    def describe(**kw):
        a = dict(head=ins["head"].ptr, cap=cap, store=ins["store"].ptr, lens=ins["store_lens"].ptr, ss=stride, rm=4.0, desc=d_desc.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_describe_device(h, a["head"], a["cap"], a["store"], a["lens"], a["ss"], a["rm"], a["desc"], stream())
    for kw in (dict(head=None), dict(store=None), dict(lens=None), dict(desc=None), dict(cap=0), dict(cap=16385), dict(ss=0), dict(ss=1 << 20),
               dict(rm=0.0), dict(rm=-1.0), dict(rm=math.nan), dict(rm=math.inf), dict(store=ins["store"].ptr + 8), dict(head=ins["head"].ptr + 4),
               dict(desc=d_desc.ptr + 4), dict(lens=ins["store_lens"].ptr + 2)):
        assert describe(**kw) == INV, kw

    def recognize(par=None, **kw):
        a = dict(head=ins["head"].ptr, nodes=ins["nodes"].ptr, cap=cap, track=ins["tracks"].ptr, store=ins["store"].ptr, lens=ins["store_lens"].ptr,
                 ss=stride, desc=d_desc.ptr)
        a.update({n: o.ptr for n, o in outs.items()})
        a.update(kw)
        p = lsdmod.pg_place(dict(case["par"], **(par or {})))
        return L.lsd_enqueue_pg_recognize_device(h, a["head"], a["nodes"], a["cap"], a["track"], a["store"], a["lens"], a["ss"], a["desc"], p, a["work"],
                                                 a["recs"], a["rep"], a["near"], a["sel"], a["row"], a["len"], a["pose"], stream())
    for name in ("head", "nodes", "track", "store", "lens", "desc", "work", "recs", "rep", "near", "sel", "row", "len", "pose"):
        assert recognize(**{name: None}) == INV, name
    for kw in (dict(cap=0), dict(cap=16385), dict(ss=0), dict(ss=1 << 20), dict(store=ins["store"].ptr + 8), dict(row=outs["row"].ptr + 8),
               dict(desc=d_desc.ptr + 4), dict(recs=outs["recs"].ptr + 4), dict(rep=outs["rep"].ptr + 4), dict(near=outs["near"].ptr + 4),
               dict(sel=outs["sel"].ptr + 4), dict(pose=outs["pose"].ptr + 4), dict(nodes=ins["nodes"].ptr + 4), dict(work=outs["work"].ptr + 2),
               dict(len=outs["len"].ptr + 2)):
        assert recognize(**kw) == INV, kw
    for par in (dict(gap=0), dict(gap=-3), dict(window=-1), dict(spread=-1), dict(k=0), dict(k=9), dict(k=2, pick=2), dict(pick=-1), dict(max_dist=16321),
                dict(min_sectors=0), dict(min_sectors=65)):
        assert recognize(par=par) == INV, par
    # the host entries
    desc, recs, rep = case["desc"][:16].copy(), np.zeros(8, pp.PLACE_REC_DTYPE), np.zeros(1, pp.PLACE_REP_DTYPE)
    ok = lsdmod.pg_place(case["par"])
    assert L.lsd_pg_recognize(h, desc.ctypes.data, 0, 3, ok, recs.ctypes.data, rep.ctypes.data) == INV
    assert L.lsd_pg_recognize(h, desc.ctypes.data, 16385, 3, ok, recs.ctypes.data, rep.ctypes.data) == INV
    assert L.lsd_pg_recognize(h, None, 16, 3, ok, recs.ctypes.data, rep.ctypes.data) == INV
    assert L.lsd_pg_recognize(h, desc.ctypes.data, 16, 3, lsdmod.pg_place(dict(case["par"], k=9)), recs.ctypes.data, rep.ctypes.data) == INV
    sc, ln, out = np.ones((2, 4, 2)), np.full(2, 4, np.int32), np.zeros(2, pp.DESC_DTYPE)
    assert L.lsd_pg_describe(h, sc.ctypes.data, ln.ctypes.data, -1, 4, 4.0, out.ctypes.data) == INV
    assert L.lsd_pg_describe(h, sc.ctypes.data, ln.ctypes.data, 2, 0, 4.0, out.ctypes.data) == INV
    assert L.lsd_pg_describe(h, sc.ctypes.data, ln.ctypes.data, 2, 4, 0.0, out.ctypes.data) == INV
    assert L.lsd_pg_describe(h, None, ln.ctypes.data, 2, 4, 4.0, out.ctypes.data) == INV
    assert not recs.view(np.uint8).any() and not rep.view(np.uint8).any() and not out.view(np.uint8).any()
    torch.cuda.synchronize()
    for buf in list(ins.values()) + [d_desc] + list(outs.values()):
        assert buf.unchanged()


# ---- 4. PoseGraph: a loop that pose proximity cannot see, closed by appearance ---------------------------------------------------------
def room_objects(lsdmod, ctx, E):
    R = pp.PLACE_ROOM
    graph = lsdmod.PoseGraph(len(E["g0"]["nodes"]), len(E["g0"]["edges"]), pp.E2E["n_beams"], ctx=ctx)
    mappers = [lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx) for _ in range(2)]
    return graph, mappers


CLOSURE = dict(zip(("cov_scale", "floor_xy", "floor_ang"), pp.E2E["closure"]))


def run_chain(lsdmod, graph, scratch, mapper, d_in):
    graph.append_device(*d_in, append=pp.E2E["append"])
    resp = graph.close_place_device(scratch, place=pp.E2E["place"], search=pp.E2E["search"], response=pp.E2E["response"], smear=(3, gm.GAUSS),
                                    closure=CLOSURE)
    graph.relax_device(pp.E2E["relax"])
    mapper.rerender_device(graph)
    return resp


def test_chain_equals_the_restatement(lsdmod, ctx):
    E = pp.end_to_end()
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    # by pose, nothing is found: the drift is beyond the radius
    graph.append_device(*d_in, append=pp.E2E["append"])
    graph.close_device(scratch, gap=pp.E2E["gap"], radius=pp.E2E["radius"], window=pp.E2E["place"]["window"], search=pp.E2E["search"],
                       response=pp.E2E["response"], smear=(3, gm.GAUSS), closure=CLOSURE)
    near_rec, crep = graph.closure_report()
    assert same(near_rec, E["near_by_pose"]) and int(crep["flags"]) == lsdmod.PG_CLOSURE_NO_ANCHOR and graph.head() == (E["n_nodes"], E["n_edges"] - 1)
    # by appearance, on a fresh graph
    graph, _ = room_objects(lsdmod, ctx, E)
    resp = run_chain(lsdmod, graph, scratch, mapper, d_in)
    near_rec, crep = graph.closure_report()
    assert same(graph.append_report(), E["append_rep"])
    assert same(graph._desc.cpu().numpy(), E["desc"])
    assert same(graph.place_records(), E["recs"]) and same(graph.place_report(), E["place_rep"])
    assert same(graph._place_work.cpu().numpy(), E["work"])
    assert same(near_rec, E["near"]) and same(graph._sel.cpu().numpy(), E["sel"]) and same(graph._q_pose.cpu().numpy(), E["q_pose"])
    assert same(resp.cpu().numpy(), E["resp"])
    assert same(crep, E["closure_rep"]) and int(crep["flags"]) == lsdmod.PG_CLOSURE_APPENDED
    assert same(graph.report(), E["relax_rep"])
    assert graph.head() == (E["n_nodes"], E["n_edges"])
    assert same(graph.nodes(), E["g3"]["nodes"][:E["n_nodes"]]) and same(graph.edges(), E["g3"]["edges"][:E["n_edges"]])
    gp, gh = mapper.counts()
    assert same(gp, E["planes"][0]) and same(gh, E["planes"][1])
    with pytest.raises(lsdmod.LsdError):
        graph.describe_device(pp.PLACE_ROOM["range_max"] * 2)                           # a graph keeps its range_max


def test_chain_does_not_synchronise(lsdmod, ctx):
    E = pp.end_to_end()
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    run_chain(lsdmod, graph, scratch, mapper, d_in)                                     # warm: every workspace has its size
    graph2, _ = room_objects(lsdmod, ctx, E)
    returns_in_front_of_the_device(lambda: run_chain(lsdmod, graph2, scratch, mapper, d_in), "append / close_place / relax / rerender")
    assert same(graph2.nodes(), E["g3"]["nodes"][:E["n_nodes"]])
