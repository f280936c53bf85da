"""The reduce of the pose graph on the device (csrc/k_pgreduce.hip: lsd_enqueue_pg_reduce_device, lsd_pg_reduce; PoseGraph.reduce_device)
against the restatement of tests/pose_graph_reduce_cases.py.  The rule fixes every operation and every order, so every comparison is byte
equality."""
import numpy as np
import pytest

import pose_graph_cases as pg
import pose_graph_loops_cases as pl
import pose_graph_place_cases as pp
import pose_graph_reduce_cases as rc
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream
from test_pose_graph_loops_gpu import room_objects, run_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def check(name, buf, want):
    got, ok = buf.back()
    assert ok, name + ": a guard was written"
    if not same(got, want):
        w = np.ascontiguousarray(want).reshape(-1)
        g = got.view(w.dtype)
        bad = [i for i in range(len(w)) if g[i].tobytes() != w[i].tobytes()][:3]
        pytest.fail("%s differ from the restatement at %r: %r != %r" % (name, bad, [g[i] for i in bad], [w[i] for i in bad]))


def reduce_par(lsdmod, par):
    return lsdmod.lsd_pg_reduce(float(par["cell"]), float(par["ang_bin"]), int(par["keep"]), int(par["max_run"]))


class Launch:
    """One reduce of a campaign case between guards; the workspace, the map and the report start as the fill pattern."""

    def __init__(self, lsdmod, ctx, case, with_rep=True):
        g = case["g"]
        self.case, self.nc, self.ec, self.stride = case, len(g["nodes"]), len(g["edges"]), g["store"].shape[1]
        self.b = {k: Guarded(g[k]) for k in ("head", "nodes", "edges", "tracks", "store", "store_lens")}
        self.desc = None if case["desc"] is None else Guarded(case["desc"])
        ws = lsdmod.pg_reduce_workspace_bytes(self.nc, self.ec, self.stride)
        assert ws > 0
        self.ws, self.map, self.rep = filled(ws), filled(4 * self.nc), filled(48) if with_rep else None
        ctx.enqueue_pg_reduce_device(self.b["head"].ptr, self.b["nodes"].ptr, self.nc, self.b["edges"].ptr, self.ec, self.b["tracks"].ptr,
                                     len(g["tracks"]), self.b["store"].ptr, self.b["store_lens"].ptr, self.stride,
                                     None if self.desc is None else self.desc.ptr, reduce_par(lsdmod, case["par"]), self.map.ptr,
                                     None if self.rep is None else self.rep.ptr, self.ws.ptr, stream())

    def check(self):
        name = self.case["name"]
        g, desc, new, rep, _ = rc.run_case(self.case)
        for k in ("head", "nodes", "edges", "tracks", "store", "store_lens"):
            check("%s: %s" % (name, k), self.b[k], g[k])
        if self.desc is not None:
            check(name + ": descriptors", self.desc, desc)
        check(name + ": map", self.map, new)
        if self.rep is not None:
            check(name + ": report", self.rep, np.array([rep]))
        assert self.ws.back()[1], name + ": a guard of the workspace was written"


# ---- 1. the campaign through the device entry ----------------------------------------------------------------------------------------------
def test_campaign_byte_for_byte_through_the_device_entry(lsdmod, ctx):
    import torch
    runs = [Launch(lsdmod, ctx, c) for c in rc.campaign()]
    twins = [Launch(lsdmod, ctx, c, with_rep=False) for c in rc.campaign()[::7]]     # the same call without the optional report
    torch.cuda.synchronize()
    for L in runs + twins:
        L.check()


def test_host_entry_equals_the_device_entry(lsdmod, ctx):
    for case in rc.campaign():
        if len(case["g"]["nodes"]) > 300:
            continue
        g0 = case["g"]
        want_g, want_d, want_map, want_rep, _ = rc.run_case(case)
        head, nodes, edges, tracks, store, lens, desc, new, rep = ctx.pg_reduce(g0["head"], g0["nodes"], g0["edges"], g0["tracks"], g0["store"],
                                                                              g0["store_lens"], case["desc"], reduce_par(lsdmod, case["par"]))
        got = dict(head=head, nodes=nodes, edges=edges, tracks=tracks, store=store, store_lens=lens)
        assert all(same(got[k], want_g[k]) for k in got), case["name"]
        assert (desc is None and want_d is None) or same(desc, want_d), case["name"]
        assert same(new, want_map) and same(rep, want_rep), case["name"]


# ---- 2. the mover alone at a larger shape -----------------------------------------------------------------------------------------------------
def test_mover_16384_rows_of_64_beams(lsdmod, ctx):
    """Every third node lies where the node two in front of it lies and is retired: 5461 runs of one node, and all but the first two of
    16384 rows of 64 readings move, through sixteen tiles."""
    import torch
    rng = np.random.default_rng(99)
    par = rc.reduce_par()
    places, top = [], 0
    for k in range(16384):
        if k % 3 == 2:
            places.append(places[k - 2])
        else:
            places.append(top)
            top += 1
    case = rc.build("mover", rng, rc.poses_of(places, rng, par), par, stride=64, cap_extra=0, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0))
    assert len(case["g"]["nodes"]) == 16384
    L = Launch(lsdmod, ctx, case)
    torch.cuda.synchronize()
    L.check()
    rep = L.rep.back()[0].view(rc.REP_DTYPE)[0]
    assert int(rep["retired"]) == 5461 and int(rep["runs"]) == 5461 and int(rep["longest_run"]) == 1


# ---- 3. every refusal leaves the outputs unchanged -------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    case = next(c for c in rc.campaign() if c["name"] == "run_4_0")
    g = case["g"]
    nc, ec, stride = len(g["nodes"]), len(g["edges"]), g["store"].shape[1]
    b = {k: Guarded(g[k]) for k in ("head", "nodes", "edges", "tracks", "store", "store_lens")}
    b["desc"] = Guarded(case["desc"])
    b["map"], b["rep"], b["ws"] = filled(4 * nc), filled(48), filled(lsdmod.pg_reduce_workspace_bytes(nc, ec, stride))

    def call(par=None, **kw):
        a = dict(nc=nc, ec=ec, nt=1, ss=stride)
        a.update({k: v.ptr for k, v in b.items()})
        a.update(kw)
        p = reduce_par(lsdmod, dict(case["par"], **(par or {})))
        return L.lsd_enqueue_pg_reduce_device(h, a["head"], a["nodes"], a["nc"], a["edges"], a["ec"], a["tracks"], a["nt"], a["store"], a["store_lens"],
                                              a["ss"], a["desc"], p, a["map"], a["rep"], a["ws"], stream())
    for name in ("head", "nodes", "edges", "tracks", "store", "store_lens", "map", "ws"):
        assert call(**{name: None}) == INV, name
    assert L.lsd_enqueue_pg_reduce_device(None, b["head"].ptr, b["nodes"].ptr, nc, b["edges"].ptr, ec, b["tracks"].ptr, 1, b["store"].ptr,
                                          b["store_lens"].ptr, stride, None, reduce_par(lsdmod, case["par"]), b["map"].ptr, None, b["ws"].ptr, stream()) == INV
    for kw in (dict(nc=0), dict(nc=16385), dict(ec=0), dict(ec=65537), dict(ss=0), dict(ss=1 << 20), dict(nt=0), dict(nt=-1),
               dict(store=b["store"].ptr + 8), dict(ws=b["ws"].ptr + 8), dict(head=b["head"].ptr + 4), dict(nodes=b["nodes"].ptr + 4),
               dict(edges=b["edges"].ptr + 4), dict(tracks=b["tracks"].ptr + 4), dict(desc=b["desc"].ptr + 4), dict(rep=b["rep"].ptr + 4),
               dict(store_lens=b["store_lens"].ptr + 2), dict(map=b["map"].ptr + 2)):
        assert call(**kw) == INV, kw
    nan, inf = float("nan"), float("inf")
    for par in (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(ang_bin=0.0), dict(ang_bin=-5.0), dict(ang_bin=nan),
                dict(ang_bin=inf), dict(ang_bin=360.5), dict(keep=0), dict(keep=-1), dict(max_run=0), dict(max_run=-2)):
        assert call(par=par) == INV, par
    ws = lsdmod.pg_reduce_workspace_bytes
    assert ws(0, 8, 4) == 0 and ws(16385, 8, 4) == 0 and ws(8, 0, 4) == 0 and ws(8, 65537, 4) == 0 and ws(8, 8, 0) == 0 and ws(8, 8, -3) == 0
    # the host entry
    hd, no, ed, tr = g["head"].copy(), g["nodes"].copy(), g["edges"].copy(), g["tracks"].copy()
    st, sl, mp, rp = g["store"].copy(), g["store_lens"].copy(), np.zeros(nc, np.int32), np.zeros(1, rc.REP_DTYPE)
    ok = reduce_par(lsdmod, case["par"])

    def host(par=ok, **kw):
        a = dict(head=hd.ctypes.data, nodes=no.ctypes.data, nc=nc, edges=ed.ctypes.data, ec=ec, tracks=tr.ctypes.data, nt=1, store=st.ctypes.data,
                 lens=sl.ctypes.data, ss=stride, map=mp.ctypes.data, rep=rp.ctypes.data)
        a.update(kw)
        return L.lsd_pg_reduce(h, a["head"], a["nodes"], a["nc"], a["edges"], a["ec"], a["tracks"], a["nt"], a["store"], a["lens"], a["ss"], None, par,
                               a["map"], a["rep"])
    for name in ("head", "nodes", "edges", "tracks", "store", "lens", "map", "rep"):
        assert host(**{name: None}) == INV, name
    for kw in (dict(nc=0), dict(nc=16385), dict(ec=0), dict(ec=65537), dict(ss=0), dict(nt=0)):
        assert host(**kw) == INV, kw
    assert host(par=reduce_par(lsdmod, dict(case["par"], keep=0))) == INV and host(par=reduce_par(lsdmod, dict(case["par"], cell=nan))) == INV
    assert same(hd, g["head"]) and same(no, g["nodes"]) and same(ed, g["edges"]) and same(st, g["store"]) and not mp.any() and not rp.view(np.uint8).any()
    torch.cuda.synchronize()
    for name, buf in b.items():
        assert buf.unchanged(), name
    with pytest.raises(lsdmod.LsdError):
        lsdmod.pg_reduce(dict(cells=3.0))


# ---- 4. PoseGraph: a full store accepts appends again ------------------------------------------------------------------------------------------
FULL = dict(append=dict(min_dist=2.0, min_ang=10.0, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0)), reduce=rc.reduce_par(), n_beams=4, cap=6)


def full_store_frames():
    rng = np.random.default_rng(5)
    poses = np.array([(12.0 * p + 2.0, 2.0, 5.0) for p in (0, 1, 2, 0, 1, 2, 3, 4)])
    return rng.uniform(0.5, 3.0, (8, FULL["n_beams"], 2)), np.full(8, FULL["n_beams"], np.int32), poses


def test_full_store_accepts_appends_again_without_a_host_wait(lsdmod, ctx):
    scans, lens, poses = full_store_frames()
    g = pg.new_graph(FULL["cap"], 8, FULL["n_beams"])
    g, _ = pg.append(g, scans[:6], lens[:6], poses[:6], 0, FULL["append"])
    refused, rep_refused = pg.append(g, scans[6:], lens[6:], poses[6:], 0, FULL["append"])
    assert int(rep_refused["flags"]) & pg.NODES_FULL and int(rep_refused["nodes"]) == 0 and same(refused["nodes"], g["nodes"])
    g2, _, new, rrep = rc.reduce(refused, np.zeros(FULL["cap"], pp.DESC_DTYPE), FULL["reduce"])
    assert int(rrep["retired"]) == 2
    g3, rep_accepted = pg.append(g2, scans[6:], lens[6:], poses[6:], 0, FULL["append"])
    assert int(rep_accepted["nodes"]) == 2 and int(rep_accepted["flags"]) == 0
    d_first, d_more = [dev(a) for a in (scans[:6], lens[:6], poses[:6])], [dev(a) for a in (scans[6:], lens[6:], poses[6:])]
    graphs = [lsdmod.PoseGraph(FULL["cap"], 8, FULL["n_beams"], ctx=ctx) for _ in range(2)]

    def run(graph):
        graph.append_device(*d_first, append=FULL["append"])
        graph.append_device(*d_more, append=FULL["append"])                   # refused: the store is full
        graph.reduce_device(FULL["reduce"])
        graph.append_device(*d_more, append=FULL["append"])
    run(graphs[0])                                                            # warm
    returns_in_front_of_the_device(lambda: run(graphs[1]), "append / reduce / append")
    graph = graphs[-1]
    assert graph.head() == (6, 5) and same(graph.append_report(), rep_accepted) and same(graph.reduce_report(), rrep)
    assert same(graph.node_map(), new)
    assert same(graph.nodes(), g3["nodes"]) and same(graph.edges(), g3["edges"][:5])
    assert same(graph._store.cpu().numpy(), g3["store"]) and same(graph._store_lens.cpu().numpy(), g3["store_lens"])
    assert same(graph._tracks.cpu().numpy(), g3["tracks"])


# ---- 5. PoseGraph: the chain of 8.1.18 reduced, driven on, recognised and relaxed ------------------------------------------------------------
def reduced_chain(lsdmod, graph, scratch, mapper, d_in, d_more):
    run_chain(lsdmod, graph, scratch, mapper, d_in)
    graph.reduce_device(rc.E2E["reduce"])
    graph.append_device(*d_more, append=pl.E2E["append"])
    graph.recognize_device(pp.PLACE_ROOM["range_max"], place=pl.E2E["place"])
    graph.relax_device(pl.E2E["relax"])
    mapper.rerender_device(graph)


def test_chain_equals_the_restatement_and_does_not_synchronise(lsdmod, ctx):
    E = rc.end_to_end()
    Lp = E["loops"]
    d_in = (dev(Lp["scans"]), dev(Lp["lens"]), dev(Lp["odom"]))
    d_more = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, Lp)
    reduced_chain(lsdmod, graph, scratch, mapper, d_in, d_more)                  # warm: every workspace has its size
    graph, _ = room_objects(lsdmod, ctx, Lp)
    returns_in_front_of_the_device(lambda: reduced_chain(lsdmod, graph, scratch, mapper, d_in, d_more),
                                   "append / close_all / optimize / reduce / append / recognize / relax / rerender")
    assert same(graph.reduce_report(), E["rep"]) and same(graph.node_map(), E["map"])
    assert same(graph.append_report(), E["append_rep"]) and same(graph._desc.cpu().numpy(), E["desc5"])
    assert same(graph.place_records(), E["place_recs"]) and same(graph.place_report(), E["place_rep"])
    assert same(graph._near.cpu().numpy(), E["near"]) and same(graph._sel.cpu().numpy(), E["sel"]) and same(graph._q_scan.cpu().numpy(), E["row"])
    n, e = (int(v) for v in E["g6"]["head"][0])
    assert graph.head() == (n, e) and same(graph.report(), E["relax_rep"])
    assert same(graph._nodes.cpu().numpy(), E["g6"]["nodes"]) and same(graph.edges(), E["g6"]["edges"][:e])
    assert same(graph._store_lens.cpu().numpy(), E["g6"]["store_lens"]) and same(graph._store.cpu().numpy()[:n], E["g6"]["store"][:n])
    gp, gh = mapper.counts()
    assert same(gp, E["planes"][0]) and same(gh, E["planes"][1])
    # what indexed the old numbering is forgotten
    with pytest.raises(lsdmod.LsdError):
        graph.find_loops_device()
    assert len(graph.marginal_records()) == 0
