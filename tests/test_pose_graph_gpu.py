"""The pose graph on the device (csrc/k_pgbuild.hip, csrc/k_posegraph.hip: lsd_enqueue_pg_append_device, lsd_enqueue_pg_near_device,
lsd_enqueue_pg_closure_device, lsd_enqueue_pg_relax_device, lsd_pg_relax, lsd_pg_append; PoseGraph, GridMapper.rerender_device,
Localizer.append_last_tick) against the restatement of tests/pose_graph_cases.py.  The rule fixes every operation and every order, so
every comparison is byte equality."""
import math

import numpy as np
import pytest

import fa_restatement as fr
import grid_match_cases as gm
import pose_graph_cases as pg
from pose_graph_device import INV, Guarded, dev, filled, returns_in_front_of_the_device, same, stream

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


# ---- 1. the relaxation: the campaign in launches of 1, 2 and 5 graphs ------------------------------------------------------------------
def relax_batches():
    """The campaign's cases grouped by their parameters (a launch has one set), each group cut into launches of 1, 2, 5, 1, 2, 5, .."""
    groups = {}
    for c in pg.relax_campaign():
        groups.setdefault(tuple(c["par"][k] for k in pg.RELAX_KEYS), []).append(c)
    out, sizes, k = [], (1, 2, 5), 0
    for cases in groups.values():
        while cases:
            out.append(cases[:sizes[k % 3]])
            cases = cases[sizes[k % 3]:]
            k += 1
    return out


def laid_out(batch, rng):
    """heads, nodes [G, nodes_cap], edges [G, edges_cap] of a launch: every graph's records in front, noise behind them."""
    nc = max(max(len(c["nodes"]) for c in batch), 1) + 2
    ec = max(max(len(c["edges"]) for c in batch), 1) + 3
    heads = np.zeros(len(batch), pg.HEAD_DTYPE)
    nodes = rng.integers(0, 256, (len(batch), nc * 64), dtype=np.uint8).view(pg.NODE_DTYPE).reshape(len(batch), nc).copy()
    edges = rng.integers(0, 256, (len(batch), ec * 96), dtype=np.uint8).view(pg.EDGE_DTYPE).reshape(len(batch), ec).copy()
    for g, c in enumerate(batch):
        heads[g]["n_nodes"], heads[g]["n_edges"] = len(c["nodes"]), len(c["edges"])
        nodes[g, :len(c["nodes"])] = c["nodes"]
        edges[g, :len(c["edges"])] = c["edges"]
    return heads, nodes, edges, nc, ec


def expected(batch, nodes, edges):
    want_n, want_e, want_r = nodes.copy(), edges.copy(), np.zeros(len(batch), pg.RELAX_REP_DTYPE)
    for g, c in enumerate(batch):
        n, e, rep, _ = pg.run_relax_case(c)
        want_n[g, :len(n)], want_e[g, :len(e)], want_r[g] = n, e, rep
    return want_n, want_e, want_r


@pytest.mark.parametrize("batch", relax_batches(), ids=lambda b: "%s_x%d" % (b[0]["name"], len(b)))
def test_relax_campaign_byte_for_byte(lsdmod, ctx, batch):
    import torch
    rng = np.random.default_rng(len(batch[0]["name"]))
    heads, nodes, edges, nc, ec = laid_out(batch, rng)
    want_n, want_e, want_r = expected(batch, nodes, edges)
    ws_bytes = lsdmod.pg_workspace_bytes(nc, ec)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    d_h, d_n, d_e = Guarded(heads), Guarded(nodes), Guarded(edges)
    d_ws, d_r = filled(ws_bytes * len(batch)), filled(56 * len(batch))
    ctx.enqueue_pg_relax_device(len(batch), d_h.ptr, d_n.ptr, nc, d_e.ptr, ec, d_ws.ptr, d_r.ptr, lsdmod.pg_relax(batch[0]["par"]), stream())
    torch.cuda.synchronize()
    assert d_h.unchanged() and d_ws.back()[1]
    for name, d, want in (("nodes", d_n, want_n), ("edges", d_e, want_e), ("reports", d_r, want_r)):
        got, ok = d.back()
        assert ok, name + ": a guard was written"
        if not same(got, want):
            dt = want.dtype
            g = got.view(dt).reshape(want.shape)
            bad = [(i, g[i], want[i]) for i in np.ndindex(want.shape) if g[i].tobytes() != want[i].tobytes()][:3]
            pytest.fail("%s differ from the restatement: %r" % (name, bad))


def test_relax_host_entry(lsdmod, ctx):
    for c in pg.relax_campaign()[::5]:
        n, e, rep, _ = pg.run_relax_case(c)
        got_n, got_e, got_r = ctx.pg_relax(c["nodes"], c["edges"], c["par"])
        assert same(got_n, n) and same(got_e, e) and same(got_r, rep), c["name"]


# ---- 2. append, near, closure ----------------------------------------------------------------------------------------------------------
GRAPH_PARTS = ("head", "nodes", "edges", "tracks", "store", "store_lens")


def noisy_poses(poses, pitch, seed):
    rec = np.random.default_rng(seed).integers(0, 256, (len(poses), pitch), dtype=np.uint8)
    rec[:, :24] = np.ascontiguousarray(poses, np.float64).view(np.uint8).reshape(len(poses), 24)
    return rec


@pytest.mark.parametrize("pitch", [24, 720])
def test_append_campaign_byte_for_byte(lsdmod, ctx, pitch):
    import torch
    for c in pg.append_campaign():
        g = c["graph"]
        d = {k: Guarded(g[k]) for k in GRAPH_PARTS}
        want = g
        for step, (sc, ln, po, track) in enumerate(c["steps"]):
            want, want_rep = pg.append(want, sc, ln, po, track, c["par"])
            ins = [Guarded(sc), Guarded(ln), Guarded(noisy_poses(po, pitch, step))]
            d_rep = filled(16)
            ctx.enqueue_pg_append_device(ins[0].ptr, ins[1].ptr, len(ln), sc.shape[1], ins[2].ptr, pitch, d["head"].ptr, d["nodes"].ptr, len(g["nodes"]),
                                         d["edges"].ptr, len(g["edges"]), d["tracks"].ptr + 32 * track, track, d["store"].ptr, d["store_lens"].ptr,
                                         g["store"].shape[1], lsdmod.pg_append(c["par"]), d_rep.ptr, stream())
            torch.cuda.synchronize()
            assert all(i.unchanged() for i in ins), c["name"]
            got, ok = d_rep.back()
            assert ok and same(got, want_rep), (c["name"], step, got.view(pg.APPEND_REP_DTYPE), want_rep)
            for k in GRAPH_PARTS:
                got, ok = d[k].back()
                assert ok and same(got, want[k]), (c["name"], step, k)


def test_append_host_entry(lsdmod, ctx):
    for c in pg.append_campaign()[::3]:
        want = got = c["graph"]
        for sc, ln, po, track in c["steps"]:
            want, want_rep = pg.append(want, sc, ln, po, track, c["par"])
            tr = got["tracks"].copy()
            hd, no, ed, tr[track], st, sl, rep = ctx.pg_append(sc, ln, po, got["head"], got["nodes"], got["edges"], got["tracks"][track], got["store"],
                                                               got["store_lens"], track, c["par"])
            got = dict(head=np.array([hd]), nodes=no, edges=ed, tracks=tr, store=st, store_lens=sl)
            assert same(rep, want_rep), c["name"]
            for k in GRAPH_PARTS:
                assert same(got[k], want[k]), (c["name"], k)


def test_near_campaign_byte_for_byte(lsdmod, ctx):
    import torch
    for c in pg.near_campaign():
        g = c["graph"]
        (rec, sel, row, q_len, q_pose), _ = pg.run_near_case(c)
        ins = {k: Guarded(g[k]) for k in GRAPH_PARTS}
        stride = g["store"].shape[1]
        outs = [filled(24), filled(24 * len(g["nodes"])), Guarded(np.full((stride, 2), 0.125)), filled(4), filled(24)]
        ctx.enqueue_pg_near_device(ins["head"].ptr, ins["nodes"].ptr, len(g["nodes"]), ins["tracks"].ptr, ins["store"].ptr, ins["store_lens"].ptr, stride,
                                   c["gap"], c["radius"], c["window"], *[o.ptr for o in outs], stream())
        torch.cuda.synchronize()
        assert all(i.unchanged() for i in ins.values()), c["name"]
        for name, o, want in zip(("rec", "sel", "row", "len", "pose"), outs, (rec, sel, row, np.int32(q_len), q_pose)):
            got, ok = o.back()
            assert ok and same(got, want), (c["name"], name)


def test_closure_campaign_byte_for_byte(lsdmod, ctx):
    import torch
    for c in pg.closure_campaign():
        g = c["graph"]
        want, want_rep = pg.closure(g, c["near"], c["resp"], c["par"])
        d = {k: Guarded(g[k]) for k in ("head", "nodes", "edges")}
        ins = [Guarded(c["near"]), Guarded(c["resp"])]
        d_rep = filled(16)
        ctx.enqueue_pg_closure_device(d["head"].ptr, d["nodes"].ptr, len(g["nodes"]), d["edges"].ptr, len(g["edges"]), ins[0].ptr, ins[1].ptr,
                                      lsdmod.pg_closure(dict(zip(("cov_scale", "floor_xy", "floor_ang"), c["par"]))), d_rep.ptr, stream())
        torch.cuda.synchronize()
        assert all(i.unchanged() for i in ins) and d["nodes"].unchanged(), c["name"]
        got, ok = d_rep.back()
        assert ok and same(got, want_rep), (c["name"], got.view(pg.CLOSURE_REP_DTYPE), want_rep)
        for k in ("head", "edges"):
            got, ok = d[k].back()
            assert ok and same(got, want[k]), (c["name"], k)


# ---- 3. every refusal leaves the outputs unchanged -------------------------------------------------------------------------------------
def test_refusals_leave_outputs_unchanged(lsdmod, ctx):
    import torch
    L, h = ctx.L, ctx.h
    c = next(c for c in pg.relax_campaign() if c["name"] == "well_posed_8_0")
    heads, nodes, edges, nc, ec = laid_out([c], np.random.default_rng(1))
    d_h, d_n, d_e, d_ws, d_r = Guarded(heads), Guarded(nodes), Guarded(edges), filled(lsdmod.pg_workspace_bytes(nc, ec)), filled(56)
    good = dict(g=1, h=d_h.ptr, n=d_n.ptr, nc=nc, e=d_e.ptr, ec=ec, ws=d_ws.ptr, r=d_r.ptr)
    par = dict(pg.RELAX_DEFAULTS)
    bad_args = [dict(g=-1), dict(h=None), dict(n=None), dict(e=None), dict(ws=None), dict(r=None), dict(nc=0), dict(nc=16385), dict(ec=0), dict(ec=65537),
                dict(n=d_n.ptr + 4), dict(r=d_r.ptr + 4), dict(ws=d_ws.ptr + 1)]
    bad_pars = [dict(lambda0=-1.0), dict(lambda0=math.nan), dict(lambda_min=math.inf), dict(up=1.0), dict(down=0.5), dict(cg_tol=-1e-3), dict(eps=math.nan),
                dict(iters=-1), dict(iters=65536), dict(cg_iters=-1), dict(cg_iters=65536)]
    for kw in bad_args:
        a = dict(good, **kw)
        st = L.lsd_enqueue_pg_relax_device(h, a["g"], a["h"], a["n"], a["nc"], a["e"], a["ec"], lsdmod.pg_relax(par), a["ws"], a["r"], stream())
        assert st == INV, kw
    for kw in bad_pars:
        st = L.lsd_enqueue_pg_relax_device(h, 1, d_h.ptr, d_n.ptr, nc, d_e.ptr, ec, lsdmod.pg_relax(dict(par, **kw)), d_ws.ptr, d_r.ptr, stream())
        assert st == INV, kw
    assert L.lsd_enqueue_pg_relax_device(h, 0, d_h.ptr, d_n.ptr, nc, d_e.ptr, ec, lsdmod.pg_relax(par), d_ws.ptr, d_r.ptr, stream()) == 0
    assert lsdmod.pg_workspace_bytes(0, 4) == 0 and lsdmod.pg_workspace_bytes(4, 65537) == 0 and lsdmod.pg_workspace_bytes(16384, 65536) > 0
    rep = np.zeros(1, pg.RELAX_REP_DTYPE)
    assert L.lsd_pg_relax(h, c["nodes"].ctypes.data, len(c["nodes"]), c["edges"].ctypes.data, len(c["edges"]), lsdmod.pg_relax(dict(par, up=0.5)),
                          rep.ctypes.data) == INV
    # append, near, closure
    ac = pg.append_campaign()[0]
    g = ac["graph"]
    sc, ln, po, _ = ac["steps"][0]
    d = {k: Guarded(g[k]) for k in pg_parts()}
    i_sc, i_ln, i_po, d_rep = Guarded(sc), Guarded(ln), Guarded(po), filled(16)
    stride = g["store"].shape[1]

    def app(**kw):
        a = dict(sc=i_sc.ptr, ln=i_ln.ptr, n=len(ln), stride=sc.shape[1], po=i_po.ptr, pitch=24, nc=len(g["nodes"]), ec=len(g["edges"]), ss=stride,
                 par=ac["par"], head=d["head"].ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_append_device(h, a["sc"], a["ln"], a["n"], a["stride"], a["po"], a["pitch"], a["head"], d["nodes"].ptr, a["nc"],
                                              d["edges"].ptr, a["ec"], d["tracks"].ptr, 0, d["store"].ptr, d["store_lens"].ptr, a["ss"],
                                              lsdmod.pg_append(a["par"]), d_rep.ptr, stream())
    for kw in (dict(sc=None), dict(n=-1), dict(stride=0), dict(stride=1 << 20), dict(pitch=16), dict(pitch=28), dict(nc=0), dict(ec=65537), dict(ss=0),
               dict(head=None), dict(sc=i_sc.ptr + 8), dict(po=i_po.ptr + 4), dict(par=dict(ac["par"], min_dist=-1.0)),
               dict(par=dict(ac["par"], min_ang=math.nan)), dict(par=dict(ac["par"], info=(1.0, 0.0, math.inf, 0.0, 0.0, 1.0)))):
        assert app(**kw) == INV, kw
    assert app(n=0) == 0
    o_rec, o_sel, o_row, o_len, o_pose = filled(24), filled(24 * len(g["nodes"])), filled(16 * stride), filled(4), filled(24)

    def near(**kw):
        a = dict(nc=len(g["nodes"]), ss=stride, gap=2, radius=3.0, window=1, rec=o_rec.ptr, row=o_row.ptr)
        a.update(kw)
        return L.lsd_enqueue_pg_near_device(h, d["head"].ptr, d["nodes"].ptr, a["nc"], d["tracks"].ptr, d["store"].ptr, d["store_lens"].ptr, a["ss"],
                                            a["gap"], a["radius"], a["window"], a["rec"], o_sel.ptr, a["row"], o_len.ptr, o_pose.ptr, stream())
    for kw in (dict(nc=0), dict(ss=0), dict(gap=0), dict(radius=-1.0), dict(radius=math.nan), dict(window=-1), dict(rec=None), dict(rec=o_rec.ptr + 4),
               dict(row=o_row.ptr + 8)):
        assert near(**kw) == INV, kw
    cc = pg.closure_campaign()[0]
    i_near, i_resp, c_rep = Guarded(cc["near"]), Guarded(cc["resp"]), filled(16)

    def clo(**kw):
        a = dict(nc=len(g["nodes"]), ec=len(g["edges"]), near=i_near.ptr, resp=i_resp.ptr, par=(1.0, 1.0, 1.0))
        a.update(kw)
        return L.lsd_enqueue_pg_closure_device(h, d["head"].ptr, d["nodes"].ptr, a["nc"], d["edges"].ptr, a["ec"], a["near"], a["resp"],
                                               lsdmod.lsd_pg_closure(*a["par"]), c_rep.ptr, stream())
    for kw in (dict(nc=0), dict(ec=0), dict(near=None), dict(resp=None), dict(near=i_near.ptr + 4), dict(par=(-1.0, 1.0, 1.0)), dict(par=(1.0, math.nan, 1.0))):
        assert clo(**kw) == INV, kw
    torch.cuda.synchronize()
    for buf in [d_h, d_n, d_e, d_ws, d_r, d_rep, o_rec, o_sel, o_row, o_len, o_pose, c_rep] + list(d.values()):
        assert buf.unchanged()


def pg_parts():
    return GRAPH_PARTS


# ---- 4. PoseGraph: the chain, and the tick ---------------------------------------------------------------------------------------------
def room_objects(lsdmod, ctx, E):
    R = gm.ROOM
    graph = lsdmod.PoseGraph(len(E["g0"]["nodes"]), len(E["g0"]["edges"]), pg.E2E["n_beams"], ctx=ctx)
    mappers = [lsdmod.GridMapper(R["cols"], R["rows"], R["resol"], 0.0, 0.0, R["range_max"], ctx=ctx) for _ in range(2)]
    return graph, mappers


def run_chain(lsdmod, graph, scratch, mapper, E, d_in):
    smear = (3, gm.GAUSS)
    graph.append_device(*d_in, append=pg.E2E["append"])
    resp = graph.close_device(scratch, gap=pg.E2E["gap"], radius=pg.E2E["radius"], window=pg.E2E["window"], search=pg.E2E["search"],
                              response=pg.E2E["response"], smear=smear, closure=dict(zip(("cov_scale", "floor_xy", "floor_ang"), pg.E2E["closure"])))
    graph.relax_device(pg.E2E["relax"])
    mapper.rerender_device(graph)
    return resp


def test_chain_equals_the_restatement(lsdmod, ctx):
    E = pg.end_to_end()
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    resp = run_chain(lsdmod, graph, scratch, mapper, E, d_in)
    near_rec, crep = graph.closure_report()
    assert same(graph.append_report(), E["append_rep"])
    assert same(near_rec, E["near"]) and same(crep, E["closure_rep"])
    assert same(resp.cpu().numpy(), E["resp"])
    assert same(graph.report(), E["relax_rep"])
    assert graph.head() == (E["n_nodes"], E["n_edges"])
    assert same(graph.nodes(), E["g3"]["nodes"][:E["n_nodes"]]) and same(graph.edges(), E["g3"]["edges"][:E["n_edges"]])
    gp, gh = mapper.counts()
    assert same(gp, E["planes"][0]) and same(gh, E["planes"][1])
    hit = graph.disable_edges(chi2_above=float(graph.edges()["chi2"].max()) / 2)
    assert len(hit) >= 1 and (graph.edges()["flags"][hit] & lsdmod.PG_EDGE_DISABLED).all()
    graph.fix(3)
    assert graph.nodes()["flags"][3] & lsdmod.PG_NODE_FIXED and graph.nodes()["flags"][0] & lsdmod.PG_NODE_FIXED


def test_chain_does_not_synchronise(lsdmod, ctx):
    E = pg.end_to_end()
    graph, (scratch, mapper) = room_objects(lsdmod, ctx, E)
    d_in = (dev(E["scans"]), dev(E["lens"]), dev(E["odom"]))
    run_chain(lsdmod, graph, scratch, mapper, E, d_in)                                  # warm: every workspace has its size
    graph2, _ = room_objects(lsdmod, ctx, E)
    returns_in_front_of_the_device(lambda: run_chain(lsdmod, graph2, scratch, mapper, E, d_in), "append / close / relax / rerender")
    assert same(graph2.nodes(), E["g3"]["nodes"][:E["n_nodes"]])


FRAMES = 20
TICK_PAR = dict(min_dist=0.5, min_ang=1.0, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0))


@pytest.fixture(scope="module")
def log(lsdmod, ctx, oracle):
    """The data log's first 20 frames: map cache, map lines, map parameters, raw lidar, odometry, the ingested scans and lengths."""
    m, mp, lid, odom = fr.load_log("data")
    lid, odom = lid[:FRAMES], odom[:FRAMES + 1]
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsdmod.z_occ_max_dis)
    ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    scans, lens = lsdmod.lidar_frames_batch(lid)
    return dict(mc=mc, ml=ml, mp=mp, lid=lid, odom=odom, scans=np.ascontiguousarray(scans), lens=np.asarray(lens, np.int32))


def states_of(lsdmod, out):
    import torch
    torch.cuda.synchronize()
    return out[0].cpu().numpy().reshape(-1).view(lsdmod.FA_STATE_DTYPE).reshape(out[0].shape[:2])


def check_graph(graph, want, rep):
    assert same(graph.append_report(), rep)
    nn, ne = int(want["head"][0]["n_nodes"]), int(want["head"][0]["n_edges"])
    assert graph.head() == (nn, ne)
    assert same(graph.nodes(), want["nodes"][:nn]) and same(graph.edges(), want["edges"][:ne])
    assert same(graph._tracks.cpu().numpy(), want["tracks"])
    assert same(graph._store.cpu().numpy(), want["store"]) and same(graph._store_lens.cpu().numpy(), want["store_lens"])


def test_localizer_appends_its_last_tick(lsdmod, ctx, log):
    loc = lsdmod.Localizer(log["mc"], log["ml"], log["mp"], 1, odom0=log["odom"][0], ctx=ctx)
    graph = lsdmod.PoseGraph(FRAMES + 2, FRAMES + 2, loc.n_beams, ctx=ctx)
    with pytest.raises(lsdmod.LsdError):
        loc.append_last_tick(graph)                                                     # no tick yet
    out = loc.step_device(dev(log["lid"][None]), dev(log["odom"][None, 1:]))
    loc.append_last_tick(graph, append=TICK_PAR)
    poses = states_of(lsdmod, out)["x"][0, :, :3]                                       # the device's own states
    want, rep = pg.append(pg.new_graph(FRAMES + 2, FRAMES + 2, loc.n_beams), log["scans"], log["lens"], poses, 0, TICK_PAR)
    assert int(rep["nodes"]) >= 2
    check_graph(graph, want, rep)


def test_fleet_appends_a_robot_of_its_map(lsdmod, ctx, log):
    S, k = 4, FRAMES // 4
    ids = [0, 1, 0, 1]
    maps = (log["mc"], log["ml"], log["mp"])
    fleet = lsdmod.FleetLocalizer([maps, maps], ids, ctx=ctx)
    od0 = np.stack([log["odom"][s * k] for s in range(S)]); od0[:, 0] = 0.0
    fleet.reset(range(S), od0)
    od = np.stack([log["odom"][s * k + 1:s * k + 1 + k] for s in range(S)])
    out = fleet.step_device(dev(log["lid"].reshape(S, k, 360, 2)), dev(od))
    graph = lsdmod.PoseGraph(k + 2, k + 2, fleet.n_beams, n_tracks=S, ctx=ctx)
    fleet.append_last_tick(graph, 0, 2, append=TICK_PAR)                                # robot 2 is on map 0: track 2
    with pytest.raises(lsdmod.LsdError):
        fleet.append_last_tick(graph, 0, 1)                                             # robot 1 is on map 1
    poses = states_of(lsdmod, out)["x"][2, :, :3]
    want, rep = pg.append(pg.new_graph(k + 2, k + 2, fleet.n_beams, S), log["scans"][2 * k:3 * k], log["lens"][2 * k:3 * k], poses, 2, TICK_PAR)
    check_graph(graph, want, rep)
