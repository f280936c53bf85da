"""lsd_enqueue_pg_reduce_device (include/lsd_hip.h, "pose graph"; csrc/k_pgreduce.hip) restated on Python floats in the
header's order, written from the header for the tests (not from the HIP code), and the generated campaign both test files run.

Python floats are IEEE doubles without contraction, so every statement rounds as the device build rounds it; sin / cos are the correctly
rounded ones pose_graph_cases uses.  reduce() gives every output: head, nodes, edges, tracks, store, lengths, descriptors, the map and
the report.  A case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
import pose_graph_cases as pg
import pose_graph_place_cases as pp

PAR_DTYPE = np.dtype([("cell", "f8"), ("ang_bin", "f8"), ("keep", "i4"), ("max_run", "i4")])
REP_DTYPE = np.dtype([("nodes_before", "i4"), ("edges_before", "i4"), ("nodes_after", "i4"), ("edges_after", "i4"), ("redundant", "i4"),
                      ("marked", "i4"), ("retired", "i4"), ("runs", "i4"), ("runs_kept", "i4"), ("longest_run", "i4"), ("dropped_edges", "i4"),
                      ("flags", "u4")])
SIZES = {"lsd_pg_reduce_par": 24, "lsd_pg_reduce_rep": 48}
EDGE_CONTRACTED, EDGE_REJECTED = 8, 4
RETIRED, SPLIT = 1, 2
DEFAULTS = dict(cell=4.0, ang_bin=10.0, keep=1, max_run=64)
TILE = 1024                                                                   # the mover's tile: rows
NAN, INF = float("nan"), float("inf")


def reduce_par(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def ffloor(v):
    return float(math.floor(v)) if math.isfinite(v) else v


def cell_of(nd, par):
    """The cell of a node record, three floats compared with ==, or None."""
    p = pg.pose_of(nd)
    if not all(math.isfinite(v) for v in p):
        return None
    return (ffloor(pg.fdiv(p[0], par["cell"])), ffloor(pg.fdiv(p[1], par["cell"])), ffloor(pg.fdiv(pg.wrap(p[2]), par["ang_bin"])))


def skipped(ed, N, nodes):
    i, j = int(ed["i"]), int(ed["j"])
    if int(ed["flags"]) & pg.EDGE_DISABLED or i == j or not (0 <= i < N and 0 <= j < N):
        return True
    vals = [float(v) for v in ed["z"]] + [float(v) for v in ed["info"]] + list(pg.pose_of(nodes[i])) + list(pg.pose_of(nodes[j]))
    return not all(math.isfinite(v) for v in vals)


def mul(A, B, transposed):
    """sum_t A(r,t) * B(t,q), or with B transposed sum_t A(r,t) * B(q,t); ascending from 0.0, every product made."""
    out = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for q in range(3):
            t = 0.0
            for u in range(3):
                t += A[r][u] * (B[q][u] if transposed else B[u][q])
            out[r][q] = t
    return out


def step(z, S, zn, Sn):
    s, c = pg.sincos_deg(z[2])
    k = gc.K_PI / 180.0
    J1 = [[1.0, 0.0, k * ((-s) * zn[0] - c * zn[1])], [0.0, 1.0, k * (c * zn[0] - s * zn[1])], [0.0, 0.0, 1.0]]
    J2 = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    U1, U2 = mul(mul(J1, S, False), J1, True), mul(mul(J2, Sn, False), J2, True)
    return pg.comp(z, zn), [[U1[r][q] + U2[r][q] for q in range(3)] for r in range(3)]


def reduce(g, desc, par, trace=None):
    """The entry on copies: (the graph after, the descriptors after or None, map int32 [nodes_cap], the report)."""
    with np.errstate(all="ignore"):
        return _reduce(g, desc, par, trace if trace is not None else {})


def _reduce(g, desc, par, tr):
    g = pg.copy_graph(g)
    desc = None if desc is None else desc.copy()
    nodes, edges, tracks = g["nodes"], g["edges"], g["tracks"]
    nodes_cap, edges_cap = len(nodes), len(edges)
    N, E = pg.clamp(g["head"][0]["n_nodes"], nodes_cap), pg.clamp(g["head"][0]["n_edges"], edges_cap)
    keep, max_run = int(par["keep"]), int(par["max_run"])
    # cells and ranks
    seen, cells, redundant = {}, [], []
    for k in range(N):
        c = cell_of(nodes[k], par)
        cells.append(c)
        rank = seen.get(c, 0) if c is not None else 0
        redundant.append(c is not None and rank >= keep)
        if c is not None:
            seen[c] = rank + 1
    # the edges that count
    skip = [skipped(edges[e], N, nodes) for e in range(E)]
    deg, n_in, n_out, in_id, out_id, no_inv = [0] * N, [0] * N, [0] * N, [None] * N, [None] * N, [False] * E
    for e in range(E):
        if skip[e]:
            continue
        i, j = int(edges[e]["i"]), int(edges[e]["j"])
        no_inv[e] = pg.inv3(pg.info_rows([float(v) for v in edges[e]["info"]]))[0] is None
        deg[i] += 1; deg[j] += 1; n_out[i] += 1; n_in[j] += 1
        out_id[i] = e if out_id[i] is None else min(out_id[i], e)
        in_id[j] = e if in_id[j] is None else min(in_id[j], e)
    lasts = set(int(t["last"]) for t in tracks)
    marked, why = [False] * N, [None] * N
    for k in range(N):
        if not redundant[k]:
            continue
        w = []
        if int(nodes[k]["flags"]) & pg.NODE_FIXED:
            w.append("fixed")
        if k in lasts:
            w.append("last")
        if not (deg[k] == 2 and n_in[k] == 1 and n_out[k] == 1):
            w.append("deg_1" if deg[k] == 1 else "two_in" if (deg[k], n_in[k]) == (2, 2) else "deg_3" if deg[k] == 3 else "deg_other")
        else:
            if (int(edges[in_id[k]]["flags"]) | int(edges[out_id[k]]["flags"])) & pg.EDGE_CLOSURE:
                w.append("closure")
            if no_inv[in_id[k]] or no_inv[out_id[k]]:
                w.append("singular")
        why[k], marked[k] = w, not w
    # runs
    retired, head_of, in_run, runs, split, walked = [False] * N, {}, set(), [], 0, set()
    for e0 in range(E):
        if skip[e0]:
            continue
        a, r, lead = int(edges[e0]["i"]), int(edges[e0]["j"]), e0
        if marked[a] or not marked[r]:
            continue
        while True:
            z = tuple(float(v) for v in edges[lead]["z"])
            S = pg.inv3(pg.info_rows([float(v) for v in edges[lead]["info"]]))[0]
            cur, ln, forced, members, dropped = r, 1, False, [], []
            while True:
                f = out_id[cur]
                members.append(cur); dropped.append(f)
                zn = tuple(float(v) for v in edges[f]["z"])
                Sn = pg.inv3(pg.info_rows([float(v) for v in edges[f]["info"]]))[0]
                z, S = step(z, S, zn, Sn)
                b = int(edges[f]["j"])
                if not marked[b]:
                    break
                if ln == max_run:
                    forced = True
                    break
                cur, ln = b, ln + 1
            ok = b != a and all(math.isfinite(v) for v in z) and all(math.isfinite(v) for row in S for v in row)
            inv = pg.inv3(S)[0] if ok else None
            ok = ok and inv is not None
            walked.update(members + ([b] if forced else []))
            runs.append(dict(head=lead, a=a, b=b, len=ln, forced=forced, contracted=ok, ring=b == a))
            if ok:
                head_of[lead] = (a, b, z, (inv[0][0], inv[0][1], inv[1][1], inv[0][2], inv[1][2], inv[2][2]))
                in_run.update(dropped)
                for m in members:
                    retired[m] = True
            if not forced:
                break
            split += 1
            a, lead = b, out_id[b]
            r = int(edges[lead]["j"])
            if not marked[r]:
                break
    # the map
    new, inv_map = np.full(nodes_cap, -1, np.int32), []
    for k in range(N):
        if not retired[k]:
            new[k] = len(inv_map)
            inv_map.append(k)
    n_new = len(inv_map)
    # edges
    old_edges, out_edges, dropped_end = edges.copy(), [], []
    for e in range(E):
        ed = old_edges[e].copy()
        i, j = int(ed["i"]), int(ed["j"])
        inside = 0 <= i < N and 0 <= j < N
        if e in head_of:
            a, b, z, info = head_of[e]
            ed["i"], ed["j"], ed["flags"], ed["reserved"], ed["z"], ed["info"], ed["chi2"] = new[a], new[b], EDGE_CONTRACTED, 0, z, info, 0.0
        elif e in in_run:
            continue
        elif inside and (retired[i] or retired[j]):
            dropped_end.append(e)
            continue
        elif inside:
            ed["i"], ed["j"] = new[i], new[j]
        out_edges.append(ed)
    e_new = len(out_edges)
    for q, ed in enumerate(out_edges):
        edges[q] = ed
    # nodes, rows, lengths, descriptors
    old = dict(nodes=nodes.copy(), store=g["store"].copy(), lens=g["store_lens"].copy(), desc=None if desc is None else desc.copy())
    for d, k in enumerate(inv_map):
        nodes[d], g["store"][d], g["store_lens"][d] = old["nodes"][k], old["store"][k], old["lens"][k]
        if desc is not None:
            desc[d] = old["desc"][k]
    g["store_lens"][n_new:N] = 0
    if desc is not None:
        desc[n_new:N] = np.zeros(1, desc.dtype)[0]
    for t in tracks:
        if 0 <= int(t["last"]) < N:
            t["last"] = new[int(t["last"])]
    g["head"][0]["n_nodes"], g["head"][0]["n_edges"] = n_new, e_new
    rep = np.zeros(1, REP_DTYPE)[0]
    contracted = [r_ for r_ in runs if r_["contracted"]]
    rep["nodes_before"], rep["edges_before"], rep["nodes_after"], rep["edges_after"] = N, E, n_new, e_new
    rep["redundant"], rep["marked"], rep["retired"] = sum(redundant), sum(marked), N - n_new
    rep["runs"], rep["runs_kept"] = len(contracted), len(runs) - len(contracted)
    rep["longest_run"], rep["dropped_edges"] = max([r_["len"] for r_ in contracted], default=0), len(dropped_end)
    rep["flags"] = (RETIRED if N - n_new else 0) | (SPLIT if split else 0)
    tr.update(N=N, E=E, n_new=n_new, e_new=e_new, cells=cells, redundant=redundant, why=why, marked=marked, retired=retired, runs=runs,
              skip=skip, dropped_end=[(e, int(old_edges[e]["flags"])) for e in dropped_end],
              outside=[e for e in range(E) if not (0 <= int(old_edges[e]["i"]) < N and 0 <= int(old_edges[e]["j"]) < N)],
              first_moved=next((k for k in range(N) if new[k] != k), None))
    tr["unreached"] = [k for k in range(N) if marked[k] and k not in walked]
    return g, desc, new, rep


# ---- graphs for the campaign -----------------------------------------------------------------------------------------------------------
def place_pose(p, rng, par, jitter=0.3):
    """A pose inside the cell of place id p: the places lie 3 cells apart along x."""
    c, ab = par["cell"], par["ang_bin"]
    return ((3.0 * p + 0.5) * c + jitter * c * rng.uniform(-1, 1), 0.5 * c + jitter * c * rng.uniform(-1, 1), 0.5 * ab + jitter * ab * rng.uniform(-1, 1))


def spd_info(rng):
    a = rng.uniform(0.5, 4.0, 3)
    return (float(a[0]), float(0.1 * rng.uniform(-1, 1)), float(a[1]), float(0.05 * rng.uniform(-1, 1)), float(0.05 * rng.uniform(-1, 1)), float(a[2]))


def build(name, rng, poses, par, track_of=None, n_tracks=1, stride=3, cap_extra=3, extra=(), fixed=(0,), lasts=None, with_desc=True, shuffle=False,
          well_posed=False, info=None):
    """A graph on the poses: an odometry edge between neighbours of a track, consistent with the poses (z = rel), then the extra edges
    (i, j, flags) or (i, j, flags, z, info); noise in every byte the entry must keep."""
    N = len(poses)
    track_of = track_of or [0] * N
    nodes_cap, n_od = N + cap_extra, 0
    ed = []
    prev = {}
    for k in range(N):
        t = track_of[k]
        if t in prev:
            ed.append((prev[t], k, 0, pg.rel(poses[prev[t]], poses[k]), info or spd_info(rng)))
        prev[t] = k
    for x in extra:
        i, j, fl = x[:3]
        inside = 0 <= i < N and 0 <= j < N
        z = x[3] if len(x) > 3 and x[3] is not None else (pg.rel(poses[i], poses[j]) if inside else (1.0, 2.0, 3.0))
        ed.append((i, j, fl, z, x[4] if len(x) > 4 else (info or spd_info(rng))))
    if shuffle:
        ed = [ed[q] for q in rng.permutation(len(ed))]
    edges_cap = max(len(ed), 1) + cap_extra
    g = pg.new_graph(nodes_cap, edges_cap, stride, n_tracks, rng)
    g["nodes"]["reserved"] = rng.integers(0, 2 ** 62, nodes_cap).astype(np.uint64)
    for k in range(N):
        nd = g["nodes"][k]
        nd["x"], nd["y"], nd["ang"] = poses[k]
        nd["raw"] = tuple(rng.normal(size=3))
        nd["flags"], nd["track"] = (pg.NODE_FIXED if k in fixed else 0), track_of[k]
    for q, (i, j, fl, z, inf) in enumerate(ed):
        e = g["edges"][q]
        e["i"], e["j"], e["flags"], e["z"], e["info"], e["chi2"] = i, j, fl, z, inf, float(rng.uniform(0, 3))
    for t in range(n_tracks):
        g["tracks"][t]["last"] = prev.get(t, -1) if lasts is None else lasts[t]
        g["tracks"][t]["reserved"], g["tracks"][t]["raw"] = int(rng.integers(0, 1000)), tuple(rng.normal(size=3))
    g["store_lens"][:] = rng.integers(0, stride + 1, nodes_cap)
    g["head"][0]["n_nodes"], g["head"][0]["n_edges"] = N, len(ed)
    desc = rng.integers(0, 256, nodes_cap * 72, dtype=np.uint8).view(pp.DESC_DTYPE).copy() if with_desc else None
    return dict(name=name, g=g, desc=desc, par=par, well_posed=well_posed)


def poses_of(places, rng, par, jitter=0.3):
    return [place_pose(p, rng, par, jitter) for p in places]


def fresh(places, n):
    """n place ids no entry of `places` has."""
    top = max(places, default=-1) + 1
    return list(range(top, top + n))


def laps(n, lap):
    return [k % lap for k in range(n)]


SIZES_N = (0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025)
ROWS = (TILE - 1, TILE, TILE + 1)
REASONS = ("fixed", "last", "closure", "deg_1", "deg_3", "two_in", "singular")
CLASSES = (["n_%d" % n for n in SIZES_N] + ["rows_%d" % n for n in ROWS] + ["beams_1", "beams_3", "beams_360", "keep_1", "keep_2", "on_boundary",
           "ang_180", "no_cell"] + ["only_" + r for r in REASONS] + ["skipped_edge_at_retired", "run_at_max_run", "run_split", "kept_whole",
           "ring_unreached", "two_tracks", "closure_dropped", "rejected_dropped", "edge_outside", "nothing_retired", "all_but_anchors", "no_desc",
           "second_tile_moves", "well_posed"])
_campaign = None


def campaign():
    global _campaign
    if _campaign is None:
        _campaign = _make_campaign()
    return _campaign


def _make_campaign():
    out = []
    P = reduce_par
    for rep in range(3):
        rng = np.random.default_rng(7000 + rep)
        par = P()
        # the sizes: laps of 40 places, so that from the second lap on every node is redundant; closures hold some of them
        for n in SIZES_N:
            pl = laps(n, 40)
            extra = [(k - 40, k, pg.EDGE_CLOSURE) for k in range(45, n, 37)]
            out.append(build("n_%d_%d" % (n, rep), rng, poses_of(pl, rng, par), P(max_run=(5, 64, 7)[rep]), stride=(1, 3, 3)[rep], extra=extra,
                             with_desc=rep != 1, shuffle=rep == 2, cap_extra=(3, 40, 1100)[rep] if n >= 1023 else 3))
        # the mover's tile: `rows` survivors, 60 retired in the middle of them
        for rows in ROWS:
            pl = list(range(500)) + [10 + k for k in range(60)] + list(range(500, rows))
            out.append(build("rows_%d_%d" % (rows, rep), rng, poses_of(pl, rng, par), P(max_run=100), stride=(3, 1, 3)[rep], cap_extra=(1, 200, 1100)[rep]))
        # 360 beams; keep 2
        out.append(build("beams_360_%d" % rep, rng, poses_of([0, 1, 2, 1, 2, 3, 0, 4], rng, par), par, stride=360, well_posed=True))
        out.append(build("keep_2_%d" % rep, rng, poses_of([0, 1, 0, 1, 0, 1, 1, 2], rng, par), P(keep=2), well_posed=True))
        # a cell boundary exactly on a coordinate: the one-ulp neighbour below is another cell
        po = poses_of([0, 1, 2, 3, 4, 5], rng, par)
        po[1], po[3], po[4] = (8.0, 2.0, 5.0), (8.0, 2.5, 5.5), (pg.below(8.0), 2.5, 5.5)
        out.append(build("boundary_%d" % rep, rng, po, par, well_posed=True))
        po = poses_of([0, 1, 2, 3, 4, 5], rng, par)
        po[1], po[3], po[4] = (10.0, 2.0, 180.0), (10.5, 2.5, -180.0), (10.5, 2.5, pg.below(180.0))
        out.append(build("ang_180_%d" % rep, rng, po, par))
        po = poses_of([0, 1, 2, 1, 2, 3, 1, 4], rng, par)
        po[4] = (NAN, 1.0, 2.0) if rep else (po[4][0], INF, 0.0)
        out.append(build("no_cell_%d" % rep, rng, po, par))
        # every reason a redundant node stays, one at a time: node 4 revisits place 1
        base = [0, 1, 2, 3, 1, 4, 5]
        out.append(build("fixed_%d" % rep, rng, poses_of(base, rng, par), par, fixed=(0, 4)))
        out.append(build("last_%d" % rep, rng, poses_of(base, rng, par), par, n_tracks=2, lasts=[6, 4]))
        c = build("closure_%d" % rep, rng, poses_of(base, rng, par), par)
        c["g"]["edges"][4 if rep else 3]["flags"] = pg.EDGE_CLOSURE                # (its outgoing or its incoming edge)
        out.append(c)
        out.append(build("deg_1_%d" % rep, rng, poses_of([0, 1, 2, 3, 1], rng, par), par, lasts=[(-1, 2, 77)[rep]]))
        out.append(build("deg_3_%d" % rep, rng, poses_of(base, rng, par), par, extra=[(4, 0, 0) if rep else (0, 4, 0)]))
        out.append(build("two_in_%d" % rep, rng, poses_of([0, 1, 2, 3, 1], rng, par), par, extra=[(0, 4, 0)], lasts=[-1]))
        c = build("singular_%d" % rep, rng, poses_of(base, rng, par), par)
        c["g"]["edges"][3 + rep % 2]["info"] = ((0.0,) * 6, (1.0, 1.0, 1.0, 0.0, 0.0, 1.0), (1.0, 0.0, -1.0, 0.0, 0.0, 1.0))[rep]
        out.append(c)
        # skipped edges do not count and go with the node: a disabled closure, a rejected one, an edge with a NaN
        fl = (pg.EDGE_CLOSURE | pg.EDGE_DISABLED, pg.EDGE_CLOSURE | pg.EDGE_DISABLED | EDGE_REJECTED, 0)[rep]
        out.append(build("skipped_at_%d" % rep, rng, poses_of(base, rng, par), par, extra=[(0, 4, fl, (NAN, 0.0, 0.0) if rep == 2 else None), (4, 6, fl | 1)]))
        out.append(build("rejected_%d" % rep, rng, poses_of(base + [2, 6], rng, par), par, shuffle=True,
                         extra=[(1, 4, pg.EDGE_CLOSURE | pg.EDGE_DISABLED | EDGE_REJECTED), (7, 2, pg.EDGE_CLOSURE | pg.EDGE_DISABLED)]))
        # runs of max_run and max_run + 1 nodes, and a longer one that max_run splits more than once
        for ln in (3, 4, 11):
            pl = [0, 1, 2, 3, 4] + [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3][:ln] + [5]
            out.append(build("run_%d_%d" % (ln, rep), rng, poses_of(pl, rng, par), P(max_run=3), well_posed=True, shuffle=rep == 1))
        # a run kept whole: a motion so large that S overflows, and a ring that comes back to its first node
        c = build("kept_overflow_%d" % rep, rng, poses_of([0, 1, 2, 1, 2, 3, 0, 1, 4], rng, par), par)
        c["g"]["edges"][3]["z"] = (1e200, 0.0, 0.0)
        out.append(c)
        out.append(build("kept_ring_%d" % rep, rng, poses_of([0, 0, 0, 1, 1], rng, par), par, track_of=[0, 0, 0, 1, 1], n_tracks=2, extra=[(2, 0, 0)],
                         lasts=[-1, 4]))
        # a ring of marked nodes that no unmarked node leads into
        out.append(build("ring_%d" % rep, rng, poses_of([0, 1, 2, 0, 0, 0], rng, par), par, track_of=[0, 0, 0, 1, 1, 1], n_tracks=2, extra=[(5, 3, 0)],
                         lasts=[2, -1 - rep]))
        # two interleaved tracks over the same places
        pl = [0, 0, 1, 1, 2, 2, 3, 3, 1, 1, 2, 2, 4, 5]
        out.append(build("two_tracks_%d" % rep, rng, poses_of(pl, rng, par), P(keep=2), track_of=[k % 2 for k in range(len(pl))], n_tracks=2, fixed=(0, 1),
                         well_posed=True, shuffle=rep == 2))
        # edges with an end outside the nodes keep their bytes
        out.append(build("outside_%d" % rep, rng, poses_of(base, rng, par), par, extra=[(-3, 4, 0), (4, 7 + rep, pg.EDGE_CLOSURE), (9, -1, 0)], shuffle=rep == 1))
        # nothing to retire; everything but the anchors
        out.append(build("nothing_%d" % rep, rng, poses_of(list(range(9 + rep)), rng, par), par, extra=[(0, 8, pg.EDGE_CLOSURE)], well_posed=True))
        out.append(build("all_but_anchors_%d" % rep, rng, poses_of([0] * (12 + rep) + [1], rng, par), P(max_run=(64, 100, 13)[rep]), well_posed=True))
        # the second tile moves and the first does not: the first retired node lies behind row 1024
        pl = list(range(1030)) + [5, 6, 7] + list(range(1030, 1040))
        out.append(build("second_tile_%d" % rep, rng, poses_of(pl, rng, par), par, stride=1, cap_extra=5 + 1100 * rep))
        # random walks over few places with closures, several tracks, the edges in any order
        for q in range(2):
            n = int(rng.integers(20, 60))
            pl = [int(v) for v in rng.integers(0, 12, n)]
            nt = 1 + q
            extra = [(int(rng.integers(0, n)), int(rng.integers(0, n)), int(rng.choice([0, 1, 2, 3, 7]))) for _ in range(6)]
            out.append(build("random_%d_%d" % (q, rep), rng, poses_of(pl, rng, par), P(keep=1 + q, max_run=int(rng.integers(1, 6))), n_tracks=nt,
                             track_of=[int(v) for v in rng.integers(0, nt, n)], extra=[x for x in extra if x[0] != x[1]], shuffle=True))
    return out


def run_case(case):
    tr = {}
    g, desc, new, rep = reduce(case["g"], case["desc"], case["par"], tr)
    return g, desc, new, rep, tr


def classes_of(case, tr):
    g, par = case["g"], case["par"]
    N = tr["N"]
    c = set()
    if N in SIZES_N:
        c.add("n_%d" % N)
    if tr["n_new"] in ROWS and tr["n_new"] < N:
        c.add("rows_%d" % tr["n_new"])
    stride = g["store"].shape[1]
    if stride in (1, 3, 360):
        c.add("beams_%d" % stride)
    if any(tr["retired"]):
        c.add("keep_%d" % par["keep"]) if par["keep"] in (1, 2) else None
    nd = g["nodes"]
    if any(math.isfinite(float(nd[k]["x"])) and float(nd[k]["x"]) != 0 and pg.fdiv(float(nd[k]["x"]), par["cell"]) == ffloor(pg.fdiv(float(nd[k]["x"]), par["cell"]))
           for k in range(N)):
        c.add("on_boundary")
    if any(abs(float(nd[k]["ang"])) == 180.0 for k in range(N)):
        c.add("ang_180")
    if any(cl is None for cl in tr["cells"]):
        c.add("no_cell")
    for k in range(N):
        if tr["why"][k] and len(tr["why"][k]) == 1 and tr["why"][k][0] in REASONS:
            c.add("only_" + tr["why"][k][0])
    for e, fl in tr["dropped_end"]:
        c.add("skipped_edge_at_retired")
        if fl & pg.EDGE_CLOSURE and fl & pg.EDGE_DISABLED:
            c.add("rejected_dropped" if fl & EDGE_REJECTED else "closure_dropped")
    for r_ in tr["runs"]:
        if r_["contracted"] and r_["len"] == par["max_run"] and not r_["forced"]:
            c.add("run_at_max_run")
        if r_["forced"]:
            c.add("run_split")
        if not r_["contracted"]:
            c.add("kept_whole")
    if tr["unreached"]:
        c.add("ring_unreached")
    if len(g["tracks"]) >= 2 and any(tr["retired"]) and len(set(int(nd[k]["track"]) for k in range(N) if tr["retired"][k])) >= 2:
        c.add("two_tracks")
    if tr["outside"]:
        c.add("edge_outside")
    if N >= 3 and not any(tr["retired"]):
        c.add("nothing_retired")
    if N >= 3 and tr["n_new"] == 2:
        c.add("all_but_anchors")
    if case["desc"] is None:
        c.add("no_desc")
    if tr["first_moved"] is not None and tr["first_moved"] >= TILE:
        c.add("second_tile_moves")
    if case["well_posed"]:
        c.add("well_posed")
    return c


# ---- end to end: 8.1.18's two laps, reduced, driven on, recognised and relaxed again ---------------------------------------------------------
E2E = dict(reduce=reduce_par(cell=4.0, ang_bin=30.0, keep=1, max_run=8), more=5)
_e2e = None


def end_to_end():
    """pose_graph_loops_cases.end_to_end() (append -> close_all -> optimize), then reduce -> append of `more` further frames -> describe ->
    recognize -> relax -> rerender, restated once and shared."""
    global _e2e
    if _e2e is not None:
        return _e2e
    import pose_graph_loops_cases as pl
    L, R = pl.end_to_end(), pp.PLACE_ROOM
    n, nb, cap = pl.E2E["n"], pl.E2E["n_beams"], len(L["g0"]["nodes"])
    tr = {}
    g4, desc4, new, rep = reduce(L["g3"], L["desc"], E2E["reduce"], tr)
    rng = np.random.default_rng(13)
    truth, odom = [tuple(L["truth"][-1])], [tuple(L["odom"][-1])]
    for k in range(n + 1, n + 1 + E2E["more"]):
        a = 363.0 * k / 24
        truth.append((30.0 + 13.0 * math.cos(math.radians(a)), 23.0 + 10.0 * math.sin(math.radians(a)), pg.wrap(a + 90.0)))
        z = pg.rel(truth[-2], truth[-1])
        odom.append(pg.comp(odom[-1], (z[0] + 0.02 * rng.normal(), z[1] + 0.02 * rng.normal(), z[2] + pl.E2E["bias"] * rng.uniform(0.8, 1.0))))
    truth, odom = np.array(truth[1:]), np.array(odom[1:])
    scans = np.stack([pp.place_room_scan(tuple(p), nb) for p in truth])
    lens = np.full(len(scans), nb, np.int32)
    g5, arep = pg.append(g4, scans, lens, odom, 0, pl.E2E["append"])
    nn = int(g5["head"][0]["n_nodes"])
    desc5 = pp.describe(nn, g5["store"], g5["store_lens"], R["range_max"], desc4.copy())
    work, recs, prep, near, sel, row, q_len, q_pose = pp.recognize(g5, 0, desc5, pl.E2E["place"], np.zeros(cap, np.uint32), L["left"][1])
    g6, rrep = pl.relaxed(g5)
    cols, rows = R["cols"], R["rows"]
    pa, hi = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g6["store"], g6["store_lens"], np.stack([g6["nodes"]["x"], g6["nodes"]["y"], g6["nodes"]["ang"]], axis=1), cols, rows, R["resol"],
                 R["range_max"], pa, hi)
    _e2e = dict(loops=L, trace=tr, g4=g4, desc4=desc4, map=new, rep=rep, truth=truth, odom=odom, scans=scans, lens=lens, g5=g5, append_rep=arep,
                desc5=desc5, place_recs=recs, place_rep=prep, near=near, sel=sel, row=row, q_len=q_len, q_pose=q_pose, g6=g6, relax_rep=rrep,
                planes=(pa, hi))
    return _e2e
