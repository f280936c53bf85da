"""Every loop of a track in one pass (include/lsd_hip.h, "pose graph": lsd_enqueue_pg_recognize_all_device, lsd_enqueue_pg_loops_device,
lsd_enqueue_pg_loop_select_device; csrc/k_pgloops.hip) restated for the tests, and the generated campaigns both test
files run.

The batch is pose_graph_place_cases.recognize once per query with the track's last set to it: nothing of the single entry is stated again.
The choice of the loops and the selection are written from the header's words.  Everything is integers but the one turned pose.  A case
class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
import grid_match_cases as gm
import grid_response_cases as gr
import pose_graph_cases as pg
import pose_graph_place_cases as pp

LOOPS_MAX = 64
LOOP_REC_DTYPE = np.dtype([("query", "i4"), ("anchor", "i4"), ("shift", "i4"), ("dist", "u4")])
LOOPS_REP_DTYPE = np.dtype([("n_pairs", "i4"), ("n_known", "i4"), ("n_loops", "i4"), ("reserved", "i4")])
SIZES = {"lsd_pg_loops_par": 8, "lsd_pg_loop_rec": 16, "lsd_pg_loops_rep": 16}
LOOPS_KEYS = ("max_loops", "spread")
LOOPS_DEFAULTS = dict(max_loops=8, spread=2)
EDGE_REJECTED = 4


def loops_par(**kw):
    assert set(kw) <= set(LOOPS_KEYS)
    return dict(LOOPS_DEFAULTS, **kw)


# ---- the batch: the single entry, query by query ---------------------------------------------------------------------------------------
def recognize_all(g, desc, par, q_lo, n_q, recs, reps, traces=None):
    """lsd_enqueue_pg_recognize_all_device: (recs [rows, k], reps [rows]) after the call (copies; rows >= n_q, the rest keeps its bytes)."""
    recs, reps = recs.copy(), reps.copy()
    gq = pg.copy_graph(g)
    work, q_scan = np.zeros(len(g["nodes"]), np.uint32), np.zeros((g["store"].shape[1], 2))
    for q in range(n_q):
        gq["tracks"][0]["last"] = q_lo + q
        tr = {}
        out = pp.recognize(gq, 0, desc, par, work, q_scan, tr)
        recs[q], reps[q] = out[1], out[2]
        if traces is not None:
            traces.append(tr)
    return recs, reps


# ---- the distinct loops ----------------------------------------------------------------------------------------------------------------
def find_loops(recs, reps, n_q, head_edges, edges, par, trace=None):
    """lsd_enqueue_pg_loops_device: (loops [max_loops], the report).  recs [rows, k], reps [rows]; edges [edges_cap]."""
    max_loops, spread = int(par["max_loops"]), int(par["spread"])
    E = pg.clamp(head_edges, len(edges))
    closures = [(max(int(e["i"]), int(e["j"])), min(int(e["i"]), int(e["j"])), x) for x, e in enumerate(edges[:E]) if int(e["flags"]) & pg.EDGE_CLOSURE]
    pairs, known = [], []
    for q in range(n_q):
        for r in recs[q]:
            if int(r["anchor"]) >= 0:
                p = (int(r["dist"]), int(reps[q]["query"]), int(r["anchor"]), int(r["shift"]))
                by = [x for hi, lo, x in closures if abs(p[1] - hi) <= spread and abs(p[2] - lo) <= spread]
                (known if by else pairs).append(p)
                if by and trace is not None:
                    trace.setdefault("known_by", []).append((p, by))
    n_pairs = len(pairs) + len(known)
    loops = np.zeros(max_loops, LOOP_REC_DTYPE)
    loops["query"], loops["anchor"] = -1, -1
    open_, rounds = list(pairs), []
    for m in range(max_loops):
        if not open_:
            break
        d, q, a, s = min(open_)                                               # (dist, query, anchor): distinct among the pairs
        loops[m]["query"], loops[m]["anchor"], loops[m]["shift"], loops[m]["dist"] = q, a, s, d
        gone = [p for p in open_ if abs(p[1] - q) <= spread and abs(p[2] - a) <= spread]
        rounds.append(dict(chosen=(d, q, a, s), open=list(open_), gone=gone))
        open_ = [p for p in open_ if p not in gone]
    rep = np.zeros((), LOOPS_REP_DTYPE)
    rep["n_pairs"], rep["n_known"], rep["n_loops"] = n_pairs, len(known), len(rounds)
    if trace is not None:
        trace.update(pairs=pairs, known=known, rounds=rounds, left=open_, E=E, closures=closures, par=dict(par))
    return loops, rep


def loops_by_sorting(recs, reps, n_q, head_edges, edges, par):
    """The same choice written a second way: the pairs sorted once, then one sweep that keeps a pair unless a kept one or a closure is
    within `spread` of it on both axes.  [(query, anchor, shift, dist)], at most max_loops."""
    sp = int(par["spread"])
    E = min(max(int(head_edges), 0), len(edges))
    cl = np.array([(max(e["i"], e["j"]), min(e["i"], e["j"])) for e in edges[:E] if e["flags"] & 2], np.int64).reshape(-1, 2)
    rows = []
    for q in range(n_q):
        for r in recs[q]:
            if r["anchor"] >= 0:
                rows.append((int(r["dist"]), int(reps[q]["query"]), int(r["anchor"]), int(r["shift"])))
    kept = []
    for d, q, a, s in sorted(rows):
        if len(cl) and bool(((np.abs(cl[:, 0] - q) <= sp) & (np.abs(cl[:, 1] - a) <= sp)).any()):
            continue
        if any(abs(q - kq) <= sp and abs(a - ka) <= sp for kq, ka, _, _ in kept):
            continue
        kept.append((q, a, s, d))
        if len(kept) == int(par["max_loops"]):
            break
    return kept


# ---- what recognize leaves, for loop m -------------------------------------------------------------------------------------------------
def loop_select(g, loops, loops_rep, m, gap, window, q_scan):
    """lsd_enqueue_pg_loop_select_device: (the near record, sel, the query's row, its length, q_pose)."""
    nodes = g["nodes"]
    n_nodes = pg.clamp(g["head"][0]["n_nodes"], len(nodes))
    L = loops[m]
    j = int(L["query"])
    has_q = 0 <= j < n_nodes
    anchor = int(L["anchor"]) if has_q and 0 <= int(L["anchor"]) < n_nodes else -1
    near = np.zeros((), pg.NEAR_DTYPE)
    near["anchor"], near["query"], near["n_cand"] = anchor, j, int(loops_rep["n_loops"])
    near["d2"] = float(int(L["dist"])) if anchor >= 0 else 0.0
    q_pose = pg.SENTINEL
    if anchor >= 0:
        pa = pg.pose_of(nodes[anchor])
        q_pose = (pa[0], pa[1], pg.wrap(pa[2] - float(int(L["shift"])) * pp.SECTOR_DEG))
    sel, row, q_len, q_pose = pp.leave_for_anchor(g, j, n_nodes, anchor, gap, window, q_scan, q_pose)
    return near, sel, row, q_len, q_pose


# ---- the batch campaign ----------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1025)
BATCH_CLASSES = (tuple("n_%d" % n for n in BATCH_SIZES) +
                 ("q_lo_positive", "n_q_0", "range_beyond_n", "head_above_cap", "head_below_0", "invalid_between", "below_min_sectors_between",
                  "j_below_gap", "candidate_at_gap", "dist_at_max", "dist_above_max", "tie_dist", "tie_shift", "k_1", "k_8", "spread_0",
                  "fewer_than_k", "query_past_n"))
BATCH_ONCE = ("big_top", "big_bottom")
NOISE_ROWS = 2                                                                # records behind the range: they keep their bytes


def bcase(name, g, desc, par, q_lo, n_q, rng, **more):
    k = int(par["k"])
    rows = n_q + NOISE_ROWS
    recs = rng.integers(0, 256, (rows, k, 16), dtype=np.uint8).view(pp.PLACE_REC_DTYPE).reshape(rows, k).copy()
    reps = rng.integers(0, 256, (rows, 16), dtype=np.uint8).view(pp.PLACE_REP_DTYPE).reshape(rows).copy()
    return dict(name=name, graph=g, desc=desc, par=par, q_lo=q_lo, n_q=n_q, recs=recs, reps=reps, **more)


def planted(n, rep, rng, gap):
    """Random descriptors in which every fifth node from 2 * gap on looks like the node a little more than gap before it."""
    d = pp.random_desc(n, rng)
    for t, j in enumerate(range(2 * gap, n, 5)):
        d[j]["v"] = pp.near_copy(d[j - gap - (t % 3)]["v"], (11 * t + rep) % 64, 3 * (t % 17) + rep, rng)
    return d


def batch_campaign(big=False):
    """Cases: dict(name, graph, desc [nodes_cap], par, q_lo, n_q, recs, reps: the outputs' bytes before the call, NOISE_ROWS rows longer
    than the range).  big: the two ranges of the one graph of 16384 nodes instead of the others."""
    rng = np.random.default_rng(20251020)
    if big:
        c = pp.recognize_campaign(big=True)[0]
        n = len(c["graph"]["nodes"])
        return [bcase("big_top", c["graph"], c["desc"], c["par"], n - 24, 24, rng, once="big_top"),
                bcase("big_bottom", c["graph"], c["desc"], c["par"], 0, 24, rng, once="big_bottom")]
    out = []
    # the single entry's own campaign with every node as a query (a range that runs past N into the capacity)
    for c in pp.recognize_campaign():
        cap = len(c["graph"]["nodes"])
        n = pg.clamp(c["graph"]["head"][0]["n_nodes"], cap)
        if "turn" in c and not c["name"].endswith("_0"):
            continue
        if n > 300:
            out.append(bcase("place_%s_top" % c["name"], c["graph"], c["desc"], c["par"], cap - 20, 20, rng))
        else:
            out.append(bcase("place_%s" % c["name"], c["graph"], c["desc"], c["par"], 0, cap, rng))
    for rep in range(3):
        for n in (0, 63, 64, 65):
            gap = 4 + rep
            g = pp.place_graph(n, n + 3, 1 + rep, rng)
            out.append(bcase("size_%d_%d" % (n, rep), g, pp.rcase("", g, planted(n, rep, rng, gap), rng)["desc"],
                             pp.place(gap=gap, spread=rep, k=(1, 4, 8)[rep], max_dist=60), 0, n, rng))
        # a range that starts past 0; an empty range; heads outside the capacity
        g = pp.place_graph(40, 44, 2, rng)
        desc = pp.rcase("", g, planted(40, rep, rng, 5), rng)["desc"]
        out.append(bcase("q_lo_%d" % rep, g, desc, pp.place(gap=5, k=3, max_dist=80), 7 + 9 * rep, 20 - rep, rng))
        out.append(bcase("n_q_0_%d" % rep, g, desc, pp.place(gap=5), (0, 13, 44)[rep], 0, rng))
        for name, head in (("head_above_cap", 44 + (1, 2, 1000)[rep]), ("head_below_0", -1 - rep)):
            g2 = pg.copy_graph(g)
            g2["head"][0]["n_nodes"] = head
            d2 = desc.copy()
            d2[40:] = planted(4, rep, rng, 1)                                 # (the clamped N reaches the capacity: rows that are described)
            out.append(bcase("%s_%d" % (name, rep), g2, d2, pp.place(gap=5, k=2, max_dist=80), 0, 44, rng))
        # queries that are not described, or see too few sectors, between good ones
        d3 = planted(40, rep, rng, 5).copy()
        d3[20 + rep]["valid"] = 0
        d3[25 + rep]["n_sectors"] = 15
        out.append(bcase("between_%d" % rep, g, pp.rcase("", g, d3, rng)["desc"], pp.place(gap=5, k=2, max_dist=80), 3, 37, rng))
    return out


_batches = {}


def run_batch_case(case):
    """((recs, reps), the traces of the queries); the results are kept."""
    if case["name"] not in _batches:
        trs = []
        _batches[case["name"]] = recognize_all(case["graph"], case["desc"], case["par"], case["q_lo"], case["n_q"], case["recs"], case["reps"], trs), trs
    return _batches[case["name"]]


def batch_classes_of(case, trs):
    c = set()
    g = case["graph"]
    cap, head = len(g["nodes"]), int(g["head"][0]["n_nodes"])
    n = pg.clamp(head, cap)
    if "once" in case:
        c.add(case["once"])
    if head in BATCH_SIZES and (case["n_q"] >= min(n, 20)):
        c.add("n_%d" % head)
    if case["q_lo"] > 0 and case["n_q"] > 0: c.add("q_lo_positive")
    if case["n_q"] == 0: c.add("n_q_0")
    if case["n_q"] > 0 and case["q_lo"] + case["n_q"] > n and case["q_lo"] < n: c.add("range_beyond_n")
    if head > cap: c.add("head_above_cap")
    if head < 0: c.add("head_below_0")
    per = [pp.recognize_classes_of(dict(desc=case["desc"]), tr) for tr in trs]
    good = [bool(tr["usable"]) and tr["limit"] >= 0 for tr in trs]
    for q, cl in enumerate(per):
        between = any(good[:q]) and any(good[q + 1:])
        if "query_invalid" in cl and between: c.add("invalid_between")
        if "query_below_min_sectors" in cl and between: c.add("below_min_sectors_between")
        if "no_query" in cl: c.add("query_past_n")
        c |= cl & {"j_below_gap", "candidate_at_gap", "dist_at_max", "dist_above_max", "tie_dist", "tie_shift", "k_1", "k_8", "spread_0", "fewer_than_k"}
    return c


# ---- the loops campaign ----------------------------------------------------------------------------------------------------------------
LOOPS_CLASSES = ("no_pair", "more_than_max", "max_loops_1", "max_loops_64", "tie_dist_queries", "tie_dist_anchors", "gone_at_spread_q",
                 "kept_at_spread_1_q", "gone_at_spread_a", "kept_at_spread_1_a", "spread_0", "known_enabled", "known_rejected", "known_swapped",
                 "odometry_not_known", "edges_behind_n", "e_0", "e_255", "e_256", "e_257", "edges_head_above_cap", "edges_head_below_0",
                 "cross_tracks", "round_unfilled")


def batch_of(n_q, k, q_lo, pairs, rng):
    """Records as the batch leaves them: pairs {query: [(anchor, shift, dist), ..]} in the order of its rounds, (-1, 0, 0, 0) behind them."""
    rows = n_q + NOISE_ROWS
    recs = rng.integers(0, 256, (rows, k, 16), dtype=np.uint8).view(pp.PLACE_REC_DTYPE).reshape(rows, k).copy()
    reps = rng.integers(0, 256, (rows, 16), dtype=np.uint8).view(pp.PLACE_REP_DTYPE).reshape(rows).copy()
    recs[:n_q] = np.zeros((), pp.PLACE_REC_DTYPE)
    recs["anchor"][:n_q] = -1
    for q in range(n_q):
        mine = pairs.get(q_lo + q, [])
        assert len(mine) <= k and len({a for a, _, _ in mine}) == len(mine)
        for r, (a, s, d) in enumerate(mine):
            recs[q, r]["anchor"], recs[q, r]["shift"], recs[q, r]["dist"] = a, s, d
        reps[q] = (q_lo + q, len(mine), len(mine), 0)
    return recs, reps


def closure_edge(i, j, flags, rng):
    e = rng.integers(0, 256, 96, dtype=np.uint8).view(pg.EDGE_DTYPE)[0].copy()
    e["i"], e["j"], e["flags"] = i, j, flags
    return e


def lcase(name, n_q, k, q_lo, pairs, edges, head_edges, rng, tracks=None, extra_edges=3, **par):
    recs, reps = batch_of(n_q, k, q_lo, pairs, rng)
    ed = rng.integers(0, 256, (len(edges) + extra_edges) * 96, dtype=np.uint8).view(pg.EDGE_DTYPE).copy()
    ed["flags"] &= ~np.uint32(pg.EDGE_CLOSURE)                                # (noise that is no closure, unless a case says so)
    for x, e in enumerate(edges):
        ed[x] = e
    return dict(name=name, n_q=n_q, k=k, q_lo=q_lo, recs=recs, reps=reps, edges=ed, head_edges=len(edges) if head_edges is None else head_edges,
                nodes_cap=q_lo + n_q + 2, par=loops_par(**par), tracks=tracks)


def random_pairs(n_q, k, q_lo, rng, fill=0.5, dist_hi=900):
    pairs = {}
    for q in range(q_lo, q_lo + n_q):
        if q >= 3 and rng.random() < fill:
            cnt = int(rng.integers(1, k + 1))
            anchors = rng.choice(max(q - 2, 1), size=min(cnt, max(q - 2, 1)), replace=False)
            pairs[q] = [(int(a), int(rng.integers(0, 64)), int(rng.integers(0, dist_hi))) for a in anchors]
    return pairs


def loops_campaign():
    """Cases: dict(name, n_q, k, q_lo, recs, reps, edges [edges_cap], head_edges, nodes_cap, par, tracks)."""
    rng = np.random.default_rng(20251021)
    out = []
    odo = lambda i, j: closure_edge(i, j, 0, rng)
    for rep in range(3):
        sp = 2 + rep
        # nothing to choose from; more than max_loops; one round; all 64
        out.append(lcase("no_pair_%d" % rep, 12 + rep, 1 + rep, rep, {}, [odo(0, 1)], None, rng, max_loops=3 + rep))
        out.append(lcase("many_%d" % rep, 300, 4, 5 * rep, random_pairs(300, 4, 5 * rep, rng), [], None, rng, max_loops=5 + rep, spread=rep))
        out.append(lcase("one_round_%d" % rep, 40, 2, 0, random_pairs(40, 2, 0, rng), [], None, rng, max_loops=1, spread=sp))
        out.append(lcase("all_64_%d" % rep, 500 + rep, 8, 0, random_pairs(500 + rep, 8, 0, rng), [], None, rng, max_loops=64, spread=1))
        out.append(lcase("few_64_%d" % rep, 60, 2, 0, random_pairs(60, 2, 0, rng, fill=0.2), [], None, rng, max_loops=64, spread=sp))
        # equal distances on two queries, and on two anchors of one query
        q0, a0 = 50 + rep, 10 + rep
        pairs = {q0: [(a0, 3, 40), (a0 + 20, 5, 40)], q0 + 20: [(a0 + 3, 7, 40)], q0 + 30: [(a0 + 9, 1, 41)]}
        out.append(lcase("ties_%d" % rep, 100, 3, 0, pairs, [], None, rng, max_loops=6, spread=sp))
        # suppression exactly at spread and one beyond it, on each axis alone (the same anchor from other queries, other anchors of the
        # same query)
        pairs = {q0: [(a0, 3, 10), (a0 + sp, 4, 22), (a0 + sp + 1, 5, 23)], q0 + sp: [(a0, 6, 20)], q0 + sp + 1: [(a0, 7, 21)],
                 q0 - sp: [(a0, 8, 24)], q0 - sp - 1: [(a0, 9, 25), (a0 - sp, 2, 27)], q0 - 2 * sp - 2: [(a0 - sp - 1, 2, 26)]}
        out.append(lcase("at_spread_%d" % rep, 100, 3, 0, pairs, [], None, rng, max_loops=8, spread=sp))
        out.append(lcase("spread_0_%d" % rep, 30, 3, 0, {20: [(5, 1, 9), (6, 2, 8)], 21: [(5, 3, 7), (6 + rep, 0, 9)]}, [], None, rng, max_loops=8,
                         spread=0))
        # pairs the graph already knows: an enabled closure, a rejected one, one stored with i > j; an odometry edge knows nothing; edges
        # behind n_edges that look like closures
        pairs = {60: [(10, 1, 5)], 70: [(20 + sp, 2, 6)], 80 - sp: [(30, 3, 7)], 90: [(40, 4, 8)], 95: [(45, 5, 9)], 99: [(50 + sp + 1, 6, 10)]}
        edges = [odo(k, k + 1) for k in range(6)] + [closure_edge(10, 60, pg.EDGE_CLOSURE, rng),
                                                    closure_edge(20, 70, pg.EDGE_CLOSURE | pg.EDGE_DISABLED | EDGE_REJECTED, rng),
                                                    closure_edge(80, 30, pg.EDGE_CLOSURE, rng), odo(40, 90), closure_edge(50, 99, pg.EDGE_CLOSURE, rng)]
        c = lcase("known_%d" % rep, 100, 2, 0, pairs, edges + [closure_edge(45, 95, pg.EDGE_CLOSURE, rng)], len(edges), rng, max_loops=8, spread=sp,
                  extra_edges=2)
        out.append(c)
        # the edge counts around the workgroup's width; heads outside the capacity
        for E in (0, 255, 256, 257):
            edges = [odo(k % 90, k % 90 + 1) for k in range(E)]
            if E:
                edges[E - 1] = closure_edge(12, 72, pg.EDGE_CLOSURE, rng)    # (the last edge below E: a pair it makes known)
                edges[E // 2] = closure_edge(33, 93, pg.EDGE_CLOSURE | pg.EDGE_DISABLED, rng)
            pairs = {72: [(12 + rep % 2, 1, 3)], 93: [(33, 2, 4)], 50: [(7, 3, 5)]}
            out.append(lcase("e_%d_%d" % (E, rep), 100, 1, 0, pairs, edges, None, rng, max_loops=4, spread=sp, extra_edges=1 if E == 0 else 0))
        edges = [odo(1, 2), closure_edge(12, 72, pg.EDGE_CLOSURE, rng), closure_edge(33, 93, pg.EDGE_CLOSURE, rng)]
        out.append(lcase("e_head_above_%d" % rep, 100, 1, 0, pairs, edges, 3 + (1, 2, 1000)[rep], rng, max_loops=4, spread=sp, extra_edges=0))
        out.append(lcase("e_head_below_%d" % rep, 100, 1, 0, pairs, edges, -1 - rep, rng, max_loops=4, spread=sp))
        # two tracks in one graph: nodes 0..39 are track 0, 40..79 track 1; the second track's keyframes look like the first one's
        tracks = np.repeat([0, 1], 40)
        pairs = {50 + 5 * t: [(8 + 5 * t + rep, t, 30 + t)] for t in range(5)}
        pairs[79] = [(60, 1, 12)]
        out.append(lcase("two_tracks_%d" % rep, 40, 2, 40, pairs, [odo(k, k + 1) for k in range(10)], None, rng, tracks=tracks, max_loops=8, spread=sp))
    return out


_loops = {}


def run_loops_case(case):
    if case["name"] not in _loops:
        tr = {}
        _loops[case["name"]] = find_loops(case["recs"], case["reps"], case["n_q"], case["head_edges"], case["edges"], case["par"], tr), tr
    return _loops[case["name"]]


def loops_classes_of(case, tr):
    c = set()
    p, rounds, sp = tr["par"], tr["rounds"], tr["par"]["spread"]
    n_pairs = len(tr["pairs"]) + len(tr["known"])
    if n_pairs == 0: c.add("no_pair")
    if len(tr["pairs"]) > p["max_loops"] and len(rounds) == p["max_loops"] and tr["left"]: c.add("more_than_max")
    if p["max_loops"] == 1 and rounds: c.add("max_loops_1")
    if p["max_loops"] == 64 and rounds: c.add("max_loops_64")
    if len(rounds) < p["max_loops"]: c.add("round_unfilled")
    if sp == 0 and len(rounds) > 1: c.add("spread_0")
    for r in rounds:
        d, q, a, _ = r["chosen"]
        same = [x for x in r["open"] if x[0] == d and x[1:3] != (q, a)]
        if any(x[1] != q for x in same): c.add("tie_dist_queries")
        if any(x[1] == q for x in same): c.add("tie_dist_anchors")
        if sp > 0:
            for x in r["open"]:
                dq, da = abs(x[1] - q), abs(x[2] - a)
                if (dq, da) == (sp, 0) and x in r["gone"]: c.add("gone_at_spread_q")
                if (dq, da) == (sp + 1, 0) and x not in r["gone"]: c.add("kept_at_spread_1_q")
                if (dq, da) == (0, sp) and x in r["gone"]: c.add("gone_at_spread_a")
                if (dq, da) == (0, sp + 1) and x not in r["gone"]: c.add("kept_at_spread_1_a")
        if case["tracks"] is not None and case["tracks"][q] != case["tracks"][a]: c.add("cross_tracks")
    ed = case["edges"]
    for _, by in tr.get("known_by", []):
        for x in by:
            f = int(ed[x]["flags"])
            if not f & pg.EDGE_DISABLED: c.add("known_enabled")
            if f & pg.EDGE_DISABLED and f & EDGE_REJECTED: c.add("known_rejected")
            if int(ed[x]["i"]) > int(ed[x]["j"]): c.add("known_swapped")
    chosen = {r["chosen"][1:3] for r in rounds}
    for x, e in enumerate(ed):
        at = (max(int(e["i"]), int(e["j"])), min(int(e["i"]), int(e["j"])))
        if x < tr["E"] and not int(e["flags"]) & pg.EDGE_CLOSURE and at in chosen: c.add("odometry_not_known")
        if x >= tr["E"] and int(e["flags"]) & pg.EDGE_CLOSURE and at in chosen: c.add("edges_behind_n")
    if case["head_edges"] in (0, 255, 256, 257): c.add("e_%d" % case["head_edges"])
    if case["head_edges"] > len(ed): c.add("edges_head_above_cap")
    if case["head_edges"] < 0: c.add("edges_head_below_0")
    return c


# ---- the select campaign ---------------------------------------------------------------------------------------------------------------
SELECT_CLASSES = ("filled", "unfilled", "window_cut_by_0", "window_cut_by_gap")


def select_campaign():
    """Cases: dict(name, graph, gap, window, loops, loops_rep, ms: the rounds to select -- every filled one and m == n_loops)."""
    out = []
    for case in batch_campaign():
        if not case["name"].startswith(("place_cut_by_0", "place_cut_by_gap", "place_tie_dist", "size_64_", "q_lo_")):
            continue
        (recs, reps), _ = run_batch_case(case)
        g = case["graph"]
        loops, rep = find_loops(recs, reps, case["n_q"], 0, np.zeros(1, pg.EDGE_DTYPE), loops_par(max_loops=8, spread=int(case["par"]["spread"])))
        n = int(rep["n_loops"])
        out.append(dict(name="select_" + case["name"], graph=g, gap=int(case["par"]["gap"]), window=int(case["par"]["window"]), loops=loops, loops_rep=rep,
                        ms=list(range(min(n + 1, 8)))))
    return out


def run_select_case(case, m):
    q0 = np.full((case["graph"]["store"].shape[1], 2), 0.125)
    return loop_select(case["graph"], case["loops"], case["loops_rep"], m, case["gap"], case["window"], q0)


def select_classes_of(case, m):
    L = case["loops"][m]
    if int(L["query"]) < 0:
        return {"unfilled"}
    c = {"filled"}
    if int(L["anchor"]) - case["window"] < 0: c.add("window_cut_by_0")
    if int(L["anchor"]) + case["window"] > int(L["query"]) - case["gap"]: c.add("window_cut_by_gap")
    return c


# ---- end to end: two laps around the off-centre box, every loop closed in one pass -----------------------------------------------------
E2E = dict(n=47, n_beams=128, bias=-1.2, place=pp.place(gap=18, window=2, spread=2, k=3, pick=0, max_dist=300, min_sectors=32),
           loops=loops_par(max_loops=8, spread=2), search=pp.E2E["search"], response=pp.E2E["response"], closure=pp.E2E["closure"],
           append=pp.E2E["append"], relax=dict(pg.RELAX_DEFAULTS, iters=12, cg_iters=75, cg_tol=1e-8))
_e2e = None


def close_tail(g, near, sel, row, q_len, q_pose):
    """What follows the choice of an anchor (PoseGraph._close_tail): (the graph after, the response record, the closure report)."""
    R = pp.PLACE_ROOM
    cols, rows = R["cols"], R["rows"]
    pa, hi = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g["store"], g["store_lens"], sel, cols, rows, R["resol"], R["range_max"], pa, hi)
    corr = gm.likelihood(pa, hi, 2, 1, 10, 3, gm.GAUSS)
    lens = np.array([q_len], np.int32)
    mrec = gm.match(row[None], lens, q_pose[None], R["resol"], R["range_max"], corr, E2E["search"])
    resp, _ = gr.response(row[None], lens, q_pose[None], mrec, R["resol"], R["range_max"], corr, E2E["search"]["ang_step"], E2E["response"])
    g2, crep = pg.closure(g, near, resp[0], E2E["closure"])
    return g2, resp[0], crep


def relaxed(g):
    nn, ne = int(g["head"][0]["n_nodes"]), int(g["head"][0]["n_edges"])
    nodes, edges, rrep = pg.relax(g["nodes"][:nn], g["edges"][:ne], E2E["relax"])
    out = pg.copy_graph(g)
    out["nodes"][:nn], out["edges"][:ne] = nodes, edges
    return out, rrep


def optimized(g):
    """PoseGraph.optimize_device with a Huber delta that no edge reaches and nothing rejected: the robust relaxation is then the plain
    one byte for byte (include/lsd_hip.h), the prune only counts, and the refit is a second plain relaxation from the poses of the first."""
    return relaxed(relaxed(g)[0])


def end_to_end():
    """The chain restated once and shared: not quite two laps (no place is seen a third time) of 24 keyframes of 128 beams around the box of pose_graph_place_cases, odometry with a
    heading under-read; append -> describe -> (a) recognize + one closure at the end of the track, relaxed; (b) recognize_all -> find_loops
    -> per round select + the closure's tail -> optimize -> rerender."""
    global _e2e
    if _e2e is not None:
        return _e2e
    R, n, nb = pp.PLACE_ROOM, E2E["n"], E2E["n_beams"]
    rng = np.random.default_rng(12)
    truth = []
    for k in range(n + 1):                                                   # two laps and a little
        a = 363.0 * k / 24
        truth.append((30.0 + 13.0 * math.cos(math.radians(a)), 23.0 + 10.0 * math.sin(math.radians(a)), pg.wrap(a + 90.0)))
    odom = [truth[0]]
    for k in range(1, n + 1):
        z = pg.rel(truth[k - 1], truth[k])
        odom.append(pg.comp(odom[-1], (z[0] + 0.02 * rng.normal(), z[1] + 0.02 * rng.normal(), z[2] + E2E["bias"] * rng.uniform(0.8, 1.0))))
    scans = np.stack([pp.place_room_scan(p, nb) for p in truth])
    lens = np.full(n + 1, nb, np.int32)
    cap = n + 4
    g0 = pg.new_graph(cap, n + 16, nb)
    g1, arep = pg.append(g0, scans, lens, np.array(odom), 0, E2E["append"])
    nn = int(g1["head"][0]["n_nodes"])
    q0 = np.zeros((nb, 2))
    desc = pp.describe(nn, g1["store"], g1["store_lens"], R["range_max"], np.zeros(cap, pp.DESC_DTYPE))
    # (a) the single closure close_place_device makes at the end of the track
    _, _, _, nrec, sel, row, q_len, q_pose = pp.recognize(g1, 0, desc, E2E["place"], np.zeros(cap, np.uint32), q0)
    ga, _, crep_a = close_tail(g1, nrec, sel, row, q_len, q_pose)
    ga_relaxed, _ = optimized(ga)
    # (b) every loop in one pass
    k = E2E["place"]["k"]
    recs, reps = recognize_all(g1, desc, E2E["place"], 0, cap, np.zeros((cap, k), pp.PLACE_REC_DTYPE), np.zeros(cap, pp.PLACE_REP_DTYPE))
    tr = {}
    loops, lrep = find_loops(recs, reps, cap, g1["head"][0]["n_edges"], g1["edges"], E2E["loops"], tr)
    g, row = g1, q0
    nears, creps, resps, left = [], [], [], None
    for m in range(E2E["loops"]["max_loops"]):
        near, sel, row, q_len, q_pose = loop_select(g, loops, lrep, m, E2E["place"]["gap"], E2E["place"]["window"], row)
        g, resp, crep = close_tail(g, near, sel, row, q_len, q_pose)
        nears.append(near); creps.append(crep); resps.append(resp)
        left = (sel, row, q_len, q_pose)
    g2 = g
    g3, rrep = optimized(g2)
    cols, rows = R["cols"], R["rows"]
    pa2, hi2 = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g3["store"], g3["store_lens"], np.stack([g3["nodes"]["x"], g3["nodes"]["y"], g3["nodes"]["ang"]], axis=1), cols, rows, R["resol"],
                 R["range_max"], pa2, hi2)
    _e2e = dict(truth=np.array(truth), odom=np.array(odom), scans=scans, lens=lens, g0=g0, g1=g1, append_rep=arep, desc=desc, single_near=nrec,
                single_closure_rep=crep_a, single=ga, single_relaxed=ga_relaxed, recs=recs, reps=reps, loops=loops, loops_rep=lrep, trace=tr,
                nears=np.array(nears), closure_reps=np.array(creps), resps=np.array(resps), left=left, g2=g2, g3=g3, relax_rep=rrep, planes=(pa2, hi2),
                n_nodes=nn, n_edges=int(g2["head"][0]["n_edges"]))
    return _e2e
