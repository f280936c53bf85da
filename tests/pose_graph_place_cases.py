"""Place recognition for the pose graph (include/lsd_hip.h, "pose graph": lsd_enqueue_pg_describe_device, lsd_enqueue_pg_recognize_device;
csrc/k_pgplace.hip) restated on Python floats and numpy integers, written from the header for the tests (not from the
HIP code), and the generated campaigns both test files run.

The one fp64 step -- a reading's sector and value -- is Python floats, which are IEEE doubles without contraction; everything after it is
integer arithmetic, which has no order.  wrap, the graph's layout and the chain behind the choice of an anchor are pose_graph_cases'.  A
case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
import grid_match_cases as gm
import grid_response_cases as gr
import pose_graph_cases as pg

SECTORS, PLACE_MAX = 64, 8
TWO_PI = 6.283185307179586
SECTOR_DEG = 5.625
NONE = 0xFFFFFFFF                                                             # d_work of a node that is no candidate
MAX_DIST = 16320
DESC_DTYPE = np.dtype([("v", "u1", (SECTORS,)), ("n_hits", "u4"), ("n_sectors", "u2"), ("valid", "u2")])
PLACE_REC_DTYPE = np.dtype([("anchor", "i4"), ("shift", "i4"), ("dist", "u4"), ("reserved", "u4")])
PLACE_REP_DTYPE = np.dtype([("query", "i4"), ("n_cand", "i4"), ("n_picked", "i4"), ("reserved", "i4")])
SIZES = {"lsd_pg_desc": 72, "lsd_pg_place_par": 32, "lsd_pg_place_rec": 16, "lsd_pg_place_rep": 16}
PLACE_KEYS = ("gap", "window", "spread", "k", "pick", "max_dist", "min_sectors")
PLACE_DEFAULTS = dict(gap=10, window=2, spread=2, k=4, pick=0, max_dist=1024, min_sectors=16)
INF, NAN = pg.INF, pg.NAN


def place(**kw):
    assert set(kw) <= set(PLACE_KEYS)
    return dict(PLACE_DEFAULTS, **kw)


# ---- describe --------------------------------------------------------------------------------------------------------------------------
def reading_used(r, a, range_max):
    return math.isfinite(r) and r > 0 and r <= range_max and math.isfinite(a)


def sector_of(a):
    """(t, f, s) of a used reading's angle."""
    t = a / TWO_PI
    f = t - math.floor(t)
    s = int(f * 64.0)
    return t, f, min(s, 63)


def value_of(r, range_max):
    return min(int(r / range_max * 255.0), 254)


def describe_row(readings, length, stride, range_max, trace=None, row=None):
    """One lsd_pg_desc (a DESC_DTYPE scalar) of the first min(max(length, 0), stride) readings."""
    n = min(max(int(length), 0), int(stride))
    sums, cnts = [0] * SECTORS, [0] * SECTORS
    for i in range(n):
        r, a = float(readings[i][0]), float(readings[i][1])
        used = reading_used(r, a, range_max)
        ev = dict(row=row, i=i, r=r, a=a, used=used)
        if used:
            t, f, s = sector_of(a)
            q = value_of(r, range_max)
            sums[s] += q
            cnts[s] += 1
            ev.update(t=t, f=f, s=s, q=q)
        if trace is not None:
            trace.append(ev)
    d = np.zeros((), DESC_DTYPE)
    d["v"] = [sums[s] // cnts[s] if cnts[s] else 255 for s in range(SECTORS)]
    d["n_hits"], d["n_sectors"], d["valid"] = sum(cnts), sum(1 for c in cnts if c), 1
    if trace is not None:
        trace.append(dict(row=row, described=True, len=int(length), sums=sums, cnts=cnts))
    return d


def describe(head_n, store, store_lens, range_max, desc, trace=None):
    """lsd_enqueue_pg_describe_device: desc [nodes_cap] after the call (a copy).  store: float64 [nodes_cap, stride, 2]."""
    out = desc.copy()
    n = pg.clamp(head_n, len(desc))
    for k in range(n):
        if int(out[k]["valid"]) == 0:
            out[k] = describe_row(store[k], store_lens[k], store.shape[1], range_max, trace, k)
    return out


# ---- the distance ----------------------------------------------------------------------------------------------------------------------
def shifted(a):
    """int64 [64 shifts, 64]: row s is a[(k + s) mod 64]."""
    a = np.asarray(a, np.int64)
    return np.stack([np.roll(a, -s) for s in range(SECTORS)])


def all_distances(a, c):
    """D [n, 64] of the query's bytes a against the candidates' bytes c [n, 64]."""
    sh = shifted(a)
    c = np.asarray(c, np.int64).reshape(-1, SECTORS)
    return np.stack([np.abs(sh[s][None, :] - c).sum(axis=1) for s in range(SECTORS)], axis=1)


def distance(a, c):
    """(dist, shift) of a query a and a candidate c (64 bytes each)."""
    D = all_distances(a, c)[0]
    s = int(np.argmin(D))                                                     # (the first of the smallest)
    return int(D[s]), s


# ---- what near leaves, for a given anchor ----------------------------------------------------------------------------------------------
def leave_for_anchor(g, j, n_nodes, anchor, gap, window, q_scan, q_pose):
    """(sel, the query's row, its length, q_pose) as lsd_enqueue_pg_near_device writes them for `anchor`; q_pose: what it holds with an
    anchor (near: the query's own pose; recognize: the anchor's, turned)."""
    nodes = g["nodes"]
    has_q = 0 <= j < n_nodes
    sel = np.zeros((len(nodes), 3))
    for k in range(len(nodes)):
        sel[k] = pg.pose_of(nodes[k]) if anchor >= 0 and abs(k - anchor) <= window and k <= j - gap else pg.SENTINEL
    row = np.array(q_scan, np.float64)
    if has_q:
        row[:] = g["store"][j]
    q_len = int(g["store_lens"][j]) if has_q else 0
    return sel, row, q_len, np.array(q_pose if anchor >= 0 else pg.SENTINEL)


# ---- recognize -------------------------------------------------------------------------------------------------------------------------
def recognize(g, track, desc, par, work, q_scan, trace=None):
    """lsd_enqueue_pg_recognize_device: (work, recs [k], rep, near record, sel, the query's row, length, pose)."""
    nodes = g["nodes"]
    n_nodes, j = pg.clamp(g["head"][0]["n_nodes"], len(nodes)), int(g["tracks"][track]["last"])
    gap, window, spread, k, pick = (int(par[n]) for n in ("gap", "window", "spread", "k", "pick"))
    max_dist, min_sectors = int(par["max_dist"]), int(par["min_sectors"])
    usable = 0 <= j < n_nodes and int(desc[j]["valid"]) != 0 and int(desc[j]["n_sectors"]) >= min_sectors
    limit = j - gap if usable else -1
    work = np.array(work, np.uint32)
    work[:n_nodes] = NONE
    D = None
    if limit >= 0:
        ok = (desc["valid"][:limit + 1] != 0) & (desc["n_sectors"][:limit + 1] >= min_sectors)
        D = all_distances(desc[j]["v"], desc["v"][:limit + 1])
        shift = np.argmin(D, axis=1)
        dist = D[np.arange(limit + 1), shift]
        cand = ok & (dist <= max_dist)
        work[:limit + 1][cand] = ((dist << 6) | shift)[cand].astype(np.uint32)
    cands = [i for i in range(limit + 1) if work[i] != NONE]
    recs = np.zeros(k, PLACE_REC_DTYPE)
    recs["anchor"] = -1
    open_ = list(cands)
    picked = []
    for r in range(k):
        if not open_:
            continue
        best = min(open_, key=lambda i: (int(work[i]) >> 6, i))
        recs[r]["anchor"], recs[r]["shift"], recs[r]["dist"] = best, int(work[best]) & 63, int(work[best]) >> 6
        picked.append(best)
        open_ = [i for i in open_ if abs(i - best) > spread]
    rep = np.zeros((), PLACE_REP_DTYPE)
    rep["query"], rep["n_cand"], rep["n_picked"] = j, len(cands), len(picked)
    anchor = int(recs[pick]["anchor"])
    near = np.zeros((), pg.NEAR_DTYPE)
    near["anchor"], near["query"], near["n_cand"] = anchor, j, len(cands)
    near["d2"] = float(int(recs[pick]["dist"])) if anchor >= 0 else 0.0
    q_pose = pg.SENTINEL
    if anchor >= 0:
        pa = pg.pose_of(nodes[anchor])
        q_pose = (pa[0], pa[1], pg.wrap(pa[2] - float(int(recs[pick]["shift"])) * SECTOR_DEG))
    sel, row, q_len, q_pose = leave_for_anchor(g, j, n_nodes, anchor, gap, window, q_scan, q_pose)
    if trace is not None:
        trace.update(j=j, n_nodes=n_nodes, usable=usable, limit=limit, D=D, cands=cands, picked=picked, anchor=anchor, par=dict(par),
                     valid_j=int(desc[j]["valid"]) if 0 <= j < n_nodes else None, sectors_j=int(desc[j]["n_sectors"]) if 0 <= j < n_nodes else None)
    return work, recs, rep, near, sel, row, q_len, q_pose


# ---- the describe campaign -------------------------------------------------------------------------------------------------------------
RANGE_MAX = 4.0
DESCRIBE_STRIDES = (1, 8, 255, 256, 257)
DESCRIBE_CLASSES = ("edge_exact", "edge_below", "edge_above", "negative_angle", "above_2pi", "f_eq_1", "range_at_max", "range_above_max",
                    "range_zero", "range_negative", "range_inf", "range_nan", "angle_nan", "len_0", "len_negative", "len_above_stride",
                    "valid_survives", "rows_past_n", "head_below_0", "head_above_cap", "mean_divides", "all_empty")


def up(v):
    return math.nextafter(v, INF)


def edge(k):
    return k * TWO_PI / 64


def special_readings(rep, range_max):
    """(range, angle) pairs that sit on the rule's edges; rep varies the sectors."""
    e = [edge(k) for k in (1 + rep, 17 + 5 * rep, 32 + rep, 63 - rep)]
    out = []
    for v in e:
        out += [(1.0 + 0.1 * rep, v), (1.5, pg.below(v)), (2.0, up(v))]
    out += [(0.7, -0.3 - rep), (0.9, -7.0 - rep), (1.1, TWO_PI + 0.4 + rep), (1.3, 13.0 + rep), (1.2, -1e-20 / (1 + rep)), (0.4, -5e-324)]
    out += [(range_max, 0.5 + rep), (up(range_max), 0.6), (0.0, 0.7), (-0.0, 0.7), (-1.0 - rep, 0.8), (INF, 0.9), (-INF, 0.9), (NAN, 1.0),
            (1.0, NAN), (1.0, INF), (1.0, -INF), (5e-324, 1.1), (pg.below(range_max), 1.2)]
    # two and three readings in one sector whose mean needs the integer division (at range_max 4.0: 63 + 96, and 63 + 95 + 96)
    out += [(1.0, 2.0), (1.52, 2.01), (1.0, 3.0 + 0.1 * rep), (1.5, 3.01 + 0.1 * rep), (1.52, 3.02 + 0.1 * rep)]
    return out


def describe_case(name, stride, rep, rng, range_max=RANGE_MAX, head=None):
    sp = special_readings(rep, range_max)
    if stride >= len(sp):
        rows_sp = 1
    else:
        rows_sp = -(-len(sp) // stride)
    n_rows = rows_sp + 6                                                      # 3 odd lengths, 1 valid row of noise, 2 random rows
    cap = n_rows + 2                                                          # and two rows past n_nodes
    store = np.stack([rng.uniform(0.05, 1.2 * range_max, (cap, stride)), rng.uniform(-7.0, 14.0, (cap, stride))], axis=2)
    lens = np.full(cap, stride, np.int32)
    flat = store[:rows_sp].reshape(-1, 2)
    for k, v in enumerate(sp):
        flat[k] = v
    if stride >= len(sp) and stride >= 200:
        lens[0] = stride - 3
    lens[rows_sp:rows_sp + 3] = (0, -3 - rep, stride + 5 + rep)
    desc = np.zeros(cap, DESC_DTYPE)
    noise = rng.integers(0, 256, (3, 72), dtype=np.uint8).view(DESC_DTYPE).reshape(3)
    noise["valid"] = (1, 0x0100, 7)                                           # (valid != 0 in either byte)
    desc[rows_sp + 3] = noise[0]
    desc[n_rows:] = noise[1:]
    return dict(name=name, head=n_rows if head is None else head, store=store, store_lens=lens, range_max=range_max, desc=desc, rep=rep, n_rows=n_rows)


def describe_campaign(long_row=False):
    """Cases: dict(name, head, store [nodes_cap, stride, 2], store_lens, range_max, desc).  long_row: the one case of stride 1025 (a context
    of raised scan capacity) instead of the others."""
    rng = np.random.default_rng(20251017)
    if long_row:
        return [describe_case("stride_1025", 1025, 0, rng)]
    out = []
    for stride in DESCRIBE_STRIDES:
        for rep in range(3):
            out.append(describe_case("stride_%d_%d" % (stride, rep), stride, rep, rng, range_max=(4.0, 3.7, 12.5)[rep]))
    for rep in range(3):
        c = describe_case("head_below_0_%d" % rep, 8, rep, rng, head=-1 - rep)
        out.append(c)
        c = describe_case("head_above_cap_%d" % rep, 8, rep, rng)
        c["head"] = len(c["desc"]) + (1, 2, 1000)[rep]
        out.append(c)
    return out


def run_describe_case(case):
    tr = []
    return describe(case["head"], case["store"], case["store_lens"], case["range_max"], case["desc"], tr), tr


def describe_classes_of(case, tr):
    c = set()
    cap, rm = len(case["desc"]), case["range_max"]
    edges = {edge(k) for k in range(1, 64)}
    for ev in tr:
        if ev.get("described"):
            if ev["len"] == 0: c.add("len_0")
            if ev["len"] < 0: c.add("len_negative")
            if ev["len"] > case["store"].shape[1]: c.add("len_above_stride")
            if not any(ev["cnts"]): c.add("all_empty")
            if any(n > 1 and s % n for s, n in zip(ev["sums"], ev["cnts"])): c.add("mean_divides")
            continue
        r, a = ev["r"], ev["a"]
        if ev["used"]:
            if a in edges: c.add("edge_exact")
            if up(a) in edges: c.add("edge_below")
            if pg.below(a) in edges: c.add("edge_above")
            if a < 0: c.add("negative_angle")
            if a > TWO_PI: c.add("above_2pi")
            if ev["f"] == 1.0 and ev["s"] == 63: c.add("f_eq_1")
            if r == rm: c.add("range_at_max")
        else:
            if r == up(rm): c.add("range_above_max")
            if r == 0: c.add("range_zero")
            if r < 0: c.add("range_negative")
            if math.isinf(r): c.add("range_inf")
            if math.isnan(r): c.add("range_nan")
            if math.isnan(a): c.add("angle_nan")
    n = pg.clamp(case["head"], cap)
    if any(int(case["desc"][k]["valid"]) for k in range(n)): c.add("valid_survives")
    if n < cap: c.add("rows_past_n")
    if case["head"] < 0: c.add("head_below_0")
    if case["head"] > cap: c.add("head_above_cap")
    return c


# ---- the recognize campaign ------------------------------------------------------------------------------------------------------------
RECOGNIZE_SIZES = (1, 2, 255, 256, 257, 1025)
RECOGNIZE_CLASSES = ("no_query", "query_invalid", "query_below_min_sectors", "j_below_gap", "candidate_at_gap", "dist_at_max", "dist_above_max",
                     "sectors_at_min", "sectors_below_min", "tie_dist", "tie_shift", "turned_0", "turned_1", "turned_31", "turned_32", "turned_63",
                     "spread_0", "suppress_cut_by_0", "suppress_cut_by_gap", "k_1", "k_8", "fewer_than_k", "pick_unfilled", "window_cut_by_0",
                     "window_cut_by_gap", "candidate_invalid") + tuple("n_%d" % n for n in RECOGNIZE_SIZES)
ONCE = ("n_16384",)
TURNS = (0, 1, 31, 32, 63)


def place_graph(n, nodes_cap, stride, rng, last=None):
    """A graph of n nodes at random poses with random store rows, and noise everywhere else."""
    g = pg.new_graph(nodes_cap, 4, stride, 1, rng)
    for k in range(n):
        g["nodes"][k]["x"], g["nodes"][k]["y"], g["nodes"][k]["ang"] = rng.uniform(5, 60), rng.uniform(5, 40), rng.uniform(-180, 180)
    g["store_lens"][:] = rng.integers(0, stride + 1, nodes_cap)
    g["head"][0]["n_nodes"] = n
    g["tracks"][0]["last"] = n - 1 if last is None else last
    return g


def random_desc(n, rng):
    d = np.zeros(n, DESC_DTYPE)
    d["v"] = rng.integers(0, 256, (n, SECTORS))
    d["n_hits"], d["n_sectors"], d["valid"] = rng.integers(64, 400, n), 64, 1
    return d


def near_copy(a, turn, bumps, rng):
    """The bytes of a candidate of the query bytes a: a seen `turn` sectors earlier (shift = turn) with `bumps` added in total, every bump
    at another sector, away from 0 and 255 so that it adds what it says."""
    c = np.roll(np.asarray(a, np.int64), -turn).copy()                          # c[k] = a[(k + turn) mod 64]
    left = int(bumps)
    for k in rng.permutation(SECTORS):
        if left == 0:
            break
        if c[k] >= 128:
            step = min(left, int(c[k]))
            c[k] -= step
        else:
            step = min(left, int(255 - c[k]))
            c[k] += step
        left -= step
    assert left == 0
    return c.astype(np.uint8)


def rcase(name, g, desc, rng, **par):
    cap = len(g["nodes"])
    full = rng.integers(0, 256, (cap, 72), dtype=np.uint8).view(DESC_DTYPE).reshape(cap).copy()      # noise past the described rows
    full[:len(desc)] = desc
    return dict(name=name, graph=g, desc=full, par=place(**par), work=rng.integers(0, 2 ** 32, cap, dtype=np.uint32))


def recognize_campaign(big=False):
    """Cases: dict(name, graph, desc [nodes_cap], par, work: the workspace's bytes before the call).  big: the one case of 16384 nodes whose
    descriptors come from rows of 8 readings, instead of the others."""
    rng = np.random.default_rng(20251018)
    if big:
        n = 16384
        g = place_graph(n, n, 8, rng)
        g["store"][:, :, 0], g["store"][:, :, 1] = rng.uniform(0.2, 4.4, (n, 8)), rng.uniform(0.0, TWO_PI, (n, 8))
        g["store_lens"][:] = 8
        for i in (5, 4000, 9000, 16000):                                      # the query's own scan, turned, at four old nodes
            g["store"][i] = g["store"][n - 1]
            g["store"][i, :, 1] -= (i % 64) * TWO_PI / 64
        g["store"][4000, 0, 0] += 0.05
        desc = describe(n, g["store"], g["store_lens"], RANGE_MAX, np.zeros(n, DESC_DTYPE))
        c = rcase("n_16384", g, desc, rng, gap=300, window=3, spread=5, k=8, pick=1, max_dist=400, min_sectors=4)
        c["n_class"] = "n_16384"
        return [c]
    out = []

    def add(name, n, desc, last=None, extra=3, **par):
        g = place_graph(n, n + extra, 1 + len(out) % 5, rng, last)
        out.append(rcase(name, g, desc, rng, **par))
        if n in RECOGNIZE_SIZES:
            out[-1]["n_class"] = "n_%d" % n
    for rep in range(3):
        # the sizes: random descriptors with planted copies of the query (the last node)
        for n in RECOGNIZE_SIZES:
            d = random_desc(n, rng)
            gap = max(1, min(10, n // 3))
            for t, i in enumerate(range(0, max(n - gap, 0), max(1, n // 7))):
                d[i]["v"] = near_copy(d[n - 1]["v"], (7 * t + rep) % 64, 10 * t + rep, rng)
            add("size_%d_%d" % (n, rep), n, d, gap=gap, window=2 + rep, spread=rep, k=(1, 4, 8)[rep], pick=0, max_dist=900)
        # no query, an invalid query, a query below min_sectors, a query younger than the gap
        d = random_desc(12, rng)
        add("no_query_%d" % rep, 12, d, last=(-1, 12, 40)[rep], gap=2)
        d = random_desc(12, rng)
        d[11]["valid"] = 0
        add("query_invalid_%d" % rep, 12, d, gap=2 + rep)
        d = random_desc(12, rng)
        d[11]["n_sectors"] = 15 - rep
        add("query_below_min_sectors_%d" % rep, 12, d, gap=2)
        add("j_below_gap_%d" % rep, 5 + rep, random_desc(5 + rep, rng), gap=6 + rep, max_dist=MAX_DIST)
        # thresholds: the only near copies sit at j - gap (dist == max_dist) and one before it (one above); min_sectors at and one below
        n = 20 + rep
        d = random_desc(n, rng)
        gap = 4 + rep
        d[n - 1 - gap]["v"] = near_copy(d[n - 1]["v"], 3, 100 + rep, rng)
        d[n - 2 - gap]["v"] = near_copy(d[n - 1]["v"], 5, 101 + rep, rng)
        d[2]["v"], d[2]["n_sectors"] = near_copy(d[n - 1]["v"], 9, 1, rng), 20
        d[3]["v"], d[3]["n_sectors"] = near_copy(d[n - 1]["v"], 9, 0, rng), 19
        d[4]["v"], d[4]["valid"] = near_copy(d[n - 1]["v"], 9, 0, rng), 0
        d[n - gap]["v"] = d[n - 1]["v"]                                       # one node too young: no candidate
        add("thresholds_%d" % rep, n, d, gap=gap, max_dist=100 + rep, min_sectors=20, spread=0, k=8, window=3)
        # equal distances on two nodes, and on two shifts (a query of period 32: D_s == D_(s + 32))
        d = random_desc(16, rng)
        d[9]["v"] = near_copy(d[15]["v"], 11, 40 + rep, rng)
        d[4]["v"] = near_copy(d[15]["v"], 50, 40 + rep, rng)
        add("tie_dist_%d" % rep, 16, d, gap=3, spread=1, k=3, pick=1)
        d = random_desc(16, rng)
        d[15]["v"] = np.tile(d[15]["v"][:32], 2)
        d[6 + rep]["v"] = near_copy(d[15]["v"], 40 + rep, 7, rng)
        add("tie_shift_%d" % rep, 16, d, gap=3, k=1)
        # suppression and selection windows cut by node 0 and by j - gap; fewer candidates than k; pick on an unfilled round
        n = 30
        d = random_desc(n, rng)
        for i, b in ((0, 1), (1, 9), (2, 8), (3, 30), (12, 20), (18, 7), (19, 6), (20, 2)):
            d[i]["v"] = near_copy(d[n - 1]["v"], i, b + rep, rng)
        add("cut_by_0_%d" % rep, n, d, gap=9, spread=2 + rep, window=1 + rep, k=4, pick=0)
        add("cut_by_gap_%d" % rep, n, d, gap=9, spread=2 + rep, window=1 + rep, k=4, pick=1)
        add("fewer_than_k_%d" % rep, n, d, gap=9, spread=25, k=8, pick=(1, 7, 2)[rep])
    # a scan against its own copy turned by m sectors: 64 beams at the sectors' centres, the query's angles m sectors further on
    for m in TURNS:
        for rep in range(3):
            n = 9
            g = place_graph(n, n + 2, 64, rng)
            g["store_lens"][:n] = 64
            g["store"][:n, :, 0] = rng.uniform(0.2, 3.9, (n, 64))
            g["store"][:n, :, 1] = (np.arange(64) + 0.5) * (TWO_PI / 64)
            anchor = 1 + rep
            g["store"][n - 1, :, 0] = g["store"][anchor, :, 0]
            g["store"][n - 1, :, 1] = (np.arange(64) + 0.5 + m) * (TWO_PI / 64)
            desc = describe(n, g["store"], g["store_lens"], RANGE_MAX, np.zeros(n, DESC_DTYPE))
            c = rcase("turned_%d_%d" % (m, rep), g, desc, rng, gap=3, k=2, spread=0, window=1, max_dist=50)
            c.update(turn=m, anchor=anchor)
            out.append(c)
    return out


_recognized = {}


def run_recognize_case(case):
    """(the outputs of recognize, the trace); the results are kept."""
    if case["name"] not in _recognized:
        tr = {}
        q_scan = np.full((case["graph"]["store"].shape[1], 2), 0.125)
        _recognized[case["name"]] = recognize(case["graph"], 0, case["desc"], case["par"], case["work"], q_scan, tr), tr
    return _recognized[case["name"]]


def recognize_classes_of(case, tr):
    c = set()
    p, j, n, limit = tr["par"], tr["j"], tr["n_nodes"], tr["limit"]
    if "n_class" in case:
        c.add(case["n_class"])
    c.add("k_%d" % p["k"])
    if not 0 <= j < n:
        return c | {"no_query"}
    if tr["valid_j"] == 0:
        return c | {"query_invalid"}
    if tr["sectors_j"] < p["min_sectors"]:
        return c | {"query_below_min_sectors"}
    if j < p["gap"]:
        return c | {"j_below_gap"}
    desc, D = case["desc"], tr["D"]
    best = D.min(axis=1)
    for i in range(limit + 1):
        if int(desc[i]["valid"]) == 0:
            c.add("candidate_invalid")
        elif int(desc[i]["n_sectors"]) == p["min_sectors"] - 1 and best[i] <= p["max_dist"]:
            c.add("sectors_below_min")
        elif int(desc[i]["n_sectors"]) >= p["min_sectors"] and best[i] == p["max_dist"] + 1:
            c.add("dist_above_max")
    for i in tr["cands"]:
        if int(desc[i]["n_sectors"]) == p["min_sectors"]: c.add("sectors_at_min")
        if best[i] == p["max_dist"]: c.add("dist_at_max")
        if i == limit: c.add("candidate_at_gap")
    before = []
    for r, a in enumerate(tr["picked"]):
        open_ = [i for i in tr["cands"] if all(abs(i - b) > p["spread"] for b in before)]
        if sum(1 for i in open_ if best[i] == best[a]) > 1: c.add("tie_dist")
        if int((D[a] == best[a]).sum()) > 1: c.add("tie_shift")
        if r + 1 < p["k"] and p["spread"] > 0:                                  # (a window that suppresses for a later round)
            if a - p["spread"] < 0: c.add("suppress_cut_by_0")
            if a + p["spread"] > limit: c.add("suppress_cut_by_gap")
        before.append(a)
    if p["spread"] == 0 and len(tr["picked"]) > 1: c.add("spread_0")
    if len(tr["picked"]) < p["k"]: c.add("fewer_than_k")
    if tr["anchor"] < 0 and p["pick"] > 0 and tr["picked"]: c.add("pick_unfilled")
    if tr["anchor"] >= 0:
        if tr["anchor"] - p["window"] < 0: c.add("window_cut_by_0")
        if tr["anchor"] + p["window"] > limit: c.add("window_cut_by_gap")
    if "turn" in case:
        c.add("turned_%d" % case["turn"])
    return c


# ---- end to end: a loop that pose proximity cannot see ---------------------------------------------------------------------------------
# A rectangle with a box off its centre: no half turn maps it onto itself (gm.ROOM is symmetric about the loop's centre: opposite
# keyframes would tie).  The walls' cell lines; x0 == x1 or y0 == y1.
PLACE_ROOM = dict(cols=61, rows=47, resol=0.05, range_max=4.0)
WALLS = ((8, 6, 52, 6), (52, 6, 52, 40), (52, 40, 8, 40), (8, 40, 8, 6), (31, 20, 37, 20), (37, 20, 37, 25), (37, 25, 31, 25), (31, 25, 31, 20))
E2E = dict(n=24, n_beams=128, gap=18, radius=10.0, bias=-2.5,
           place=place(gap=18, window=2, spread=2, k=3, pick=0, max_dist=1500, min_sectors=32),
           search=gm.search(4, 4, 6, 1.0, min_beams=40, min_num=1, min_den=2), response=gr.params(2, 2, 1), closure=(1.0, 0.25, 0.25),
           append=dict(min_dist=1.0, min_ang=5.0, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0)), relax=dict(pg.RELAX_DEFAULTS, iters=12, cg_iters=75, cg_tol=1e-8))
_e2e = None


def place_room_scan(pose, n_beams):
    """The scan of PLACE_ROOM from `pose` (x, y in cells, ang in degrees): ranges in metres to the nearest wall, the beams evenly spread."""
    x, y, ang = pose
    out = []
    for k in range(n_beams):
        a = -math.pi + 2 * math.pi * (k + 0.5) / n_beams
        th = a + math.radians(ang)
        c, s = math.cos(th), math.sin(th)
        best = math.inf
        for x0, y0, x1, y1 in WALLS:
            if x0 == x1 and c != 0:
                t = (x0 - x) / c
                if t > 0 and min(y0, y1) <= y + t * s <= max(y0, y1):
                    best = min(best, t)
            if y0 == y1 and s != 0:
                t = (y0 - y) / s
                if t > 0 and min(x0, x1) <= x + t * c <= max(x0, x1):
                    best = min(best, t)
        out.append((best * PLACE_ROOM["resol"], a))
    return np.array(out)


def end_to_end():
    """The chain restated once and shared: one lap of 24 keyframes of 128 beams around the box, odometry with a heading bias that opens the
    loop beyond near's radius; append -> (near finds nothing) -> describe -> recognize -> integrate at the selection -> likelihood -> match
    -> response -> closure -> relax -> rerender.  Returns a dict with the inputs, every intermediate record and the re-rendered planes."""
    global _e2e
    if _e2e is not None:
        return _e2e
    R, n, nb = PLACE_ROOM, E2E["n"], E2E["n_beams"]
    rng = np.random.default_rng(12)
    truth = []
    for k in range(n + 1):                                                   # one lap and a little: the last frame is near the first
        a = 363.0 * k / n
        truth.append((30.0 + 13.0 * math.cos(math.radians(a)), 23.0 + 10.0 * math.sin(math.radians(a)), pg.wrap(a + 90.0)))
    odom = [truth[0]]
    for k in range(1, n + 1):
        z = pg.rel(truth[k - 1], truth[k])
        odom.append(pg.comp(odom[-1], (z[0] + 0.02 * rng.normal(), z[1] + 0.02 * rng.normal(), z[2] + E2E["bias"] * rng.uniform(0.8, 1.0))))
    scans = np.stack([place_room_scan(p, nb) for p in truth])
    lens = np.full(n + 1, nb, np.int32)
    g0 = pg.new_graph(n + 4, n + 8, nb)
    g1, arep = pg.append(g0, scans, lens, np.array(odom), 0, E2E["append"])
    q0 = np.zeros((nb, 2))
    near_by_pose = pg.near(g1, 0, E2E["gap"], E2E["radius"], E2E["place"]["window"], q0)[0]
    desc = describe(g1["head"][0]["n_nodes"], g1["store"], g1["store_lens"], R["range_max"], np.zeros(n + 4, DESC_DTYPE))
    tr = {}
    work, recs, prep, nrec, sel, row, q_len, q_pose = recognize(g1, 0, desc, E2E["place"], np.zeros(n + 4, np.uint32), q0, tr)
    cols, rows = R["cols"], R["rows"]
    pa, hi = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g1["store"], g1["store_lens"], sel, cols, rows, R["resol"], R["range_max"], pa, hi)
    corr = gm.likelihood(pa, hi, 2, 1, 10, 3, gm.GAUSS)
    mrec = gm.match(row[None], np.array([q_len], np.int32), q_pose[None], R["resol"], R["range_max"], corr, E2E["search"])
    resp, _ = gr.response(row[None], np.array([q_len], np.int32), q_pose[None], mrec, R["resol"], R["range_max"], corr, E2E["search"]["ang_step"],
                          E2E["response"])
    g2, crep = pg.closure(g1, nrec, resp[0], E2E["closure"])
    nn, ne = int(g2["head"][0]["n_nodes"]), int(g2["head"][0]["n_edges"])
    nodes, edges, rrep = pg.relax(g2["nodes"][:nn], g2["edges"][:ne], E2E["relax"])
    g3 = pg.copy_graph(g2)
    g3["nodes"][:nn], g3["edges"][:ne] = nodes, edges
    pa2, hi2 = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g3["store"], g3["store_lens"], np.stack([g3["nodes"]["x"], g3["nodes"]["y"], g3["nodes"]["ang"]], axis=1), cols, rows, R["resol"],
                 R["range_max"], pa2, hi2)
    _e2e = dict(truth=np.array(truth), odom=np.array(odom), scans=scans, lens=lens, g0=g0, g1=g1, append_rep=arep, near_by_pose=near_by_pose, desc=desc,
                work=work, recs=recs, place_rep=prep, near=nrec, sel=sel, q_row=row, q_len=q_len, q_pose=q_pose, trace=tr, corr=corr, match=mrec, resp=resp,
                g2=g2, closure_rep=crep, g3=g3, relax_rep=rrep, planes=(pa2, hi2), n_nodes=nn, n_edges=ne)
    return _e2e
