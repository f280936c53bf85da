"""The robust relaxation and the rejection of closures (include/lsd_hip.h: lsd_enqueue_pg_relax_robust_device, lsd_enqueue_pg_prune_device;
csrc/k_posegraph.hip, csrc/k_pgprune.hip) restated on Python floats, in the header's order, written from the header for the
tests (not from the HIP code), the chain of the two (optimize), and the generated campaigns both test files run.

Everything the plain relaxation has is pose_graph_cases' own text (edge_blocks, reduce_shape, inv3, ..); math.sqrt and IEEE's division are
the device's sqrt and / (-fno-fast-math).  One thing is restated and not left to the host that runs the tests: a NaN made from finite
numbers (inf - inf, 0 * inf, inf / inf) is the quiet NaN with the sign set, 0xfff8000000000000, on gfx950 as on x86 -- another host's default
may differ; no operation of the rule turns a NaN's sign and an input that is not finite is skipped, so every NaN among the outputs is
written as that one (canon()).  A case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import pose_graph_cases as pg

ROBUST_REP_DTYPE = np.dtype([("chi2_plain", "f8"), ("w_min", "f8"), ("downweighted", "i4"), ("w_min_edge", "i4")])
PRUNE_REP_DTYPE = np.dtype([("candidates", "i4"), ("rejected", "i4"), ("worst_edge", "i4"), ("closures_left", "i4"), ("worst_chi2", "f8")])
SIZES = {"lsd_pg_robust_par": 16, "lsd_pg_robust_rep": 24, "lsd_pg_prune_par": 16, "lsd_pg_prune_rep": 24}
NONE, HUBER, GM = 0, 1, 2
CLOSURES, ALL = 0, 1
EDGE_REJECTED = 4
MAX_REJECT = 64
ROBUST_KEYS = ("kernel", "scope", "delta")
GATE = 11.345                                                                 # chi2 of 3 degrees of freedom at 1 %
INF, NAN = pg.INF, pg.NAN
CLOSURE_INFO = (25.0, 0.0, 25.0, 0.0, 0.0, 9.0)


def rob(kernel, delta=1.0, scope=CLOSURES):
    return dict(kernel=int(kernel), scope=int(scope), delta=float(delta))


MADE_NAN = float(np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0])


def canon(v):
    """A NaN as the device makes it (the module's text)."""
    return v if v == v else MADE_NAN


# ---- the weight and the cost -----------------------------------------------------------------------------------------------------------
def weight(r, in_scope, s):
    """(w, rho) of an edge whose plain chi2_e is s."""
    if not in_scope or r["kernel"] == NONE:
        return 1.0, s
    delta = r["delta"]
    c = delta * delta
    if r["kernel"] == HUBER:
        if s <= c:
            return 1.0, s
        q = math.sqrt(s)
        return pg.fdiv(delta, q), (2.0 * delta) * q - c
    t = pg.fdiv(c, c + s)
    return t * t, pg.fdiv(c * s, c + s)


# ---- the robust relaxation -------------------------------------------------------------------------------------------------------------
def relax_robust(nodes, edges, par, r, trace=None):
    """lsd_enqueue_pg_relax_robust_device on one graph: nodes NODE_DTYPE [N], edges EDGE_DTYPE [E] (the clamped counts) -> (nodes after,
    edges after, the report, the robust report).  par: a dict of pg.RELAX_KEYS; r: rob()."""
    with np.errstate(all="ignore"):
        return _relax_robust(nodes, edges, par, r, trace if trace is not None else {})


def _relax_robust(nodes, edges, par, rb, tr):
    nodes, edges = nodes.copy(), edges.copy()
    N, E = len(nodes), len(edges)
    lam, lam_min, up, down = float(par["lambda0"]), float(par["lambda_min"]), float(par["up"]), float(par["down"])
    cg_tol, eps, iters, cg_iters = float(par["cg_tol"]), float(par["eps"]), int(par["iters"]), int(par["cg_iters"])
    P = [pg.pose_of(n) for n in nodes]
    fixed = [bool(int(n["flags"]) & pg.NODE_FIXED) for n in nodes]
    singular = [False] * N
    valid, why = [], []
    for e in edges:
        i, j = int(e["i"]), int(e["j"])
        w = None
        if int(e["flags"]) & pg.EDGE_DISABLED:
            w = "disabled"
        elif i == j:
            w = "self"
        elif not (0 <= i < N and 0 <= j < N):
            w = "range"
        elif not all(math.isfinite(float(v)) for v in list(e["z"]) + list(e["info"]) + list(P[i]) + list(P[j])):
            w = "not_finite"
        valid.append(w is None)
        why.append(w)
    scope = [valid[e] and (rb["scope"] == ALL or bool(int(edges[e]["flags"]) & pg.EDGE_CLOSURE)) for e in range(E)]
    lists = [[] for _ in range(N)]
    for e in range(E):
        if valid[e]:
            lists[int(edges[e]["i"])].append((e, 0))
            lists[int(edges[e]["j"])].append((e, 1))
    ei, ej = [int(e["i"]) for e in edges], [int(e["j"]) for e in edges]
    Z = [[float(v) for v in e["z"]] for e in edges]
    W = [pg.info_rows([float(v) for v in e["info"]]) for e in edges]
    seen = []                                                                 # every (edge, s) a weight was made from, for the classes

    def chi2s(poses):
        return [pg.edge_chi2(poses[ei[e]], poses[ej[e]], Z[e], W[e]) if valid[e] else 0.0 for e in range(E)]

    def objective(ce):
        for e in range(E):
            if scope[e]:
                seen.append((e, ce[e]))
        return pg.reduce_shape([weight(rb, scope[e], ce[e])[1] if valid[e] else 0.0 for e in range(E)])
    ce = chi2s(P)
    F = objective(ce)
    rep = np.zeros(1, pg.RELAX_REP_DTYPE)[0]
    rep["chi2_before"] = canon(F)
    flags, done, cg_total, accepted, rejected = 0, 0, 0, 0, 0
    tr.update(N=N, E=E, why=why, scope=scope, steps=[])
    moved = set()
    if not math.isfinite(F):
        flags |= pg.RELAX_NOT_FINITE
    while not flags & pg.RELAX_NOT_FINITE and done < iters:
        blk = [None] * E                                                     # 1: the blocks from W' = w_e * W
        for e in range(E):
            if valid[e]:
                we = weight(rb, scope[e], ce[e])[0]
                Wp = [[we * W[e][r][t] for t in range(3)] for r in range(3)]
                blk[e] = pg.edge_blocks(P[ei[e]], P[ej[e]], Z[e], Wp)[:5]
        H, b, M = [None] * N, [None] * N, [None] * N
        for n in range(N):                                                   # 2, 3
            Hn, bn = [[0.0] * 3 for _ in range(3)], [0.0] * 3
            for e, side in lists[n]:
                src, sb = blk[e][2 if side else 0], blk[e][4 if side else 3]
                for r in range(3):
                    for q in range(3):
                        Hn[r][q] += src[r][q]
                    bn[r] += sb[r]
            H[n], b[n] = Hn, bn
            if not fixed[n] and not singular[n]:
                D = [[Hn[r][q] if r != q else Hn[r][r] + lam * Hn[r][r] for q in range(3)] for r in range(3)]
                M[n], _ = pg.inv3(D)
                if M[n] is None:
                    singular[n] = True
        free = [not fixed[n] and not singular[n] for n in range(N)]
        zero = [0.0, 0.0, 0.0]
        dl = [list(zero) for _ in range(N)]                                  # 4
        r_ = [[-b[n][q] for q in range(3)] if free[n] else list(zero) for n in range(N)]
        z_ = [[pg.dot3(M[n][q], r_[n]) for q in range(3)] if free[n] else list(zero) for n in range(N)]
        p_ = [list(v) for v in z_]
        rz = pg.reduce_shape([pg.dot3(r_[n], z_[n]) for n in range(N)])
        thr = (cg_tol * cg_tol) * rz
        steps = 0
        while steps < cg_iters and not rz <= thr:
            q_ = []
            for n in range(N):
                if not free[n]:
                    q_.append(list(zero))
                    continue
                Hn = H[n]
                qv = [pg.dot3([Hn[r][c] if c != r else Hn[r][r] + lam * Hn[r][r] for c in range(3)], p_[n]) for r in range(3)]
                for e, side in lists[n]:
                    hab = blk[e][1]
                    po = p_[ei[e]] if side else p_[ej[e]]
                    for r in range(3):
                        t = 0.0
                        for c in range(3):
                            t += (hab[c][r] if side else hab[r][c]) * po[c]
                        qv[r] = qv[r] + t
                q_.append(qv)
            pq = pg.reduce_shape([pg.dot3(p_[n], q_[n]) for n in range(N)])
            if not pq > 0:
                flags |= pg.BREAKDOWN
                break
            alpha = pg.fdiv(rz, pq)
            for n in range(N):
                if free[n]:
                    for c in range(3):
                        dl[n][c] = dl[n][c] + alpha * p_[n][c]
                        r_[n][c] = r_[n][c] - alpha * q_[n][c]
                    z_[n] = [pg.dot3(M[n][c], r_[n]) for c in range(3)]
            rzn = pg.reduce_shape([pg.dot3(r_[n], z_[n]) for n in range(N)])
            beta = pg.fdiv(rzn, rz)
            for n in range(N):
                if free[n]:
                    for c in range(3):
                        p_[n][c] = z_[n][c] + beta * p_[n][c]
            rz = rzn
            steps += 1
        cg_total += steps
        trial, maxd = [], 0.0                                                # 5
        for n in range(N):
            if free[n]:
                trial.append((P[n][0] + dl[n][0], P[n][1] + dl[n][1], pg.wrap(P[n][2] + dl[n][2])))
                for c in range(3):
                    v = abs(dl[n][c])
                    maxd = v if v > maxd else maxd
            else:
                trial.append(P[n])
        cen = chi2s(trial)
        Fn = objective(cen)
        done += 1
        if Fn <= F:
            P, ce, F = trial, cen, Fn
            moved.update(n for n in range(N) if free[n])
            l = pg.fdiv(lam, down)
            lam = l if l > lam_min else lam_min
            accepted += 1
            tr["steps"].append("accepted")
            if maxd < eps:
                flags |= pg.CONVERGED
                break
        else:
            lam = lam * up
            rejected += 1
            tr["steps"].append("rejected")
    for n in sorted(moved):                                                  # every other node keeps its bytes
        nodes[n]["x"], nodes[n]["y"], nodes[n]["ang"] = P[n]
    for e in range(E):
        edges[e]["chi2"] = canon(ce[e])
    rep["chi2_after"], rep["lambda"] = canon(F), lam
    rep["iters"], rep["cg_iters"], rep["accepted"], rep["rejected"] = done, cg_total, accepted, rejected
    rep["skipped_edges"], rep["singular_nodes"], rep["flags"] = sum(1 for v in valid if not v), sum(singular), flags
    # the robust report: the weights at the final poses
    rr = np.zeros(1, ROBUST_REP_DTYPE)[0]
    rr["chi2_plain"] = canon(pg.reduce_shape(ce))
    w_fin = {e: weight(rb, True, ce[e])[0] for e in range(E) if scope[e]}
    nans = [e for e, w in w_fin.items() if w != w]
    w_min, w_edge = 1.0, -1
    if nans:
        w_min, w_edge = MADE_NAN, min(nans)
    elif w_fin:
        w_min = min(w_fin.values())
        w_edge = min(e for e, w in w_fin.items() if w == w_min)
    rr["w_min"], rr["w_min_edge"], rr["downweighted"] = w_min, w_edge, sum(1 for w in w_fin.values() if w < 1.0)
    tr.update(flags=flags, seen=seen, w_fin=w_fin)
    return nodes, edges, rep, rr


# ---- prune -----------------------------------------------------------------------------------------------------------------------------
def prune(n_edges, edges, gate, max_reject, trace=None):
    """lsd_enqueue_pg_prune_device on one graph: n_edges as the head holds it, edges EDGE_DTYPE [edges_cap] -> (edges after, the report)."""
    edges = edges.copy()
    E = pg.clamp(n_edges, len(edges))
    fl, chi = edges["flags"][:E].astype(np.int64), edges["chi2"][:E]
    with np.errstate(all="ignore"):
        cand = [e for e in range(E) if fl[e] & pg.EDGE_CLOSURE and not fl[e] & pg.EDGE_DISABLED and not chi[e] <= gate]
    order = sorted(cand, key=lambda e: (-(INF if chi[e] != chi[e] else float(chi[e])), e))
    hit = order[:min(max_reject, len(order))]
    for e in hit:
        edges["flags"][e] |= pg.EDGE_DISABLED | EDGE_REJECTED
    rep = np.zeros(1, PRUNE_REP_DTYPE)[0]
    rep["candidates"], rep["rejected"], rep["worst_edge"] = len(cand), len(hit), order[0] if order else -1
    if order:
        rep["worst_chi2"] = edges["chi2"][order[0]]                          # (its bytes as they stand, a NaN's too)
    fl = edges["flags"][:E].astype(np.int64)
    rep["closures_left"] = int(np.count_nonzero((fl & pg.EDGE_CLOSURE != 0) & (fl & pg.EDGE_DISABLED == 0)))
    if trace is not None:
        trace.update(E=E, cand=cand, order=order, hit=hit, n_edges=int(n_edges), cap=len(edges), gate=gate, max_reject=max_reject)
    return edges, rep


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
def optimize(nodes, edges, r, gate, max_reject=8, relax=None, refit=None):
    """PoseGraph.optimize_device on the clamped counts: the robust relaxation, prune, the plain relaxation over the survivors.  Returns a dict:
    nodes, edges, and the reports robust_relax, robust, prune, refit."""
    relax = dict(pg.RELAX_DEFAULTS, **(relax or {}))
    refit = relax if refit is None else dict(pg.RELAX_DEFAULTS, **refit)
    n1, e1, rep1, rr = relax_robust(nodes, edges, relax, r)
    e2, prep = prune(len(e1), e1, gate, max_reject)
    n3, e3, rep3 = pg.relax(n1, e2, refit)
    return dict(nodes=n3, edges=e3, robust_relax=rep1, robust=rr, prune=prep, refit=rep3)


# ---- the inputs of DESIGN.md 8.1.16's table: graphs with closures that are confidently wrong -------------------------------------------
def false_closure(truth, i, j, offset=(6.0, -5.0, 25.0), info=CLOSURE_INFO):
    zt = pg.rel(tuple(truth[i]), tuple(truth[j]))
    return pg.edge(i, j, (zt[0] + offset[0], zt[1] + offset[1], pg.wrap(zt[2] + offset[2])), info, pg.EDGE_CLOSURE)


def drifted(n, seed, closures, falses, offset=(6.0, -5.0, 25.0)):
    """loop_graph(n, rng(seed), closures=) and the same with false closures appended: (nodes, clean edges, edges, the false indices)."""
    nodes, edges, truth = pg.loop_graph(n, np.random.default_rng(seed), closures=closures)
    bad = np.array([false_closure(truth, i, j, offset) for i, j in falses], pg.EDGE_DTYPE).reshape(-1)
    return nodes, edges, np.concatenate([edges, bad]), list(range(len(edges), len(edges) + len(bad)))


DRIFTED = (dict(name="drifted_24_1_1", n=24, seed=2400, closures=1, falses=[(3, 14)]),
           dict(name="drifted_24_2_2", n=24, seed=2401, closures=2, falses=[(3, 14), (5, 20)]),
           dict(name="drifted_100_3_1", n=100, seed=10000, closures=3, falses=[(10, 60)]))


def relaxed_with_false_closure(offset=(6.0, -5.0, 25.0)):
    """The relaxed end-to-end graph of pose_graph_cases with a false closure 5 -> 17: (nodes, clean edges, edges, the false indices)."""
    E = pg.end_to_end()
    nn, ne = E["n_nodes"], E["n_edges"]
    nodes, edges = E["g3"]["nodes"][:nn].copy(), E["g3"]["edges"][:ne].copy()
    bad = np.array([false_closure(E["truth"], 5, 17, offset)], pg.EDGE_DTYPE)
    return nodes, edges, np.concatenate([edges, bad]), [ne]


# ---- the relaxation campaign -----------------------------------------------------------------------------------------------------------
def rcase(name, nodes, edges, r, **par):
    c = pg.rcase(name, nodes, edges, **par)
    c["rob"] = r
    return c


PLAIN_NAMES = ("well_posed_8_0", "well_posed_8_1", "n_0_0", "n_1_0", "n_2_0", "n_3_0", "hub_0", "wrap_0", "all_fixed_0", "none_fixed_0", "skipped_0",
               "far_start_0", "breakdown_0", "singular_0", "cg_tol_end_0", "e_1024_0")
HUGE = 1e150                                                                  # a delta above every sqrt(chi2_e) that is finite


def hub_edges(e_count, rng):
    """The hub graph of pose_graph_cases' e_ cases: 40 nodes, a chain and random chords until there are e_count edges."""
    nodes, _ = pg.chain_graph(40, rng)
    es = [pg.edge(k - 1, k, (2.0, 0.0, 0.0)) for k in range(1, 40)]
    while len(es) < e_count:
        i, j = sorted(int(v) for v in rng.choice(40, 2, replace=False))
        es.append(pg.edge(i, j, (2.0 * (j - i), 0.0, 0.0), (0.5, 0.0, 0.5, 0.0, 0.0, 0.5)))
    return nodes, es


def relax_campaign():
    rng = np.random.default_rng(20261021)
    out = []
    by_name = {c["name"]: c for c in pg.relax_campaign()}
    for k, name in enumerate(PLAIN_NAMES):                                   # the plain entry's bytes: NONE, and a delta nothing reaches
        c = by_name[name]
        r = rob(NONE, 0.0, k % 2) if k % 2 == 0 else rob(HUBER, HUGE, ALL if k % 4 == 1 else CLOSURES)
        out.append(dict(c, name="%s_as_%s" % ("none" if k % 2 == 0 else "huge", name), rob=r, plain=name))
    c = by_name["not_finite_0"]
    out.append(dict(c, name="none_as_not_finite_0", rob=rob(NONE, -1.0), plain="not_finite_0"))
    for rep in range(3):                                                     # s exactly at c = 9.0 and one ulp above, at the start
        y = 0.5 * rep
        nodes = [pg.node(0.0, y, 0.0, pg.NODE_FIXED), pg.node(5.0, y, 0.0), pg.node(7.0, y, 0.0)]
        odo = [pg.edge(0, 1, (5.0, 0.0, 0.0)), pg.edge(1, 2, (2.5, 0.0, 0.0))]
        at = pg.edge(0, 1, (2.0, 0.0, 0.0), flags=pg.EDGE_CLOSURE)                                      # the error is (3, 0, 0): s = 9.0
        above = pg.edge(0, 2, (6.0, 0.0, 0.0), (math.nextafter(9.0, INF), 0.0, 1.0, 0.0, 0.0, 1.0), pg.EDGE_CLOSURE)   # (1, 0, 0): s = 9 + 1 ulp
        out.append(rcase("s_at_c_%d" % rep, nodes, odo + [at, above], rob(HUBER, 3.0, rep % 2), iters=3, cg_iters=12))
    for rep in range(5):                                                     # both kernels x both scopes, a true and a false closure;
        nodes, _, edges, _ = drifted(12, 500 + rep, 1, [(2, 8)])             # five graphs share the closures' settings: one launch of five
        for kname, kernel, delta in (("huber", HUBER, 1.0), ("gm", GM, 3.0)):
            for sname, scope in (("closures", CLOSURES), ("all", ALL)):
                if rep >= 2 and sname == "all":
                    continue
                out.append(rcase("%s_%s_%d" % (kname, sname, rep), nodes, edges, rob(kernel, delta, scope), iters=4, cg_iters=36))
    nodes, _, edges, _ = drifted(12, 502, 1, [(2, 8)])
    out.append(rcase("huber_all_2", nodes, edges, rob(HUBER, 0.5, ALL), iters=2, cg_iters=36))
    out.append(rcase("gm_all_2", nodes, edges, rob(GM, 1.0, ALL), iters=2, cg_iters=36))
    for rep in range(3):
        nodes, edges = pg.chain_graph(5 + rep, rng, extra=1)                  # no closure at all: nothing is in scope
        out.append(rcase("no_closure_%d" % rep, nodes, edges, rob((HUBER, GM, HUBER)[rep], 1.0), iters=2, cg_iters=20))
        nodes, _, edges, bad = drifted(12, 510 + rep, 1, [(2, 8)])           # the false closure is disabled
        edges["flags"][bad] |= pg.EDGE_DISABLED
        out.append(rcase("disabled_closure_%d" % rep, nodes, edges, rob((GM, HUBER, GM)[rep], 2.0), iters=2, cg_iters=36))
        neg = edges.copy()                                                   # an indefinite information on a closure: s < 0
        neg["flags"][bad] = pg.EDGE_CLOSURE
        neg["info"][bad] = (-3.0, 0.0, -3.0, 0.0, 0.0, -0.5)
        out.append(rcase("s_negative_%d" % rep, nodes, neg, rob((GM, HUBER, GM)[rep], 30.0 if rep == 2 else 2.0), iters=2, cg_iters=36))
        big = edges.copy()                                                   # s = +inf: NOT_FINITE, w = 0
        big["flags"][bad] = pg.EDGE_CLOSURE
        big["info"][bad] = (1e308, 0.0, 1e308, 0.0, 0.0, 1e308)
        big["z"][bad] = (1e200, 0.0, 0.0)
        out.append(rcase("s_inf_%d" % rep, nodes, big, rob((HUBER, GM, HUBER)[rep], 1.0, (CLOSURES, CLOSURES, ALL)[rep]), iters=3))
        nan = big.copy()                                                     # s = inf - inf: a NaN, on two edges
        nan["info"][bad] = (1e308, -1e308, 1e308, 0.0, 0.0, 1.0)
        nan["z"][bad] = (-1e200, -1e200, 0.0)
        nan = np.concatenate([nan[:3 + rep], nan[bad], nan[3 + rep:]])
        out.append(rcase("s_nan_%d" % rep, nodes, nan, rob((HUBER, GM, GM)[rep], 1.0, (CLOSURES, CLOSURES, ALL)[rep]), iters=3))
        far = nodes.copy()                                                   # a far start without damping: a step the robust objective rejects
        far["ang"][1:] += 100.0 + 20.0 * rep
        far["x"][1:] += 30.0
        clean = edges.copy()
        clean["flags"][bad] = pg.EDGE_CLOSURE
        out.append(rcase("far_start_%d" % rep, far, clean, rob((HUBER, GM, HUBER)[rep], 1.0, (ALL, ALL, CLOSURES)[rep]), iters=6, cg_iters=60, lambda0=0.0,
                         lambda_min=0.0))
        out.append(rcase("iters_0_%d" % rep, nodes, clean, rob((HUBER, GM, GM)[rep], 1.0, rep % 2), iters=0))
        # to the end: steps near the minimum of the robust objective no longer lower it and are rejected
        out.append(rcase("to_the_end_%d" % rep, nodes, clean, rob((HUBER, GM, HUBER)[rep], (1.0, 3.0, 2.0)[rep], (CLOSURES, CLOSURES, ALL)[rep]), iters=20,
                         cg_iters=36))
    for e_count in (1023, 1024, 1025):                                       # E beside the reduction's stride, edges downweighted on both sides
        for rep in range(3):
            nodes, es = hub_edges(e_count, rng)
            for k in (3, 500, e_count - 1):                                  # (the last index of 1025 edges is beyond the stride)
                es[k]["z"][0] += 4.0 + rep
            out.append(rcase("e_%d_%d" % (e_count, rep), nodes, es, rob((HUBER, GM, HUBER)[rep], 1.0, ALL), iters=1, cg_iters=4))
    return out


RELAX_CLASSES = ("huber_closures", "huber_all", "gm_closures", "gm_all", "none", "huge_delta", "s_at_c", "s_ulp_above_c", "s_negative", "s_inf", "s_nan",
                 "not_finite", "rejected_step", "every_closure_downweighted", "no_closure", "disabled_closure", "e_1023", "e_1024", "e_1025",
                 "downweighted_beyond_stride", "iters_0", "nan_on_two_edges")


def relax_classes_of(case, tr):
    r, edges = case["rob"], case["edges"]
    c = set()
    real = r["kernel"] != NONE and r["delta"] != HUGE
    if real:
        c.add("%s_%s" % ("huber" if r["kernel"] == HUBER else "gm", "all" if r["scope"] == ALL else "closures"))
    if r["kernel"] == NONE:
        c.add("none")
    if r["delta"] == HUGE:
        c.add("huge_delta")
    cc = r["delta"] * r["delta"]
    for e, s in tr["seen"]:
        if real and r["kernel"] == HUBER and s == cc:
            c.add("s_at_c")
        if real and r["kernel"] == HUBER and s == math.nextafter(cc, INF):
            c.add("s_ulp_above_c")
        if real and s < 0:
            c.add("s_negative")
        if real and s == INF:
            c.add("s_inf")
        if real and s != s:
            c.add("s_nan")
    if tr["flags"] & pg.RELAX_NOT_FINITE:
        c.add("not_finite")
    if real and "rejected" in tr["steps"]:
        c.add("rejected_step")
    closures = [e for e in range(tr["E"]) if int(edges["flags"][e]) & pg.EDGE_CLOSURE]
    live = [e for e in closures if tr["scope"][e]]
    if real and live and all(tr["w_fin"][e] < 1.0 for e in live):
        c.add("every_closure_downweighted")
    if real and not closures and tr["E"]:
        c.add("no_closure")
    if real and any(tr["why"][e] == "disabled" for e in closures):
        c.add("disabled_closure")
    if real and tr["E"] in (1023, 1024, 1025):
        c.add("e_%d" % tr["E"])
    down = [e for e, w in tr["w_fin"].items() if w < 1.0]
    if real and any(e >= pg.SHAPE for e in down) and any(e < pg.SHAPE for e in down):
        c.add("downweighted_beyond_stride")
    if case["par"]["iters"] == 0:
        c.add("iters_0")
    if sum(1 for w in tr["w_fin"].values() if w != w) >= 2:
        c.add("nan_on_two_edges")
    return c


_relax_results = {}


def run_relax_case(case):
    """(nodes, edges, report, robust report, trace) of a campaign case, computed once and shared."""
    if case["name"] not in _relax_results:
        tr = {}
        _relax_results[case["name"]] = relax_robust(case["nodes"], case["edges"], case["par"], case["rob"], tr) + (tr,)
    return _relax_results[case["name"]]


# ---- the prune campaign ----------------------------------------------------------------------------------------------------------------
def pcase(name, rng, rows, gate=GATE, max_reject=8, cap_extra=3, n_edges=None):
    """rows: (flags, chi2) of the edges in front; behind them cap_extra records of noise.  n_edges: what the head says (default: len(rows))."""
    cap = max(len(rows) + cap_extra, 1)
    edges = rng.integers(0, 256, cap * 96, dtype=np.uint8).view(pg.EDGE_DTYPE).copy()
    for k, (fl, chi) in enumerate(rows):
        edges["flags"][k], edges["chi2"][k] = fl, chi
    return dict(name=name, edges=edges, n_edges=len(rows) if n_edges is None else n_edges, gate=float(gate), max_reject=int(max_reject))


def nan_bits(bits):
    return float(np.array([bits], np.uint64).view(np.float64)[0])


def prune_campaign():
    rng = np.random.default_rng(20261022)
    CL, ODO, DIS = pg.EDGE_CLOSURE, 0, pg.EDGE_DISABLED
    out = []

    def filler(n):
        """n edges that are no candidates: odometry edges of any chi2, closures within the gate, disabled closures beyond it."""
        kinds = ((ODO, 1e9), (CL, 2.5), (CL | DIS, 500.0), (ODO | 8, 0.5), (CL | 16, 0.0))
        return [kinds[int(k)] for k in rng.integers(0, len(kinds), n)]
    for rep in range(3):
        out.append(pcase("no_candidate_%d" % rep, rng, filler(6 + rep) + [(CL, GATE), (CL, 11.0 - rep)]))
        out.append(pcase("more_than_max_reject_%d" % rep, rng, filler(4) + [(CL, 20.0 + 3 * k) for k in range(5 + rep)] + filler(3), max_reject=2 + rep))
        out.append(pcase("equal_chi2_%d" % rep, rng, [(CL, 50.0), (ODO, 1e6), (CL, 70.0), (CL, 50.0), (CL, 70.0), (CL, 70.0)] + filler(rep), max_reject=2 + rep))
        out.append(pcase("at_gate_%d" % rep, rng, [(CL, 4.0 + rep), (CL, math.nextafter(4.0 + rep, INF)), (CL, math.nextafter(4.0 + rep, -INF))] + filler(5),
                         gate=4.0 + rep))
        nans = (NAN, nan_bits(0xFFF8000000000000), nan_bits(0x7FF8000000012345))[rep]
        out.append(pcase("nan_and_inf_%d" % rep, rng, filler(2) + [(CL, 1e300), (CL, INF), (CL, nans), (CL, INF), (CL, -INF), (CL, -nans)][rep:] + filler(2),
                         max_reject=3))
        out.append(pcase("ignored_%d" % rep, rng, [(ODO, INF), (CL | DIS, NAN), (CL | DIS | EDGE_REJECTED, 1e5), (ODO, 99.0 + rep), (CL, 12.0), (ODO | DIS, 1e4)],
                         max_reject=4))
        out.append(pcase("e_0_%d" % rep, rng, [], cap_extra=1 + 2 * rep, max_reject=rep))
        for e_count in (255, 256, 257, 1025):                                # the lanes' stride: candidates in the last places
            rows = filler(e_count)
            for k in (0, 1 + rep, e_count - 2, e_count - 1):
                rows[k] = (CL, 30.0 + (k % 7))
            out.append(pcase("e_%d_%d" % (e_count, rep), rng, rows, max_reject=3))
        rows = filler(90)
        for k in rng.choice(90, 70, replace=False):
            rows[int(k)] = (CL, float(rng.integers(12, 40)))                  # many equal values among 70 candidates
        out.append(pcase("max_reject_64_%d" % rep, rng, rows, max_reject=64))
        out.append(pcase("max_reject_0_%d" % rep, rng, filler(5) + [(CL, 13.0), (CL, 90.0 + rep), (CL, NAN)][:2 + (rep > 0)], max_reject=0))
        rows = filler(3) + [(CL, 44.0), (CL, 45.0 + rep)]
        out.append(pcase("n_edges_above_%d" % rep, rng, rows, cap_extra=0, n_edges=len(rows) + 1 + 1000 * rep))
        out.append(pcase("n_edges_below_%d" % rep, rng, rows, n_edges=-1 - 1000 * rep))
    return out


PRUNE_CLASSES = ("no_candidate", "more_than_max_reject", "equal_chi2_by_index", "at_gate_kept", "ulp_above_gate", "nan_candidate", "inf_candidate",
                 "nan_ties_inf", "negative_nan", "disabled_closure_ignored", "odometry_ignored", "e_0", "e_255", "e_256", "e_257", "e_1025",
                 "max_reject_0", "max_reject_64", "n_edges_above", "n_edges_below", "noise_behind", "noise_is_candidate_like", "all_rejected")


def prune_classes_of(case, tr):
    ed, E, gate = case["edges"], tr["E"], case["gate"]
    fl, chi = ed["flags"].astype(np.int64), ed["chi2"]
    c = set()
    if not tr["cand"] and E:
        c.add("no_candidate")
    if len(tr["cand"]) > case["max_reject"] > 0:
        c.add("more_than_max_reject")
    for a, b in zip(tr["order"], tr["order"][1:]):                           # a tie that the cut of max_reject or the worst edge tells apart
        if chi[a] == chi[b] and (b not in tr["hit"] or a == tr["order"][0]):
            c.add("equal_chi2_by_index")
    closures = [e for e in range(E) if fl[e] & pg.EDGE_CLOSURE and not fl[e] & pg.EDGE_DISABLED]
    if any(chi[e] == gate for e in closures):
        c.add("at_gate_kept")
    if any(chi[e] == math.nextafter(gate, INF) for e in tr["cand"]):
        c.add("ulp_above_gate")
    nans, infs = [e for e in tr["cand"] if chi[e] != chi[e]], [e for e in tr["cand"] if chi[e] == INF]
    if nans:
        c.add("nan_candidate")
    if infs:
        c.add("inf_candidate")
    if nans and infs:                                                        # equal in the order: the index decides
        c.add("nan_ties_inf")
    if any(np.signbit(chi[e]) for e in nans):
        c.add("negative_nan")
    with np.errstate(all="ignore"):
        if any(fl[e] & pg.EDGE_CLOSURE and fl[e] & pg.EDGE_DISABLED and not chi[e] <= gate for e in range(E)):
            c.add("disabled_closure_ignored")
        if any(not fl[e] & pg.EDGE_CLOSURE and not fl[e] & pg.EDGE_DISABLED and not chi[e] <= gate for e in range(E)):
            c.add("odometry_ignored")
        if any(fl[e] & pg.EDGE_CLOSURE and not fl[e] & pg.EDGE_DISABLED and not chi[e] <= gate for e in range(E, tr["cap"])):
            c.add("noise_is_candidate_like")
    if E in (0, 255, 256, 257, 1025):
        c.add("e_%d" % E)
    if case["max_reject"] in (0, 64) and (tr["cand"] if case["max_reject"] == 0 else len(tr["cand"]) > 64):
        c.add("max_reject_%d" % case["max_reject"])
    if tr["n_edges"] > tr["cap"]:
        c.add("n_edges_above")
    if tr["n_edges"] < 0:
        c.add("n_edges_below")
    if tr["cap"] > E:
        c.add("noise_behind")
    if tr["cand"] and len(tr["hit"]) == len(tr["cand"]):
        c.add("all_rejected")
    return c


def run_prune_case(case):
    tr = {}
    return prune(case["n_edges"], case["edges"], case["gate"], case["max_reject"], tr) + (tr,)
