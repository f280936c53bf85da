"""Marginal covariances of a pose graph and the gate on new closures (include/lsd_hip.h: lsd_enqueue_pg_marginals_device,
lsd_enqueue_pg_vet_device; csrc/k_pgmarg.hip) restated on Python floats, in the header's order, written from the header
for the tests (not from the HIP code), and the generated campaigns both test files run.

The blocks of an edge, inv3, the one reduction shape, the canonical NaN, the chain edges, the positions, the factor and its apply are
pose_graph_cases', pose_graph_robust_cases' and pose_graph_chain_cases' own text; what is restated here is what the new entries add: the
cut of the edges at the prior's count, the matrix at lambda = 0.0, the three kinds of query and their right-hand sides, the three solves
and their ends, the record, the report -- and the gate's seven tests.  A case class is a predicate on the restatement's own TRACE, never
on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
import pose_graph_cases as pg
import pose_graph_chain_cases as cc
import pose_graph_robust_cases as rc

QUERY_DTYPE = np.dtype([("kind", "i4"), ("a", "i4"), ("b", "i4"), ("reserved", "i4")])
REC_DTYPE = np.dtype([("cov", "f8", (9,)), ("steps", "i4", (3,)), ("flags", "u4"), ("kind", "i4"), ("edge", "i4"), ("i", "i4"), ("j", "i4")])
REP_DTYPE = np.dtype([("n_nodes", "i4"), ("n_edges", "i4"), ("skipped_edges", "i4"), ("singular_nodes", "i4"), ("chain_edges", "i4"),
                      ("paths", "i4"), ("longest_path", "i4"), ("fallbacks", "i4")])
VET_REP_DTYPE = np.dtype([("d2", "f8"), ("det", "f8"), ("edge", "i4"), ("flags", "u4")])
SIZES = {"lsd_pg_marg_query": 16, "lsd_pg_marg_par": 24, "lsd_pg_marg_rec": 104, "lsd_pg_marg_rep": 32, "lsd_pg_vet_rep": 24}
NODE, PAIR, NEW_EDGE = 0, 1, 2
CONVERGED_0, MAXED_0, BREAKDOWN_0, CONVERGED = 0x1, 0x10, 0x100, 0x7
FIXED, SINGULAR, BAD_QUERY, NO_EDGE = 0x1000, 0x2000, 0x4000, 0x8000
VET_UNUSED, VET_NO_EDGE, VET_SKIPPED, VET_NO_MARGINAL, VET_SINGULAR, VET_REJECTED, VET_PASSED = 1, 2, 4, 8, 16, 32, 64
VET_NAMES = {VET_UNUSED: "unused", VET_NO_EDGE: "no_edge", VET_SKIPPED: "skipped", VET_NO_MARGINAL: "no_marginal", VET_SINGULAR: "singular",
             VET_REJECTED: "rejected", VET_PASSED: "passed"}
BLOCK, CHAIN = cc.BLOCK, cc.CHAIN
MARG_DEFAULTS = dict(cg_tol=1e-8, cg_iters=200, precond=CHAIN, slots=256)
GATE_999 = 16.27                                                             # the 0.999 quantile of chi-square with 3 degrees of freedom
INT_MAX = 2 ** 31 - 1


def queries(*rows):
    q = np.zeros(len(rows), QUERY_DTYPE)
    for k, r in enumerate(rows):
        q[k]["kind"], q[k]["a"], q[k]["b"] = r
    return q


def skipped_why(e, N, P):
    """Why the relaxation skips an edge, or None."""
    i, j = int(e["i"]), int(e["j"])
    if int(e["flags"]) & pg.EDGE_DISABLED:
        return "disabled"
    if i == j:
        return "self"
    if not (0 <= i < N and 0 <= j < N):
        return "range"
    if not all(math.isfinite(float(v)) for v in list(e["z"]) + list(e["info"]) + list(P[i]) + list(P[j])):
        return "not_finite"
    return None


def jacobians(pa, pb):
    """A and B (rows) of the relaxation's rule for an edge (i = a, j = b) at the poses pa, pb."""
    _, s, c, dx, dy = pg.edge_error(pa, pb, (0.0, 0.0, 0.0))
    k = gc.K_PI / 180.0
    return ([[-c, -s, k * (c * dy - s * dx)], [s, -c, k * ((-c) * dx - s * dy)], [0.0, 0.0, -1.0]],
            [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
def matrix(nodes, edges, kind, tr):
    """The shared part: what the first launch leaves.  edges: the E_h edges of the matrix."""
    N, E = len(nodes), len(edges)
    lam = 0.0
    P = [pg.pose_of(n) for n in nodes]
    fixed = [bool(int(n["flags"]) & pg.NODE_FIXED) for n in nodes]
    why = [skipped_why(e, N, P) for e in edges]
    valid = [w is None for w in why]
    ei, ej = [int(e["i"]) for e in edges], [int(e["j"]) for e in edges]
    lists = [[] for _ in range(N)]
    blk = [None] * E
    for e in range(E):
        if valid[e]:
            lists[ei[e]].append((e, 0))
            lists[ej[e]].append((e, 1))
            W = pg.info_rows([float(v) for v in edges[e]["info"]])
            blk[e] = pg.edge_blocks(P[ei[e]], P[ej[e]], [float(v) for v in edges[e]["z"]], W)[:3]
    H, M, D, singular = [None] * N, [None] * N, [None] * N, [False] * N
    for n in range(N):
        Hn = [[0.0] * 3 for _ in range(3)]
        for e, side in lists[n]:
            src = blk[e][2 if side else 0]
            for r in range(3):
                for q in range(3):
                    Hn[r][q] += src[r][q]
        H[n] = Hn
        if not fixed[n]:
            D[n] = [[Hn[r][q] if r != q else Hn[r][r] + lam * Hn[r][r] for q in range(3)] for r in range(3)]
            M[n], _ = pg.inv3(D[n])
            singular[n] = M[n] is None
    free = [not fixed[n] and not singular[n] for n in range(N)]
    rep = np.zeros(1, REP_DTYPE)[0]
    rep["n_nodes"], rep["n_edges"], rep["skipped_edges"], rep["singular_nodes"] = N, E, sum(1 for v in valid if not v), sum(singular)
    Fc, node_at = None, None
    if kind == CHAIN:
        chain, up_edge, before, _, _, _, lo, hi = cc.chain_of(N, edges, valid)
        node_at, paths = cc.positions(N, up_edge, before, hi)
        rep["chain_edges"], rep["paths"], rep["longest_path"] = sum(chain), len(paths), max([len(p) for p in paths] + [0])
        Dg = [D[n] if free[n] else cc.IDENTITY for n in node_at]
        Cs = []
        for t in range(N - 1):
            n, m = node_at[t], node_at[t + 1]
            e = up_edge[n]
            if e >= 0 and hi[e] == m and free[n] and free[m]:
                hab = blk[e][1]
                Cs.append(hab if ei[e] == n else [[hab[q][r] for q in range(3)] for r in range(3)])
            else:
                Cs.append([[0.0] * 3 for _ in range(3)])
        Fc = cc.factor(Dg, Cs)
        rep["fallbacks"] = 1 if Fc is None else 0
        tr["pure_chain"] = all(valid[e] and chain[e] for e in range(E)) and E > 0
    tr.update(N=N, E_h=E, why=why, fixed=fixed, singular=singular, degrees=[len(l) for l in lists], fallback=kind == CHAIN and Fc is None, kind=kind)
    return dict(N=N, P=P, fixed=fixed, singular=singular, free=free, lists=lists, blk=blk, H=H, M=M, ei=ei, ej=ej, Fc=Fc, node_at=node_at, lam=lam), rep


def precond(G, r_):
    N, free, zero = G["N"], G["free"], [0.0, 0.0, 0.0]
    if G["Fc"] is None:
        return [[pg.dot3(G["M"][n][q], r_[n]) for q in range(3)] if free[n] else list(zero) for n in range(N)]
    x = cc.apply(G["Fc"], [r_[n] for n in G["node_at"]])
    z_ = [None] * N
    for t, n in enumerate(G["node_at"]):
        z_[n] = x[t] if free[n] else list(zero)
    return z_


def column(G, u, cg_tol, cg_iters):
    """PCG on H x = u: (x, steps, the end: "tol", "start", "iters" or "breakdown")."""
    N, free, H, lam, lists, blk, ei, ej = G["N"], G["free"], G["H"], G["lam"], G["lists"], G["blk"], G["ei"], G["ej"]
    zero = [0.0, 0.0, 0.0]
    x = [list(zero) for _ in range(N)]
    r_ = [list(u[n]) if free[n] else list(zero) for n in range(N)]
    z_ = precond(G, r_)
    p_ = [list(v) for v in z_]
    rz = pg.reduce_shape([pg.dot3(r_[n], z_[n]) for n in range(N)])
    thr = (cg_tol * cg_tol) * rz
    steps = 0
    while True:
        if not steps < cg_iters:
            return x, steps, ("tol" if steps else "start") if rz <= thr else "iters"
        if rz <= thr:
            return x, steps, "tol" if steps else "start"
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
            return x, steps, "breakdown"
        alpha = pg.fdiv(rz, pq)
        for n in range(N):
            if free[n]:
                for c in range(3):
                    x[n][c] = x[n][c] + alpha * p_[n][c]
                    r_[n][c] = r_[n][c] - alpha * q_[n][c]
        z_ = precond(G, r_)
        rzn = pg.reduce_shape([pg.dot3(r_[n], z_[n]) for n in range(N)])
        beta = pg.fdiv(rzn, rz)
        for n in range(N):
            if free[n]:
                for c in range(3):
                    p_[n][c] = z_[n][c] + beta * p_[n][c]
        rz = rzn
        steps += 1


# ---- a query ---------------------------------------------------------------------------------------------------------------------------
def record(G, edges, E, prior_clamped, query, par, qtr):
    rec = np.zeros(1, REC_DTYPE)[0]
    kind, a, b = int(query["kind"]), int(query["a"]), int(query["b"])
    N = G["N"]
    flags, edge = 0, -1
    pair = kind != NODE
    if kind == NEW_EDGE:
        k, a, b = a, -1, -1
        if prior_clamped is None or k < 0:
            flags |= BAD_QUERY
        else:
            e = prior_clamped + k
            edge = min(e, INT_MAX)
            if e >= E:
                flags |= NO_EDGE
            else:
                a, b = int(edges[e]["i"]), int(edges[e]["j"])
    elif kind not in (NODE, PAIR):
        flags |= BAD_QUERY
    if not flags and (not 0 <= a < N or (pair and (not 0 <= b < N or a == b))):
        flags |= BAD_QUERY
    if not flags:
        ends = [a, b] if pair else [a]
        if any(G["fixed"][n] for n in ends):
            flags |= FIXED
        if any(G["singular"][n] for n in ends):
            flags |= SINGULAR
    solve = not flags & (BAD_QUERY | NO_EDGE) and (pair or not flags)
    cov = [0.0] * 9
    steps, ends_ = [0, 0, 0], []
    if solve:
        A, B = cc.IDENTITY, None
        if pair:
            A, B = jacobians(G["P"][a], G["P"][b])
        for c in range(3):
            u = [[0.0, 0.0, 0.0] for _ in range(N)]
            u[a] = list(A[c])
            if pair:
                u[b] = list(B[c])
            x, steps[c], end = column(G, u, par["cg_tol"], par["cg_iters"])
            ends_.append(end)
            flags |= {"tol": CONVERGED_0, "start": CONVERGED_0, "iters": MAXED_0, "breakdown": BREAKDOWN_0}[end] << c
            for r in range(3):
                v = pg.dot3(A[r], x[a])
                if pair:
                    v = v + pg.dot3(B[r], x[b])
                cov[3 * r + c] = v
    rec["cov"], rec["steps"], rec["flags"] = [rc.canon(v) for v in cov], steps, flags
    rec["kind"], rec["edge"], rec["i"], rec["j"] = kind, edge, a, b
    qtr.append(dict(kind=kind, flags=flags, ends=ends_, steps=steps, a=a, b=b, edge=edge, solved=solve))
    return rec


def marginals(nodes, edges, qu, par, prior=None, edges_cap=None, trace=None):
    """lsd_enqueue_pg_marginals_device on one graph: nodes [N], edges [E] (the clamped counts), prior: None or the prior head's n_edges as
    it stands (clamped here to edges_cap, default E) -> (records [n_q], the report)."""
    tr = trace if trace is not None else {}
    with np.errstate(all="ignore"):
        E = len(edges)
        cap = E if edges_cap is None else int(edges_cap)
        pc = None if prior is None else min(max(int(prior), 0), cap)
        E_h = E if pc is None else min(E, pc)
        G, rep = matrix(nodes, edges[:E_h], int(par["precond"]), tr)
        tr["queries"] = []
        recs = np.zeros(len(qu), REC_DTYPE)
        for k in range(len(qu)):
            recs[k] = record(G, edges, E, pc, qu[k], par, tr["queries"])
        tr.update(E=E, prior_clamped=pc, prior=prior)
        return recs, rep


# ---- the gate --------------------------------------------------------------------------------------------------------------------------
def vet(nodes, edges, qu, recs, gate, trace=None):
    """lsd_enqueue_pg_vet_device: (edges after, reports [n_q])."""
    tr = trace if trace is not None else {}
    out_e = edges.copy()
    N, E = len(nodes), len(edges)
    P = [pg.pose_of(n) for n in nodes]
    reps = np.zeros(len(qu), VET_REP_DTYPE)
    tr["outcomes"] = []
    with np.errstate(all="ignore"):
        for k in range(len(qu)):
            rec = recs[k]
            d2, det, e, out = 0.0, 0.0, -1, 0
            if int(qu[k]["kind"]) != NEW_EDGE:
                out = VET_UNUSED
            elif int(rec["flags"]) & (NO_EDGE | BAD_QUERY) or not 0 <= int(rec["edge"]) < E:
                out = VET_NO_EDGE
            else:
                e = int(rec["edge"])
                ed = edges[e]
                if not int(ed["flags"]) & pg.EDGE_CLOSURE or skipped_why(ed, N, P) is not None:
                    out = VET_SKIPPED
                elif int(rec["flags"]) & CONVERGED != CONVERGED:
                    out = VET_NO_MARGINAL
                else:
                    W = pg.info_rows([float(v) for v in ed["info"]])
                    R, det = pg.inv3(W)
                    if R is None:
                        out = VET_SINGULAR
                    else:
                        S = [[float(rec["cov"][3 * r + q]) + R[r][q] for q in range(3)] for r in range(3)]
                        Si, det = pg.inv3(S)
                        if Si is None:
                            out = VET_SINGULAR
                        else:
                            er = pg.edge_error(P[int(ed["i"])], P[int(ed["j"])], [float(v) for v in ed["z"]])[0]
                            t = [pg.dot3(Si[r], er) for r in range(3)]
                            d2 = pg.dot3(er, t)
                            out = VET_REJECTED if not d2 <= gate else VET_PASSED
            if out == VET_REJECTED:
                out_e[e]["flags"] = int(out_e[e]["flags"]) | pg.EDGE_DISABLED | rc.EDGE_REJECTED
            reps[k]["d2"], reps[k]["det"], reps[k]["edge"], reps[k]["flags"] = rc.canon(d2), rc.canon(det), e, out
            tr["outcomes"].append(VET_NAMES[out])
    return out_e, reps


def new_edge_queries(n):
    return queries(*[(NEW_EDGE, k, 0) for k in range(n)])


def vetted_closures(nodes, edges, prior, n_new, vet_par, edges_cap=None):
    """What follows the closures in PoseGraph.close_*_device(.., vet=): the marginals of the NEW_EDGE queries k = 0 .. n_new - 1 on the
    graph as the prior saw it, then the gate.  -> (edges after, records, the report, the vet's reports)."""
    qu = new_edge_queries(n_new)
    par = dict(MARG_DEFAULTS, **(vet_par.get("marg") or {}))
    par["slots"] = max(1, min(par["slots"], n_new))
    recs, rep = marginals(nodes, edges, qu, par, prior, edges_cap)
    out_e, vreps = vet(nodes, edges, qu, recs, vet_par["gate"])
    return out_e, recs, rep, vreps


# ---- the dense reference (numpy, for the accuracy test) ----------------------------------------------------------------------------------
def dense_inverse(nodes, edges):
    """(inv(H) over all nodes with zero rows and columns at the nodes that are not free, free[n]) by numpy.linalg.inv."""
    G, _ = matrix(nodes, edges, BLOCK, {})
    N = G["N"]
    Hd = np.zeros((3 * N, 3 * N))
    for n in range(N):
        Hd[3 * n:3 * n + 3, 3 * n:3 * n + 3] = G["H"][n]
    for e, b in enumerate(G["blk"]):
        if b is not None:
            i, j = G["ei"][e], G["ej"][e]
            Hd[3 * i:3 * i + 3, 3 * j:3 * j + 3] += np.array(b[1])
            Hd[3 * j:3 * j + 3, 3 * i:3 * i + 3] += np.array(b[1]).T
    idx = np.array([3 * n + q for n in range(N) if G["free"][n] for q in range(3)], dtype=int)
    full = np.zeros((3 * N, 3 * N))
    full[np.ix_(idx, idx)] = np.linalg.inv(Hd[np.ix_(idx, idx)])
    return full, G


def dense_cov(full, G, kind, a, b):
    if kind == NODE:
        return full[3 * a:3 * a + 3, 3 * a:3 * a + 3]
    A, B = jacobians(G["P"][a], G["P"][b])
    J = np.zeros((3, full.shape[0]))
    J[:, 3 * a:3 * a + 3], J[:, 3 * b:3 * b + 3] = A, B
    return J @ full @ J.T


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
def mcase(name, nodes, edges, qu, prior=None, cap_extra=3, **par):
    p = dict(MARG_DEFAULTS)
    p.update(par)
    edges = np.array(edges, pg.EDGE_DTYPE).reshape(-1)
    return dict(name=name, nodes=np.array(nodes, pg.NODE_DTYPE).reshape(-1), edges=edges, queries=qu, prior=prior, edges_cap=max(len(edges), 1) + cap_extra,
                par=p)


SIZES_3 = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025)
# Seeds found by running the restatement over a range of them and keeping those whose TRACE shows the class (the device was not asked):
# a chain without a fixed node has a singular M, and whether its last pivot comes out > 0 is rounding's doing.
FALLBACK_SEEDS = tuple(range(12))
INDEFINITE_SCALES = (0.5, 1.0, 2.0)


def closure_between(nodes, i, j, info=rc.CLOSURE_INFO, flags=pg.EDGE_CLOSURE, off=(0.0, 0.0, 0.0)):
    z = pg.rel(pg.pose_of(nodes[i]), pg.pose_of(nodes[j]))
    return pg.edge(i, j, (z[0] + off[0], z[1] + off[1], z[2] + off[2]), info, flags)


def campaign():
    rng = np.random.default_rng(20261021)
    out = []
    for n in SIZES_3:                                                        # the sizes: the lane count's and the reduction shape's edges
        for rep in range(3):
            nodes, edges = pg.chain_graph(n, rng, extra=rep if n >= 8 else 0)
            kind = BLOCK if rep == 1 else CHAIN
            iters = 12 if n < 255 else (6 if n < 1023 else (3 if kind == BLOCK else 5))
            rows = [(NODE, 0, 0), (NODE, n - 1, 0), (NODE, n // 2, 0), (NODE, n, 0)] + ([(PAIR, 0, n - 1), (PAIR, n - 1, n // 2)] if n >= 3 else [])
            out.append(mcase("n_%d_%d" % (n, rep), nodes, edges, queries(*rows[:4 if n >= 1023 else 6]), precond=kind, cg_iters=iters, slots=1 + rep))
    for rep in range(3):
        nodes, edges = pg.chain_graph(3 + rep, rng)                          # E = 0: every node without an edge
        out.append(mcase("e_0_%d" % rep, nodes, edges[:0], queries((NODE, 0, 0), (NODE, 1, 0), (PAIR, 1, 2)), precond=rep % 2))
        # the nodes' classes on a loop with two closures
        nodes, edges, _ = pg.loop_graph(12 + rep, rng, closures=2, noisy=True)
        N = len(nodes)
        both = []
        for kind, kname in ((BLOCK, "block"), (CHAIN, "chain")):             # BLOCK and CHAIN on one graph, ended by cg_tol
            c = mcase("nodes_%s_%d" % (kname, rep), nodes, edges,
                      queries((NODE, 0, 0), (NODE, 5, 0), (NODE, N, 0), (NODE, -1, 0), (PAIR, 3, 3), (PAIR, 7, 2), (PAIR, 0, 6), (PAIR, 6, 0), (PAIR, 2, N),
                              (7, 1, 2), (NEW_EDGE, 0, 0)), precond=kind, cg_iters=200, cg_tol=1e-9, slots=4)
            both.append(c)
            out.append(c)
        two = nodes.copy()
        two["flags"][4 + rep] |= pg.NODE_FIXED
        out.append(mcase("both_fixed_%d" % rep, two, edges, queries((PAIR, 0, 4 + rep), (PAIR, 4 + rep, 0), (PAIR, 4 + rep, 9), (NODE, 4 + rep, 0)), cg_iters=60))
        allf, nonef = nodes.copy(), nodes.copy()
        allf["flags"] |= pg.NODE_FIXED
        nonef["flags"] &= ~np.uint32(pg.NODE_FIXED)
        out.append(mcase("all_fixed_%d" % rep, allf, edges, queries((NODE, 1, 0), (PAIR, 1, 5)), precond=rep % 2))
        out.append(mcase("none_fixed_%d" % rep, nonef, edges, queries((NODE, 1, 0), (PAIR, 1, 5)), precond=rep % 2, cg_iters=30))
        lone = np.concatenate([nodes[:4], np.array([pg.node(1.0, 2.0, 3.0)], pg.NODE_DTYPE), nodes[4:]])   # node 4 has no edge
        ed = edges.copy()
        ed["i"] += ed["i"] >= 4
        ed["j"] += ed["j"] >= 4
        out.append(mcase("degree_0_%d" % rep, lone, ed, queries((NODE, 4, 0), (PAIR, 4, 6), (PAIR, 2, 4), (NODE, 6, 0)), precond=rep % 2, cg_iters=80))
        # two tracks interleaved: the second floats (no fixed node, no closure to the first), then a closure joins them
        tn, te = cc.interleaved(2, 7 + rep, rng)
        tn["flags"][1] &= ~np.uint32(pg.NODE_FIXED)
        for kind, kname in ((BLOCK, "block"), (CHAIN, "chain")):
            out.append(mcase("floating_%s_%d" % (kname, rep), tn, te, queries((NODE, 3, 0), (NODE, 2, 0), (PAIR, 3, 7), (PAIR, 2, 3)), precond=kind,
                             cg_iters=40))
        joined = np.concatenate([te, np.array([closure_between(tn, 4, 9)], pg.EDGE_DTYPE)])
        out.append(mcase("joined_%d" % rep, tn, joined, queries((PAIR, 2, 5), (PAIR, 11, 0), (NODE, 3, 0)), cg_iters=200))
        # NEW_EDGE: a loop whose last two edges are closures appended behind the prior
        nodes, edges, _ = pg.loop_graph(14 + rep, rng, closures=2)
        E = len(edges)
        ks = queries(*[(NEW_EDGE, k, 0) for k in (0, 1, 2, 3, -1)])
        out.append(mcase("new_edges_%d" % rep, nodes, edges, ks, prior=E - 2, precond=rep % 2))
        out.append(mcase("no_prior_%d" % rep, nodes, edges, ks[:2]))
        out.append(mcase("prior_is_head_%d" % rep, nodes, edges, ks[:2], prior=E))
        out.append(mcase("prior_above_%d" % rep, nodes, edges, ks[:2], prior=E + 5 + rep, cap_extra=2))
        out.append(mcase("prior_below_0_%d" % rep, nodes, edges, ks[:2], prior=-3 - rep))
        odo = np.concatenate([edges, np.array([pg.edge(3, 9, pg.rel(pg.pose_of(nodes[3]), pg.pose_of(nodes[9])))], pg.EDGE_DTYPE)])
        out.append(mcase("new_odometry_%d" % rep, nodes, odo, ks[:2], prior=E))
        dis = np.concatenate([edges, np.array([closure_between(nodes, 2, 8, flags=pg.EDGE_CLOSURE | pg.EDGE_DISABLED), closure_between(nodes, 5, 5)],
                                              pg.EDGE_DTYPE)])
        out.append(mcase("new_disabled_and_self_%d" % rep, nodes, dis, ks[:3], prior=E))
        # the solves' ends
        nodes4, edges4, _ = pg.loop_graph(40 + rep, rng, closures=4)
        qs = queries((NODE, 20, 0), (PAIR, 3, 30))
        out.append(mcase("cg_tol_end_%d" % rep, nodes4, edges4, qs, precond=BLOCK, cg_iters=400, cg_tol=1e-3))
        out.append(mcase("cg_iters_end_%d" % rep, nodes4, edges4, qs, precond=rep % 2, cg_iters=2, cg_tol=1e-12))
        out.append(mcase("cg_iters_0_%d" % rep, nodes4, edges4, qs, precond=rep % 2, cg_iters=0))
        # slots: 1, 2, n_q - 1, n_q, above n_q on one graph and one list of queries
        q7 = queries(*[(NODE, 1 + k, 0) for k in range(5)] + [(PAIR, 2, 9), (PAIR, 12, 1)])
        for slots in (1, 2, 6, 7, 9 + rep):
            out.append(mcase("slots_%d_%d" % (slots, rep), nodes, edges, q7, slots=slots, cg_iters=100))
    for k, scale in enumerate(INDEFINITE_SCALES):                            # an indefinite information on a closure: p^T H p <= 0 is met
        nodes, edges, _ = pg.loop_graph(10, np.random.default_rng(9100 + k), closures=1)
        neg = edges.copy()
        neg["info"][-1] = (-scale * 4.0, 0.0, -scale * 4.0, 0.0, 0.0, -scale)
        for kind, kname in ((BLOCK, "block"), (CHAIN, "chain")):
            out.append(mcase("indefinite_%s_%d" % (kname, k), nodes, neg, queries((NODE, 4, 0), (PAIR, 0, 9), (PAIR, 2, 7)), precond=kind, cg_iters=60))
    for seed in FALLBACK_SEEDS:                                              # no fixed node, no closure: M is the matrix and singular
        r2 = np.random.default_rng(9200 + seed)
        nodes, edges = pg.chain_graph(5 + seed % 4, r2)
        nodes["flags"] &= ~np.uint32(pg.NODE_FIXED)
        out.append(mcase("fallback_%d" % seed, nodes, edges, queries((NODE, 2, 0), (PAIR, 0, 3)), cg_iters=20))
    return out


CLASSES = (["n_%d" % n for n in SIZES_3] +
           ["e_0", "query_fixed", "query_singular_degree_0", "query_outside", "floating", "all_fixed", "none_fixed", "pair_a_is_b", "pair_descending",
            "pair_one_fixed", "pair_both_fixed", "pair_across_tracks", "bad_kind", "new_edge_on", "new_edge_last", "new_edge_beyond", "new_edge_negative",
            "new_edge_without_prior", "prior_is_head", "prior_above_head", "prior_below_0", "new_odometry", "new_disabled", "new_self", "cg_end_tol",
            "cg_end_iters", "cg_end_breakdown", "cg_iters_0", "fallback", "block", "chain", "slots_1", "slots_2", "slots_n_q_minus_1", "slots_n_q",
            "slots_above_n_q"])


def classes_of(case, tr):
    c = set()
    N, qs, par = tr["N"], tr["queries"], case["par"]
    E, pc = tr["E"], tr["prior_clamped"]
    if N in SIZES_3 and case["name"].startswith("n_"):
        c.add("n_%d" % N)
    if tr["E_h"] == 0 and N >= 2 and case["prior"] is None:
        c.add("e_0")
    if N and all(tr["fixed"]):
        c.add("all_fixed")
    if N and not any(tr["fixed"]):
        c.add("none_fixed")
    if any(q["solved"] for q in qs):
        c.add("chain" if tr["kind"] == CHAIN else "block")
    if tr["fallback"] and any(q["solved"] for q in qs):
        c.add("fallback")
    n_q = len(qs)
    for name, hit in (("slots_1", par["slots"] == 1), ("slots_2", par["slots"] == 2), ("slots_n_q_minus_1", par["slots"] == n_q - 1),
                      ("slots_n_q", par["slots"] == n_q), ("slots_above_n_q", par["slots"] > n_q)):
        if hit and n_q >= 4 and case["name"].startswith("slots_"):
            c.add(name)
    for q, given in zip(qs, case["queries"]):
        kind, fl = q["kind"], q["flags"]
        if kind == NODE and fl == FIXED:
            c.add("query_fixed")
        if kind == NODE and fl == SINGULAR and tr["degrees"][q["a"]] == 0:
            c.add("query_singular_degree_0")
        if kind == NODE and fl == BAD_QUERY:
            c.add("query_outside")
        if kind not in (NODE, PAIR, NEW_EDGE) and fl == BAD_QUERY:
            c.add("bad_kind")
        if kind == PAIR:
            if q["a"] == q["b"] and fl == BAD_QUERY:
                c.add("pair_a_is_b")
            if q["solved"] and q["a"] > q["b"]:
                c.add("pair_descending")
            if q["solved"] and 0 <= q["a"] < N and 0 <= q["b"] < N:
                fa, fb = tr["fixed"][q["a"]], tr["fixed"][q["b"]]
                if fa != fb and not all(tr["fixed"]):
                    c.add("pair_one_fixed")
                if fa and fb and not all(tr["fixed"]) and q["steps"] == [0, 0, 0] and fl & CONVERGED == CONVERGED:
                    c.add("pair_both_fixed")
                if case["name"].startswith("joined_") and (q["a"] - q["b"]) % 2 and fl & CONVERGED == CONVERGED:
                    c.add("pair_across_tracks")
        if case["name"].startswith("floating_") and q["solved"] and q["a"] % 2 == 1 and kind == NODE:
            c.add("floating_converged" if fl & CONVERGED == CONVERGED else "floating")
        if kind == NEW_EDGE:
            k = int(given["a"])
            n_new = E - pc if pc is not None else 0
            if pc is None:
                c.add("new_edge_without_prior")
            elif k < 0:
                c.add("new_edge_negative")
            elif n_new >= 2 and k == n_new - 1 and not fl & NO_EDGE:
                c.add("new_edge_last")
            elif n_new >= 2 and k == n_new and fl == NO_EDGE:
                c.add("new_edge_on")                                         # (on the head's count: the first index that names no edge)
            elif n_new >= 2 and k == n_new + 1 and fl == NO_EDGE:
                c.add("new_edge_beyond")
            if pc is not None and case["prior"] is not None:
                if case["prior"] == E and fl == NO_EDGE:
                    c.add("prior_is_head")
                if case["prior"] > E and fl == NO_EDGE:
                    c.add("prior_above_head")
                if case["prior"] < 0 and pc == 0 and k == 0:
                    c.add("prior_below_0")
            if q["edge"] >= 0 and q["edge"] < E:
                ed = case["edges"][q["edge"]]
                if not int(ed["flags"]) & pg.EDGE_CLOSURE:
                    c.add("new_odometry")
                if int(ed["flags"]) & pg.EDGE_DISABLED:
                    c.add("new_disabled")
                if int(ed["i"]) == int(ed["j"]) and fl == BAD_QUERY:
                    c.add("new_self")
        for end, steps in zip(q["ends"], q["steps"]):
            if end == "tol" and steps:
                c.add("cg_end_tol")
            if end == "iters" and par["cg_iters"]:
                c.add("cg_end_iters")
            if end == "breakdown":
                c.add("cg_end_breakdown")
            if par["cg_iters"] == 0 and end == "iters":
                c.add("cg_iters_0")
    return c


_results = {}


def run_case(case):
    """(records, report, trace) of a campaign case, computed once and shared."""
    if case["name"] not in _results:
        tr = {}
        _results[case["name"]] = marginals(case["nodes"], case["edges"], case["queries"], case["par"], case["prior"], case["edges_cap"], tr) + (tr,)
    return _results[case["name"]]


# ---- the vet's campaign ----------------------------------------------------------------------------------------------------------------
def hand_record(edge, i, j, cov=None, flags=CONVERGED):
    rec = np.zeros(1, REC_DTYPE)[0]
    rec["cov"] = [0.0] * 9 if cov is None else cov
    rec["flags"], rec["kind"], rec["edge"], rec["i"], rec["j"] = flags, NEW_EDGE, edge, i, j
    return rec


def vcase(name, nodes, edges, qu, recs, gate):
    return dict(name=name, nodes=nodes, edges=np.array(edges, pg.EDGE_DTYPE).reshape(-1), queries=qu, recs=np.array(recs, REC_DTYPE).reshape(-1), gate=float(gate))


def vet_campaign():
    rng = np.random.default_rng(20261022)
    out = []
    for rep in range(3):
        nodes, edges, _ = pg.loop_graph(16 + rep, rng, closures=1)
        E0 = len(edges)
        true_c = [closure_between(nodes, 2 + rep, 9 + rep, off=(0.05, -0.03, 0.1))]
        false_c = [closure_between(nodes, 3, 12 + rep, off=(9.0, -7.0, 30.0))]
        odo = [pg.edge(4, 10, pg.rel(pg.pose_of(nodes[4]), pg.pose_of(nodes[10])))]
        dis = [closure_between(nodes, 1, 8, flags=pg.EDGE_CLOSURE | pg.EDGE_DISABLED | rc.EDGE_REJECTED)]
        selfe = [closure_between(nodes, 6, 6)]
        sing = [closure_between(nodes, 5, 11, info=(1.0, 1.0, 1.0, 0.0, 0.0, 1.0))]       # det(W) == 0
        nf = [closure_between(nodes, 7, 13)]
        nf[0]["z"][1] = pg.NAN
        new = true_c + false_c + odo + dis + selfe + sing + nf
        ed = np.concatenate([edges, np.array(new, pg.EDGE_DTYPE)])
        n_new = len(new)
        # every outcome from the marginals' own records: k over the new edges, one beyond, a second query on the false one, a NODE query
        rows = [(NEW_EDGE, k, 0) for k in range(n_new + 1)] + [(NEW_EDGE, 1, 0), (NODE, 4, 0), (PAIR, 2, 9)]
        qu = queries(*rows)
        par = dict(MARG_DEFAULTS, slots=3)
        recs, _ = marginals(nodes, ed, qu, par, E0, len(ed) + 3)
        out.append(vcase("outcomes_%d" % rep, nodes, ed, qu, recs, GATE_999))
        # the same with solves that are cut short: NO_MARGINAL where the covariance is not known, nothing rejected on that ground
        recs2, _ = marginals(nodes, ed, qu, dict(par, cg_iters=1, precond=BLOCK), E0, len(ed) + 3)
        out.append(vcase("cut_short_%d" % rep, nodes, ed, qu, recs2, GATE_999))
        # S singular: a covariance that cancels R
        W = pg.info_rows([float(v) for v in true_c[0]["info"]])
        R, _ = pg.inv3(W)
        neg = [-R[r][q] for r in range(3) for q in range(3)]
        e_t = E0
        q1 = queries((NEW_EDGE, 0, 0))
        out.append(vcase("s_singular_%d" % rep, nodes, ed, q1, [hand_record(e_t, int(ed[e_t]["i"]), int(ed[e_t]["j"]), neg)], GATE_999))
        # records that name no edge of the graph
        out.append(vcase("edge_outside_%d" % rep, nodes, ed, queries((NEW_EDGE, 0, 0), (NEW_EDGE, 1, 0)),
                         [hand_record(len(ed), 1, 2), hand_record(-1, 1, 2)], GATE_999))
        # d2 exactly at the gate and one ulp on either side of it: the gate is the restatement's own d2 of the true closure
        _, r0 = vet(nodes, ed, qu[:1], recs[:1], 1e300)
        d2 = float(r0[0]["d2"])
        for name, g in (("at", d2), ("ulp_below", float(np.nextafter(d2, 0.0))), ("ulp_above", float(np.nextafter(d2, math.inf)))):
            out.append(vcase("gate_%s_%d" % (name, rep), nodes, ed, qu[:1], recs[:1], g))
        # a NaN d2: poses far apart under an information with a negative off-diagonal -- inf - inf in t
        # (which of the signs makes the two infinities meet is the heading's doing: the first whose restated d2 is a NaN)
        big = ed.copy()
        big["info"][e_t] = (1e20, -0.5e20, 1e20, 0.0, 0.0, 1.0)
        hand = [hand_record(e_t, int(ed[e_t]["i"]), int(ed[e_t]["j"]))]
        for sx, sy in ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, 0.1), (0.1, 1.0)):
            far = nodes.copy()
            far["x"][9 + rep], far["y"][9 + rep] = sx * 1e300, sy * 1.5e300
            d2n = float(vet(far, big, q1, np.array(hand, REC_DTYPE), GATE_999)[1][0]["d2"])
            if d2n != d2n:
                break
        out.append(vcase("nan_d2_%d" % rep, far, big, q1, hand, GATE_999))
    return out


VET_CLASSES = (list(VET_NAMES.values()) + ["s_singular", "w_singular", "edge_outside", "at_gate_passed", "ulp_below_gate_rejected", "ulp_above_gate_passed",
                                            "nan_d2", "two_queries_one_edge", "skipped_odometry", "skipped_disabled", "skipped_not_finite", "no_edge_self"])


def vet_classes_of(case, tr, reps, edges_after):
    c = set(tr["outcomes"])
    E = len(case["edges"])
    seen = {}
    for k, name in enumerate(tr["outcomes"]):
        rec, rp = case["recs"][k], reps[k]
        e = int(rec["edge"])
        if name == "no_edge" and not 0 <= e < E:
            c.add("edge_outside")
        if name == "no_edge" and 0 <= e < E and int(case["edges"][e]["i"]) == int(case["edges"][e]["j"]):
            c.add("no_edge_self")
        if name == "skipped":
            ed = case["edges"][e]
            c.add("skipped_odometry" if not int(ed["flags"]) & pg.EDGE_CLOSURE else "skipped_disabled" if int(ed["flags"]) & pg.EDGE_DISABLED else
                  "skipped_not_finite")
        if name == "singular":
            c.add("s_singular" if case["name"].startswith("s_singular") else "w_singular")
        d2 = float(rp["d2"])
        if name == "rejected" and d2 != d2:
            c.add("nan_d2")
        if name == "passed" and d2 == case["gate"]:
            c.add("at_gate_passed")
        if name == "rejected" and case["gate"] == float(np.nextafter(d2, 0.0)):
            c.add("ulp_below_gate_rejected")
        if name == "passed" and case["gate"] == float(np.nextafter(d2, math.inf)):
            c.add("ulp_above_gate_passed")
        if name == "rejected":
            if e in seen:
                c.add("two_queries_one_edge")
            seen[e] = k
    return c


_vet_results = {}


def run_vet_case(case):
    if case["name"] not in _vet_results:
        tr = {}
        _vet_results[case["name"]] = vet(case["nodes"], case["edges"], case["queries"], case["recs"], case["gate"], tr) + (tr,)
    return _vet_results[case["name"]]


# ---- the gate's fixture ----------------------------------------------------------------------------------------------------------------
FIXTURE = dict(n=50, lap=40, radius=20.0, seed=3, odo_info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0), closure_info=rc.CLOSURE_INFO, true=(0, 3, 6, 9), false=(5, 30),
               marg=dict(cg_tol=1e-10, cg_iters=200, precond=CHAIN, slots=256))


def gate_fixture(seed=None):
    """A track of 1.25 laps round a circle whose odometry errors are zero-mean draws at the standard deviations its information states
    (0.5 px, 0.5 px, 1 degree a step), node 0 fixed; behind the odometry edges four TRUE closures (k, k + lap), measured with draws at the
    closure information's standard deviations (0.2 px, 0.2 px, 1/3 degree), and one FALSE closure between node 30 and node 5, which claims
    that they are one place.  -> (nodes, edges, the prior's n_edges, the index of the false closure, the indices of the true ones)."""
    F = FIXTURE
    rng = np.random.default_rng(F["seed"] if seed is None else seed)
    n, lap = F["n"], F["lap"]
    truth = []
    for k in range(n):
        a = 360.0 * k / lap
        truth.append((60.0 + F["radius"] * math.cos(math.radians(a)), 60.0 + F["radius"] * math.sin(math.radians(a)), pg.wrap(a + 90.0)))
    sd = lambda info: (1.0 / math.sqrt(info[0]), 1.0 / math.sqrt(info[2]), 1.0 / math.sqrt(info[5]))
    so, sc = sd(F["odo_info"]), sd(F["closure_info"])
    edges, poses = [], [truth[0]]
    for k in range(1, n):
        z = pg.rel(truth[k - 1], truth[k])
        z = tuple(z[q] + so[q] * rng.normal() for q in range(3))
        edges.append(pg.edge(k - 1, k, z, F["odo_info"]))
        poses.append(pg.comp(poses[-1], z))
    prior = len(edges)
    true_idx = []
    for k in F["true"]:
        z = pg.rel(truth[k], truth[k + lap])
        true_idx.append(len(edges))
        edges.append(pg.edge(k, k + lap, tuple(z[q] + sc[q] * rng.normal() for q in range(3)), F["closure_info"], pg.EDGE_CLOSURE))
    false_idx = len(edges)
    edges.insert(prior + 2, pg.edge(F["false"][0], F["false"][1], tuple(sc[q] * rng.normal() for q in range(3)), F["closure_info"], pg.EDGE_CLOSURE))
    false_idx = prior + 2
    true_idx = [e + (e >= false_idx) for e in true_idx]
    nodes = np.array([pg.node(*poses[k], flags=pg.NODE_FIXED if k == 0 else 0) for k in range(n)], pg.NODE_DTYPE)
    return nodes, np.array(edges, pg.EDGE_DTYPE).reshape(-1), prior, false_idx, true_idx


# ---- the gate's fixture with scans: the closure chain end to end -------------------------------------------------------------------------
VET_E2E = dict(seed=0, look_alike=(40, 4), vet=dict(gate=GATE_999, marg=dict(cg_tol=1e-9, cg_iters=100, precond=CHAIN, slots=256)),
               robust=rc.rob(rc.HUBER, 2.0))
_vet_e2e = {}


def vet_end_to_end(seed=None):
    """pose_graph_loops_cases' two laps around the off-centre box with the odometry of the gate's fixture -- zero-mean draws at the standard
    deviations the appended information states instead of a steady under-read -- and one keyframe (look_alike[0]) whose scan is the one
    seen from another keyframe's place (look_alike[1]), as a second room that looks the same would give it: place recognition finds that
    place, the matcher fits it, and the closure chain appends a FALSE closure beside the true ones.  The chain restated: append ->
    snapshot -> recognize_all -> find_loops -> per round select + the closure's tail -> the marginals of the new edges on the prior's
    graph -> the gate -> optimize (Huber 2.0, prune at rc.GATE, refit) -> rerender."""
    import pose_graph_loops_cases as pl
    import pose_graph_place_cases as pp
    seed = VET_E2E["seed"] if seed is None else seed
    if seed in _vet_e2e:
        return _vet_e2e[seed]
    E2E = pl.E2E
    R, n, nb = pp.PLACE_ROOM, E2E["n"], E2E["n_beams"]
    rng = np.random.default_rng(seed)
    truth = []
    for k in range(n + 1):
        a = 363.0 * k / 24
        truth.append((30.0 + 13.0 * math.cos(math.radians(a)), 23.0 + 10.0 * math.sin(math.radians(a)), pg.wrap(a + 90.0)))
    info = E2E["append"]["info"]
    sd = (1.0 / math.sqrt(info[0]), 1.0 / math.sqrt(info[2]), 1.0 / math.sqrt(info[5]))
    odom = [truth[0]]
    for k in range(1, n + 1):
        z = pg.rel(truth[k - 1], truth[k])
        odom.append(pg.comp(odom[-1], tuple(z[q] + sd[q] * rng.normal() for q in range(3))))
    seen_from = list(truth)
    seen_from[VET_E2E["look_alike"][0]] = truth[VET_E2E["look_alike"][1]]
    scans = np.stack([pp.place_room_scan(p, nb) for p in seen_from])
    lens = np.full(n + 1, nb, np.int32)
    cap = n + 4
    g0 = pg.new_graph(cap, n + 16, nb)
    g1, arep = pg.append(g0, scans, lens, np.array(odom), 0, E2E["append"])
    nn, prior = int(g1["head"][0]["n_nodes"]), int(g1["head"][0]["n_edges"])
    desc = pp.describe(nn, g1["store"], g1["store_lens"], R["range_max"], np.zeros(cap, pp.DESC_DTYPE))
    k = E2E["place"]["k"]
    recs, reps = pl.recognize_all(g1, desc, E2E["place"], 0, cap, np.zeros((cap, k), pp.PLACE_REC_DTYPE), np.zeros(cap, pp.PLACE_REP_DTYPE))
    loops, lrep = pl.find_loops(recs, reps, cap, g1["head"][0]["n_edges"], g1["edges"], E2E["loops"], {})
    g, row = g1, np.zeros((nb, 2))
    nears, creps = [], []
    for m in range(E2E["loops"]["max_loops"]):
        near, sel, row, q_len, q_pose = pl.loop_select(g, loops, lrep, m, E2E["place"]["gap"], E2E["place"]["window"], row)
        g, _, crep = pl.close_tail(g, near, sel, row, q_len, q_pose)
        nears.append(near)
        creps.append(crep)
    ne = int(g["head"][0]["n_edges"])
    nodes, edges = g["nodes"][:nn], g["edges"][:ne]
    vetted, mrecs, mrep, vreps = vetted_closures(nodes, edges, prior, E2E["loops"]["max_loops"], VET_E2E["vet"], len(g["edges"]))
    opt = rc.optimize(nodes, vetted, VET_E2E["robust"], rc.GATE, 8, E2E["relax"])
    cols, rows = R["cols"], R["rows"]
    pa, hi = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    poses = np.zeros((cap, 3))
    poses[:] = np.stack([g["nodes"]["x"], g["nodes"]["y"], g["nodes"]["ang"]], axis=1)
    poses[:nn] = np.stack([opt["nodes"]["x"], opt["nodes"]["y"], opt["nodes"]["ang"]], axis=1)
    gc.integrate(g["store"], g["store_lens"], poses, cols, rows, R["resol"], R["range_max"], pa, hi)
    false_edges = [e for e in range(prior, ne) if max(int(edges[e]["i"]), int(edges[e]["j"])) == VET_E2E["look_alike"][0]]
    _vet_e2e[seed] = dict(truth=np.array(truth), odom=np.array(odom), scans=scans, lens=lens, cap=cap, edges_cap=len(g["edges"]), n_nodes=nn, n_edges=ne,
                          prior=prior, nears=np.array(nears), closure_reps=np.array(creps), nodes=nodes, edges=edges, vetted=vetted, recs=mrecs,
                          rep=mrep, vet_reps=vreps, opt=opt, planes=(pa, hi), false_edges=false_edges)
    return _vet_e2e[seed]
