"""The relaxation with a choice of preconditioner (include/lsd_hip.h: lsd_enqueue_pg_relax_pc_device; csrc/k_pgchain.hip,
csrc/pgrelax_dev.h) restated on Python floats, in the header's order, written from the header for the tests (not from the
HIP code), and the generated campaign both test files run.

The blocks of an edge, the weights, inv3, the one reduction shape, the canonical NaN and the graphs are pose_graph_cases' and
pose_graph_robust_cases' own text; what is restated here is what the new entry adds: the chain edges, the paths and positions, the blocks
Dg and C, the block cyclic reduction, its apply, the fallback -- and the outer loop that chooses between z_n = M_n r_n and z = M^-1 r,
which with kind BLOCK must give pose_graph_robust_cases' bytes (test_pose_graph_chain_cpu.py holds it to that).  The factor is written
sequentially, position after position in ascending order: that IS the header's order of the two sides.  A case class is a predicate on
the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import pose_graph_cases as pg
import pose_graph_robust_cases as rc

PRECOND_REP_DTYPE = np.dtype([("chain_edges", "i4"), ("paths", "i4"), ("longest_path", "i4"), ("fallbacks", "i4")])
SIZES = {"lsd_pg_precond_par": 8, "lsd_pg_precond_rep": 16}
BLOCK, CHAIN = 0, 1
INF, NAN = pg.INF, pg.NAN


# ---- the chain edges, the paths, the positions (integers only) ---------------------------------------------------------------------------
def chain_of(N, edges, valid):
    """(chain[e], up_edge[n] or -1, before[n] or -1, up[n], down[n]) of the edges that are not skipped."""
    E = len(edges)
    lo = [min(int(e["i"]), int(e["j"])) for e in edges]
    hi = [max(int(e["i"]), int(e["j"])) for e in edges]
    cand = [valid[e] and not int(edges[e]["flags"]) & pg.EDGE_CLOSURE for e in range(E)]
    up, down = [None] * N, [None] * N
    for e in range(E):                                                       # ascending: the first one met is the smallest index
        if cand[e]:
            if up[lo[e]] is None:
                up[lo[e]] = e
            if down[hi[e]] is None:
                down[hi[e]] = e
    chain = [bool(cand[e] and up[lo[e]] == e and down[hi[e]] == e) for e in range(E)]
    up_edge, before = [-1] * N, [-1] * N
    for e in range(E):
        if chain[e]:
            up_edge[lo[e]] = e
            before[hi[e]] = lo[e]
    return chain, up_edge, before, up, down, cand, lo, hi


def positions(N, up_edge, before, hi):
    """node(t) for t = 0 .. N-1 and the paths (lists of nodes): the paths in ascending head index, each walked from its head."""
    paths = []
    for h in range(N):
        if before[h] < 0:
            path, n = [h], h
            while up_edge[n] >= 0:
                n = hi[up_edge[n]]
                path.append(n)
            paths.append(path)
    return [n for p in paths for n in p], paths


# ---- 3 x 3 products, every sum ascending from +0.0 -------------------------------------------------------------------------------------
def mm(X, Y, tx=False, ty=False):
    """out(r,q) = sum_u X(r,u) * Y(u,q); tx: X(u,r) in the place of X(r,u); ty: Y(q,u) in the place of Y(u,q)."""
    out = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for q in range(3):
            t = 0.0
            for u in range(3):
                t += (X[u][r] if tx else X[r][u]) * (Y[q][u] if ty else Y[u][q])
            out[r][q] = t
    return out


def mv_sub(X, u, v, tx=False):
    """v(r) - sum_q X(r,q) * u(q)   (tx: X(q,r))."""
    out = []
    for r in range(3):
        t = 0.0
        for q in range(3):
            t += (X[q][r] if tx else X[r][q]) * u[q]
        out.append(v[r] - t)
    return out


def msub(X, Y):
    return [[X[r][q] - Y[r][q] for q in range(3)] for r in range(3)]


IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


# ---- the factor and the apply ----------------------------------------------------------------------------------------------------------
def factor(Dg, C):
    """Block cyclic reduction of the block-tridiagonal matrix with diagonal blocks Dg[t] and couplings C[t] = (t, t+1), rows of t.
    Returns None where an inv3 fails, else the dict the apply reads."""
    N = len(Dg)
    Dg = [[list(r) for r in D] for D in Dg]
    Cc = [[list(r) for r in c] for c in C] + [None]                           # the current coupling (t, t + s) at t
    P, GL, GU, Ls, Rs = [None] * N, [None] * N, [None] * N, [None] * N, [None] * N
    s = 1
    while s < N:
        for t in range(s, N, 2 * s):
            a, c = t - s, t + s
            L, R = Cc[a], (Cc[t] if c < N else None)
            P[t], _ = pg.inv3(Dg[t])
            if P[t] is None:
                return None
            GL[t], Ls[t], Rs[t] = mm(L, P[t]), L, R
            if c < N:
                GU[t] = mm(R, P[t], tx=True)
                Dg[c] = msub(Dg[c], mm(GU[t], R))                            # (c receives from its lower side here, from its upper side later)
            Dg[a] = msub(Dg[a], mm(GL[t], L, ty=True))
            if c < N:
                Cc[a] = [[-v for v in row] for row in mm(GL[t], R)]
        s *= 2
    if N:
        P[0], _ = pg.inv3(Dg[0])
        if P[0] is None:
            return None
    return dict(N=N, P=P, GL=GL, GU=GU, L=Ls, R=Rs)


def apply(F, r):
    """x = M^-1 r in position order."""
    N = F["N"]
    y = [list(v) for v in r]
    levels = []
    s = 1
    while s < N:
        levels.append(s)
        for t in range(s, N, 2 * s):
            a, c = t - s, t + s
            if c < N:
                y[c] = mv_sub(F["GU"][t], y[t], y[c])
            y[a] = mv_sub(F["GL"][t], y[t], y[a])
        s *= 2
    x = [None] * N
    if N:
        x[0] = [pg.dot3(F["P"][0][q], y[0]) for q in range(3)]
    for s in reversed(levels):
        for t in range(s, N, 2 * s):
            a, c = t - s, t + s
            v = mv_sub(F["L"][t], x[a], y[t], tx=True)
            if c < N:
                v = mv_sub(F["R"][t], x[c], v)
            x[t] = [pg.dot3(F["P"][t][q], v) for q in range(3)]
    return x


def dense_of(Dg, C):
    """The block-tridiagonal matrix the factor is of, assembled densely (numpy, for the accuracy test)."""
    N = len(Dg)
    M = np.zeros((3 * N, 3 * N))
    for t in range(N):
        M[3 * t:3 * t + 3, 3 * t:3 * t + 3] = Dg[t]
        if t + 1 < N:
            M[3 * t:3 * t + 3, 3 * t + 3:3 * t + 6] = C[t]
            M[3 * t + 3:3 * t + 6, 3 * t:3 * t + 3] = np.array(C[t]).T
    return M


# ---- the relaxation --------------------------------------------------------------------------------------------------------------------
def relax_pc(nodes, edges, par, r, kind, trace=None):
    """lsd_enqueue_pg_relax_pc_device on one graph: nodes NODE_DTYPE [N], edges EDGE_DTYPE [E] (the clamped counts) -> (nodes after, edges
    after, the report, the robust report, the preconditioner's report).  par: a dict of pg.RELAX_KEYS; r: rc.rob(); kind: BLOCK or CHAIN."""
    with np.errstate(all="ignore"):
        return _relax_pc(nodes, edges, par, r, kind, trace if trace is not None else {})


def _relax_pc(nodes, edges, par, rb, kind, tr):
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
    scope = [valid[e] and (rb["scope"] == rc.ALL or bool(int(edges[e]["flags"]) & pg.EDGE_CLOSURE)) for e in range(E)]
    lists = [[] for _ in range(N)]
    for e in range(E):
        if valid[e]:
            lists[int(edges[e]["i"])].append((e, 0))
            lists[int(edges[e]["j"])].append((e, 1))
    ei, ej = [int(e["i"]) for e in edges], [int(e["j"]) for e in edges]
    Z = [[float(v) for v in e["z"]] for e in edges]
    W = [pg.info_rows([float(v) for v in e["info"]]) for e in edges]
    pc = np.zeros(1, PRECOND_REP_DTYPE)[0]
    tr.update(N=N, E=E, why=why, scope=scope, steps=[], cg_ends=[], cg_steps=[], fell_back=[], lambdas=[], fixed=fixed,
              degrees=[len(l) for l in lists], singular_at=[None] * N, kind=kind)
    if kind == CHAIN:                                                        # once per call, beside the lists
        chain, up_edge, before, upn, downn, cand, lo, hi = chain_of(N, edges, valid)
        node_at, paths = positions(N, up_edge, before, hi)
        pc["chain_edges"], pc["paths"], pc["longest_path"] = sum(chain), len(paths), max([len(p) for p in paths] + [0])
        tr.update(chain=chain, up_edge=up_edge, before=before, up=upn, down=downn, cand=cand, lo=lo, hi=hi, node_at=node_at, paths=paths)

    def chi2s(poses):
        return [pg.edge_chi2(poses[ei[e]], poses[ej[e]], Z[e], W[e]) if valid[e] else 0.0 for e in range(E)]

    def objective(ce):
        return pg.reduce_shape([rc.weight(rb, scope[e], ce[e])[1] if valid[e] else 0.0 for e in range(E)])
    ce = chi2s(P)
    F = objective(ce)
    rep = np.zeros(1, pg.RELAX_REP_DTYPE)[0]
    rep["chi2_before"] = rc.canon(F)
    flags, done, cg_total, accepted, rejected, fallbacks = 0, 0, 0, 0, 0, 0
    moved = set()
    zero = [0.0, 0.0, 0.0]
    if not math.isfinite(F):
        flags |= pg.RELAX_NOT_FINITE
    while not flags & pg.RELAX_NOT_FINITE and done < iters:
        blk = [None] * E                                                     # 1
        for e in range(E):
            if valid[e]:
                we = rc.weight(rb, scope[e], ce[e])[0]
                Wp = [[we * W[e][r][t] for t in range(3)] for r in range(3)]
                blk[e] = pg.edge_blocks(P[ei[e]], P[ej[e]], Z[e], Wp)[:5]
        H, b, M, D = [None] * N, [None] * N, [None] * N, [None] * N
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
                D[n] = [[Hn[r][q] if r != q else Hn[r][r] + lam * Hn[r][r] for q in range(3)] for r in range(3)]
                M[n], _ = pg.inv3(D[n])
                if M[n] is None:
                    singular[n] = True
                    tr["singular_at"][n] = done
        free = [not fixed[n] and not singular[n] for n in range(N)]
        Fc = None
        if kind == CHAIN:                                                    # the blocks and the factor, behind step 3
            Dg = [D[n] if free[n] else IDENTITY for n in node_at]
            Cs = []
            for t in range(N - 1):
                n, m = node_at[t], node_at[t + 1]
                e = up_edge[n]
                if e >= 0 and hi[e] == m and free[n] and free[m]:
                    hab = blk[e][1]
                    Cs.append(hab if ei[e] == n else [[hab[q][r] for q in range(3)] for r in range(3)])
                else:
                    Cs.append([list(zero) for _ in range(3)])
            Fc = factor(Dg, Cs)
            if Fc is None:
                fallbacks += 1
            tr["last_blocks"] = (Dg, Cs)
        tr["fell_back"].append(kind == CHAIN and Fc is None)
        tr["lambdas"].append(lam)

        def precond(r_):
            if Fc is None:
                return [[pg.dot3(M[n][q], r_[n]) for q in range(3)] if free[n] else list(zero) for n in range(N)]
            x = apply(Fc, [r_[n] for n in node_at])
            z_ = [None] * N
            for t, n in enumerate(node_at):
                z_[n] = x[t] if free[n] else list(zero)
            return z_
        dl = [list(zero) for _ in range(N)]                                  # 4
        r_ = [[-b[n][q] for q in range(3)] if free[n] else list(zero) for n in range(N)]
        z_ = precond(r_)
        p_ = [list(v) for v in z_]
        rz = pg.reduce_shape([pg.dot3(r_[n], z_[n]) for n in range(N)])
        thr = (cg_tol * cg_tol) * rz
        steps, end = 0, None
        while True:
            if not steps < cg_iters:
                end = "iters"
                break
            if rz <= thr:
                end = "tol" if steps else "start"
                break
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
                end = "breakdown"
                break
            alpha = pg.fdiv(rz, pq)
            for n in range(N):
                if free[n]:
                    for c in range(3):
                        dl[n][c] = dl[n][c] + alpha * p_[n][c]
                        r_[n][c] = r_[n][c] - alpha * q_[n][c]
            z_ = precond(r_)
            rzn = pg.reduce_shape([pg.dot3(r_[n], z_[n]) for n in range(N)])
            beta = pg.fdiv(rzn, rz)
            for n in range(N):
                if free[n]:
                    for c in range(3):
                        p_[n][c] = z_[n][c] + beta * p_[n][c]
            rz = rzn
            steps += 1
        cg_total += steps
        tr["cg_ends"].append(end)
        tr["cg_steps"].append(steps)
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
        edges[e]["chi2"] = rc.canon(ce[e])
    rep["chi2_after"], rep["lambda"] = rc.canon(F), lam
    rep["iters"], rep["cg_iters"], rep["accepted"], rep["rejected"] = done, cg_total, accepted, rejected
    rep["skipped_edges"], rep["singular_nodes"], rep["flags"] = sum(1 for v in valid if not v), sum(singular), flags
    rr = np.zeros(1, rc.ROBUST_REP_DTYPE)[0]                                 # the robust report: the weights at the final poses
    rr["chi2_plain"] = rc.canon(pg.reduce_shape(ce))
    w_fin = {e: rc.weight(rb, True, ce[e])[0] for e in range(E) if scope[e]}
    nans = [e for e, w in w_fin.items() if w != w]
    w_min, w_edge = 1.0, -1
    if nans:
        w_min, w_edge = rc.MADE_NAN, min(nans)
    elif w_fin:
        w_min = min(w_fin.values())
        w_edge = min(e for e, w in w_fin.items() if w == w_min)
    rr["w_min"], rr["w_min_edge"], rr["downweighted"] = w_min, w_edge, sum(1 for w in w_fin.values() if w < 1.0)
    pc["fallbacks"] = fallbacks
    tr.update(flags=flags, singular=singular)
    return nodes, edges, rep, rr, pc


def optimize_pc(nodes, edges, r, gate, kind, max_reject=8, relax=None, refit=None):
    """PoseGraph.optimize_device(.., precond=) on the clamped counts: rc.optimize with both relaxations preconditioned as `kind` says."""
    relax = dict(pg.RELAX_DEFAULTS, **(relax or {}))
    refit = relax if refit is None else dict(pg.RELAX_DEFAULTS, **refit)
    n1, e1, rep1, rr, pc1 = relax_pc(nodes, edges, relax, r, kind)
    e2, prep = rc.prune(len(e1), e1, gate, max_reject)
    n3, e3, rep3, _, pc3 = relax_pc(n1, e2, refit, rc.rob(rc.NONE, 0.0), kind)
    return dict(nodes=n3, edges=e3, robust_relax=rep1, robust=rr, prune=prep, refit=rep3, precond=pc3)


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def interleaved(tracks, n_each, rng, closures=1, fix_first=True):
    """`tracks` loops of n_each nodes whose nodes alternate in the store (node k belongs to track k mod tracks), as the fleet's appends
    onto one graph leave them; `closures` true closures per track.  Node 0 of every track is fixed."""
    nodes, edges = [None] * (tracks * n_each), []
    for t in range(tracks):
        no, ed, _ = pg.loop_graph(n_each, rng, radius=15.0 + 5.0 * t, closures=closures, fix=(0,) if fix_first else ())
        for k in range(n_each):
            nodes[k * tracks + t] = no[k]
        for e in ed:
            e = e.copy()
            e["i"], e["j"] = int(e["i"]) * tracks + t, int(e["j"]) * tracks + t
            edges.append((int(e["j"]), t, e))
    edges.sort(key=lambda v: (v[0], v[1]))                                   # in the order the appends made them
    return np.array(nodes, pg.NODE_DTYPE), np.array([e for _, _, e in edges], pg.EDGE_DTYPE).reshape(-1)


def ccase(name, nodes, edges, r=None, kind=CHAIN, **par):
    c = rc.rcase(name, nodes, edges, rc.rob(rc.NONE, 0.0) if r is None else r, **par)
    c["kind"] = kind
    return c


def well_posed():
    """The graphs of the comparison with the dense reference: pose_graph_cases' well_posed() and loops of 100 and 256 nodes with 4 closures."""
    out = [ccase(c["name"], c["nodes"], c["edges"], **c["par"]) for c in pg.well_posed()]
    for n in (100, 256):
        nodes, edges, _ = pg.loop_graph(n, np.random.default_rng(7000 + n), closures=4)
        out.append(ccase("loop_%d_4" % n, nodes, edges, cg_iters=3 * n, iters=30, cg_tol=1e-10, eps=1e-10))
    return out


SIZES_3 = (0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024)
ONCE = ("n_1025", "n_4097")
# Seeds found by running the restatement over a range of them and keeping those whose TRACE shows the class (the device was not asked).
# Without a fixed node, damping and closures M is singular: whether its last pivot comes out > 0 is rounding's doing, and so is the sign of
# p^T D p -- the same family gives the fallbacks (0, 1, 2, 3, 4, 13, 15) and the BREAKDOWNs of a solve the chain preconditioned (4, 11, 13, 15).
FALLBACK_SEEDS = (0, 1, 2, 3, 4, 11, 13, 15)
SINGULAR_LATER_SEEDS = (0, 3, 4, 9)
REJECTED_SEEDS = (2, 3, 6, 9)
INDEFINITE_SCALES = (0.5, 1.0, 2.0)


def campaign():
    rng = np.random.default_rng(20261023)
    out = []
    quick = dict(iters=1, cg_iters=4)
    robs = (rc.rob(rc.NONE, 0.0, rc.CLOSURES), rc.rob(rc.HUBER, 1.0, rc.CLOSURES), rc.rob(rc.GM, 3.0, rc.ALL))
    for n in SIZES_3:                                                        # the sizes: levels with and without an upper neighbour
        for rep in range(3):
            nodes, edges = pg.chain_graph(n, rng, extra=rep if n >= 8 else 0)
            par = dict(iters=3, cg_iters=12) if n < 255 else (dict(iters=2, cg_iters=6) if n < 1023 else quick)
            out.append(ccase("n_%d_%d" % (n, rep), nodes, edges, robs[rep], **par))
    for n in (1025, 4097):
        nodes, edges = pg.chain_graph(n, rng, extra=2)
        out.append(ccase("n_%d" % n, nodes, edges, **quick))
    for rep in range(3):
        # no chain edge at all: closures only
        nodes, edges, _ = pg.loop_graph(8 + rep, rng, closures=2)
        only = edges.copy()
        only["flags"] |= pg.EDGE_CLOSURE
        out.append(ccase("no_chain_edge_%d" % rep, nodes, only, robs[rep], iters=3, cg_iters=40))
        # two and three tracks interleaved in the store, all six robust settings between them
        for tracks in (2, 3):
            nodes, edges = interleaved(tracks, 9 + rep, rng, closures=2)
            kernel = (rc.NONE, rc.HUBER, rc.GM)[rep]
            out.append(ccase("interleaved_%d_%d" % (tracks, rep), nodes, edges, rc.rob(kernel, 2.0, rc.CLOSURES if tracks == 2 else rc.ALL), iters=4,
                             cg_iters=60))
        nodes, edges = interleaved(2, 6 + rep, rng)                          # the three kernels with both scopes on one graph
        for kname, kernel in (("none", rc.NONE), ("huber", rc.HUBER), ("gm", rc.GM)):
            for sname, scope in (("closures", rc.CLOSURES), ("all", rc.ALL)):
                out.append(ccase("%s_%s_%d" % (kname, sname, rep), nodes, edges, rc.rob(kernel, 0.5 + 0.5 * rep, scope), iters=3, cg_iters=40))
        # a path cut by a DISABLED edge and by a skipped (non-finite) edge; a chain edge stored with i > j; two candidates between one pair
        nodes, edges, _ = pg.loop_graph(14 + rep, rng, closures=2, noisy=True)
        cut = edges.copy()
        cut["flags"][4 + rep] |= pg.EDGE_DISABLED
        cut["z"][8][1] = NAN
        i, j = int(cut["i"][2]), int(cut["j"][2])
        cut[2] = pg.edge(j, i, pg.rel(pg.pose_of(nodes[j]), pg.pose_of(nodes[i])), (4.0, 0.0, 4.0, 0.0, 0.0, 1.0))
        twin = pg.edge(5 + rep, 6 + rep, (3.0, 0.5, 4.0), (1.0, 0.0, 1.0, 0.0, 0.0, 0.5))
        cut = np.concatenate([cut[:10], np.array([twin], pg.EDGE_DTYPE), cut[10:]])
        out.append(ccase("cut_%d" % rep, nodes, cut, iters=3, cg_iters=60))
        # a chord (n, n+2) that loses to (n, n+1) by index and one that wins; a closure between neighbours; up and down that disagree
        nodes, edges, truth = pg.loop_graph(12 + rep, rng, closures=1)
        chord = lambda a, b, fl=0: pg.edge(a, b, pg.rel(tuple(truth[a]), tuple(truth[b])), (2.0, 0.0, 2.0, 0.0, 0.0, 1.0), fl)
        es = list(edges)
        es.insert(7, chord(3, 5))                                            # behind (3, 4) and (4, 5): loses
        es.insert(6 + 1, chord(7, 9))                                        # in front of (7, 8) and (8, 9): wins, node 8 is a path of one
        es.append(chord(1, 2, pg.EDGE_CLOSURE))
        es.insert(0, chord(0, 2 + rep))                                      # up[0] is this one, down[2 + rep] is (1 + rep, 2 + rep): disagree
        out.append(ccase("chords_%d" % rep, nodes, np.array(es, pg.EDGE_DTYPE), robs[rep], iters=3, cg_iters=60))
        # node states
        nodes, edges, _ = pg.loop_graph(12 + rep, rng, noisy=True)
        mid = nodes.copy()
        mid["flags"][5 + rep] |= pg.NODE_FIXED
        out.append(ccase("fixed_mid_%d" % rep, mid, edges, iters=3, cg_iters=40))
        allf, nonef = nodes.copy(), nodes.copy()
        allf["flags"] |= pg.NODE_FIXED
        nonef["flags"] &= ~np.uint32(pg.NODE_FIXED)
        out.append(ccase("all_fixed_%d" % rep, allf, edges, iters=2, cg_iters=20))
        out.append(ccase("none_fixed_%d" % rep, nonef, edges, iters=4, cg_iters=40))
        lone = np.concatenate([nodes[:4], np.array([pg.node(1.0, 2.0, 3.0)], pg.NODE_DTYPE), nodes[4:]])   # node 4 has no edge
        ed = edges.copy()
        ed["i"] += ed["i"] >= 4
        ed["j"] += ed["j"] >= 4
        out.append(ccase("degree_0_%d" % rep, lone, ed, iters=3, cg_iters=40))
        # the solver's ends
        out.append(ccase("iters_0_%d" % rep, nodes, edges, robs[rep], iters=0))
        out.append(ccase("cg_iters_0_%d" % rep, nodes, edges, iters=2, cg_iters=0))
        out.append(ccase("cg_tol_end_%d" % rep, nodes, edges, iters=2, cg_iters=200, cg_tol=1e-3))
        nodes4, edges4, _ = pg.loop_graph(40 + rep, rng, closures=4)
        out.append(ccase("cg_iters_end_%d" % rep, nodes4, edges4, iters=2, cg_iters=2, cg_tol=1e-12))
    for seed in REJECTED_SEEDS:                                              # a far start: rejected steps, lambda changes between two factors
        r2 = np.random.default_rng(9400 + seed)
        nodes, edges, _ = pg.loop_graph(12 + seed % 3, r2, noisy=True)
        far = nodes.copy()
        far["ang"][1:] += 100.0 + 10.0 * seed
        far["x"][1:] += 30.0
        out.append(ccase("far_start_%d" % seed, far, edges, iters=8, cg_iters=60, lambda0=1e-3))
    for k, scale in enumerate(INDEFINITE_SCALES):                            # an indefinite information on a closure: M fails with it (fallback,
        nodes, edges, _ = pg.loop_graph(10, np.random.default_rng(9100 + k), closures=1)                # BREAKDOWN) or a node's block does
        neg = edges.copy()
        neg["info"][-1] = (-scale * 4.0, 0.0, -scale * 4.0, 0.0, 0.0, -scale)
        out.append(ccase("indefinite_%d" % k, nodes, neg, iters=2, cg_iters=60))
    for seed in FALLBACK_SEEDS:                                              # no fixed node, no damping, no closure: M is singular
        r2 = np.random.default_rng(9200 + seed)
        nodes, edges = pg.chain_graph(5 + seed % 4, r2)
        nodes["flags"] &= ~np.uint32(pg.NODE_FIXED)
        out.append(ccase("fallback_%d" % seed, nodes, edges, iters=3, cg_iters=30, lambda0=0.0, lambda_min=0.0))
    for seed in SINGULAR_LATER_SEEDS:                                        # a node whose only edge knows nothing of its heading: det(D_n) is
        r2 = np.random.default_rng(9300 + seed)                              # lambda's doing in the first iteration and rounding's from then on
        nodes, edges, _ = pg.loop_graph(8, r2)
        extra = np.array([pg.node(50.0 + r2.normal(), 50.0 + r2.normal(), 10.0 * r2.normal())], pg.NODE_DTYPE)
        e = pg.edge(8, 3, (1.0 + r2.normal(), 2.0, 3.0), (1.0, 0.0, 1.0, 0.0, 0.0, 0.0))
        out.append(ccase("singular_later_%d" % seed, np.concatenate([nodes, extra]), np.concatenate([edges, np.array([e], pg.EDGE_DTYPE)]), iters=4,
                         cg_iters=60, down=1e300, lambda_min=0.0))
    return out


CLASSES = (["n_%d" % n for n in SIZES_3 + (1025, 4097)] +
           ["no_chain_edge", "interleaved_2", "interleaved_3", "cut_by_disabled", "cut_by_skipped", "chain_edge_descending", "duplicate_pair", "chord_loses",
            "chord_wins", "closure_between_neighbours", "up_down_disagree", "fixed_mid_path", "all_fixed", "none_fixed", "degree_0_inside",
            "singular_later", "iters_0", "cg_iters_0", "cg_end_tol", "cg_end_iters", "cg_end_breakdown", "rejected_between_factors", "fallback",
            "none_closures", "none_all", "huber_closures", "huber_all", "gm_closures", "gm_all"])
ONCE_CLASSES = ("n_1025", "n_4097")


def classes_of(case, tr):
    edges, r = case["edges"], case["rob"]
    c = set()
    N, E = tr["N"], tr["E"]
    if N in SIZES_3 + (1025, 4097) and case["name"].startswith("n_"):
        c.add("n_%d" % N)
    chain, lo, hi, cand = tr["chain"], tr["lo"], tr["hi"], tr["cand"]
    if E and N and not any(chain):
        c.add("no_chain_edge")
    long_paths = [p for p in tr["paths"] if len(p) >= 2]
    if len(long_paths) in (2, 3) and all(any(b - a > 1 for a, b in zip(p, p[1:])) for p in long_paths):
        c.add("interleaved_%d" % len(long_paths))
    pairs = {}
    for e in range(E):
        closure = bool(int(edges["flags"][e]) & pg.EDGE_CLOSURE)
        joined = any(chain[f] and (lo[f], hi[f]) == (lo[e], hi[e]) for f in range(E))
        if tr["why"][e] == "disabled" and not closure and not joined:
            c.add("cut_by_disabled")
        if tr["why"][e] == "not_finite" and not closure and not joined:
            c.add("cut_by_skipped")
        if chain[e] and int(edges["i"][e]) > int(edges["j"][e]):
            c.add("chain_edge_descending")
        if cand[e]:
            first = pairs.setdefault((lo[e], hi[e]), e)
            if first != e and chain[first] and not chain[e]:
                c.add("duplicate_pair")
            if hi[e] - lo[e] == 2:
                rival = [f for f in range(E) if cand[f] and lo[f] == lo[e] and hi[f] == lo[e] + 1]
                if rival and not chain[e] and rival[0] < e and chain[rival[0]]:
                    c.add("chord_loses")
                if rival and chain[e] and rival[0] > e:
                    c.add("chord_wins")
            if (tr["up"][lo[e]] == e) != (tr["down"][hi[e]] == e):
                c.add("up_down_disagree")
        if closure and tr["why"][e] is None and hi[e] - lo[e] == 1:
            c.add("closure_between_neighbours")
    for n in range(N):
        if tr["fixed"][n] and tr["before"][n] >= 0 and tr["up_edge"][n] >= 0 and not all(tr["fixed"]):
            c.add("fixed_mid_path")
        if tr["degrees"][n] == 0 and n < N - 1:
            c.add("degree_0_inside")
        if tr["singular_at"][n] is not None and tr["singular_at"][n] >= 1:
            c.add("singular_later")
    if N and all(tr["fixed"]):
        c.add("all_fixed")
    if N and not any(tr["fixed"]):
        c.add("none_fixed")
    if case["par"]["iters"] == 0:
        c.add("iters_0")
    if case["par"]["cg_iters"] == 0 and tr["cg_ends"]:
        c.add("cg_iters_0")
    for end, fb, steps in zip(tr["cg_ends"], tr["fell_back"], tr["cg_steps"]):   # the ends of a solve the CHAIN preconditioned
        if not fb and end in ("tol", "iters", "breakdown") and (steps or end == "breakdown") and case["par"]["cg_iters"]:
            c.add("cg_end_" + end)
    for k in range(1, len(tr["steps"])):
        if tr["steps"][k - 1] == "rejected" and not tr["fell_back"][k - 1] and not tr["fell_back"][k] and tr["lambdas"][k] != tr["lambdas"][k - 1]:
            c.add("rejected_between_factors")
    if any(tr["fell_back"]):
        c.add("fallback")
    if tr["cg_ends"] and any(tr["scope"]) or r["kernel"] == rc.NONE and tr["cg_ends"]:
        c.add("%s_%s" % (("none", "huber", "gm")[r["kernel"]], "all" if r["scope"] == rc.ALL else "closures"))
    return c


_results = {}


def run_case(case):
    """(nodes, edges, report, robust report, preconditioner's report, trace) of a campaign case, computed once and shared."""
    if case["name"] not in _results:
        tr = {}
        _results[case["name"]] = relax_pc(case["nodes"], case["edges"], case["par"], case["rob"], case["kind"], tr) + (tr,)
    return _results[case["name"]]
