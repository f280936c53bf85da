"""The pose graph (include/lsd_hip.h, "pose graph"; csrc/k_pgbuild.hip, csrc/k_posegraph.hip) restated on Python floats,
in the header's order, written from the header for the tests (not from the HIP code), and the generated campaign both test files run.

Python floats are IEEE doubles without contraction, so every statement below rounds as the device build (-ffp-contract=off) rounds it;
every sum runs ascending from 0.0 unless its parentheses say otherwise; sin / cos are the correctly rounded ones of oracle.lib_cr(),
which is what the device computes (grid_cases.cr()).  Where the chain runs through the grid it uses the grid's own restatements
(grid_cases, grid_match_cases, grid_response_cases).  A case class is a predicate on the restatement's own TRACE, never on what the
device gives.
"""
import math

import numpy as np

import grid_cases as gc
import grid_match_cases as gm
import grid_response_cases as gr

HEAD_DTYPE = np.dtype([("n_nodes", "i4"), ("n_edges", "i4")])
NODE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("raw", "f8", (3,)), ("flags", "u4"), ("track", "i4"), ("reserved", "u8")])
EDGE_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("flags", "u4"), ("reserved", "u4"), ("z", "f8", (3,)), ("info", "f8", (6,)), ("chi2", "f8")])
TRACK_DTYPE = np.dtype([("last", "i4"), ("reserved", "i4"), ("raw", "f8", (3,))])
APPEND_REP_DTYPE = np.dtype([("nodes", "i4"), ("edges", "i4"), ("dropped", "i4"), ("flags", "u4")])
NEAR_DTYPE = np.dtype([("anchor", "i4"), ("query", "i4"), ("n_cand", "i4"), ("reserved", "i4"), ("d2", "f8")])
CLOSURE_REP_DTYPE = np.dtype([("edge", "i4"), ("flags", "u4"), ("det", "f8")])
RELAX_REP_DTYPE = np.dtype([("chi2_before", "f8"), ("chi2_after", "f8"), ("lambda", "f8"), ("iters", "i4"), ("cg_iters", "i4"), ("accepted", "i4"),
                            ("rejected", "i4"), ("skipped_edges", "i4"), ("singular_nodes", "i4"), ("flags", "u4"), ("reserved", "u4")])
SIZES = {"lsd_pg_head": 8, "lsd_pg_node": 64, "lsd_pg_edge": 96, "lsd_pg_track": 32, "lsd_pg_append_par": 64, "lsd_pg_append_rep": 16,
         "lsd_pg_near_rec": 24, "lsd_pg_closure_par": 24, "lsd_pg_closure_rep": 16, "lsd_pg_relax_par": 56, "lsd_pg_relax_rep": 56}
NODE_FIXED = 1
EDGE_DISABLED, EDGE_CLOSURE = 1, 2
NODES_FULL, EDGES_FULL = 1, 2
APPENDED, NO_ANCHOR, NO_RESPONSE, NOT_FINITE, SINGULAR, FULL = 1, 2, 4, 8, 16, 32
CONVERGED, BREAKDOWN, RELAX_NOT_FINITE = 1, 2, 4
SHAPE = 1024                                                                  # the reduction shape
RELAX_KEYS = ("lambda0", "lambda_min", "up", "down", "cg_tol", "eps", "iters", "cg_iters")
RELAX_DEFAULTS = dict(lambda0=1e-3, lambda_min=1e-9, up=10.0, down=10.0, cg_tol=1e-8, eps=1e-9, iters=20, cg_iters=200)
INF, NAN = float("inf"), float("nan")
SENTINEL = (-1.0, 0.0, 0.0)


# ---- the shared text -------------------------------------------------------------------------------------------------------------------
def sincos_deg(a):
    th = a / 180.0 * gc.K_PI
    return gc.cr().cr_sin(th), gc.cr().cr_cos(th)


def wrap(v):
    return v - 360.0 * math.floor((v + 180.0) / 360.0)


def rel(p, q):
    s, c = sincos_deg(p[2])
    dx, dy = q[0] - p[0], q[1] - p[1]
    return (c * dx + s * dy, c * dy - s * dx, wrap(q[2] - p[2]))


def comp(p, z):
    s, c = sincos_deg(p[2])
    return (p[0] + (c * z[0] - s * z[1]), p[1] + (s * z[0] + c * z[1]), wrap(p[2] + z[2]))


def fdiv(a, b):
    """a / b as IEEE gives it (Python raises where b is zero)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def inv3(S):
    """(inverse rows or None, det) of the 3 x 3 rows S, in the cofactor form."""
    def cof(a, b):
        a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
        return S[a1][b1] * S[a2][b2] - S[a1][b2] * S[a2][b1]
    det = (cof(0, 0) * S[0][0] + cof(1, 0) * S[1][0]) + cof(2, 0) * S[2][0]
    invdet = fdiv(1.0, det)
    if not det > 0 or not math.isfinite(invdet):
        return None, det
    inv = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            inv[j][i] = cof(i, j) * invdet
    return inv, det


def dot3(u, v):
    t = 0.0
    for q in range(3):
        t += u[q] * v[q]
    return t


def reduce_shape(v):
    """The one reduction shape: partial sums of stride 1024, then the halving tree (numpy's element-wise add is IEEE's)."""
    v = np.asarray(v, np.float64)
    n = len(v)
    s = np.zeros(SHAPE)
    m = min(n, SHAPE)
    s[:m] = v[:m]
    k = SHAPE
    with np.errstate(all="ignore"):
        while k < n:
            w = min(n - k, SHAPE)
            s[:w] = s[:w] + v[k:k + w]
            k += SHAPE
        h = SHAPE // 2
        while h >= 1:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
    return float(s[0])


def pose_skipped(q):
    return (not all(math.isfinite(v) for v in q)) or abs(q[0] + 1) < 1e-4 or abs(q[0]) > 1048576.0 or abs(q[1]) > 1048576.0


def clamp(n, cap):
    return min(max(int(n), 0), int(cap))


# ---- a graph as the entries see it -----------------------------------------------------------------------------------------------------
def new_graph(nodes_cap, edges_cap, store_stride, n_tracks=1, rng=None):
    """head, nodes, edges, tracks, store, store_lens of an empty graph; with rng the unused bytes are noise the entries must keep."""
    g = dict(head=np.zeros(1, HEAD_DTYPE), nodes=np.zeros(nodes_cap, NODE_DTYPE), edges=np.zeros(edges_cap, EDGE_DTYPE),
             tracks=np.zeros(n_tracks, TRACK_DTYPE), store=np.zeros((nodes_cap, store_stride, 2)), store_lens=np.zeros(nodes_cap, np.int32))
    if rng is not None:
        g["nodes"] = rng.integers(0, 256, nodes_cap * 64, dtype=np.uint8).view(NODE_DTYPE).copy()
        g["edges"] = rng.integers(0, 256, edges_cap * 96, dtype=np.uint8).view(EDGE_DTYPE).copy()
        g["store"] = rng.normal(size=g["store"].shape)
    g["tracks"]["last"] = -1
    return g


def copy_graph(g):
    return {k: v.copy() for k, v in g.items()}


def pose_of(rec):
    return (float(rec["x"]), float(rec["y"]), float(rec["ang"]))


# ---- append ----------------------------------------------------------------------------------------------------------------------------
def append(g, scans, lens, poses, track, par, trace=None):
    """lsd_enqueue_pg_append_device on a copy of g: (the graph after, the report).  poses float64 [n, 3]; par: dict(min_dist, min_ang, info)."""
    g = copy_graph(g)
    nodes, edges, tr = g["nodes"], g["edges"], g["tracks"][track]
    nodes_cap, edges_cap, store_stride = len(nodes), len(edges), g["store"].shape[1]
    stride = scans.shape[1]
    n_nodes, n_edges = clamp(g["head"][0]["n_nodes"], nodes_cap), clamp(g["head"][0]["n_edges"], edges_cap)
    last, raw = int(tr["last"]), tuple(float(v) for v in tr["raw"])
    md, ma = float(par["min_dist"]), float(par["min_ang"])
    rep = np.zeros(1, APPEND_REP_DTYPE)[0]
    flags = 0
    for t in range(len(lens)):
        q = tuple(float(v) for v in poses[t])
        ev = dict(cand=t, what=None)
        made = -1
        if pose_skipped(q) or int(lens[t]) <= 0:
            rep["dropped"] += 1
            ev["what"] = "dropped_pose" if pose_skipped(q) else "dropped_empty"
        elif last < 0 or last >= n_nodes:
            if n_nodes == nodes_cap:
                flags |= NODES_FULL
                ev["what"] = "nodes_full"
            else:
                made = n_nodes
                nd = nodes[made]
                nd["x"], nd["y"], nd["ang"] = q
                nd["raw"] = q
                nd["flags"], nd["track"], nd["reserved"] = (NODE_FIXED if made == 0 else 0), track, 0
                ev["what"] = "first"
        else:
            z = rel(raw, q)
            d2, thr = z[0] * z[0] + z[1] * z[1], md * md
            ev.update(d2=d2, thr=thr, za=abs(z[2]), ma=ma)
            if d2 >= thr or abs(z[2]) >= ma:
                if n_nodes == nodes_cap:
                    flags |= NODES_FULL
                    ev["what"] = "nodes_full"
                elif n_edges == edges_cap:
                    flags |= EDGES_FULL
                    ev["what"] = "edges_full"
                else:
                    made = n_nodes
                    at = comp(pose_of(nodes[last]), z)
                    nd = nodes[made]
                    nd["x"], nd["y"], nd["ang"] = at
                    nd["raw"] = q
                    nd["flags"], nd["track"], nd["reserved"] = 0, track, 0
                    ed = edges[n_edges]
                    ed["i"], ed["j"], ed["flags"], ed["reserved"] = last, made, 0, 0
                    ed["z"], ed["info"], ed["chi2"] = z, par["info"], 0.0
                    n_edges += 1
                    rep["edges"] += 1
                    ev["what"] = "keyframe"
            else:
                ev["what"] = "not_keyframe"
        if made >= 0:
            n_nodes += 1
            rep["nodes"] += 1
            last, raw = made, q
            g["store_lens"][made] = min(int(lens[t]), stride, store_stride)
            w = min(stride, store_stride)
            g["store"][made, :w] = scans[t, :w]
        if trace is not None:
            trace.append(ev)
    g["head"][0]["n_nodes"], g["head"][0]["n_edges"] = n_nodes, n_edges
    tr["last"], tr["raw"] = last, raw
    rep["flags"] = flags
    return g, rep


# ---- near ------------------------------------------------------------------------------------------------------------------------------
def near(g, track, gap, radius, window, q_scan, trace=None):
    """lsd_enqueue_pg_near_device: (the record, sel float64 [nodes_cap, 3], the query's row, length and pose).  q_scan: the row as it was."""
    nodes = g["nodes"]
    nodes_cap = len(nodes)
    n_nodes, j = clamp(g["head"][0]["n_nodes"], nodes_cap), int(g["tracks"][track]["last"])
    rec = np.zeros(1, NEAR_DTYPE)[0]
    has_q = 0 <= j < n_nodes
    anchor, best, count, d2s = -1, 0.0, 0, {}
    if has_q:
        xj, yj, r2 = float(nodes[j]["x"]), float(nodes[j]["y"]), radius * radius
        for i in range(0, j - gap + 1):
            dx, dy = float(nodes[i]["x"]) - xj, float(nodes[i]["y"]) - yj
            d2 = dx * dx + dy * dy
            d2s[i] = d2
            if d2 <= r2:
                count += 1
                if anchor < 0 or d2 < best:
                    anchor, best = i, d2
    rec["anchor"], rec["query"], rec["n_cand"], rec["d2"] = anchor, j, count, best if anchor >= 0 else 0.0
    sel = np.zeros((nodes_cap, 3))
    for k in range(nodes_cap):
        sel[k] = pose_of(nodes[k]) if anchor >= 0 and abs(k - anchor) <= window and k <= j - gap else SENTINEL
    row = np.array(q_scan, np.float64)
    if has_q:
        row[:] = g["store"][j]
    q_len = int(g["store_lens"][j]) if has_q else 0
    q_pose = np.array(pose_of(nodes[j]) if anchor >= 0 else SENTINEL)
    if trace is not None:
        trace.update(j=j, gap=gap, r2=radius * radius, d2=d2s, anchor=anchor, count=count, window=window, n_nodes=n_nodes)
    return rec, sel, row, q_len, q_pose


# ---- closure ---------------------------------------------------------------------------------------------------------------------------
def closure(g, near_rec, r, par):
    """lsd_enqueue_pg_closure_device on a copy of g: (the graph after, the report).  r: one RESPONSE_DTYPE record; par: (cov_scale,
    floor_xy, floor_ang)."""
    g = copy_graph(g)
    nodes, edges = g["nodes"], g["edges"]
    n_nodes, n_edges = clamp(g["head"][0]["n_nodes"], len(nodes)), clamp(g["head"][0]["n_edges"], len(edges))
    cov_scale, floor_xy, floor_ang = (float(v) for v in par)
    anchor, query = int(near_rec["anchor"]), int(near_rec["query"])
    rep = np.zeros(1, CLOSURE_REP_DTYPE)[0]
    rep["edge"] = -1
    rf = int(r["flags"])
    z = [float(r["x"]), float(r["y"]), float(r["ang"])]
    c = [float(v) for v in r["cov"]]
    if not (0 <= anchor < n_nodes and 0 <= query < n_nodes) or anchor == query:
        rep["flags"] = NO_ANCHOR
    elif not rf & gr.VALID or rf & (gr.NONE | gr.EMPTY | gr.MISMATCH):
        rep["flags"] = NO_RESPONSE
    elif not all(math.isfinite(v) for v in z + c):
        rep["flags"] = NOT_FINITE
    else:
        R = [[c[0] * cov_scale + floor_xy, c[1] * cov_scale, c[3] * cov_scale],
             [c[1] * cov_scale, c[2] * cov_scale + floor_xy, c[4] * cov_scale],
             [c[3] * cov_scale, c[4] * cov_scale, c[5] * cov_scale + floor_ang]]
        inv, det = inv3(R)
        rep["det"] = det
        if inv is None:
            rep["flags"] = SINGULAR
        elif n_edges == len(edges):
            rep["flags"] = FULL
        else:
            pa = pose_of(nodes[anchor])
            zz = rel(pa, z)
            s, co = sincos_deg(pa[2])
            T = [[inv[q][0] * co + inv[q][1] * s, inv[q][1] * co - inv[q][0] * s, inv[q][2]] for q in range(3)]
            J = [[co * T[0][q] + s * T[1][q] for q in range(3)], [co * T[1][q] - s * T[0][q] for q in range(3)], [T[2][q] for q in range(3)]]
            ed = edges[n_edges]
            ed["i"], ed["j"], ed["flags"], ed["reserved"] = anchor, query, EDGE_CLOSURE, 0
            ed["z"], ed["chi2"] = zz, 0.0
            ed["info"] = (J[0][0], J[0][1], J[1][1], J[0][2], J[1][2], J[2][2])
            rep["edge"], rep["flags"] = n_edges, APPENDED
            g["head"][0]["n_edges"] = n_edges + 1
    return g, rep


# ---- the relaxation --------------------------------------------------------------------------------------------------------------------
def edge_error(pi, pj, z):
    s, c = sincos_deg(pi[2])
    dx, dy = pj[0] - pi[0], pj[1] - pi[1]
    return [(c * dx + s * dy) - z[0], (c * dy - s * dx) - z[1], wrap((pj[2] - pi[2]) - z[2])], s, c, dx, dy


def info_rows(info):
    return [[info[0], info[1], info[3]], [info[1], info[2], info[4]], [info[3], info[4], info[5]]]


def edge_chi2(pi, pj, z, W):
    e = edge_error(pi, pj, z)[0]
    return dot3(e, [dot3(W[r], e) for r in range(3)])


def edge_blocks(pi, pj, z, W):
    """Haa, Hab, Hbb (rows), ba, bb, chi2_e of one edge."""
    e, s, c, dx, dy = edge_error(pi, pj, z)
    k = gc.K_PI / 180.0
    A = [[-c, -s, k * (c * dy - s * dx)], [s, -c, k * ((-c) * dx - s * dy)], [0.0, 0.0, -1.0]]
    B = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]

    def mm(X, Y):                                                            # sum_t X(r,t) * Y(t,q)
        out = [[0.0] * 3 for _ in range(3)]
        for r in range(3):
            for q in range(3):
                t = 0.0
                for u in range(3):
                    t += X[r][u] * Y[u][q]
                out[r][q] = t
        return out

    def tm(X, Y):                                                            # sum_t X(t,r) * Y(t,q)
        out = [[0.0] * 3 for _ in range(3)]
        for r in range(3):
            for q in range(3):
                t = 0.0
                for u in range(3):
                    t += X[u][r] * Y[u][q]
                out[r][q] = t
        return out

    def tv(X, v):
        out = [0.0] * 3
        for r in range(3):
            t = 0.0
            for u in range(3):
                t += X[u][r] * v[u]
            out[r] = t
        return out
    WA, WB, We = mm(W, A), mm(W, B), [dot3(W[r], e) for r in range(3)]
    return tm(A, WA), tm(A, WB), tm(B, WB), tv(A, We), tv(B, We), dot3(e, We)


def relax(nodes, edges, par, trace=None):
    """lsd_enqueue_pg_relax_device on one graph: nodes NODE_DTYPE [N], edges EDGE_DTYPE [E] (the clamped counts) -> (nodes after, edges
    after, the report).  par: a dict of RELAX_KEYS.  trace: a dict that receives what classes_of reads."""
    with np.errstate(all="ignore"):
        return _relax(nodes, edges, par, trace if trace is not None else {})


def _relax(nodes, edges, par, tr):
    nodes, edges = nodes.copy(), edges.copy()
    N, E = len(nodes), len(edges)
    lam, lam_min, up, down = float(par["lambda0"]), float(par["lambda_min"]), float(par["up"]), float(par["down"])
    cg_tol, eps, iters, cg_iters = float(par["cg_tol"]), float(par["eps"]), int(par["iters"]), int(par["cg_iters"])
    P = [pose_of(n) for n in nodes]
    fixed = [bool(int(n["flags"]) & NODE_FIXED) for n in nodes]
    singular = [False] * N
    valid, why = [], []
    for e in edges:
        i, j = int(e["i"]), int(e["j"])
        w = None
        if int(e["flags"]) & EDGE_DISABLED:
            w = "disabled"
        elif i == j:
            w = "self"
        elif not (0 <= i < N and 0 <= j < N):
            w = "range"
        elif not all(math.isfinite(float(v)) for v in list(e["z"]) + list(e["info"]) + list(P[i]) + list(P[j])):
            w = "not_finite"
        valid.append(w is None)
        why.append(w)
    lists = [[] for _ in range(N)]
    for e in range(E):                                                       # ascending edge index by construction
        if valid[e]:
            lists[int(edges[e]["i"])].append((e, 0))
            lists[int(edges[e]["j"])].append((e, 1))
    ei, ej = [int(e["i"]) for e in edges], [int(e["j"]) for e in edges]
    Z = [[float(v) for v in e["z"]] for e in edges]
    W = [info_rows([float(v) for v in e["info"]]) for e in edges]

    def chi2s(poses):
        return [edge_chi2(poses[ei[e]], poses[ej[e]], Z[e], W[e]) if valid[e] else 0.0 for e in range(E)]
    ce = chi2s(P)
    chi2 = reduce_shape(ce)
    rep = np.zeros(1, RELAX_REP_DTYPE)[0]
    rep["chi2_before"] = chi2
    flags, done, cg_total, accepted, rejected = 0, 0, 0, 0, 0
    tr.update(N=N, E=E, why=why, degrees=[len(l) for l in lists], fixed=fixed, cg_ends=[], steps=[], wraps=0)
    moved = set()
    if not math.isfinite(chi2):
        flags |= RELAX_NOT_FINITE
    while not flags & RELAX_NOT_FINITE and done < iters:
        blk = [edge_blocks(P[ei[e]], P[ej[e]], Z[e], W[e]) if valid[e] else None for e in range(E)]      # 1
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
                M[n], _ = inv3(D)
                if M[n] is None:
                    singular[n] = True
        free = [not fixed[n] and not singular[n] for n in range(N)]
        zero = [0.0, 0.0, 0.0]
        dl = [list(zero) for _ in range(N)]                                  # 4
        r_ = [[-b[n][q] for q in range(3)] if free[n] else list(zero) for n in range(N)]
        z_ = [[dot3(M[n][q], r_[n]) for q in range(3)] if free[n] else list(zero) for n in range(N)]
        p_ = [list(v) for v in z_]
        rz = reduce_shape([dot3(r_[n], z_[n]) for n in range(N)])
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
                qv = [dot3([Hn[r][c] if c != r else Hn[r][r] + lam * Hn[r][r] for c in range(3)], p_[n]) for r in range(3)]
                for e, side in lists[n]:
                    hab = blk[e][1]
                    po = p_[ei[e]] if side else p_[ej[e]]
                    for r in range(3):
                        t = 0.0
                        for c in range(3):
                            t += (hab[c][r] if side else hab[r][c]) * po[c]
                        qv[r] = qv[r] + t
                q_.append(qv)
            pq = reduce_shape([dot3(p_[n], q_[n]) for n in range(N)])
            if not pq > 0:
                flags |= BREAKDOWN
                end = "breakdown"
                break
            alpha = fdiv(rz, pq)
            for n in range(N):
                if free[n]:
                    for c in range(3):
                        dl[n][c] = dl[n][c] + alpha * p_[n][c]
                        r_[n][c] = r_[n][c] - alpha * q_[n][c]
                    z_[n] = [dot3(M[n][c], r_[n]) for c in range(3)]
            rzn = reduce_shape([dot3(r_[n], z_[n]) for n in range(N)])
            beta = fdiv(rzn, rz)
            for n in range(N):
                if free[n]:
                    for c in range(3):
                        p_[n][c] = z_[n][c] + beta * p_[n][c]
            rz = rzn
            steps += 1
        cg_total += steps
        tr["cg_ends"].append(end)
        trial, maxd = [], 0.0                                                # 5
        for n in range(N):
            if free[n]:
                a = P[n][2] + dl[n][2]
                if wrap(a) != a:
                    tr["wraps"] += 1
                trial.append((P[n][0] + dl[n][0], P[n][1] + dl[n][1], wrap(a)))
                for c in range(3):
                    v = abs(dl[n][c])
                    maxd = v if v > maxd else maxd
            else:
                trial.append(P[n])
        cen = chi2s(trial)
        chi2n = reduce_shape(cen)
        done += 1
        if chi2n <= chi2:
            P, ce, chi2 = trial, cen, chi2n
            moved.update(n for n in range(N) if free[n])
            l = fdiv(lam, down)
            lam = l if l > lam_min else lam_min
            accepted += 1
            tr["steps"].append("accepted")
            if maxd < eps:
                flags |= CONVERGED
                break
        else:
            lam = lam * up
            rejected += 1
            tr["steps"].append("rejected")
    for n in sorted(moved):                                                  # every other node keeps its bytes
        nodes[n]["x"], nodes[n]["y"], nodes[n]["ang"] = P[n]
    for e in range(E):
        edges[e]["chi2"] = ce[e]
    rep["chi2_after"], rep["lambda"] = chi2, lam
    rep["iters"], rep["cg_iters"], rep["accepted"], rep["rejected"] = done, cg_total, accepted, rejected
    rep["skipped_edges"], rep["singular_nodes"], rep["flags"] = sum(1 for v in valid if not v), sum(singular), flags
    tr.update(singular=singular, flags=flags)
    return nodes, edges, rep


# ---- the independent reference: a dense Gauss-Newton on the same error model ------------------------------------------------------------
def dense_gauss_newton(nodes, edges, max_iters=100, tol=1e-12):
    """Poses float64 [N, 3] of the minimum: H assembled densely, numpy.linalg.solve, fixed nodes removed, until the step is below tol."""
    N = len(nodes)
    P = np.array([pose_of(n) for n in nodes])
    free = [n for n in range(N) if not int(nodes[n]["flags"]) & NODE_FIXED]
    idx = {n: 3 * k for k, n in enumerate(free)}
    k = math.pi / 180.0
    for _ in range(max_iters):
        H, g = np.zeros((3 * len(free), 3 * len(free))), np.zeros(3 * len(free))
        for e in edges:
            i, j = int(e["i"]), int(e["j"])
            W = np.array(info_rows([float(v) for v in e["info"]]))
            s, c = math.sin(math.radians(P[i, 2])), math.cos(math.radians(P[i, 2]))
            dx, dy = P[j, 0] - P[i, 0], P[j, 1] - P[i, 1]
            err = np.array([c * dx + s * dy - e["z"][0], -s * dx + c * dy - e["z"][1], wrap(P[j, 2] - P[i, 2] - e["z"][2])])
            A = np.array([[-c, -s, k * (-s * dx + c * dy)], [s, -c, k * (-c * dx - s * dy)], [0, 0, -1.0]])
            B = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
            for (u, Ju) in ((i, A), (j, B)):
                if u not in idx:
                    continue
                g[idx[u]:idx[u] + 3] += Ju.T @ W @ err
                for (v, Jv) in ((i, A), (j, B)):
                    if v in idx:
                        H[idx[u]:idx[u] + 3, idx[v]:idx[v] + 3] += Ju.T @ W @ Jv
        d = np.linalg.solve(H, -g)
        for n in free:
            P[n] += d[idx[n]:idx[n] + 3]
            P[n, 2] = wrap(P[n, 2])
        if np.abs(d).max() < tol:
            break
    return P


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def node(x, y, ang, flags=0, rng=None):
    n = np.zeros(1, NODE_DTYPE)[0]
    if rng is not None:                                                      # raw, track and the reserved word: bytes a relaxation must keep
        n = rng.integers(0, 256, 64, dtype=np.uint8).view(NODE_DTYPE)[0].copy()
    n["x"], n["y"], n["ang"] = x, y, ang
    n["flags"] = (int(n["flags"]) & ~NODE_FIXED & 0xFFFFFFFF) | flags if rng is not None else flags
    return n


def edge(i, j, z, info=(1.0, 0.0, 1.0, 0.0, 0.0, 1.0), flags=0):
    e = np.zeros(1, EDGE_DTYPE)[0]
    e["i"], e["j"], e["z"], e["info"], e["flags"] = i, j, z, info, flags
    e["chi2"] = -7.0                                                         # (a value the relaxation must overwrite)
    return e


def loop_graph(n, rng, radius=20.0, noise=0.05, bias=0.6, closures=1, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0), fix=(0,), noisy=False, step=None):
    """A closed loop of n poses on a circle: the nodes composed from odometry edges with noise and a heading bias of `bias` degrees per
    node, and `closures` true closure edges (one per n / closures nodes) back to the start of their stretch.  Returns (nodes, edges, truth)."""
    truth = []
    for k in range(n):
        a = 360.0 * k / n
        truth.append((40.0 + radius * math.cos(math.radians(a)), 40.0 + radius * math.sin(math.radians(a)), wrap(a + 90.0)))
    edges, poses = [], [truth[0]]
    for k in range(1, n):
        z = rel(truth[k - 1], truth[k])
        z = (z[0] + noise * rng.normal(), z[1] + noise * rng.normal(), z[2] + bias * rng.uniform(0.2, 1.0))
        edges.append(edge(k - 1, k, z, info))
        poses.append(comp(poses[-1], z))
    span = n // closures
    for c in range(closures):
        i, j = c * span, min((c + 1) * span, n) - 1
        if c == closures - 1:
            i, j = 0, n - 1
        if j - i >= 2:
            edges.append(edge(i, j, rel(truth[i], truth[j]), (25.0, 0.0, 25.0, 0.0, 0.0, 9.0), EDGE_CLOSURE))
    nodes = np.array([node(*poses[k], flags=NODE_FIXED if k in fix else 0, rng=rng if noisy else None) for k in range(n)], NODE_DTYPE)
    return nodes, np.array(edges, EDGE_DTYPE).reshape(-1), np.array(truth)


def chain_graph(n, rng, extra=0):
    """A cheap graph of n nodes for the sizes beside the reduction shape: a chain with a little noise, node 0 fixed, `extra` chords."""
    nodes = np.array([node(2.0 * k + 0.1 * rng.normal(), 0.1 * rng.normal(), 0.5 * rng.normal(), NODE_FIXED if k == 0 else 0) for k in range(n)],
                     NODE_DTYPE).reshape(-1)
    edges = [edge(k - 1, k, (2.0, 0.0, 0.0)) for k in range(1, n)]
    for _ in range(extra):
        i = int(rng.integers(0, max(n - 3, 1)))
        edges.append(edge(i, min(i + 2, n - 1), (4.0, 0.0, 0.0)))
    return nodes, np.array(edges, EDGE_DTYPE).reshape(-1)


def rcase(name, nodes, edges, **par):
    p = dict(RELAX_DEFAULTS)
    p.update(par)
    return dict(name=name, nodes=np.array(nodes, NODE_DTYPE).reshape(-1), edges=np.array(edges, EDGE_DTYPE).reshape(-1), par=p)


WELL_POSED_SIZES = (8, 24, 100)


def well_posed():
    """The class the dense reference is run on: connected loops, one fixed node, noise and a heading bias <= 0.6 deg per node, one true
    closure; cg_iters = 3 N."""
    out = []
    for n in WELL_POSED_SIZES:
        for seed in range(2):
            nodes, edges, _ = loop_graph(n, np.random.default_rng(100 * n + seed))
            out.append(rcase("well_posed_%d_%d" % (n, seed), nodes, edges, cg_iters=3 * n, iters=30, cg_tol=1e-10, eps=1e-10))
    return out


def relax_campaign():
    rng = np.random.default_rng(20261020)
    out = list(well_posed())
    quick = dict(iters=1, cg_iters=4)
    for n in (0, 1, 2, 3):
        for rep in range(3):
            nodes, edges = chain_graph(n, rng)
            out.append(rcase("n_%d_%d" % (n, rep), nodes, edges, iters=3, cg_iters=12))
    for n in (1023, 1024):
        for rep in range(3):
            nodes, edges = chain_graph(n, rng, extra=rep)
            out.append(rcase("n_%d_%d" % (n, rep), nodes, edges, **quick))
    nodes, edges = chain_graph(1025, rng)
    out.append(rcase("n_1025", nodes, edges, **quick))
    for e_count in (1023, 1024, 1025):                                       # E on and beside the boundary, on a small hub graph
        for rep in range(3):
            nodes, _ = chain_graph(40, rng)
            es = [edge(k - 1, k, (2.0, 0.0, 0.0)) for k in range(1, 40)]
            while len(es) < e_count:
                i, j = sorted(int(v) for v in rng.choice(40, 2, replace=False))
                es.append(edge(i, j, (2.0 * (j - i), 0.0, 0.0), (0.5, 0.0, 0.5, 0.0, 0.0, 0.5)))
            out.append(rcase("e_%d_%d" % (e_count, rep), nodes, es, **quick))
    for rep in range(3):                                                     # a hub of degree >= 65, a node of degree 0, descending edges
        n = 70 + rep
        nodes = [node(0.0, 0.0, 0.0, NODE_FIXED)] + [node(10.0 * math.cos(k) + 0.2 * rng.normal(), 10.0 * math.sin(k), 5.0 * rng.normal())
                                                     for k in range(1, n)]
        es = [edge(0, k, (10.0 * math.cos(k), 10.0 * math.sin(k), 0.0)) for k in range(1, n - 1)]       # node n - 1 has no edge
        es += [edge(k, 0, rel((10.0 * math.cos(k), 10.0 * math.sin(k), 0.0), (0.0, 0.0, 0.0)), (0.3, 0.1, 0.7, 0.0, 0.05, 0.2)) for k in range(1, 8)]
        es.sort(key=lambda e: max(int(e["i"]), int(e["j"])))
        out.append(rcase("hub_%d" % rep, nodes, es[::-1], iters=3, cg_iters=30))                        # descending: the ascending sum shows
    for rep in range(3):                                                     # angles at +-180, a wrap inside e and in a trial pose
        nodes = [node(0.0, 0.0, 179.5 + 0.2 * rep, NODE_FIXED), node(-2.0, 0.1, -179.8), node(-4.0, 0.0, 180.0), node(-6.0, -0.1, -180.0)]
        es = [edge(0, 1, (2.0, 0.0, 1.0)), edge(1, 2, (2.0, 0.0, 0.5)), edge(2, 3, (2.0, 0.0, -0.5)), edge(0, 3, (6.0, 0.0, 0.5))]
        out.append(rcase("wrap_%d" % rep, nodes, es, iters=6, cg_iters=30))
    for rep in range(3):
        nodes, edges, _ = loop_graph(12, rng, noisy=True)
        fixed_all, fixed_none = nodes.copy(), nodes.copy()
        fixed_all["flags"] |= NODE_FIXED
        fixed_none["flags"] &= ~np.uint32(NODE_FIXED)
        out.append(rcase("all_fixed_%d" % rep, fixed_all, edges, iters=2, cg_iters=20))
        out.append(rcase("none_fixed_%d" % rep, fixed_none, edges, iters=4, cg_iters=40))
        es = edges.copy()                                                    # the four ways an edge is skipped
        bad = [edge(3, 7, (1.0, 1.0, 1.0), flags=EDGE_DISABLED), edge(5, 5, (0.0, 0.0, 0.0)), edge(2, 12 + rep, (1.0, 0.0, 0.0)), edge(-1, 4, (1.0, 0.0, 0.0)),
               edge(1, 6, (NAN, 0.0, 0.0)), edge(2, 8, (1.0, 0.0, 0.0), (1.0, 0.0, INF, 0.0, 0.0, 1.0))]
        out.append(rcase("skipped_%d" % rep, nodes, np.concatenate([es[:4], np.array(bad, EDGE_DTYPE), es[4:]]), iters=3, cg_iters=40))
        out.append(rcase("iters_0_%d" % rep, nodes, edges, iters=0))
        out.append(rcase("cg_iters_end_%d" % rep, nodes, edges, iters=2, cg_iters=3))
        out.append(rcase("cg_tol_end_%d" % rep, nodes, edges, iters=2, cg_iters=200, cg_tol=1e-3))
        # a far start, without damping
        far = nodes.copy()
        far["ang"][1:] += 100.0 + 20.0 * rep
        far["x"][1:] += 30.0
        out.append(rcase("far_start_%d" % rep, far, edges, iters=6, cg_iters=60, lambda0=0.0, lambda_min=0.0))
        # an indefinite information: p^T A p <= 0
        neg = edges.copy()
        neg["info"][2 + rep] = (-3.0, 0.0, -3.0, 0.0, 0.0, -0.5)
        out.append(rcase("breakdown_%d" % rep, nodes, neg, iters=2, cg_iters=60))
        # a singular block: an edge without information on the heading is node 12's only edge
        sing_nodes = np.concatenate([nodes, np.array([node(50.0, 50.0, 10.0)], NODE_DTYPE)])
        sing = np.concatenate([edges, np.array([edge(rep, 12, (1.0, 2.0, 3.0), (1.0, 0.0, 1.0, 0.0, 0.0, 0.0))], EDGE_DTYPE)])
        out.append(rcase("singular_%d" % rep, sing_nodes, sing, iters=3, cg_iters=60))
        # chi2 overflows: NOT_FINITE, the poses stay
        big = edges.copy()
        big["info"][1] = (1e308, 0.0, 1e308, 0.0, 0.0, 1e308)
        big["z"][1] = (1e200, 0.0, 0.0)
        out.append(rcase("not_finite_%d" % rep, nodes, big, iters=3))
    return out


RELAX_CLASSES = (["n_%d" % n for n in (0, 1, 2, 3, 1023, 1024, 1025)] + ["e_0", "e_1023", "e_1024", "e_1025", "degree_0", "hub_65", "descending",
                 "angle_at_180", "wrap_in_e", "all_fixed", "none_fixed", "skip_disabled", "skip_self", "skip_range", "skip_not_finite",
                 "rejected_step", "cg_end_iters", "cg_end_tol", "cg_end_breakdown", "singular_block", "iters_0", "converged", "not_finite",
                 "noisy_records", "well_posed"])
ONCE = ("n_1025",)


def relax_classes_of(case, tr):
    nodes, edges = case["nodes"], case["edges"]
    c = set()
    if tr["N"] in (0, 1, 2, 3, 1023, 1024, 1025):
        c.add("n_%d" % tr["N"])
    if tr["E"] in (0, 1023, 1024, 1025):
        c.add("e_%d" % tr["E"])
    if any(d == 0 for d in tr["degrees"]):
        c.add("degree_0")
    if any(d >= 65 for d in tr["degrees"]):
        c.add("hub_65")
    far = [max(int(e["i"]), int(e["j"])) for e in edges]
    if tr["E"] >= 2 and all(far[k] >= far[k + 1] for k in range(tr["E"] - 1)) and far[0] > far[-1]:
        c.add("descending")
    if any(abs(float(a)) == 180.0 for a in nodes["ang"]):
        c.add("angle_at_180")
    for e in range(tr["E"]):
        if tr["why"][e] is None:
            v = (float(nodes["ang"][edges["j"][e]]) - float(nodes["ang"][edges["i"][e]])) - float(edges["z"][e][2])
            if wrap(v) != v:
                c.add("wrap_in_e")
    if tr["N"] and all(tr["fixed"]):
        c.add("all_fixed")
    if tr["N"] and not any(tr["fixed"]):
        c.add("none_fixed")
    for w in tr["why"]:
        if w:
            c.add("skip_" + w)
    if "rejected" in tr["steps"]:
        c.add("rejected_step")
    for end in tr["cg_ends"]:
        if end in ("iters", "tol", "breakdown"):
            c.add("cg_end_" + end)
    if any(tr["singular"][n] and tr["degrees"][n] > 0 for n in range(tr["N"])):
        c.add("singular_block")
    if case["par"]["iters"] == 0:
        c.add("iters_0")
    if tr["flags"] & CONVERGED:
        c.add("converged")
    if tr["flags"] & RELAX_NOT_FINITE:
        c.add("not_finite")
    if tr["N"] and any(int(r) != 0 for r in nodes["reserved"]):
        c.add("noisy_records")
    if case["name"].startswith("well_posed"):
        c.add("well_posed")
    return c


_relax_results = {}


def run_relax_case(case):
    """(nodes, edges, report, trace) of a campaign case, computed once and shared."""
    if case["name"] not in _relax_results:
        tr = {}
        _relax_results[case["name"]] = relax(case["nodes"], case["edges"], case["par"], tr) + (tr,)
    return _relax_results[case["name"]]


# ---- the build campaign: append, near, closure -----------------------------------------------------------------------------------------
APPEND_PAR = dict(min_dist=2.0, min_ang=10.0, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0))


def below(v):
    return math.nextafter(v, -INF)


def scans_for(rng, n, stride, lens=None):
    sc = rng.uniform(0.5, 3.0, size=(n, stride, 2))
    return sc, np.array(lens if lens is not None else [stride] * n, np.int32)


def append_campaign():
    """Cases: dict(name, graph, steps: [(scans, lens, poses, track)], par)."""
    rng = np.random.default_rng(7)
    out = []

    def case(name, poses_by_step, nodes_cap=8, edges_cap=8, stride=5, store_stride=5, lens=None, n_tracks=1, par=APPEND_PAR, noisy=True):
        g = new_graph(nodes_cap, edges_cap, store_stride, n_tracks, rng if noisy else None)
        steps = []
        for k, (poses, track) in enumerate(poses_by_step):
            sc, ln = scans_for(rng, len(poses), stride, lens[k] if lens else None)
            steps.append((sc, ln, np.array(poses, np.float64).reshape(-1, 3), track))
        out.append(dict(name=name, graph=g, steps=steps, par=par))
    for rep in range(3):
        o = 3.0 * rep
        case("first_and_motion_%d" % rep, [([(10.0 + o, 10.0, 0.0), (10.5 + o, 10.0, 1.0), (12.5 + o, 10.0, 3.0), (12.5 + o, 10.0, 14.0)], 0)])
        # exactly at and one ulp below min_dist (along x from a pose at angle 0: z.x = dx exactly) and min_ang
        case("thresholds_%d" % rep, [([(0.0, 4.0 + rep, 0.0), (below(2.0), 4.0 + rep, 0.0), (2.0, 4.0 + rep, 0.0), (2.0, 4.0 + rep, below(10.0)),
                                       (2.0, 4.0 + rep, 10.0)], 0)])
        case("sentinel_and_empty_%d" % rep, [([(5.0, 5.0, 0.0), (-1.0, 0.0, 0.0), (9.0, 5.0 + rep, 0.0), (NAN, 0.0, 0.0), (13.0, 5.0, 0.0), (2e6, 0.0, 0.0),
                                               (17.0, 5.0, 0.0)], 0)], lens=[[5, 5, 5, 5, 0, 5, 3]])
        case("nodes_full_%d" % rep, [([(3.0 * k, 1.0 * rep, 0.0) for k in range(5)], 0)], nodes_cap=3)
        case("edges_full_%d" % rep, [([(3.0 * k, 1.0 * rep, 0.0) for k in range(5)], 0)], edges_cap=2)
        case("two_tracks_%d" % rep, [([(3.0 * k, 0.0, 0.0) for k in range(3)], 0), ([(3.0 * k, 20.0 + rep, 90.0) for k in range(3)], 1),
                                      ([(9.0, 0.0, 5.0), (12.0, 0.5, 20.0)], 0)], nodes_cap=12, edges_cap=12, n_tracks=2)
        case("strides_%d" % rep, [([(3.0 * k, 0.0, 30.0 * k) for k in range(3)], 0)], stride=7, store_stride=4 + rep, lens=[[7, 2, 6]])
    return out


def run_append_case(case):
    """(graph after every step, reports, the events)."""
    g, reps, events = case["graph"], [], []
    for sc, ln, po, track in case["steps"]:
        g, rep = append(g, sc, ln, po, track, case["par"], events)
        reps.append(rep)
    return g, reps, events


APPEND_CLASSES = ("first", "keyframe", "not_keyframe", "at_min_dist", "below_min_dist", "at_min_ang", "below_min_ang", "dropped_pose",
                  "dropped_empty", "sentinel_between", "nodes_full", "edges_full", "two_tracks", "truncated_row")


def append_classes_of(case, events):
    c = set()
    for k, ev in enumerate(events):
        c.add(ev["what"])
        if "d2" in ev:
            if ev["d2"] == ev["thr"]:
                c.add("at_min_dist")
            if below(math.sqrt(ev["thr"])) ** 2 <= ev["d2"] < ev["thr"] and ev["za"] < ev["ma"]:
                c.add("below_min_dist")
            if ev["za"] == ev["ma"] and ev["d2"] < ev["thr"]:
                c.add("at_min_ang")
            if ev["za"] == below(ev["ma"]) and ev["d2"] < ev["thr"]:
                c.add("below_min_ang")
        if ev["what"] == "dropped_pose" and 0 < k < len(events) - 1 and events[k - 1]["what"] in ("first", "keyframe") and events[k + 1]["what"] == "keyframe":
            c.add("sentinel_between")
    if len({s[3] for s in case["steps"]}) > 1:
        c.add("two_tracks")
    if case["graph"]["store"].shape[1] < case["steps"][0][0].shape[1]:
        c.add("truncated_row")
    return c & set(APPEND_CLASSES)


def graph_of_poses(poses, store_stride=4, nodes_cap=None, rng=None):
    """A graph whose nodes sit at `poses` (a chain of one track), with random store rows."""
    rng = rng or np.random.default_rng(3)
    n = len(poses)
    g = new_graph(nodes_cap or n + 3, n + 3, store_stride, 1, rng)
    for k, p in enumerate(poses):
        g["nodes"][k] = node(*p, flags=NODE_FIXED if k == 0 else 0, rng=rng)
        g["store_lens"][k] = 1 + k % store_stride
        if k:
            g["edges"][k - 1] = edge(k - 1, k, rel(poses[k - 1], p))
    g["head"][0]["n_nodes"], g["head"][0]["n_edges"] = n, max(n - 1, 0)
    g["tracks"][0]["last"] = n - 1
    return g


def near_campaign():
    """Cases: dict(name, graph, gap, radius, window)."""
    out = []
    line = [(float(k), 0.0, 0.0) for k in range(10)]
    back = line[:9] + [(2.5, 0.0, 0.0)]                                      # the query between nodes 2 and 3: a tie in distance
    for rep in range(3):
        out.append(dict(name="no_candidate_%d" % rep, graph=graph_of_poses(line), gap=3, radius=(1.0, 2.0, 2.5)[rep], window=2))
        out.append(dict(name="tie_%d" % rep, graph=graph_of_poses(back), gap=3 + rep, radius=2.0, window=1))
        # node 9 - gap sits exactly at the radius: (3, 4, 5)
        far = line[:9] + [(float(6 - rep) + 3.0, 4.0, 0.0)]
        out.append(dict(name="at_gap_and_radius_%d" % rep, graph=graph_of_poses(far), gap=3 + rep, radius=5.0, window=2))
        home = line[:9] + [(0.25 * rep, 0.5, 0.0)]                           # the anchor is node 0: the window is cut by 0
        out.append(dict(name="window_cut_by_0_%d" % rep, graph=graph_of_poses(home), gap=2, radius=3.0, window=3))
        late = line[:9] + [(6.0 + 0.25 * rep, 0.5, 0.0)]                     # the anchor is j - gap: the window is cut there
        out.append(dict(name="window_cut_by_gap_%d" % rep, graph=graph_of_poses(late), gap=3, radius=3.0, window=3))
        empty = graph_of_poses(line)                                         # the track has no last node, or one past the nodes
        empty["tracks"][0]["last"] = (-1, 10, 12)[rep]
        out.append(dict(name="no_query_%d" % rep, graph=empty, gap=1, radius=3.0, window=1))
    return out


NEAR_CLASSES = ("no_candidate", "tie", "at_gap", "at_radius", "window_cut_by_0", "window_cut_by_gap", "no_query")


def run_near_case(case):
    tr = {}
    q_scan = np.full((case["graph"]["store"].shape[1], 2), 0.125)
    return near(case["graph"], 0, case["gap"], case["radius"], case["window"], q_scan, tr), tr


def near_classes_of(case, tr):
    c = set()
    if not 0 <= tr["j"] < tr["n_nodes"]:
        return {"no_query"}
    if tr["anchor"] < 0:
        c.add("no_candidate")
        return c
    best = tr["d2"][tr["anchor"]]
    if sum(1 for v in tr["d2"].values() if v == best) > 1:
        c.add("tie")
    if tr["anchor"] == tr["j"] - tr["gap"]:
        c.add("at_gap")
    if any(v == tr["r2"] for v in tr["d2"].values()):
        c.add("at_radius")
    if tr["anchor"] - tr["window"] < 0:
        c.add("window_cut_by_0")
    if tr["anchor"] + tr["window"] > tr["j"] - tr["gap"]:
        c.add("window_cut_by_gap")
    return c


def response_rec(x, y, ang, cov=(0.5, 0.1, 0.4, 0.0, 0.02, 0.3), flags=gr.VALID):
    r = np.zeros(1, gr.RESPONSE_DTYPE)[0]
    r["x"], r["y"], r["ang"], r["cov"], r["flags"] = x, y, ang, cov, flags
    return r


def closure_campaign():
    """Cases: dict(name, graph, near, resp, par), three of every outcome."""
    out = []
    sq = [(0.0, 0.0, 0.0), (5.0, 0.0, 90.0), (5.0, 5.0, 180.0), (0.2, 5.1, -91.0), (0.1, 0.3, 2.0)]
    for rep in range(3):
        g = graph_of_poses(sq)
        g["nodes"][0]["ang"] = 30.0 * rep                                    # the rotation into the anchor's frame at three angles

        def nr(anchor, query):
            r = np.zeros(1, NEAR_DTYPE)[0]
            r["anchor"], r["query"] = anchor, query
            return r
        ok = response_rec(0.05 * rep, -0.1, 1.5)
        par = (1.0 + rep, 0.25, 0.5)
        out.append(dict(name="appended_%d" % rep, graph=g, near=nr(0, 4), resp=ok, par=par))
        out.append(dict(name="no_anchor_%d" % rep, graph=g, near=nr((-1, 7, 4)[rep], 4), resp=ok, par=par))
        out.append(dict(name="no_response_%d" % rep, graph=g, near=nr(0, 4), resp=response_rec(0.0, 0.0, 0.0, flags=(0, gr.VALID | gr.EMPTY, gr.NONE)[rep]), par=par))
        bad = (response_rec(NAN, 0.0, 0.0), response_rec(0.0, 0.0, INF), response_rec(0.0, 0.0, 0.0, cov=(1.0, 0.0, NAN, 0.0, 0.0, 1.0)))[rep]
        out.append(dict(name="not_finite_%d" % rep, graph=g, near=nr(0, 4), resp=bad, par=par))
        flat = response_rec(0.0, 0.0, 0.0, cov=((0.0,) * 6, (1.0, 1.0, 1.0, 0.0, 0.0, 1.0), (1.0, 0.0, 1.0, 0.0, 0.0, -1.0))[rep])
        out.append(dict(name="singular_%d" % rep, graph=g, near=nr(0, 4), resp=flat, par=(1.0, 0.0, 0.0)))
        full = copy_graph(g)
        full["head"][0]["n_edges"] = len(full["edges"]) + (5 if rep == 2 else 0)
        out.append(dict(name="full_%d" % rep, graph=full, near=nr(0, 4), resp=ok, par=par))
    return out


CLOSURE_NAMES = {APPENDED: "appended", NO_ANCHOR: "no_anchor", NO_RESPONSE: "no_response", NOT_FINITE: "not_finite", SINGULAR: "singular", FULL: "full"}


# ---- end to end: append -> close -> relax -> rerender in the room of grid_match_cases --------------------------------------------------
E2E = dict(n=24, n_beams=90, gap=18, radius=6.0, window=2, search=gm.search(8, 8, 14, 1.0, min_beams=30, min_num=1, min_den=2),
           response=gr.params(2, 2, 1), closure=(1.0, 0.25, 0.25), append=dict(min_dist=1.0, min_ang=5.0, info=(4.0, 0.0, 4.0, 0.0, 0.0, 1.0)),
           relax=dict(RELAX_DEFAULTS, iters=12, cg_iters=75, cg_tol=1e-8))
_e2e = None


def end_to_end():
    """The chain restated once and shared: a loop of 24 keyframes of 90 beams in the room (61 x 47 cells), odometry with a heading bias;
    returns a dict with the inputs, every intermediate record and the planes of the re-rendered grid."""
    global _e2e
    if _e2e is not None:
        return _e2e
    R, n = gm.ROOM, E2E["n"]
    rng = np.random.default_rng(11)
    truth = []
    for k in range(n + 1):                                                   # one lap and a step: the last frame is back near the first
        a = 360.0 * k / n
        truth.append((30.0 + 12.0 * math.cos(math.radians(a)), 23.0 + 9.0 * math.sin(math.radians(a)), wrap(a + 90.0)))
    odom = [truth[0]]
    for k in range(1, n + 1):
        z = rel(truth[k - 1], truth[k])
        odom.append(comp(odom[-1], (z[0] + 0.02 * rng.normal(), z[1] + 0.02 * rng.normal(), z[2] + 0.6 * rng.uniform(0.5, 1.0))))
    scans = np.stack([gm.room_scan(p, E2E["n_beams"]) for p in truth])
    lens = np.full(n + 1, E2E["n_beams"], np.int32)
    g0 = new_graph(n + 4, n + 8, E2E["n_beams"])
    g1, arep = append(g0, scans, lens, np.array(odom), 0, E2E["append"])
    q_scan = np.zeros((E2E["n_beams"], 2))
    nrec, sel, row, q_len, q_pose = near(g1, 0, E2E["gap"], E2E["radius"], E2E["window"], q_scan)
    cols, rows = R["cols"], R["rows"]
    pa, hi = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g1["store"], g1["store_lens"], sel, cols, rows, R["resol"], R["range_max"], pa, hi)
    corr = gm.likelihood(pa, hi, 2, 1, 10, 3, gm.GAUSS)
    mrec = gm.match(row[None], np.array([q_len], np.int32), q_pose[None], R["resol"], R["range_max"], corr, E2E["search"])
    resp, _ = gr.response(row[None], np.array([q_len], np.int32), q_pose[None], mrec, R["resol"], R["range_max"], corr, E2E["search"]["ang_step"],
                          E2E["response"])
    g2, crep = closure(g1, nrec, resp[0], E2E["closure"])
    nn, ne = int(g2["head"][0]["n_nodes"]), int(g2["head"][0]["n_edges"])
    # chi2 of the edges before the relaxation: a call of no iterations
    _, e_before, _ = relax(g2["nodes"][:nn], g2["edges"][:ne], dict(E2E["relax"], iters=0))
    nodes, edges, rrep = relax(g2["nodes"][:nn], g2["edges"][:ne], E2E["relax"])
    g3 = copy_graph(g2)
    g3["nodes"][:nn], g3["edges"][:ne] = nodes, edges
    pa2, hi2 = np.zeros((rows, cols), np.uint32), np.zeros((rows, cols), np.uint32)
    gc.integrate(g3["store"], g3["store_lens"], np.stack([g3["nodes"]["x"], g3["nodes"]["y"], g3["nodes"]["ang"]], axis=1), cols, rows, R["resol"],
                 R["range_max"], pa2, hi2)
    _e2e = dict(truth=np.array(truth), odom=np.array(odom), scans=scans, lens=lens, g0=g0, g1=g1, append_rep=arep, near=nrec, sel=sel, q_row=row,
                q_len=q_len, q_pose=q_pose, corr=corr, match=mrec, resp=resp, g2=g2, closure_rep=crep, e_before=e_before, g3=g3, relax_rep=rrep,
                planes=(pa2, hi2), n_nodes=nn, n_edges=ne)
    return _e2e
