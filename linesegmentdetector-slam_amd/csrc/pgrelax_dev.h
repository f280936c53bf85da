// pgrelax_dev.h -- the body of the pose graph's relaxation as ONE text (include/lsd_hip.h, "pose graph", is the rule; DESIGN.md 8.1.15,
// 8.1.16, 8.1.19; restated in tests/pose_graph_cases.py, tests/pose_graph_robust_cases.py and tests/pose_graph_chain_cases.py).  k_posegraph.hip
// compiles it without and with the robust kernels, k_pgchain.hip with the block-tridiagonal preconditioner (the CHAIN section below) beside them.
// fp64 without FMA; no atomics on fp64 -- a node sums over its own list of edges in ascending edge index, and every reduction has the one
// shape of pg_reduce, which depends on the element count alone (never on kPgLanes or on where a vector lives).
//
// The workspace of a graph (pg_ws_bytes), all of it global memory: the blocks of every edge (33 doubles, one plane per entry), chi2_e at
// the poses and at the trial poses, H, M, b and the five CG vectors, the trial poses; then the words: an edge's validity, the lists
// (2 E entries, entry = 2 e + side), their offsets and fill cursors, a node's state.  The lists are built once per call: count (integer
// atomics), scan, fill 256 edges at a time -- so an entry is at most 2 x 256 places from where it belongs -- and an insertion sort per node.
//
// kRobust = false is lsd_enqueue_pg_relax_device.  kRobust = true is lsd_enqueue_pg_relax_robust_device: an edge in scope gets a weight w_e
// from its plain chi2_e at the current poses, its blocks come from w_e * W, and the objective that is accepted against is the reduction of
// rho(chi2_e); ce / cen keep the PLAIN values, so a weight costs no workspace.  valid[e] carries the scope in bit 1.  kChain = true is
// lsd_enqueue_pg_relax_pc_device with LSD_PG_PRECOND_CHAIN: z = M^-1 r comes from pg_chain_apply wherever an outer iteration's factor stands.
#pragma once
#include "lsd_internal.h"
#include "posegraph_dev.h"

namespace lsdhip {

constexpr int kPgLanes = 256, kPgShape = 1024;
constexpr int kPgFree = 0, kPgFixed = 1, kPgSingular = 2;

struct PgWs {
    double *blk, *ce, *cen, *H, *M, *b, *dl, *r, *z, *p, *q, *tp;
    int *valid, *ent, *off, *cur, *st;
};

__host__ __device__ inline size_t pg_ws_doubles(int nc, int ec) { return (size_t)35 * ec + (size_t)39 * nc; }
__host__ __device__ inline size_t pg_ws_words(int nc, int ec) { return (size_t)3 * ec + (size_t)3 * nc + 1; }
__device__ inline PgWs pg_ws_of(uint8_t* base, int nc, int ec) {
    PgWs w;
    double* d = reinterpret_cast<double*>(base);
    w.blk = d; d += (size_t)33 * ec;
    w.ce = d; d += ec;
    w.cen = d; d += ec;
    w.H = d; d += (size_t)9 * nc;
    w.M = d; d += (size_t)9 * nc;
    w.b = d; d += (size_t)3 * nc;
    w.dl = d; d += (size_t)3 * nc;
    w.r = d; d += (size_t)3 * nc;
    w.z = d; d += (size_t)3 * nc;
    w.p = d; d += (size_t)3 * nc;
    w.q = d; d += (size_t)3 * nc;
    w.tp = d; d += (size_t)3 * nc;
    int* i = reinterpret_cast<int*>(d);
    w.valid = i; i += ec;
    w.ent = i; i += (size_t)2 * ec;
    w.off = i; i += nc + 1;
    w.cur = i; i += nc;
    w.st = i;
    return w;
}

// the one reduction shape (the header's REDUCTIONS): s has kPgShape doubles of LDS; every lane gets the result
template <class V>
__device__ inline double pg_reduce(int n, V v, double* s) {
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < kPgShape; t += kPgLanes) {
        double a = 0.0;
        if (t < n) {
            a = v(t);
            for (int k = t + kPgShape; k < n; k += kPgShape) a = a + v(k);
        }
        s[t] = a;
    }
    __syncthreads();
    for (int h = kPgShape / 2; h >= 1; h >>= 1) {
        for (int t = tid; t < h; t += kPgLanes) s[t] = s[t] + s[t + h];
        __syncthreads();
    }
    const double res = s[0];
    __syncthreads();
    return res;
}

__device__ inline double pg_dot3(const double* u, const double* v) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 3; q++) t += u[q] * v[q];
    return t;
}

// the robust kernels (the header's rule): w and rho of an edge whose plain chi2_e is s; in: the edge is in scope
__device__ inline void pg_weight(const lsd_pg_robust_par& rp, bool in, double s, double& w, double& rho) {
    w = 1.0;
    rho = s;
    if (!in || rp.kernel == LSD_PG_KERNEL_NONE) return;
    const double c = rp.delta * rp.delta;
    if (rp.kernel == LSD_PG_KERNEL_HUBER) {
        if (s <= c) return;
        const double r = s != s ? s : sqrt(s);      // (IEEE: the square root of a NaN is that NaN)
        w = rp.delta / r;
        rho = (2.0 * rp.delta) * r - c;
    } else {
        const double t = c / (c + s);
        w = t * t;
        rho = (c * s) / (c + s);
    }
}

__device__ inline double pg_rho(const lsd_pg_robust_par& rp, int valid, double s) {
    double w, rho;
    pg_weight(rp, (valid & 2) != 0, s, w, rho);
    return rho;
}

// the error of an edge at the poses pi, pj, and (s, c) of pi's angle, dx, dy for the blocks
__device__ inline void pg_error(const PgPose& pi, const PgPose& pj, const double* z, double* e, double& s, double& c, double& dx, double& dy) {
    sincos_g(deg2rad_ref(pi.a), s, c);
    dx = pj.x - pi.x;
    dy = pj.y - pi.y;
    e[0] = (c * dx + s * dy) - z[0];
    e[1] = (c * dy - s * dx) - z[1];
    e[2] = pg_wrap((pj.a - pi.a) - z[2]);
}

__device__ inline void pg_info(const lsd_pg_edge& ed, double* W) {
    W[0] = ed.info[0]; W[1] = ed.info[1]; W[2] = ed.info[3];
    W[3] = ed.info[1]; W[4] = ed.info[2]; W[5] = ed.info[4];
    W[6] = ed.info[3]; W[7] = ed.info[4]; W[8] = ed.info[5];
}

__device__ inline PgPose pg_pose_of(const lsd_pg_node& n) { return PgPose{n.x, n.y, n.ang}; }

// chi2_e of every edge into out[], at the nodes' poses (trial == nullptr) or at the trial poses; with blocks: the blocks too
template <bool kRobust>
__device__ inline void pg_edges(const lsd_pg_node* nodes, const lsd_pg_edge* edges, int E, int ec, const PgWs& w, const double* trial, double* out,
                                bool blocks, const lsd_pg_robust_par& rp) {
    for (int e = (int)threadIdx.x; e < E; e += kPgLanes) {
        const int vl = w.valid[e];
        if (!vl) { out[e] = 0.0; continue; }
        const lsd_pg_edge ed = edges[e];
        PgPose pi, pj;
        if (trial) {
            pi = PgPose{trial[3 * ed.i], trial[3 * ed.i + 1], trial[3 * ed.i + 2]};
            pj = PgPose{trial[3 * ed.j], trial[3 * ed.j + 1], trial[3 * ed.j + 2]};
        } else {
            pi = pg_pose_of(nodes[ed.i]);
            pj = pg_pose_of(nodes[ed.j]);
        }
        double er[3], s, c, dx, dy, W[9], We[3];
        pg_error(pi, pj, ed.z, er, s, c, dx, dy);
        pg_info(ed, W);
#pragma unroll
        for (int r = 0; r < 3; r++) We[r] = pg_dot3(W + 3 * r, er);
        const double ce = pg_dot3(er, We);
        out[e] = ce;
        if (!blocks) continue;
        if constexpr (kRobust) {                                                                     // W' = w_e * W, We from W'
            double we, rho;
            pg_weight(rp, (vl & 2) != 0, ce, we, rho);
#pragma unroll
            for (int q = 0; q < 9; q++) W[q] = we * W[q];
#pragma unroll
            for (int r = 0; r < 3; r++) We[r] = pg_dot3(W + 3 * r, er);
        }
        const double k = kPi / 180.0;
        const double A[9] = {-c, -s, k * (c * dy - s * dx), s, -c, k * ((-c) * dx - s * dy), 0.0, 0.0, -1.0};
        const double B[9] = {c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0};
        double WA[9], WB[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double ta = 0.0, tb = 0.0;
#pragma unroll
                for (int t = 0; t < 3; t++) { ta += W[3 * r + t] * A[3 * t + q]; tb += W[3 * r + t] * B[3 * t + q]; }
                WA[3 * r + q] = ta;
                WB[3 * r + q] = tb;
            }
        double* o = w.blk + e;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double haa = 0.0, hab = 0.0, hbb = 0.0;
#pragma unroll
                for (int t = 0; t < 3; t++) {
                    haa += A[3 * t + r] * WA[3 * t + q];
                    hab += A[3 * t + r] * WB[3 * t + q];
                    hbb += B[3 * t + r] * WB[3 * t + q];
                }
                o[(size_t)(3 * r + q) * ec] = haa;
                o[(size_t)(9 + 3 * r + q) * ec] = hab;
                o[(size_t)(18 + 3 * r + q) * ec] = hbb;
            }
            double ba = 0.0, bb = 0.0;
#pragma unroll
            for (int t = 0; t < 3; t++) { ba += A[3 * t + r] * We[t]; bb += B[3 * t + r] * We[t]; }
            o[(size_t)(27 + r) * ec] = ba;
            o[(size_t)(30 + r) * ec] = bb;
        }
    }
    __syncthreads();
}

// ---- CHAIN: the block-tridiagonal preconditioner (the header's rule at lsd_enqueue_pg_relax_pc_device) ----------------
// Behind the workspace of pg_ws_bytes: five planes of 9 doubles per position -- P (Dg until a position is eliminated), Cc (the current
// coupling (t, t + s); an eliminated position's R stays there), GL, GU, Ls (L as it was when t was eliminated) --, y and x, then the
// words: node(t), the chain edge behind a position (2 e + side, -1 without one) and four planes the set-up works in.
struct PgChainWs {
    double *P, *Cc, *GL, *GU, *Ls, *y, *x;
    int *nd, *ce, *wa, *wb, *wc, *wd;
};

__host__ __device__ inline size_t pg_chain_ws_bytes(int nc) {
    const size_t b = (size_t)51 * nc * 8 + (size_t)6 * nc * 4;
    return (b + 255) & ~(size_t)255;
}

__device__ inline PgChainWs pg_chain_ws_of(uint8_t* base, int nc) {
    PgChainWs c;
    double* d = reinterpret_cast<double*>(base);
    c.P = d; d += (size_t)9 * nc;
    c.Cc = d; d += (size_t)9 * nc;
    c.GL = d; d += (size_t)9 * nc;
    c.GU = d; d += (size_t)9 * nc;
    c.Ls = d; d += (size_t)9 * nc;
    c.y = d; d += (size_t)3 * nc;
    c.x = d; d += (size_t)3 * nc;
    int* i = reinterpret_cast<int*>(d);
    c.nd = i; i += nc;
    c.ce = i; i += nc;
    c.wa = i; i += nc;
    c.wb = i; i += nc;
    c.wc = i; i += nc;
    c.wd = i;
    return c;
}

// out(r,q) = sum_t X(r,t) * Y(t,q), X and Y row major; kTx: X(t,r) in the place of X(r,t); kTy: Y(q,t) in the place of Y(t,q)
template <bool kTx, bool kTy>
__device__ __forceinline__ void pg_mm3(const double* X, const double* Y, double* out) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            double t = 0.0;
#pragma unroll
            for (int u = 0; u < 3; u++) t += (kTx ? X[3 * u + r] : X[3 * r + u]) * (kTy ? Y[3 * q + u] : Y[3 * u + q]);
            out[3 * r + q] = t;
        }
}

// v(r) = v(r) - sum_q X(r,q) * u(q)   (kT: X(q,r))
template <bool kT>
__device__ __forceinline__ void pg_mv3_sub(const double* X, const double* u, double* v) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 3; q++) t += (kT ? X[3 * q + r] : X[3 * r + q]) * u[q];
        v[r] = v[r] - t;
    }
}

// The chain edges, the paths and the positions, once per call (integers only).  rep3: chain edges, paths, the longest path's nodes.
__device__ inline void pg_chain_setup(const lsd_pg_edge* edges, int N, int E, const int* valid, const PgChainWs& c, int* s_cnt, int* rep3) {
    __shared__ int s_ch[3];
    const int tid = (int)threadIdx.x;
    constexpr int kNone = 0x7fffffff;
    if (tid < 3) s_ch[tid] = 0;
    for (int n = tid; n < N; n += kPgLanes) { c.wa[n] = kNone; c.wb[n] = kNone; }                     // up, down
    __syncthreads();
    for (int e = tid; e < E; e += kPgLanes) {
        if (!(valid[e] & 1) || (edges[e].flags & LSD_PG_EDGE_CLOSURE)) continue;
        atomicMin(&c.wa[min(edges[e].i, edges[e].j)], e);
        atomicMin(&c.wb[max(edges[e].i, edges[e].j)], e);
    }
    __syncthreads();
    int n_ch = 0, n_paths = 0;
    for (int n = tid; n < N; n += kPgLanes) {                                                         // wd: the chain edge upwards; wc: the node before
        const int e = c.wa[n], f = c.wb[n];
        const bool up_ok = e != kNone && c.wb[max(edges[e].i, edges[e].j)] == e;
        const bool dn_ok = f != kNone && c.wa[min(edges[f].i, edges[f].j)] == f;
        c.wd[n] = up_ok ? e : -1;
        c.wc[n] = dn_ok ? min(edges[f].i, edges[f].j) : -1;
        n_ch += up_ok;
        n_paths += !dn_ok;
    }
    if (n_ch) atomicAdd(&s_ch[0], n_ch);
    if (n_paths) atomicAdd(&s_ch[1], n_paths);
    __syncthreads();
    // pointer doubling towards the head: a word is (the node pointed at) | (the distance to it) << 14, both below 16384
    int *src = c.wa, *dst = c.wb;
    for (int n = tid; n < N; n += kPgLanes) {
        const int before = c.wc[n];
        src[n] = before >= 0 ? (before | (1 << 14)) : n;
        c.wc[n] = 0;                                                                                  // from here: nodes per head
    }
    __syncthreads();
    for (int k = 1; k < N; k <<= 1) {
        for (int n = tid; n < N; n += kPgLanes) {
            const int v = src[n], u = src[v & 0x3fff];
            dst[n] = (u & 0x3fff) | (((v >> 14) + (u >> 14)) << 14);
        }
        __syncthreads();
        int* t = src; src = dst; dst = t;
    }
    int longest = 0;
    for (int n = tid; n < N; n += kPgLanes) {
        atomicAdd(&c.wc[src[n] & 0x3fff], 1);
        longest = max(longest, (src[n] >> 14) + 1);
    }
    if (longest) atomicMax(&s_ch[2], longest);
    __syncthreads();
    {   // where a head's path begins: the nodes of the heads in front of it (the offsets' scan of the lists)
        const int run = (N + kPgLanes - 1) / kPgLanes, lo = min(tid * run, N), hi = min(lo + run, N);
        int sum = 0;
        for (int n = lo; n < hi; n++) sum += c.wc[n];
        s_cnt[tid] = sum;
        __syncthreads();
        int at = 0;
        for (int t = 0; t < tid; t++) at += s_cnt[t];
        for (int n = lo; n < hi; n++) { const int d = c.wc[n]; c.wc[n] = at; at += d; }
        __syncthreads();
    }
    for (int n = tid; n < N; n += kPgLanes) {
        c.nd[c.wc[src[n] & 0x3fff] + (src[n] >> 14)] = n;
    }
    __syncthreads();
    for (int t = tid; t < N; t += kPgLanes) {
        const int n = c.nd[t], e = c.wd[n];
        c.ce[t] = (e >= 0 && t + 1 < N) ? 2 * e + (edges[e].i == n ? 0 : 1) : -1;                     // (node(t + 1) is the other end: ranks ascend)
    }
    __syncthreads();
    rep3[0] = s_ch[0]; rep3[1] = s_ch[1]; rep3[2] = s_ch[2];
    __syncthreads();
}

// Dg, C and the factor of one outer iteration; false where an inv3 fails (every lane gets the answer).  s_fail is stored plainly by every
// lane whose inv3 fails -- all of them store the same 1 -- and only in the first half of a level; it is read behind that half's barrier, so
// every lane sees one value and the levels behind a failure, whose result nobody reads, are left out.
__device__ inline bool pg_chain_factor(const PgWs& w, const PgChainWs& c, int N, int ec, double lambda) {
    __shared__ int s_fail;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_fail = 0;
    for (int t = tid; t < N; t += kPgLanes) {
        const int n = c.nd[t];
        const bool fr = w.st[n] == kPgFree;
        double* Dg = c.P + 9 * t;
#pragma unroll
        for (int q = 0; q < 9; q++) Dg[q] = fr ? w.H[9 * n + q] : 0.0;
#pragma unroll
        for (int q = 0; q < 3; q++) Dg[4 * q] = fr ? w.H[9 * n + 4 * q] + lambda * w.H[9 * n + 4 * q] : 1.0;
        if (t + 1 >= N) continue;
        const int en = c.ce[t];
        const bool on = en >= 0 && fr && w.st[c.nd[t + 1]] == kPgFree;
        const double* o = w.blk + (en >= 0 ? en >> 1 : 0) + (size_t)9 * ec;
        const int side = en & 1;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) c.Cc[9 * t + 3 * r + q] = on ? o[(size_t)(side ? 3 * q + r : 3 * r + q) * ec] : 0.0;
    }
    __syncthreads();
    for (int s = 1; s < N; s <<= 1) {
        for (int t = s + 2 * s * tid; t < N; t += 2 * s * kPgLanes) {                                 // the eliminated positions
            double Dg[9], P[9], L[9], G[9], det;
#pragma unroll
            for (int q = 0; q < 9; q++) { Dg[q] = c.P[9 * t + q]; L[q] = c.Cc[9 * (t - s) + q]; }
            if (!pg_inv3(Dg, P, det)) {
                s_fail = 1;
#pragma unroll
                for (int q = 0; q < 9; q++) P[q] = 0.0;
            }
            pg_mm3<false, false>(L, P, G);
#pragma unroll
            for (int q = 0; q < 9; q++) { c.P[9 * t + q] = P[q]; c.Ls[9 * t + q] = L[q]; c.GL[9 * t + q] = G[q]; }
            if (t + s < N) {
                pg_mm3<true, false>(c.Cc + 9 * t, P, G);
#pragma unroll
                for (int q = 0; q < 9; q++) c.GU[9 * t + q] = G[q];
            }
        }
        __syncthreads();
        if (s_fail) break;                                                                            // (uniform: nobody stores before the next barrier)
        for (int u = 2 * s * tid; u < N; u += 2 * s * kPgLanes) {                                     // the positions that stay: the lower side first
            double Dg[9], T[9];
#pragma unroll
            for (int q = 0; q < 9; q++) Dg[q] = c.P[9 * u + q];
            if (u >= s) {
                pg_mm3<false, false>(c.GU + 9 * (u - s), c.Cc + 9 * (u - s), T);
#pragma unroll
                for (int q = 0; q < 9; q++) Dg[q] = Dg[q] - T[q];
            }
            if (u + s < N) {
                pg_mm3<false, true>(c.GL + 9 * (u + s), c.Ls + 9 * (u + s), T);
#pragma unroll
                for (int q = 0; q < 9; q++) Dg[q] = Dg[q] - T[q];
                if (u + 2 * s < N) {
                    pg_mm3<false, false>(c.GL + 9 * (u + s), c.Cc + 9 * (u + s), T);
#pragma unroll
                    for (int q = 0; q < 9; q++) c.Cc[9 * u + q] = -T[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 9; q++) c.P[9 * u + q] = Dg[q];
        }
        __syncthreads();
    }
    if (tid == 0 && N > 0 && !s_fail) {
        double Dg[9], P[9], det;
#pragma unroll
        for (int q = 0; q < 9; q++) Dg[q] = c.P[q];
        if (!pg_inv3(Dg, P, det)) {
            s_fail = 1;
#pragma unroll
            for (int q = 0; q < 9; q++) P[q] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < 9; q++) c.P[q] = P[q];
    }
    __syncthreads();
    const bool ok = s_fail == 0;
    __syncthreads();
    return ok;
}

// z = M^-1 r: w.z at every node from w.r (x at the free nodes, +0.0 elsewhere)
__device__ inline void pg_chain_apply(const PgWs& w, const PgChainWs& c, int N) {
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < N; t += kPgLanes) {
        const int n = c.nd[t];
#pragma unroll
        for (int q = 0; q < 3; q++) c.y[3 * t + q] = w.r[3 * n + q];
    }
    __syncthreads();
    int top = 0;
    for (int s = 1; s < N; s <<= 1) {
        for (int u = 2 * s * tid; u < N; u += 2 * s * kPgLanes) {
            double v[3] = {c.y[3 * u], c.y[3 * u + 1], c.y[3 * u + 2]};
            if (u >= s) pg_mv3_sub<false>(c.GU + 9 * (u - s), c.y + 3 * (u - s), v);
            if (u + s < N) pg_mv3_sub<false>(c.GL + 9 * (u + s), c.y + 3 * (u + s), v);
#pragma unroll
            for (int q = 0; q < 3; q++) c.y[3 * u + q] = v[q];
        }
        __syncthreads();
        top = s;
    }
    if (tid == 0 && N > 0) {
        const int n = c.nd[0];
        const bool fr = w.st[n] == kPgFree;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double xv = pg_dot3(c.P + 3 * q, c.y);
            c.x[q] = xv;
            w.z[3 * n + q] = fr ? xv : 0.0;
        }
    }
    __syncthreads();
    for (int s = top; s >= 1; s >>= 1) {
        for (int t = s + 2 * s * tid; t < N; t += 2 * s * kPgLanes) {
            double v[3] = {c.y[3 * t], c.y[3 * t + 1], c.y[3 * t + 2]};
            pg_mv3_sub<true>(c.Ls + 9 * t, c.x + 3 * (t - s), v);
            if (t + s < N) pg_mv3_sub<false>(c.Cc + 9 * t, c.x + 3 * (t + s), v);
            const int n = c.nd[t];
            const bool fr = w.st[n] == kPgFree;
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const double xv = pg_dot3(c.P + 9 * t + 3 * q, v);
                c.x[3 * t + q] = xv;
                w.z[3 * n + q] = fr ? xv : 0.0;
            }
        }
        __syncthreads();
    }
}

template <bool kRobust, bool kChain>
__device__ __forceinline__ void pg_relax_body(const lsd_pg_head* heads, lsd_pg_node* all_nodes, int nc, lsd_pg_edge* all_edges, int ec,
                                              const lsd_pg_relax_par& par, uint8_t* ws_all, size_t ws_bytes, lsd_pg_relax_rep* reps,
                                              const lsd_pg_robust_par& rp, lsd_pg_robust_rep* rob_reps, lsd_pg_precond_rep* pc_reps) {
    __shared__ double s_red[kPgShape];
    __shared__ int s_cnt[kPgLanes];
    __shared__ int s_int[kRobust ? 3 : 2];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    lsd_pg_node* nodes = all_nodes + (size_t)g * nc;
    lsd_pg_edge* edges = all_edges + (size_t)g * ec;
    const PgWs w = pg_ws_of(ws_all + (size_t)g * ws_bytes, nc, ec);
    PgChainWs cw{};                                                                                   // (kChain: behind the workspace of pg_ws_bytes)
    if constexpr (kChain) cw = pg_chain_ws_of(ws_all + (size_t)g * ws_bytes + (ws_bytes - pg_chain_ws_bytes(nc)), nc);
    const int N = min(max(heads[g].n_nodes, 0), nc), E = min(max(heads[g].n_edges, 0), ec);

    // --- the edges that count, the nodes' states, the lists -----------------------------------------------------------------------------
    if (tid < (kRobust ? 3 : 2)) s_int[tid] = 0;
    for (int n = tid; n < N; n += kPgLanes) {
        w.cur[n] = 0;
        w.st[n] = (nodes[n].flags & LSD_PG_NODE_FIXED) ? kPgFixed : kPgFree;
    }
    __syncthreads();
    int skipped = 0;
    for (int e = tid; e < E; e += kPgLanes) {
        const lsd_pg_edge ed = edges[e];
        bool ok = !(ed.flags & LSD_PG_EDGE_DISABLED) && ed.i != ed.j && ed.i >= 0 && ed.i < N && ed.j >= 0 && ed.j < N;
#pragma unroll
        for (int q = 0; q < 3; q++) ok = ok && isfinite(ed.z[q]);
#pragma unroll
        for (int q = 0; q < 6; q++) ok = ok && isfinite(ed.info[q]);
        if (ok) {
            const lsd_pg_node &a = nodes[ed.i], &b = nodes[ed.j];
            ok = isfinite(a.x) && isfinite(a.y) && isfinite(a.ang) && isfinite(b.x) && isfinite(b.y) && isfinite(b.ang);
        }
        if constexpr (kRobust) w.valid[e] = ok ? ((rp.scope == LSD_PG_ROBUST_ALL || (ed.flags & LSD_PG_EDGE_CLOSURE)) ? 3 : 1) : 0;
        else w.valid[e] = ok ? 1 : 0;
        if (ok) { atomicAdd(&w.cur[ed.i], 1); atomicAdd(&w.cur[ed.j], 1); }
        else skipped++;
    }
    if (skipped) atomicAdd(&s_int[0], skipped);
    __syncthreads();
    {   // offsets: a lane sums a run of nodes, the runs in front of it, then hands its nodes their starts; the cursors start there
        const int run = (N + kPgLanes - 1) / kPgLanes, lo = min(tid * run, N), hi = min(lo + run, N);
        int sum = 0;
        for (int n = lo; n < hi; n++) sum += w.cur[n];
        s_cnt[tid] = sum;
        __syncthreads();
        int at = 0;
        for (int t = 0; t < tid; t++) at += s_cnt[t];
        for (int n = lo; n < hi; n++) { const int d = w.cur[n]; w.off[n] = at; w.cur[n] = at; at += d; }
        if (tid == kPgLanes - 1) w.off[N] = at;
        __syncthreads();
    }
    for (int e0 = 0; e0 < E; e0 += kPgLanes) {
        const int e = e0 + tid;
        if (e < E && w.valid[e]) {
            w.ent[atomicAdd(&w.cur[edges[e].i], 1)] = 2 * e;
            w.ent[atomicAdd(&w.cur[edges[e].j], 1)] = 2 * e + 1;
        }
        __syncthreads();
    }
    for (int n = tid; n < N; n += kPgLanes) {
        const int lo = w.off[n], hi = w.off[n + 1];
        for (int m = lo + 1; m < hi; m++) {
            const int v = w.ent[m];
            int k = m;
            while (k > lo && w.ent[k - 1] > v) { w.ent[k] = w.ent[k - 1]; k--; }
            w.ent[k] = v;
        }
    }
    __syncthreads();
    int chain_rep[3] = {0, 0, 0}, fallbacks = 0;
    if constexpr (kChain) pg_chain_setup(edges, N, E, w.valid, cw, s_cnt, chain_rep);

    // --- chi2 at the poses ------------------------------------------------------------------------------------------------------------------
    // (kRobust: chi2 is the objective F, the reduction of rho; ce and cen hold the plain chi2_e)
    auto objective = [&](const double* v) {
        if constexpr (kRobust) return pg_reduce(E, [&](int e) { return pg_rho(rp, w.valid[e], v[e]); }, s_red);
        else return pg_reduce(E, [&](int e) { return v[e]; }, s_red);
    };
    pg_edges<kRobust>(nodes, edges, E, ec, w, nullptr, w.ce, false, rp);
    double chi2 = objective(w.ce);
    const double chi2_before = chi2;
    double lambda = par.lambda0;
    int done = 0, cg_total = 0, accepted = 0, rejected = 0;
    uint32_t flags = 0;
    if (!isfinite(chi2)) flags |= LSD_PG_RELAX_NOT_FINITE;

    while (!(flags & LSD_PG_RELAX_NOT_FINITE) && done < par.iters) {
        pg_edges<kRobust>(nodes, edges, E, ec, w, nullptr, w.ce, true, rp);                           // 1
        for (int n = tid; n < N; n += kPgLanes) {                                                     // 2, 3
            double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
            for (int m = w.off[n]; m < w.off[n + 1]; m++) {
                const int en = w.ent[m], e = en >> 1, side = en & 1;
                const double* o = w.blk + e;
#pragma unroll
                for (int q = 0; q < 9; q++) H[q] += o[(size_t)((side ? 18 : 0) + q) * ec];
#pragma unroll
                for (int q = 0; q < 3; q++) b[q] += o[(size_t)((side ? 30 : 27) + q) * ec];
            }
#pragma unroll
            for (int q = 0; q < 9; q++) w.H[9 * n + q] = H[q];
#pragma unroll
            for (int q = 0; q < 3; q++) w.b[3 * n + q] = b[q];
            if (w.st[n] == kPgFree) {
                double D[9], M[9], det;
#pragma unroll
                for (int q = 0; q < 9; q++) D[q] = H[q];
#pragma unroll
                for (int q = 0; q < 3; q++) D[4 * q] = H[4 * q] + lambda * H[4 * q];
                if (pg_inv3(D, M, det)) {
#pragma unroll
                    for (int q = 0; q < 9; q++) w.M[9 * n + q] = M[q];
                } else w.st[n] = kPgSingular;
            }
            const bool fr = w.st[n] == kPgFree;                                                        // 4: the start
#pragma unroll
            for (int q = 0; q < 3; q++) {
                w.dl[3 * n + q] = 0.0;
                w.r[3 * n + q] = fr ? -b[q] : 0.0;
            }
            double z[3] = {0.0, 0.0, 0.0};
            if (fr) {
                const double rn[3] = {-b[0], -b[1], -b[2]};
#pragma unroll
                for (int q = 0; q < 3; q++) z[q] = pg_dot3(w.M + 9 * n + 3 * q, rn);
            }
#pragma unroll
            for (int q = 0; q < 3; q++) { w.z[3 * n + q] = z[q]; w.p[3 * n + q] = z[q]; }
        }
        __syncthreads();
        bool jacobi = true;                                                                           // z_n = M_n r_n, or the chain's z = M^-1 r
        if constexpr (kChain) {
            jacobi = !pg_chain_factor(w, cw, N, ec, lambda);
            if (jacobi) fallbacks++;
            else {
                pg_chain_apply(w, cw, N);
                for (int n = tid; n < N; n += kPgLanes)
#pragma unroll
                    for (int q = 0; q < 3; q++) w.p[3 * n + q] = w.z[3 * n + q];
                __syncthreads();
            }
        }
        double rz = pg_reduce(N, [&](int n) { return pg_dot3(w.r + 3 * n, w.z + 3 * n); }, s_red);
        const double thr = (par.cg_tol * par.cg_tol) * rz;
        int steps = 0;
        while (steps < par.cg_iters && !(rz <= thr)) {
            for (int n = tid; n < N; n += kPgLanes) {
                double qv[3] = {0.0, 0.0, 0.0};
                if (w.st[n] == kPgFree) {
                    const double* H = w.H + 9 * n;
                    const double* pn = w.p + 3 * n;
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        double t = 0.0;
#pragma unroll
                        for (int q = 0; q < 3; q++) t += (q == r ? H[4 * r] + lambda * H[4 * r] : H[3 * r + q]) * pn[q];
                        qv[r] = t;
                    }
                    for (int m = w.off[n]; m < w.off[n + 1]; m++) {
                        const int en = w.ent[m], e = en >> 1, side = en & 1;
                        const double* o = w.blk + e + (size_t)9 * ec;
                        const double* po = w.p + 3 * (side ? edges[e].i : edges[e].j);
                        double hb[9], pv[3];                                                      // (all twelve loads in front of the sums)
#pragma unroll
                        for (int q = 0; q < 9; q++) hb[q] = o[(size_t)q * ec];
#pragma unroll
                        for (int q = 0; q < 3; q++) pv[q] = po[q];
#pragma unroll
                        for (int r = 0; r < 3; r++) {
                            double t = 0.0;
#pragma unroll
                            for (int q = 0; q < 3; q++) t += hb[side ? 3 * q + r : 3 * r + q] * pv[q];
                            qv[r] = qv[r] + t;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 3; q++) w.q[3 * n + q] = qv[q];
            }
            __syncthreads();
            const double pq = pg_reduce(N, [&](int n) { return pg_dot3(w.p + 3 * n, w.q + 3 * n); }, s_red);
            if (!(pq > 0)) { flags |= LSD_PG_RELAX_BREAKDOWN; break; }
            const double alpha = rz / pq;
            for (int n = tid; n < N; n += kPgLanes) {
                if (w.st[n] != kPgFree) continue;
                double rn[3];
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    w.dl[3 * n + q] = w.dl[3 * n + q] + alpha * w.p[3 * n + q];
                    rn[q] = w.r[3 * n + q] - alpha * w.q[3 * n + q];
                    w.r[3 * n + q] = rn[q];
                }
                if (jacobi) {
#pragma unroll
                    for (int q = 0; q < 3; q++) w.z[3 * n + q] = pg_dot3(w.M + 9 * n + 3 * q, rn);
                }
            }
            __syncthreads();
            if constexpr (kChain) {
                if (!jacobi) pg_chain_apply(w, cw, N);
            }
            const double rzn = pg_reduce(N, [&](int n) { return pg_dot3(w.r + 3 * n, w.z + 3 * n); }, s_red);
            const double beta = rzn / rz;
            for (int n = tid; n < N; n += kPgLanes) {
                if (w.st[n] != kPgFree) continue;
#pragma unroll
                for (int q = 0; q < 3; q++) w.p[3 * n + q] = w.z[3 * n + q] + beta * w.p[3 * n + q];
            }
            __syncthreads();
            rz = rzn;
            steps++;
        }
        cg_total += steps;
        double mine = 0.0;                                                                            // 5
        for (int n = tid; n < N; n += kPgLanes) {
            const lsd_pg_node& nd = nodes[n];
            if (w.st[n] == kPgFree) {
                const double* d = w.dl + 3 * n;
                w.tp[3 * n] = nd.x + d[0];
                w.tp[3 * n + 1] = nd.y + d[1];
                w.tp[3 * n + 2] = pg_wrap(nd.ang + d[2]);
#pragma unroll
                for (int q = 0; q < 3; q++) { const double a = fabs(d[q]); mine = a > mine ? a : mine; }
            } else { w.tp[3 * n] = nd.x; w.tp[3 * n + 1] = nd.y; w.tp[3 * n + 2] = nd.ang; }
        }
        s_red[tid] = mine;
        __syncthreads();
        double maxd = 0.0;
        for (int t = 0; t < kPgLanes; t++) maxd = s_red[t] > maxd ? s_red[t] : maxd;
        __syncthreads();
        pg_edges<kRobust>(nodes, edges, E, ec, w, w.tp, w.cen, false, rp);
        const double chi2n = objective(w.cen);
        done++;
        if (chi2n <= chi2) {
            for (int n = tid; n < N; n += kPgLanes) {
                if (w.st[n] != kPgFree) continue;
                nodes[n].x = w.tp[3 * n]; nodes[n].y = w.tp[3 * n + 1]; nodes[n].ang = w.tp[3 * n + 2];
            }
            for (int e = tid; e < E; e += kPgLanes) w.ce[e] = w.cen[e];
            __syncthreads();
            chi2 = chi2n;
            const double l = lambda / par.down;
            lambda = l > par.lambda_min ? l : par.lambda_min;
            accepted++;
            if (maxd < par.eps) { flags |= LSD_PG_RELAX_CONVERGED; break; }
        } else {
            lambda = lambda * par.up;
            rejected++;
        }
    }

    for (int e = tid; e < E; e += kPgLanes) edges[e].chi2 = w.ce[e];
    int sing = 0;
    for (int n = tid; n < N; n += kPgLanes) sing += w.st[n] == kPgSingular;
    if (sing) atomicAdd(&s_int[1], sing);
    __syncthreads();
    if (tid == 0) {
        lsd_pg_relax_rep* o = reps + g;
        o->chi2_before = chi2_before; o->chi2_after = chi2; o->lambda = lambda;
        o->iters = done; o->cg_iters = cg_total; o->accepted = accepted; o->rejected = rejected;
        o->skipped_edges = s_int[0]; o->singular_nodes = s_int[1]; o->flags = flags; o->reserved = 0;
    }
    if constexpr (kChain) {
        if (tid == 0 && pc_reps) {
            lsd_pg_precond_rep* o = pc_reps + g;
            o->chain_edges = chain_rep[0]; o->paths = chain_rep[1]; o->longest_path = chain_rep[2]; o->fallbacks = fallbacks;
        }
    }
    if constexpr (kRobust) {
        if (!rob_reps) return;
        // the robust report: the plain chi2, and the weights at the final poses.  A lane keeps the first of the order (a NaN before every
        // number, then the smaller w, among equals the smaller index) over its edges, lane 0 the first over the lanes.
        const double plain = pg_reduce(E, [&](int e) { return w.ce[e]; }, s_red);
        auto before = [](double wa, int ia, double wb, int ib) {      // (wa, ia) comes before (wb, ib); ib < 0: nothing there yet
            if (ib < 0) return true;
            const bool na = wa != wa, nb = wb != wb;
            if (na || nb) return na && (!nb || ia < ib);
            return wa < wb || (wa == wb && ia < ib);
        };
        double wm = 1.0;
        int im = -1, down = 0;
        for (int e = tid; e < E; e += kPgLanes) {
            if (!(w.valid[e] & 2)) continue;
            double we, rho;
            pg_weight(rp, true, w.ce[e], we, rho);
            down += we < 1.0;
            if (before(we, e, wm, im)) { wm = we; im = e; }
        }
        if (down) atomicAdd(&s_int[2], down);
        s_red[tid] = wm;
        s_cnt[tid] = im;
        __syncthreads();
        if (tid == 0) {
            for (int t = 1; t < kPgLanes; t++)
                if (s_cnt[t] >= 0 && before(s_red[t], s_cnt[t], wm, im)) { wm = s_red[t]; im = s_cnt[t]; }
            lsd_pg_robust_rep* o = rob_reps + g;
            o->chi2_plain = plain; o->w_min = wm; o->downweighted = s_int[2]; o->w_min_edge = im;
        }
    }
}

}  // namespace lsdhip
