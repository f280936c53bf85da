// k_pgmarg.hip -- marginal covariances of a pose graph and the gate that vets new closures with them (lsd_enqueue_pg_marginals_device,
// lsd_enqueue_pg_vet_device; include/lsd_hip.h, "pose graph", is the rule; restated in tests/pose_graph_marginal_cases.py).
// A marginal is a solve with the relaxation's normal matrix at lambda = 0.0, and the solves do not depend on each other:
//   k_pg_marg_prepare  ONE workgroup: the front of pgrelax_dev.h's body -- the edges that count (below the prior's count), the nodes'
//                      states, the lists, the blocks, H and M, and with CHAIN the positions and the factor -- into the SHARED part of the
//                      workspace, which nobody writes afterwards.
//   k_pg_marg_solve    min(n_q, slots) workgroups; workgroup s serves the queries s, s + slots, ..: three PCG solves each, the vectors in
//                      slice s of the workspace.  The matrix-vector product, the updates, the reductions and the chain's apply are the
//                      relaxation's own text (pg_reduce, pg_chain_apply); a record depends on the graph and the query alone.
//   k_pg_vet           ONE workgroup, a lane per query: every outcome is decided from the edges as they stand when the launch begins, the
//                      rejected edges are remembered in LDS (a bit per query) and flagged behind a barrier, so two queries on one edge
//                      decide alike.
// fp64 without FMA, no atomics on fp64; every loop is bounded by a parameter and no workgroup waits for another.
#include "pgrelax_dev.h"

namespace lsdhip {

constexpr int kMargMaxQueries = 65536;

size_t pg_marg_slice_bytes(int nodes_cap, int kind) {
    const size_t b = (size_t)(kind == LSD_PG_PRECOND_CHAIN ? 21 : 15) * nodes_cap * 8;
    return (b + 255) & ~(size_t)255;
}

size_t pg_marg_ws_bytes(int nodes_cap, int edges_cap, int kind, int slots) {
    return pg_ws_pc_bytes(nodes_cap, edges_cap, kind) + (size_t)slots * pg_marg_slice_bytes(nodes_cap, kind);
}

// the count of the edges that make the matrix: all E of the head, or no more than the prior head had
__device__ inline int pg_marg_edges(const lsd_pg_head* head, const lsd_pg_head* prior, int ec) {
    const int E = pg_n_edges(head, ec);
    return prior ? min(E, pg_n_edges(prior, ec)) : E;
}

// Behind this launch the shared part holds valid, the lists, st, blk, H, M and the factor; cur[0] says whether the factor stands.
template <bool kChain>
__global__ __launch_bounds__(kPgLanes) void k_pg_marg_prepare(const lsd_pg_head* head, const lsd_pg_head* prior, const lsd_pg_node* nodes, int nc,
                                                              const lsd_pg_edge* edges, int ec, uint8_t* ws, size_t shared_bytes,
                                                              lsd_pg_marg_rep* rep) {
    __shared__ int s_cnt[kPgLanes];
    __shared__ int s_int[2];
    const int tid = (int)threadIdx.x;
    const PgWs w = pg_ws_of(ws, nc, ec);
    PgChainWs cw{};
    if constexpr (kChain) cw = pg_chain_ws_of(ws + (shared_bytes - pg_chain_ws_bytes(nc)), nc);
    const int N = pg_n_nodes(head, nc), E = pg_marg_edges(head, prior, ec);

    // --- the edges that count, the nodes' states, the lists: the relaxation's, over the E edges of the matrix -------------------------------
    if (tid < 2) s_int[tid] = 0;
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
        w.valid[e] = ok ? 1 : 0;
        if (ok) { atomicAdd(&w.cur[ed.i], 1); atomicAdd(&w.cur[ed.j], 1); }
        else skipped++;
    }
    if (skipped) atomicAdd(&s_int[0], skipped);
    __syncthreads();
    {
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
    int chain_rep[3] = {0, 0, 0};
    if constexpr (kChain) pg_chain_setup(edges, N, E, w.valid, cw, s_cnt, chain_rep);

    // --- the blocks at the nodes' poses with plain weights, H, M = inv3(D) at lambda = 0.0 --------------------------------------------------
    const double lambda = 0.0;
    pg_edges<false>(nodes, edges, E, ec, w, nullptr, w.ce, true, lsd_pg_robust_par{});
    for (int n = tid; n < N; n += kPgLanes) {
        double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int m = w.off[n]; m < w.off[n + 1]; m++) {
            const int en = w.ent[m], e = en >> 1, side = en & 1;
            const double* o = w.blk + e;
#pragma unroll
            for (int q = 0; q < 9; q++) H[q] += o[(size_t)((side ? 18 : 0) + q) * ec];
        }
#pragma unroll
        for (int q = 0; q < 9; q++) w.H[9 * n + q] = H[q];
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
    }
    __syncthreads();
    bool factor_ok = false;
    if constexpr (kChain) factor_ok = pg_chain_factor(w, cw, N, ec, lambda);
    int sing = 0;
    for (int n = tid; n < N; n += kPgLanes) sing += w.st[n] == kPgSingular;
    if (sing) atomicAdd(&s_int[1], sing);
    __syncthreads();
    if (tid == 0) {
        w.cur[0] = factor_ok ? 1 : 0;                                                                  // (nc >= 1; the cursors are done with)
        rep->n_nodes = N; rep->n_edges = E; rep->skipped_edges = s_int[0]; rep->singular_nodes = s_int[1];
        rep->chain_edges = chain_rep[0]; rep->paths = chain_rep[1]; rep->longest_path = chain_rep[2];
        rep->fallbacks = (kChain && !factor_ok) ? 1 : 0;
    }
}

template <bool kChain>
__global__ __launch_bounds__(kPgLanes) void k_pg_marg_solve(const lsd_pg_head* head, const lsd_pg_head* prior, const lsd_pg_node* nodes, int nc,
                                                            const lsd_pg_edge* edges, int ec, const lsd_pg_marg_query* queries, int n_q,
                                                            lsd_pg_marg_par par, uint8_t* ws, size_t shared_bytes, size_t slice_bytes,
                                                            lsd_pg_marg_rec* recs) {
    __shared__ double s_red[kPgShape];
    const int tid = (int)threadIdx.x, slot = (int)blockIdx.x;
    PgWs w = pg_ws_of(ws, nc, ec);                                                                    // the shared part, read only ..
    PgChainWs cw{};
    if constexpr (kChain) cw = pg_chain_ws_of(ws + (shared_bytes - pg_chain_ws_bytes(nc)), nc);
    {
        double* d = reinterpret_cast<double*>(ws + shared_bytes + (size_t)slot * slice_bytes);        // .. and this slot's own vectors
        w.dl = d; d += (size_t)3 * nc;
        w.r = d; d += (size_t)3 * nc;
        w.z = d; d += (size_t)3 * nc;
        w.p = d; d += (size_t)3 * nc;
        w.q = d; d += (size_t)3 * nc;
        if constexpr (kChain) { cw.y = d; d += (size_t)3 * nc; cw.x = d; }
    }
    const int N = pg_n_nodes(head, nc), E = pg_n_edges(head, ec);
    const bool jacobi = !kChain || w.cur[0] == 0;
    const double lambda = 0.0;

    for (int qi = slot; qi < n_q; qi += par.slots) {
        const lsd_pg_marg_query qu = queries[qi];
        uint32_t flags = 0;
        int a = qu.a, b = qu.b, edge = -1, steps[3] = {0, 0, 0};
        bool pair = qu.kind != LSD_PG_MARG_NODE;
        if (qu.kind == LSD_PG_MARG_NEW_EDGE) {
            a = -1; b = -1;
            if (!prior || qu.a < 0) flags |= LSD_PG_MARG_BAD_QUERY;
            else {
                const long long e = (long long)pg_n_edges(prior, ec) + qu.a;
                edge = (int)(e < 2147483647ll ? e : 2147483647ll);
                if (e >= E) flags |= LSD_PG_MARG_NO_EDGE;
                else { a = edges[e].i; b = edges[e].j; }
            }
        } else if (qu.kind != LSD_PG_MARG_NODE && qu.kind != LSD_PG_MARG_PAIR) flags |= LSD_PG_MARG_BAD_QUERY;
        if (!flags) {
            if (a < 0 || a >= N || (pair && (b < 0 || b >= N || a == b))) flags |= LSD_PG_MARG_BAD_QUERY;
        }
        int sta = kPgFree, stb = kPgFree;
        if (!flags) {
            sta = w.st[a];
            if (pair) stb = w.st[b];
            if (sta == kPgFixed || (pair && stb == kPgFixed)) flags |= LSD_PG_MARG_FIXED;
            if (sta == kPgSingular || (pair && stb == kPgSingular)) flags |= LSD_PG_MARG_SINGULAR;
        }
        const bool solve = !(flags & (LSD_PG_MARG_BAD_QUERY | LSD_PG_MARG_NO_EDGE)) && (pair || !flags);
        // J = [A | B]: the rows of the right-hand side (NODE: A is the identity, there is no B)
        double A[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, B[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (solve && pair) {
            const double zero[3] = {0.0, 0.0, 0.0};
            double er[3], s, c, dx, dy;
            pg_error(pg_pose_of(nodes[a]), pg_pose_of(nodes[b]), zero, er, s, c, dx, dy);
            const double k = kPi / 180.0;
            A[0] = -c; A[1] = -s; A[2] = k * (c * dy - s * dx); A[3] = s; A[4] = -c; A[5] = k * ((-c) * dx - s * dy); A[6] = 0.0; A[7] = 0.0; A[8] = -1.0;
            B[0] = c; B[1] = s; B[2] = 0.0; B[3] = -s; B[4] = c; B[5] = 0.0; B[6] = 0.0; B[7] = 0.0; B[8] = 1.0;
        }
        double cov[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int col = 0; solve && col < 3; col++) {
            // the start: delta = 0, r = u, z = M^-1 r, p = z
            for (int n = tid; n < N; n += kPgLanes) {
                const bool fr = w.st[n] == kPgFree;
                double rn[3] = {0.0, 0.0, 0.0};
                if (fr && n == a) { rn[0] = A[3 * col]; rn[1] = A[3 * col + 1]; rn[2] = A[3 * col + 2]; }
                if (fr && pair && n == b) { rn[0] = B[3 * col]; rn[1] = B[3 * col + 1]; rn[2] = B[3 * col + 2]; }
                double z[3] = {0.0, 0.0, 0.0};
                if (fr) {
#pragma unroll
                    for (int q = 0; q < 3; q++) z[q] = pg_dot3(w.M + 9 * n + 3 * q, rn);
                }
#pragma unroll
                for (int q = 0; q < 3; q++) { w.dl[3 * n + q] = 0.0; w.r[3 * n + q] = rn[q]; w.z[3 * n + q] = z[q]; w.p[3 * n + q] = z[q]; }
            }
            __syncthreads();
            if constexpr (kChain) {
                if (!jacobi) {
                    pg_chain_apply(w, cw, N);
                    for (int n = tid; n < N; n += kPgLanes)
#pragma unroll
                        for (int q = 0; q < 3; q++) w.p[3 * n + q] = w.z[3 * n + q];
                    __syncthreads();
                }
            }
            double rz = pg_reduce(N, [&](int n) { return pg_dot3(w.r + 3 * n, w.z + 3 * n); }, s_red);
            const double thr = (par.cg_tol * par.cg_tol) * rz;
            int st = 0;
            bool broke = false;
            while (st < par.cg_iters && !(rz <= thr)) {
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
                            double hb[9], pv[3];
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
                if (!(pq > 0)) { broke = true; break; }
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
                st++;
            }
            steps[col] = st;
            flags |= (broke ? LSD_PG_MARG_BREAKDOWN_0 : (rz <= thr ? LSD_PG_MARG_CONVERGED_0 : LSD_PG_MARG_MAXED_0)) << col;
            // cov(r, col) = sum_q A(r,q) * x_a[q] + sum_q B(r,q) * x_b[q]; x is +0.0 at a node that is not free
            const double* xa = w.dl + 3 * a;
#pragma unroll
            for (int r = 0; r < 3; r++) cov[3 * r + col] = pg_dot3(A + 3 * r, xa);
            if (pair) {
                const double* xb = w.dl + 3 * b;
#pragma unroll
                for (int r = 0; r < 3; r++) cov[3 * r + col] = cov[3 * r + col] + pg_dot3(B + 3 * r, xb);
            }
            __syncthreads();                                                                          // (every lane has read delta before the next start)
        }
        if (tid == 0) {
            lsd_pg_marg_rec* o = recs + qi;
#pragma unroll
            for (int q = 0; q < 9; q++) o->cov[q] = cov[q];
#pragma unroll
            for (int q = 0; q < 3; q++) o->steps[q] = steps[q];
            o->flags = flags; o->kind = qu.kind; o->edge = edge; o->i = a; o->j = b;
        }
    }
}

__global__ __launch_bounds__(kPgLanes) void k_pg_vet(const lsd_pg_head* head, const lsd_pg_node* nodes, int nc, lsd_pg_edge* edges, int ec,
                                                     const lsd_pg_marg_query* queries, const lsd_pg_marg_rec* recs, int n_q, double gate,
                                                     lsd_pg_vet_rep* reps) {
    __shared__ uint32_t s_rej[kMargMaxQueries / 32];
    const int tid = (int)threadIdx.x;
    const int N = pg_n_nodes(head, nc), E = pg_n_edges(head, ec);
    for (int t = tid; t < kMargMaxQueries / 32; t += kPgLanes) s_rej[t] = 0u;
    __syncthreads();
    for (int qi = tid; qi < n_q; qi += kPgLanes) {
        const lsd_pg_marg_rec rc = recs[qi];
        uint32_t out = 0;
        int e = -1;
        double d2 = 0.0, det = 0.0;
        if (queries[qi].kind != LSD_PG_MARG_NEW_EDGE) out = LSD_PG_VET_UNUSED;
        else if ((rc.flags & (LSD_PG_MARG_NO_EDGE | LSD_PG_MARG_BAD_QUERY)) || rc.edge < 0 || rc.edge >= E) out = LSD_PG_VET_NO_EDGE;      // 1
        else {
            e = rc.edge;
            const lsd_pg_edge ed = edges[e];
            bool ok = (ed.flags & LSD_PG_EDGE_CLOSURE) && !(ed.flags & LSD_PG_EDGE_DISABLED) && ed.i != ed.j && ed.i >= 0 && ed.i < N && ed.j >= 0 &&
                      ed.j < N;
#pragma unroll
            for (int q = 0; q < 3; q++) ok = ok && isfinite(ed.z[q]);
#pragma unroll
            for (int q = 0; q < 6; q++) ok = ok && isfinite(ed.info[q]);
            if (ok) {
                const lsd_pg_node &a = nodes[ed.i], &b = nodes[ed.j];
                ok = isfinite(a.x) && isfinite(a.y) && isfinite(a.ang) && isfinite(b.x) && isfinite(b.y) && isfinite(b.ang);
            }
            const uint32_t conv = LSD_PG_MARG_CONVERGED_0 | (LSD_PG_MARG_CONVERGED_0 << 1) | (LSD_PG_MARG_CONVERGED_0 << 2);
            double W[9], R[9], S[9], Si[9];
            if (!ok) out = LSD_PG_VET_SKIPPED;                                                         // 2
            else if ((rc.flags & conv) != conv) out = LSD_PG_VET_NO_MARGINAL;                          // 3
            else {
                pg_info(ed, W);
                if (!pg_inv3(W, R, det)) out = LSD_PG_VET_SINGULAR;                                    // 4
                else {
#pragma unroll
                    for (int q = 0; q < 9; q++) S[q] = rc.cov[q] + R[q];
                    if (!pg_inv3(S, Si, det)) out = LSD_PG_VET_SINGULAR;                               // 5
                    else {
                        double er[3], s, c, dx, dy, t[3];
                        pg_error(pg_pose_of(nodes[ed.i]), pg_pose_of(nodes[ed.j]), ed.z, er, s, c, dx, dy);
#pragma unroll
                        for (int r = 0; r < 3; r++) t[r] = pg_dot3(Si + 3 * r, er);
                        d2 = pg_dot3(er, t);
                        out = !(d2 <= gate) ? LSD_PG_VET_REJECTED : LSD_PG_VET_PASSED;                 // 6, 7
                    }
                }
            }
        }
        if (out == LSD_PG_VET_REJECTED) atomicOr(&s_rej[qi >> 5], 1u << (qi & 31));
        if (reps) { lsd_pg_vet_rep* o = reps + qi; o->d2 = d2; o->det = det; o->edge = e; o->flags = out; }
    }
    __syncthreads();                                                                                  // every outcome stands before an edge changes
    for (int qi = tid; qi < n_q; qi += kPgLanes) {
        if (s_rej[qi >> 5] & (1u << (qi & 31))) atomicOr(&edges[recs[qi].edge].flags, LSD_PG_EDGE_DISABLED | LSD_PG_EDGE_REJECTED);
    }
}

void launch_pg_marginals(const lsd_pg_head* head, const lsd_pg_head* prior, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_edge* edges,
                         int edges_cap, const lsd_pg_marg_query* queries, int n_q, lsd_pg_marg_par par, void* ws, lsd_pg_marg_rec* recs,
                         lsd_pg_marg_rep* rep, hipStream_t st) {
    const size_t shared = pg_ws_pc_bytes(nodes_cap, edges_cap, par.precond), slice = pg_marg_slice_bytes(nodes_cap, par.precond);
    uint8_t* base = static_cast<uint8_t*>(ws);
    const int groups = n_q < par.slots ? n_q : par.slots;
    if (par.precond == LSD_PG_PRECOND_CHAIN) {
        hipLaunchKernelGGL(k_pg_marg_prepare<true>, dim3(1), dim3(kPgLanes), 0, st, head, prior, nodes, nodes_cap, edges, edges_cap, base, shared, rep);
        hipLaunchKernelGGL(k_pg_marg_solve<true>, dim3(groups), dim3(kPgLanes), 0, st, head, prior, nodes, nodes_cap, edges, edges_cap, queries, n_q,
                           par, base, shared, slice, recs);
    } else {
        hipLaunchKernelGGL(k_pg_marg_prepare<false>, dim3(1), dim3(kPgLanes), 0, st, head, prior, nodes, nodes_cap, edges, edges_cap, base, shared, rep);
        hipLaunchKernelGGL(k_pg_marg_solve<false>, dim3(groups), dim3(kPgLanes), 0, st, head, prior, nodes, nodes_cap, edges, edges_cap, queries, n_q,
                           par, base, shared, slice, recs);
    }
}

void launch_pg_vet(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                   const lsd_pg_marg_query* queries, const lsd_pg_marg_rec* recs, int n_q, double gate, lsd_pg_vet_rep* reps, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_vet, dim3(1), dim3(kPgLanes), 0, st, head, nodes, nodes_cap, edges, edges_cap, queries, recs, n_q, gate, reps);
}

}  // namespace lsdhip
