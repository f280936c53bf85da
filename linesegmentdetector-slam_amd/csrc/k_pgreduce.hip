// k_pgreduce.hip -- redundant keyframes retired, the odometry chain contracted across them, and nodes, edges, tracks, store rows, lengths and
// descriptors compacted in place (lsd_enqueue_pg_reduce_device; include/lsd_hip.h, "pose graph", is the rule; restated in
// tests/pose_graph_reduce_cases.py).  A fixed sequence of launches sized by the capacities -- the host does not know the counts, and a
// launch that finds nothing to do ends at once:
//   k_pgr_init     the workspace's integers
//   k_pgr_rank     one workgroup per 256 nodes; the cells of the nodes in front go through LDS in tiles of 256; REDUNDANT
//   k_pgr_edges    one lane per edge: skipped or not, its information invertible or not, and per node the degree, the incoming and the
//                  outgoing count and edge (integer atomics: sums and minima, so no order enters)
//   k_pgr_mark     one lane per node: REMOVABLE, MARKED
//   k_pgr_runs     one lane per edge; the lane whose edge heads a run walks it, and the runs max_run splits off it, ALONE: every sum has one
//                  order, and nobody else writes the run's nodes or edges.  The marks it reads are k_pgr_mark's and never change; what is
//                  retired goes into an array of its own, so a node no walk reaches stays
//   k_pgr_scan     one workgroup: d_map, its inverse and the new counts from a scan over the nodes kept, the edges' places from one over the
//                  edges kept
//   k_pgr_out      the surviving nodes, lengths, descriptors and edges (renumbered) into the workspace ..
//   k_pgr_in       .. and from there to their places, so that no place is written before it was read; tracks, head and report
//   k_pgr_rows     the store: tile t is the kPgrTile surviving rows of the new indices t * kPgrTile ..; launch t copies tile t into one half of
//                  a scratch of two tiles and tile t - 1 from the other half to its places.  new index <= old index and the order is kept, so
//                  the places of tile t - 1 (below t * kPgrTile) are never sources of tile t or a later one; a row that stays where it is (every
//                  row in front of the first retired node) is not touched.  16-byte loads and stores, one workgroup per row
// No workgroup waits for another, every loop is bounded by N, E or a parameter, the atomics are on integers, nothing is allocated.
#include "posegraph_dev.h"

namespace lsdhip {

constexpr int kPgrLanes = 256, kPgrScanLanes = 1024, kPgrTile = 1024;
constexpr int kPgrNone = 0x7fffffff;
// an edge's state
constexpr int kPgrSkipped = 1, kPgrNoInv = 2, kPgrHead = 4, kPgrInRun = 8;
// a node's state
constexpr int kPgrRedundant = 1, kPgrMarked = 2;
// the counters
enum { PGR_N = 0, PGR_E, PGR_N_NEW, PGR_E_NEW, PGR_REDUNDANT, PGR_MARKED, PGR_RETIRED, PGR_RUNS, PGR_KEPT, PGR_LONGEST, PGR_DROPPED, PGR_SPLIT, PGR_COUNTERS = 16 };

// the workspace of one call, every part 16-byte aligned
struct PgrWs {
    int *cnt, *state, *deg, *n_in, *n_out, *in_id, *out_id, *retired, *inv, *est, *epos, *lens;
    lsd_pg_node* nodes;
    lsd_pg_edge* edges;
    lsd_pg_desc* desc;
    lsd_polar* rows;                       // 2 tiles of kPgrTile rows (min(kPgrTile, nodes_cap) each)
    size_t bytes;
};

static inline size_t pgr_up(size_t v) { return (v + 15) & ~(size_t)15; }
static inline int pgr_tile(int nodes_cap) { return nodes_cap < kPgrTile ? nodes_cap : kPgrTile; }

static PgrWs pgr_carve(void* ws, int nc, int ec, int stride) {
    uint8_t* p = (uint8_t*)ws;
    size_t at = 0;
    auto take = [&](size_t n) { uint8_t* r = p + at; at += pgr_up(n); return r; };
    PgrWs w;
    w.cnt = (int*)take(PGR_COUNTERS * sizeof(int));
    int** per_node[] = {&w.state, &w.deg, &w.n_in, &w.n_out, &w.in_id, &w.out_id, &w.retired, &w.inv, &w.lens};
    for (int** q : per_node) *q = (int*)take((size_t)nc * sizeof(int));
    w.est = (int*)take((size_t)ec * sizeof(int));
    w.epos = (int*)take((size_t)ec * sizeof(int));
    w.nodes = (lsd_pg_node*)take((size_t)nc * sizeof(lsd_pg_node));
    w.edges = (lsd_pg_edge*)take((size_t)ec * sizeof(lsd_pg_edge));
    w.desc = (lsd_pg_desc*)take((size_t)nc * sizeof(lsd_pg_desc));
    w.rows = (lsd_polar*)take((size_t)2 * pgr_tile(nc) * stride * sizeof(lsd_polar));
    w.bytes = at;
    return w;
}

size_t pg_reduce_ws_bytes(int nodes_cap, int edges_cap, int store_stride) { return pgr_carve(nullptr, nodes_cap, edges_cap, store_stride).bytes; }

__device__ __forceinline__ bool pgr_finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }
__device__ __forceinline__ bool pgr_pose_finite(const lsd_pg_node& n) { return isfinite(n.x) && isfinite(n.y) && isfinite(n.ang); }

// W, the symmetric matrix of an edge's information (xx, xy, yy, xa, ya, aa), row major
__device__ __forceinline__ void pgr_w(const double* info, double* W) {
    W[0] = info[0]; W[1] = info[1]; W[2] = info[3];
    W[3] = info[1]; W[4] = info[2]; W[5] = info[4];
    W[6] = info[3]; W[7] = info[4]; W[8] = info[5];
}

// C(r,q) = sum_t A(r,t) * B(t,q), or with B transposed sum_t A(r,t) * B(q,t); ascending from 0.0, every product made
template <bool kTransposed>
__device__ __forceinline__ void pgr_mul(const double* A, const double* B, double* Cm) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) t += A[r * 3 + k] * (kTransposed ? B[q * 3 + k] : B[k * 3 + q]);
            Cm[r * 3 + q] = t;
        }
}

__global__ __launch_bounds__(kPgrLanes) void k_pgr_init(PgrWs w, int nc, int ec) {
    const int t = (int)(blockIdx.x * kPgrLanes + threadIdx.x);
    if (t < PGR_COUNTERS) w.cnt[t] = 0;
    if (t < nc) { w.state[t] = 0; w.deg[t] = 0; w.n_in[t] = 0; w.n_out[t] = 0; w.in_id[t] = kPgrNone; w.out_id[t] = kPgrNone; w.retired[t] = 0; }
    if (t < ec) w.est[t] = 0;
}

// REDUNDANT: node k has a cell and at least `keep` nodes in front of it have the same one.  A cell is three fp64 values, the floors as
// they are: integers of any size, or an infinity where the quotient overflowed; == compares them.  The own cell first, then every tile of
// 256 nodes in front goes through LDS and is compared with it
__global__ __launch_bounds__(kPgrLanes) void k_pgr_rank(const lsd_pg_head* head, const lsd_pg_node* nodes, int nc, lsd_pg_reduce_par par, PgrWs w) {
    __shared__ double s_cx[kPgrLanes], s_cy[kPgrLanes], s_ca[kPgrLanes];
    const int N = pg_n_nodes(head, nc), tid = (int)threadIdx.x, base = (int)blockIdx.x * kPgrLanes;
    if (base >= N) return;
    const int k = base + tid;
    // a node without a cell gets a NaN for x, which equals nothing: the compare loop needs no flag, has no branch and unrolls
    auto cell_of = [&](int i, double& x, double& y, double& a) {
        x = __builtin_nan(""); y = a = 0.0;
        if (i >= N) return 0;
        const double px = nodes[i].x, py = nodes[i].y, pa = nodes[i].ang;
        if (!(isfinite(px) && isfinite(py) && isfinite(pa))) return 0;
        x = floor(px / par.cell); y = floor(py / par.cell); a = floor(pg_wrap(pa) / par.ang_bin);
        return 1;
    };
    double cx, cy, ca;
    const int has = cell_of(k, cx, cy, ca);
    int rank = 0;
    for (int tile = 0; tile <= (int)blockIdx.x; tile++) {
        double x, y, a;
        cell_of(tile * kPgrLanes + tid, x, y, a);
        __syncthreads();                                                      // (the tile before has been read)
        s_cx[tid] = x; s_cy[tid] = y; s_ca[tid] = a;
        __syncthreads();
        const int upto = k - tile * kPgrLanes;                                // (the nodes i < k)
#pragma unroll 16
        for (int j = 0; j < kPgrLanes; j++) rank += (int)(j < upto) & (int)(s_cx[j] == cx) & (int)(s_cy[j] == cy) & (int)(s_ca[j] == ca);
    }
    if (k < N) w.state[k] = has && rank >= par.keep ? kPgrRedundant : 0;
}

__global__ __launch_bounds__(kPgrLanes) void k_pgr_edges(const lsd_pg_head* head, const lsd_pg_node* nodes, int nc, const lsd_pg_edge* edges, int ec,
                                                         PgrWs w) {
    const int N = pg_n_nodes(head, nc), E = pg_n_edges(head, ec);
    const int e = (int)(blockIdx.x * kPgrLanes + threadIdx.x);
    if (e >= E) return;
    const lsd_pg_edge ed = edges[e];
    bool skipped = (ed.flags & LSD_PG_EDGE_DISABLED) || ed.i == ed.j || ed.i < 0 || ed.i >= N || ed.j < 0 || ed.j >= N;
    if (!skipped) {
        skipped = !pgr_finite3(ed.z) || !pgr_finite3(ed.info) || !pgr_finite3(ed.info + 3) || !pgr_pose_finite(nodes[ed.i]) || !pgr_pose_finite(nodes[ed.j]);
    }
    if (skipped) { w.est[e] = kPgrSkipped; return; }
    double W[9], I[9], det;
    pgr_w(ed.info, W);
    w.est[e] = pg_inv3(W, I, det) ? 0 : kPgrNoInv;
    atomicAdd(&w.deg[ed.i], 1); atomicAdd(&w.deg[ed.j], 1);
    atomicAdd(&w.n_out[ed.i], 1); atomicAdd(&w.n_in[ed.j], 1);
    atomicMin(&w.out_id[ed.i], e); atomicMin(&w.in_id[ed.j], e);
}

__global__ __launch_bounds__(kPgrLanes) void k_pgr_mark(const lsd_pg_head* head, const lsd_pg_node* nodes, int nc, const lsd_pg_edge* edges,
                                                        const lsd_pg_track* tracks, int n_tracks, PgrWs w) {
    const int N = pg_n_nodes(head, nc);
    const int k = (int)(blockIdx.x * kPgrLanes + threadIdx.x);
    if (k >= N) return;
    const int redundant = w.state[k] & kPgrRedundant;
    if (!redundant) return;
    atomicAdd(&w.cnt[PGR_REDUNDANT], 1);
    bool ok = !(nodes[k].flags & LSD_PG_NODE_FIXED) && w.deg[k] == 2 && w.n_in[k] == 1 && w.n_out[k] == 1;
    if (ok) {
        const int ei = w.in_id[k], eo = w.out_id[k];
        ok = !((edges[ei].flags | edges[eo].flags) & LSD_PG_EDGE_CLOSURE) && !((w.est[ei] | w.est[eo]) & kPgrNoInv);
    }
    for (int t = 0; ok && t < n_tracks; t++) ok = tracks[t].last != k;
    if (!ok) return;
    w.state[k] = kPgrRedundant | kPgrMarked;
    atomicAdd(&w.cnt[PGR_MARKED], 1);
}

// one step of a run: S = J1 S J1^T + J2 Sn J2^T at z's angle, then z = comp(z, zn)
__device__ __forceinline__ void pgr_step(PgPose& z, double* S, const PgPose& zn, const double* Sn) {
    double s, c;
    sincos_g(deg2rad_ref(z.a), s, c);
    const double k = kPi / 180.0;
    const double J1[9] = {1.0, 0.0, k * ((-s) * zn.x - c * zn.y), 0.0, 1.0, k * (c * zn.x - s * zn.y), 0.0, 0.0, 1.0};
    const double J2[9] = {c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0};
    double T[9], U1[9], U2[9];
    pgr_mul<false>(J1, S, T);
    pgr_mul<true>(T, J1, U1);
    pgr_mul<false>(J2, Sn, T);
    pgr_mul<true>(T, J2, U2);
#pragma unroll
    for (int q = 0; q < 9; q++) S[q] = U1[q] + U2[q];
    z = pg_comp(z, zn);
}

__global__ __launch_bounds__(kPgrLanes) void k_pgr_runs(const lsd_pg_head* head, int nc, const lsd_pg_edge* edges, int ec, lsd_pg_reduce_par par,
                                                        PgrWs w) {
    const int N = pg_n_nodes(head, nc), E = pg_n_edges(head, ec);
    const int e0 = (int)(blockIdx.x * kPgrLanes + threadIdx.x);
    if (e0 >= E || (w.est[e0] & kPgrSkipped)) return;
    int a = edges[e0].i, r = edges[e0].j, lead = e0;
    if ((w.state[a] & kPgrMarked) || !(w.state[r] & kPgrMarked)) return;
    for (int walked = 0; walked < N;) {                                       // one run per turn; the marked nodes walked bound the turns
        PgPose z{edges[lead].z[0], edges[lead].z[1], edges[lead].z[2]};
        double W[9], S[9], det;
        pgr_w(edges[lead].info, W);
        pg_inv3(W, S, det);                                                   // (r is marked: it succeeds)
        int cur = r, len = 1, b;
        bool forced = false;
        // at most min(max_run, N) steps: a marked node has exactly one incoming edge that counts, the first node's comes from the unmarked a,
        // and every later node is entered through the one edge of its predecessor -- so the walk never enters a node a second time, and it
        // ends at the first unmarked node or at max_run, whichever comes first (len < N is that argument as a guard, never the reason)
        for (;;) {
            const int oe = w.out_id[cur];
            const PgPose zn{edges[oe].z[0], edges[oe].z[1], edges[oe].z[2]};
            double Sn[9];
            pgr_w(edges[oe].info, W);
            pg_inv3(W, Sn, det);
            pgr_step(z, S, zn, Sn);
            b = edges[oe].j;
            if (!(w.state[b] & kPgrMarked)) break;
            if (len == par.max_run || len >= N) { forced = true; break; }
            cur = b;
            len++;
        }
        walked += len;
        double I[9];
        bool ok = b != a && isfinite(z.x) && isfinite(z.y) && isfinite(z.a);
#pragma unroll
        for (int q = 0; q < 9; q++) ok = ok && isfinite(S[q]);
        ok = ok && pg_inv3(S, I, det);
        if (ok) {
            lsd_pg_edge* o = w.edges + lead;
            o->i = a; o->j = b; o->flags = LSD_PG_EDGE_CONTRACTED; o->reserved = 0u;
            o->z[0] = z.x; o->z[1] = z.y; o->z[2] = z.a;
            o->info[0] = I[0]; o->info[1] = I[1]; o->info[2] = I[4]; o->info[3] = I[2]; o->info[4] = I[5]; o->info[5] = I[8];
            o->chi2 = 0.0;
            w.est[lead] |= kPgrHead;
            cur = r;
            for (int t = 0; t < len; t++) {
                const int oe = w.out_id[cur];
                w.retired[cur] = 1;
                w.est[oe] |= kPgrInRun;
                cur = edges[oe].j;
            }
            atomicAdd(&w.cnt[PGR_RUNS], 1);
            atomicMax(&w.cnt[PGR_LONGEST], len);
        } else {
            atomicAdd(&w.cnt[PGR_KEPT], 1);
        }
        if (!forced) break;
        atomicAdd(&w.cnt[PGR_SPLIT], 1);
        a = b;                                                                // b stays: it ends this run and heads the next one
        walked++;
        lead = w.out_id[b];
        r = edges[lead].j;
        if (!(w.state[r] & kPgrMarked)) break;
    }
}

// the exclusive scan of one flag per lane over the workgroup; returns the lane's offset, `total` the sum
__device__ __forceinline__ int pgr_block_scan(int flag, int* s, int tid, int& total) {
    s[tid] = flag;
    __syncthreads();
    for (int h = 1; h < kPgrScanLanes; h <<= 1) {
        const int v = tid >= h ? s[tid - h] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    const int incl = s[tid];
    total = s[kPgrScanLanes - 1];
    __syncthreads();
    return incl - flag;
}

__global__ __launch_bounds__(kPgrScanLanes) void k_pgr_scan(const lsd_pg_head* head, int nc, const lsd_pg_edge* edges, int ec, int32_t* map, PgrWs w) {
    __shared__ int s[kPgrScanLanes];
    const int N = pg_n_nodes(head, nc), E = pg_n_edges(head, ec), tid = (int)threadIdx.x;
    int at = 0;
    for (int base = 0; base < nc; base += kPgrScanLanes) {
        const int k = base + tid;
        const int keep = k < N && !w.retired[k];
        int total;
        const int off = pgr_block_scan(keep, s, tid, total);
        if (k < nc) map[k] = keep ? at + off : -1;
        if (keep) w.inv[at + off] = k;
        at += total;
    }
    const int n_new = at;
    int dropped = 0;
    at = 0;
    for (int base = 0; base < E; base += kPgrScanLanes) {
        const int e = base + tid;
        int keep = 0;
        if (e < E) {
            const int st = w.est[e], i = edges[e].i, j = edges[e].j;
            const bool inside = i >= 0 && i < N && j >= 0 && j < N;
            if (st & kPgrHead) keep = 1;
            else if (st & kPgrInRun) keep = 0;
            else if (inside && (w.retired[i] || w.retired[j])) { keep = 0; dropped++; }
            else keep = 1;
        }
        int total;
        const int off = pgr_block_scan(keep, s, tid, total);
        if (e < E) w.epos[e] = keep ? at + off : -1;
        at += total;
    }
    if (dropped) atomicAdd(&w.cnt[PGR_DROPPED], dropped);
    if (tid == 0) { w.cnt[PGR_N] = N; w.cnt[PGR_E] = E; w.cnt[PGR_N_NEW] = n_new; w.cnt[PGR_E_NEW] = at; w.cnt[PGR_RETIRED] = N - n_new; }
}

// from here on the counts are the workspace's: the head is written by k_pgr_in
__global__ __launch_bounds__(kPgrLanes) void k_pgr_out(const lsd_pg_node* nodes, const lsd_pg_edge* edges, const int* store_lens, const lsd_pg_desc* desc,
                                                       const int32_t* map, PgrWs w) {
    const int N = w.cnt[PGR_N], E = w.cnt[PGR_E];
    for (int k = (int)(blockIdx.x * kPgrLanes + threadIdx.x); k < N; k += (int)gridDim.x * kPgrLanes) {
        if (map[k] < 0 || map[k] == k) continue;
        w.nodes[k] = nodes[k];
        w.lens[k] = store_lens[k];
        if (desc) w.desc[k] = desc[k];
    }
    for (int e = (int)(blockIdx.x * kPgrLanes + threadIdx.x); e < E; e += (int)gridDim.x * kPgrLanes) {
        if (w.epos[e] < 0) continue;
        const lsd_pg_edge* from = (w.est[e] & kPgrHead) ? w.edges + e : edges + e;
        const int i = from->i, j = from->j;
        const bool inside = i >= 0 && i < N && j >= 0 && j < N;
        if (from != w.edges + e) w.edges[e] = *from;
        if (inside) { w.edges[e].i = map[i]; w.edges[e].j = map[j]; }
    }
}

__global__ __launch_bounds__(kPgrLanes) void k_pgr_in(lsd_pg_head* head, lsd_pg_node* nodes, lsd_pg_edge* edges, lsd_pg_track* tracks, int n_tracks,
                                                      int* store_lens, lsd_pg_desc* desc, const int32_t* map, lsd_pg_reduce_rep* rep, PgrWs w) {
    const int N = w.cnt[PGR_N], E = w.cnt[PGR_E], n_new = w.cnt[PGR_N_NEW], e_new = w.cnt[PGR_E_NEW];
    const int t0 = (int)(blockIdx.x * kPgrLanes + threadIdx.x), step = (int)gridDim.x * kPgrLanes;
    for (int k = t0; k < N; k += step) {
        const int d = map[k];
        if (d >= 0 && d != k) {
            nodes[d] = w.nodes[k];
            store_lens[d] = w.lens[k];
            if (desc) desc[d] = w.desc[k];
        }
        if (k >= n_new) {                                                     // (no place: nothing above writes here)
            store_lens[k] = 0;
            if (desc) desc[k] = lsd_pg_desc{};
        }
    }
    for (int e = t0; e < E; e += step)
        if (w.epos[e] >= 0) edges[w.epos[e]] = w.edges[e];
    for (int t = t0; t < n_tracks; t += step) {
        const int last = tracks[t].last;
        if (last >= 0 && last < N) tracks[t].last = map[last];
    }
    if (t0 == 0) {
        head->n_nodes = n_new;
        head->n_edges = e_new;
        if (rep) {
            rep->nodes_before = N; rep->edges_before = E; rep->nodes_after = n_new; rep->edges_after = e_new;
            rep->redundant = w.cnt[PGR_REDUNDANT]; rep->marked = w.cnt[PGR_MARKED]; rep->retired = w.cnt[PGR_RETIRED];
            rep->runs = w.cnt[PGR_RUNS]; rep->runs_kept = w.cnt[PGR_KEPT]; rep->longest_run = w.cnt[PGR_LONGEST];
            rep->dropped_edges = w.cnt[PGR_DROPPED];
            rep->flags = (w.cnt[PGR_RETIRED] ? LSD_PG_REDUCE_RETIRED : 0u) | (w.cnt[PGR_SPLIT] ? LSD_PG_REDUCE_SPLIT : 0u);
        }
    }
}

// launch t: workgroups 0 .. tile-1 bring tile t - 1 from its half of the scratch to its places, workgroups tile .. 2 tile - 1 take tile t out
__global__ __launch_bounds__(kPgrLanes) void k_pgr_rows(lsd_polar* store, int stride, int tile, int t, PgrWs w) {
    const int n_new = w.cnt[PGR_N_NEW];
    const bool out = (int)blockIdx.x >= tile;
    const int slot = (int)blockIdx.x - (out ? tile : 0), which = out ? t : t - 1;
    if (which < 0) return;
    const int d = which * tile + slot;
    if (d >= n_new) return;
    const int src = w.inv[d];
    if (src == d) return;
    lsd_polar* scratch = w.rows + ((size_t)(which & 1) * tile + slot) * (size_t)stride;
    const double2* from = reinterpret_cast<const double2*>(out ? store + (size_t)src * stride : scratch);
    double2* to = reinterpret_cast<double2*>(out ? scratch : store + (size_t)d * stride);
    for (int i = (int)threadIdx.x; i < stride; i += kPgrLanes) to[i] = from[i];
}

void launch_pg_reduce(lsd_pg_head* head, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, lsd_pg_track* tracks, int n_tracks,
                      lsd_polar* store, int* store_lens, int store_stride, lsd_pg_desc* desc, lsd_pg_reduce_par par, int32_t* map,
                      lsd_pg_reduce_rep* rep, void* ws, hipStream_t st) {
    const PgrWs w = pgr_carve(ws, nodes_cap, edges_cap, store_stride);
    auto blocks = [](int n) { return dim3((unsigned)((n + kPgrLanes - 1) / kPgrLanes)); };
    const int both = nodes_cap > edges_cap ? nodes_cap : edges_cap;
    const dim3 lanes(kPgrLanes), strided = blocks(both < 2048 * kPgrLanes ? both : 2048 * kPgrLanes);
    hipLaunchKernelGGL(k_pgr_init, blocks(both > PGR_COUNTERS ? both : PGR_COUNTERS), lanes, 0, st, w, nodes_cap, edges_cap);
    hipLaunchKernelGGL(k_pgr_rank, blocks(nodes_cap), lanes, 0, st, head, nodes, nodes_cap, par, w);
    hipLaunchKernelGGL(k_pgr_edges, blocks(edges_cap), lanes, 0, st, head, nodes, nodes_cap, edges, edges_cap, w);
    hipLaunchKernelGGL(k_pgr_mark, blocks(nodes_cap), lanes, 0, st, head, nodes, nodes_cap, edges, tracks, n_tracks, w);
    hipLaunchKernelGGL(k_pgr_runs, blocks(edges_cap), lanes, 0, st, head, nodes_cap, edges, edges_cap, par, w);
    hipLaunchKernelGGL(k_pgr_scan, dim3(1), dim3(kPgrScanLanes), 0, st, head, nodes_cap, edges, edges_cap, map, w);
    hipLaunchKernelGGL(k_pgr_out, strided, lanes, 0, st, nodes, edges, store_lens, desc, map, w);
    hipLaunchKernelGGL(k_pgr_in, strided, lanes, 0, st, head, nodes, edges, tracks, n_tracks, store_lens, desc, map, rep, w);
    const int tile = pgr_tile(nodes_cap), tiles = (nodes_cap + tile - 1) / tile;
    for (int t = 0; t <= tiles; t++) hipLaunchKernelGGL(k_pgr_rows, dim3(2 * tile), lanes, 0, st, store, store_stride, tile, t, w);
}

}  // namespace lsdhip
