// k_pgloops.hip -- every loop of a track in one pass (include/lsd_hip.h, "pose graph", is the rule; restated in
// tests/pose_graph_loops_cases.py): place recognition with a RANGE of keyframes as queries in one launch (k_pg_recognize_all: the hot
// path, integers only; a query's records are the bytes lsd_enqueue_pg_recognize_device writes for it), the distinct loops among the
// records of the batch (k_pg_loops_closures, k_pg_loops_mark, k_pg_loops_pick, after k_pg_prune's rounds) and what recognize leaves for
// one of them (k_pg_loop_select: posegraph_dev.h's pg_hand_over), so that the closure chain runs on it unchanged.
#include "lsd_internal.h"
#include "pgplace_dev.h"
#include "posegraph_dev.h"

namespace lsdhip {

constexpr int kLpLanes = 256;
static_assert(kLpLanes == kPlLanes, "pl_pick_rounds is written for workgroups of kPlLanes");
static_assert(sizeof(lsd_polar) == 16 && sizeof(lsd_pg_loop_rec) == 16 && sizeof(lsd_pg_loops_rep) == 16, "the loops' records");

// ONE WORKGROUP PER QUERY; block b takes query n_q - 1 - b, so that the heaviest (largest j: the work is triangular) start first and the
// tail of the launch is the light ones.  The lanes stride over the candidates i <= j - gap (pl_score, the single entry's text); the keys
// go into an LDS row of nodes_cap words in the place of d_work; k_pg_place_pick's rounds (pl_pick_rounds) run over that row.  Keys are integers and a
// round's winner is the minimum of distinct (dist, i): nothing depends on the schedule.  No workgroup waits for another.
__global__ __launch_bounds__(kLpLanes) void k_pg_recognize_all(const lsd_pg_head* head, int nodes_cap, const lsd_pg_desc* __restrict__ desc,
                                                               lsd_pg_place_par par, int q_lo, int n_q, lsd_pg_place_rec* recs,
                                                               lsd_pg_place_rep* reps) {
    extern __shared__ uint32_t s_row[];                                       // nodes_cap keys
    __shared__ uint32_t s_q[4][32];
    __shared__ unsigned long long s_key[kLpLanes];
    __shared__ int s_n;
    const int tid = (int)threadIdx.x;
    const int q = n_q - 1 - (int)blockIdx.x, j = q_lo + q;
    const int n_nodes = pg_n_nodes(head, nodes_cap);
    const bool usable = pl_usable(desc, j, n_nodes, par.min_sectors);         // (q_lo + n_q <= nodes_cap: desc[j] exists)
    if (usable) pl_stage_query(desc, j, s_q, tid, kLpLanes);
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int limit = usable ? j - par.gap : -1;                              // < n_nodes <= nodes_cap: the row holds it
    int cand = 0;
    for (int i = tid; i <= limit; i += kLpLanes) {
        const uint32_t key = pl_score(desc, i, s_q, par.min_sectors, par.max_dist);
        s_row[i] = key;
        cand += key != kPlNone;
    }
    if (cand) atomicAdd(&s_n, cand);
    __syncthreads();

    lsd_pg_place_rec unused;
    const int n_picked = pl_pick_rounds([&](int i) { return s_row[i]; }, limit, par, recs + (size_t)q * (size_t)par.k, s_key, tid, unused);
    if (tid == 0) { reps[q].query = j; reps[q].n_cand = s_n; reps[q].n_picked = n_picked; reps[q].reserved = 0; }
}

// ---- the distinct loops ---------------------------------------------------------------------------------------------------------------
// The workspace: a count, the closure edges below E as (max(i, j), min(i, j)) in no particular order, one state word per record.
constexpr uint32_t kLpNoPair = 0u, kLpOpen = 1u, kLpKnown = 2u, kLpGone = 3u;
struct LpWs { int* n_closures; int2* closures; uint32_t* state; };

__host__ __device__ inline size_t lp_ws_bytes(int n_q, int k, int edges_cap) {
    return 16 + (size_t)edges_cap * sizeof(int2) + (size_t)n_q * (size_t)k * sizeof(uint32_t);
}
__host__ __device__ inline LpWs lp_carve(void* ws, int edges_cap) {
    uint8_t* b = static_cast<uint8_t*>(ws);
    return LpWs{reinterpret_cast<int*>(b), reinterpret_cast<int2*>(b + 16), reinterpret_cast<uint32_t*>(b + 16 + (size_t)edges_cap * sizeof(int2))};
}

// One workgroup: the closure edges, compacted.  Their order in the list is the atomics'; a pair is known or not whatever it is.
__global__ __launch_bounds__(kLpLanes) void k_pg_loops_closures(const lsd_pg_head* head, const lsd_pg_edge* edges, int edges_cap, void* ws) {
    __shared__ int s_n;
    const LpWs w = lp_carve(ws, edges_cap);
    const int tid = (int)threadIdx.x, E = pg_n_edges(head, edges_cap);
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int e = tid; e < E; e += kLpLanes) {
        if (!(edges[e].flags & LSD_PG_EDGE_CLOSURE)) continue;
        const int a = edges[e].i, b = edges[e].j;
        w.closures[atomicAdd(&s_n, 1)] = make_int2(max(a, b), min(a, b));     // (at most E <= edges_cap of them)
    }
    __syncthreads();
    if (tid == 0) *w.n_closures = s_n;
}

// One lane per record: no pair, known, or open for the rounds.  The closures pass through LDS a tile at a time.
__global__ __launch_bounds__(kLpLanes) void k_pg_loops_mark(const lsd_pg_place_rec* __restrict__ recs, const lsd_pg_place_rep* __restrict__ reps,
                                                            int n_pairs_cap, int k, int spread, int edges_cap, void* ws) {
    __shared__ int2 s_c[kLpLanes];
    const LpWs w = lp_carve(ws, edges_cap);
    const int tid = (int)threadIdx.x, p = (int)blockIdx.x * kLpLanes + tid;
    const int n_c = min(max(*w.n_closures, 0), edges_cap);
    const bool mine = p < n_pairs_cap;
    const int a = mine ? recs[p].anchor : -1, q = mine ? reps[p / k].query : 0;
    bool known = false;
    for (int base = 0; base < n_c; base += kLpLanes) {                        // (n_c is the same for every lane: the barriers are met by all)
        if (base + tid < n_c) s_c[tid] = w.closures[base + tid];
        __syncthreads();
        const int n_t = min(kLpLanes, n_c - base);
        if (a >= 0)
            for (int t = 0; t < n_t; t++)
                known |= abs((long long)q - (long long)s_c[t].x) <= spread && abs((long long)a - (long long)s_c[t].y) <= spread;
        __syncthreads();
    }
    if (mine) w.state[p] = a < 0 ? kLpNoPair : known ? kLpKnown : kLpOpen;
}

// One workgroup: the counts, then max_loops rounds of one arg-min each over the open pairs.  (dist, query, anchor) are distinct among the
// pairs, so the minimum has no order; the lane that owns a record (p mod 256) is the only one that reads or writes its state.
__global__ __launch_bounds__(kLpLanes) void k_pg_loops_pick(const lsd_pg_place_rec* __restrict__ recs, const lsd_pg_place_rep* __restrict__ reps,
                                                            int n_pairs_cap, int k, lsd_pg_loops_par par, int edges_cap, void* ws,
                                                            lsd_pg_loop_rec* loops, lsd_pg_loops_rep* rep) {
    __shared__ unsigned long long s_key[kLpLanes];
    __shared__ int s_idx[kLpLanes];
    __shared__ int s_int[2];
    const LpWs w = lp_carve(ws, edges_cap);
    const int tid = (int)threadIdx.x;
    if (tid < 2) s_int[tid] = 0;
    __syncthreads();
    int pairs = 0, known = 0;
    for (int p = tid; p < n_pairs_cap; p += kLpLanes) { pairs += w.state[p] != kLpNoPair; known += w.state[p] == kLpKnown; }
    if (pairs) atomicAdd(&s_int[0], pairs);
    if (known) atomicAdd(&s_int[1], known);

    int n_loops = 0;
    bool dry = false;
    for (int m = 0; m < par.max_loops; m++) {
        int best = -1;
        if (!dry) {
            unsigned long long km = ~0ull;
            int im = -1;
            for (int p = tid; p < n_pairs_cap; p += kLpLanes) {
                if (w.state[p] != kLpOpen) continue;
                const unsigned long long key = ((unsigned long long)recs[p].dist << 32) | ((unsigned long long)((uint32_t)reps[p / k].query & 0xffffu) << 16) |
                                               (unsigned long long)((uint32_t)recs[p].anchor & 0xffffu);
                if (key < km) { km = key; im = p; }
            }
            s_key[tid] = km;
            s_idx[tid] = im;
            __syncthreads();
            for (int h = kLpLanes / 2; h >= 1; h >>= 1) {
                if (tid < h && s_key[tid + h] < s_key[tid]) { s_key[tid] = s_key[tid + h]; s_idx[tid] = s_idx[tid + h]; }
                __syncthreads();
            }
            best = s_idx[0];
            __syncthreads();                                                  // (every lane has read s_idx[0] before the next round writes)
            if (best < 0) dry = true;                                         // (the same for every lane)
        }
        if (best < 0) {
            if (tid == 0) { loops[m].query = -1; loops[m].anchor = -1; loops[m].shift = 0; loops[m].dist = 0u; }
            continue;
        }
        const int bq = reps[best / k].query, ba = recs[best].anchor;
        if (tid == 0) { loops[m].query = bq; loops[m].anchor = ba; loops[m].shift = recs[best].shift; loops[m].dist = recs[best].dist; }
        n_loops++;
        for (int p = tid; p < n_pairs_cap; p += kLpLanes) {
            if (w.state[p] != kLpOpen) continue;
            if (abs((long long)reps[p / k].query - (long long)bq) <= par.spread && abs((long long)recs[p].anchor - (long long)ba) <= par.spread)
                w.state[p] = kLpGone;
        }
    }
    __syncthreads();
    if (tid == 0) { rep->n_pairs = s_int[0]; rep->n_known = s_int[1]; rep->n_loops = n_loops; rep->reserved = 0; }
}

// One workgroup: pg_hand_over for loop m.  An anchor or a query outside the nodes (records that no batch left) reads as none.
__global__ __launch_bounds__(kLpLanes) void k_pg_loop_select(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_polar* store,
                                                             const int* store_lens, int store_stride, int gap, int window,
                                                             const lsd_pg_loop_rec* loops, const lsd_pg_loops_rep* loops_rep, int m, PgHandOver out) {
    const int tid = (int)threadIdx.x;
    const int n_nodes = pg_n_nodes(head, nodes_cap);
    const lsd_pg_loop_rec L = loops[m];
    const int j = L.query;
    const bool has_q = j >= 0 && j < n_nodes;
    const int anchor = has_q && L.anchor >= 0 && L.anchor < n_nodes ? L.anchor : -1;
    const PgPose qp = tid == 0 && anchor >= 0 ? pg_turned(nodes, anchor, L.shift) : PgPose{0.0, 0.0, 0.0};
    pg_hand_over(nodes, nodes_cap, n_nodes, store, store_lens, store_stride, gap, window, j, anchor, loops_rep->n_loops, (double)L.dist, qp, out, tid, kLpLanes);
}

hipError_t launch_pg_recognize_all(const lsd_pg_head* head, int nodes_cap, const lsd_pg_desc* desc, lsd_pg_place_par par, int q_lo, int n_q,
                                   lsd_pg_place_rec* recs, lsd_pg_place_rep* reps, hipStream_t st) {
    const size_t lds = (size_t)nodes_cap * sizeof(uint32_t);                  // 64 KiB at 16384 nodes, beside 2.6 KB of static LDS
    if (lds > 60 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pg_recognize_all), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_pg_recognize_all, dim3(n_q), dim3(kLpLanes), lds, st, head, nodes_cap, desc, par, q_lo, n_q, recs, reps);
    return hipSuccess;
}

size_t pg_loops_ws_bytes(int n_q, int k, int edges_cap) { return lp_ws_bytes(n_q, k, edges_cap); }

void launch_pg_loops(const lsd_pg_place_rec* recs, const lsd_pg_place_rep* reps, int n_q, int k, const lsd_pg_head* head, const lsd_pg_edge* edges,
                     int edges_cap, lsd_pg_loops_par par, void* ws, lsd_pg_loop_rec* loops, lsd_pg_loops_rep* rep, hipStream_t st) {
    const int n = n_q * k;                                                    // <= 16384 * 8
    hipLaunchKernelGGL(k_pg_loops_closures, dim3(1), dim3(kLpLanes), 0, st, head, edges, edges_cap, ws);
    if (n) hipLaunchKernelGGL(k_pg_loops_mark, dim3((n + kLpLanes - 1) / kLpLanes), dim3(kLpLanes), 0, st, recs, reps, n, k, par.spread, edges_cap, ws);
    hipLaunchKernelGGL(k_pg_loops_pick, dim3(1), dim3(kLpLanes), 0, st, recs, reps, n, k, par, edges_cap, ws, loops, rep);
}

void launch_pg_loop_select(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_polar* store, const int* store_lens,
                           int store_stride, int gap, int window, const lsd_pg_loop_rec* loops, const lsd_pg_loops_rep* loops_rep, int m,
                           PgHandOver out, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_loop_select, dim3(1), dim3(kLpLanes), 0, st, head, nodes, nodes_cap, store, store_lens, store_stride, gap, window, loops,
                       loops_rep, m, out);
}

}  // namespace lsdhip
