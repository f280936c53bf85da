// k_pgprune.hip -- the rejection of closure edges by their chi2 (lsd_enqueue_pg_prune_device; include/lsd_hip.h, "pose graph", is the rule;
// DESIGN.md 8.1.16; restated in tests/pose_graph_robust_cases.py).  ONE WORKGROUP PER GRAPH, no workspace, no atomics on fp64: a round finds
// the first candidate of the order (chi2 descending, a NaN as +infinity, equals by ascending index) with one arg-max over the workgroup and
// disables it, so that the next round no longer sees it; at most max(max_reject, 1) rounds of E / 256 edges per lane.  The lane that owns an
// edge (e mod 256) is the only one that reads or writes its flags.
#include "lsd_internal.h"

namespace lsdhip {

constexpr int kPrLanes = 256;

__device__ inline bool pr_candidate(const lsd_pg_edge& ed, double gate) {
    return (ed.flags & LSD_PG_EDGE_CLOSURE) && !(ed.flags & LSD_PG_EDGE_DISABLED) && !(ed.chi2 <= gate);
}

// (ka, ia) comes before (kb, ib) in the order; the keys hold +infinity for a NaN; ib < 0: nothing there
__device__ inline bool pr_before(double ka, int ia, double kb, int ib) { return ib < 0 || ka > kb || (ka == kb && ia < ib); }

__global__ __launch_bounds__(kPrLanes) void k_pg_prune(const lsd_pg_head* heads, lsd_pg_edge* all_edges, int ec, lsd_pg_prune_par par,
                                                       lsd_pg_prune_rep* reps) {
    __shared__ double s_key[kPrLanes];
    __shared__ int s_idx[kPrLanes];
    __shared__ int s_int[2];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    lsd_pg_edge* edges = all_edges + (size_t)g * ec;
    const int E = min(max(heads[g].n_edges, 0), ec);
    if (tid < 2) s_int[tid] = 0;
    __syncthreads();
    int cand = 0;
    for (int e = tid; e < E; e += kPrLanes) cand += pr_candidate(edges[e], par.gate);
    if (cand) atomicAdd(&s_int[0], cand);

    int rejected = 0, worst = -1;
    double worst_chi2 = 0.0;
    const int rounds = par.max_reject > 1 ? par.max_reject : 1;               // (round 0 also finds the worst edge when max_reject is 0)
    for (int round = 0; round < rounds; round++) {
        double km = 0.0;
        int im = -1;
        for (int e = tid; e < E; e += kPrLanes) {
            const lsd_pg_edge ed = edges[e];
            if (!pr_candidate(ed, par.gate)) continue;
            const double k = ed.chi2 != ed.chi2 ? __builtin_huge_val() : ed.chi2;
            if (pr_before(k, e, km, im)) { km = k; im = e; }
        }
        s_key[tid] = km;
        s_idx[tid] = im;
        __syncthreads();
        for (int h = kPrLanes / 2; h >= 1; h >>= 1) {
            if (tid < h && s_idx[tid + h] >= 0 && pr_before(s_key[tid + h], s_idx[tid + h], s_key[tid], s_idx[tid])) {
                s_key[tid] = s_key[tid + h];
                s_idx[tid] = s_idx[tid + h];
            }
            __syncthreads();
        }
        const int best = s_idx[0];
        __syncthreads();                                                      // (every lane has read s_idx[0] before the next round writes)
        if (best < 0) break;                                                  // (the same for every lane)
        if (round == 0) { worst = best; if (tid == 0) worst_chi2 = edges[best].chi2; }
        if (round >= par.max_reject) break;
        if ((best & (kPrLanes - 1)) == tid) edges[best].flags |= LSD_PG_EDGE_DISABLED | LSD_PG_EDGE_REJECTED;
        rejected++;
    }
    int left = 0;
    for (int e = tid; e < E; e += kPrLanes) left += (edges[e].flags & LSD_PG_EDGE_CLOSURE) && !(edges[e].flags & LSD_PG_EDGE_DISABLED);
    if (left) atomicAdd(&s_int[1], left);
    __syncthreads();
    if (tid == 0) {
        lsd_pg_prune_rep* o = reps + g;
        o->candidates = s_int[0]; o->rejected = rejected; o->worst_edge = worst; o->closures_left = s_int[1]; o->worst_chi2 = worst_chi2;
    }
}

void launch_pg_prune(int n_graphs, const lsd_pg_head* heads, lsd_pg_edge* edges, int edges_cap, lsd_pg_prune_par par, lsd_pg_prune_rep* rep,
                     hipStream_t st) {
    hipLaunchKernelGGL(k_pg_prune, dim3(n_graphs), dim3(kPrLanes), 0, st, heads, edges, edges_cap, par, rep);
}

}  // namespace lsdhip
