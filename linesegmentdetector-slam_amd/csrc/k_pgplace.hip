// k_pgplace.hip -- place recognition for the pose graph (include/lsd_hip.h, "pose graph", is the rule; restated in
// tests/pose_graph_place_cases.py): a 64-sector descriptor of every keyframe's scan (k_pg_describe), the distance of the query's descriptor
// to every old one at every circular shift (k_pg_place_score: the hot path, integers only), and the best distinct places with the near
// record, the selection and the gathered query of the chosen one (k_pg_place_pick: pgplace_dev.h's pl_pick_rounds, posegraph_dev.h's pg_hand_over).
// One quantisation in fp64 without FMA; every sum after it is an integer's, so no order matters.
#include "lsd_internal.h"
#include "pgplace_dev.h"
#include "posegraph_dev.h"

namespace lsdhip {

constexpr int kPlScoreLanes = 64;
static_assert(sizeof(lsd_polar) == 16, "a reading is one 16-byte access");

// One workgroup per row: the lanes stride over the readings (16 bytes each), two arrays of 64 counters in LDS, 64 lanes write the record.
__global__ __launch_bounds__(kPlLanes) void k_pg_describe(const lsd_pg_head* head, int nodes_cap, const lsd_polar* __restrict__ store,
                                                          const int* __restrict__ store_lens, int store_stride, double range_max,
                                                          lsd_pg_desc* desc) {
    __shared__ uint32_t s_sum[kPlSectors], s_cnt[kPlSectors], s_tot[2];
    const int tid = (int)threadIdx.x;
    const int n_nodes = pg_n_nodes(head, nodes_cap);
    for (int k = (int)blockIdx.x; k < n_nodes; k += (int)gridDim.x) {
        if (desc[k].valid != 0) continue;                                     // (the same for every lane; nobody else writes row k)
        if (tid < kPlSectors) { s_sum[tid] = 0u; s_cnt[tid] = 0u; }
        if (tid < 2) s_tot[tid] = 0u;
        __syncthreads();
        const int len = min(max(store_lens[k], 0), store_stride);
        const double2* row = reinterpret_cast<const double2*>(store + (size_t)k * (size_t)store_stride);
        for (int i = tid; i < len; i += kPlLanes) {
            const double2 b = row[i];                                         // (range, angle)
            if (!(isfinite(b.x) && b.x > 0 && b.x <= range_max && isfinite(b.y))) continue;
            const double t = b.y / 6.283185307179586;
            const double f = t - floor(t);
            int s = (int)(f * 64.0);
            if (s > 63) s = 63;
            int q = (int)(b.x / range_max * 255.0);
            if (q > 254) q = 254;
            atomicAdd(&s_sum[s], (uint32_t)q);
            atomicAdd(&s_cnt[s], 1u);
        }
        __syncthreads();
        if (tid < kPlSectors) {
            const uint32_t c = s_cnt[tid];
            desc[k].v[tid] = (uint8_t)(c ? s_sum[tid] / c : 255u);
            if (c) { atomicAdd(&s_tot[0], c); atomicAdd(&s_tot[1], 1u); }
        }
        __syncthreads();
        if (tid == 0) { desc[k].n_hits = s_tot[0]; desc[k].n_sectors = (uint16_t)s_tot[1]; desc[k].valid = 1; }
        __syncthreads();                                                      // (the counters are cleared again for the next row)
    }
}

// One lane per candidate (pgplace_dev.h: pl_score); the query is the same for every lane and sits in LDS (pl_stage_query).
// Workgroups of one wavefront: 16384 nodes are 256 of them, one per CU.
__global__ __launch_bounds__(kPlScoreLanes) void k_pg_place_score(const lsd_pg_head* head, int nodes_cap, const lsd_pg_track* track,
                                                             const lsd_pg_desc* __restrict__ desc, int gap, uint32_t max_dist,
                                                             uint32_t min_sectors, uint32_t* __restrict__ work) {
    __shared__ uint32_t s_q[4][32];
    const int tid = (int)threadIdx.x;
    const int n_nodes = pg_n_nodes(head, nodes_cap), j = track->last;
    const bool usable = pl_usable(desc, j, n_nodes, min_sectors);
    if (usable) pl_stage_query(desc, j, s_q, tid, kPlScoreLanes);
    __syncthreads();
    const int limit = usable ? j - gap : -1;                                  // the last index that can be a candidate
    for (int i = (int)blockIdx.x * kPlScoreLanes + tid; i < n_nodes; i += (int)gridDim.x * kPlScoreLanes)
        work[i] = i <= limit ? pl_score(desc, i, s_q, min_sectors, max_dist) : kPlNone;
}

// pl_pick_rounds over d_work, then pg_hand_over for the anchor of round `pick`, turned by its shift.  The host entry passes
// out.rec == nullptr: the records and the report only.  (The candidates are added to s_n with no barrier of their own: the rounds' -- the
// first round always meets them -- and the one in front of the report stand between the atomics and the reads.)
__global__ __launch_bounds__(kPlLanes) void k_pg_place_pick(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap,
                                                            const lsd_pg_track* track, const lsd_polar* store, const int* store_lens,
                                                            int store_stride, const lsd_pg_desc* desc, lsd_pg_place_par par,
                                                            const uint32_t* work, lsd_pg_place_rec* recs, lsd_pg_place_rep* rep, PgHandOver out) {
    __shared__ unsigned long long s_key[kPlLanes];
    __shared__ int s_n;
    const int tid = (int)threadIdx.x;
    const int n_nodes = pg_n_nodes(head, nodes_cap), j = track->last;
    const int limit = pl_usable(desc, j, n_nodes, par.min_sectors) ? j - par.gap : -1;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int cand = 0;
    for (int i = tid; i <= limit; i += kPlLanes) cand += work[i] != kPlNone;
    if (cand) atomicAdd(&s_n, cand);

    lsd_pg_place_rec a;                                                       // the record of round `pick`
    const int n_picked = pl_pick_rounds([&](int i) { return work[i]; }, limit, par, recs, s_key, tid, a);
    __syncthreads();
    if (tid == 0) { rep->query = j; rep->n_cand = s_n; rep->n_picked = n_picked; rep->reserved = 0; }
    if (!out.rec) return;
    const PgPose qp = tid == 0 && a.anchor >= 0 ? pg_turned(nodes, a.anchor, a.shift) : PgPose{0.0, 0.0, 0.0};
    pg_hand_over(nodes, nodes_cap, n_nodes, store, store_lens, store_stride, par.gap, par.window, j, a.anchor, s_n, (double)a.dist, qp, out, tid, kPlLanes);
}

void launch_pg_describe(const lsd_pg_head* head, int nodes_cap, const lsd_polar* store, const int* store_lens, int store_stride, double range_max,
                        lsd_pg_desc* desc, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_describe, dim3(min(nodes_cap, 2048)), dim3(kPlLanes), 0, st, head, nodes_cap, store, store_lens, store_stride, range_max,
                       desc);
}

void launch_pg_recognize(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_track* track, const lsd_polar* store,
                         const int* store_lens, int store_stride, const lsd_pg_desc* desc, lsd_pg_place_par par, uint32_t* work,
                         lsd_pg_place_rec* recs, lsd_pg_place_rep* rep, PgHandOver out, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_place_score, dim3((nodes_cap + kPlScoreLanes - 1) / kPlScoreLanes), dim3(kPlScoreLanes), 0, st, head, nodes_cap, track, desc, par.gap,
                       par.max_dist, par.min_sectors, work);
    hipLaunchKernelGGL(k_pg_place_pick, dim3(1), dim3(kPlLanes), 0, st, head, nodes, nodes_cap, track, store, store_lens, store_stride, desc, par, work,
                       recs, rep, out);
}

}  // namespace lsdhip
