// k_pgplace.hip -- place recognition for the pose graph (include/lsd_hip.h, "pose graph", is the rule; restated in
// tests/pose_graph_place_cases.py): a 64-sector descriptor of every keyframe's scan (k_pg_describe), the distance of the query's descriptor
// to every old one at every circular shift (k_pg_place_score: the hot path, integers only), and the best distinct places with the near
// record, the selection and the gathered query of the chosen one (k_pg_place_pick, after k_pg_prune's rounds and k_pg_near's outputs).
// One quantisation in fp64 without FMA; every sum after it is an integer's, so no order matters.
#include "lsd_internal.h"
#include "pgplace_dev.h"
#include "posegraph_dev.h"

namespace lsdhip {

constexpr int kPlLanes = 256, kPlScoreLanes = 64;
static_assert(sizeof(lsd_polar) == 16, "a reading is one 16-byte access");

// One workgroup per row: the lanes stride over the readings (16 bytes each), two arrays of 64 counters in LDS, 64 lanes write the record.
__global__ __launch_bounds__(kPlLanes) void k_pg_describe(const lsd_pg_head* head, int nodes_cap, const lsd_polar* __restrict__ store,
                                                          const int* __restrict__ store_lens, int store_stride, double range_max,
                                                          lsd_pg_desc* desc) {
    __shared__ uint32_t s_sum[kPlSectors], s_cnt[kPlSectors], s_tot[2];
    const int tid = (int)threadIdx.x;
    const int n_nodes = min(max(head->n_nodes, 0), nodes_cap);
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
    const int n_nodes = min(max(head->n_nodes, 0), nodes_cap), j = track->last;
    const bool usable = pl_usable(desc, j, n_nodes, min_sectors);
    if (usable) pl_stage_query(desc, j, s_q, tid, kPlScoreLanes);
    __syncthreads();
    const int limit = usable ? j - gap : -1;                                  // the last index that can be a candidate
    for (int i = (int)blockIdx.x * kPlScoreLanes + tid; i < n_nodes; i += (int)gridDim.x * kPlScoreLanes)
        work[i] = i <= limit ? pl_score(desc, i, s_q, min_sectors, max_dist) : kPlNone;
}

// The rounds of k_pg_prune with (dist, i) ascending as the order, then the outputs of k_pg_near for the anchor of round `pick`.  The host
// entry passes near_rec == nullptr: the records and the report only.
__global__ __launch_bounds__(kPlLanes) void k_pg_place_pick(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap,
                                                            const lsd_pg_track* track, const lsd_polar* store, const int* store_lens,
                                                            int store_stride, const lsd_pg_desc* desc, lsd_pg_place_par par,
                                                            const uint32_t* work, lsd_pg_place_rec* recs, lsd_pg_place_rep* rep,
                                                            lsd_pg_near_rec* near_rec, lsd_position* sel, lsd_polar* q_scan, int* q_len,
                                                            lsd_position* q_pose) {
    __shared__ unsigned long long s_key[kPlLanes];
    __shared__ int s_n;
    const int tid = (int)threadIdx.x;
    const int n_nodes = min(max(head->n_nodes, 0), nodes_cap), j = track->last;
    const bool has_q = j >= 0 && j < n_nodes;
    const int limit = pl_usable(desc, j, n_nodes, par.min_sectors) ? j - par.gap : -1;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int cand = 0;
    for (int i = tid; i <= limit; i += kPlLanes) cand += work[i] != kPlNone;
    if (cand) atomicAdd(&s_n, cand);

    int picked[LSD_PG_PLACE_MAX];                                             // the anchors so far: the same in every lane
    int n_picked = 0, anchor = -1, a_shift = 0;
    uint32_t a_dist = 0u;
    bool dry = false;
#pragma unroll
    for (int r = 0; r < LSD_PG_PLACE_MAX; r++) {
        if (r >= par.k) break;
        int best_i = -1, best_shift = 0;
        uint32_t best_dist = 0u;
        if (!dry) {
            unsigned long long km = ~0ull;
            for (int i = tid; i <= limit; i += kPlLanes) {
                const uint32_t w = work[i];
                if (w == kPlNone) continue;
                bool open = true;
#pragma unroll
                for (int p = 0; p < LSD_PG_PLACE_MAX; p++) if (p < n_picked && abs(i - picked[p]) <= par.spread) open = false;
                if (open) km = min(km, ((unsigned long long)(w >> 6) << 32) | (unsigned long long)(uint32_t)i);
            }
            s_key[tid] = km;
            __syncthreads();
            for (int h = kPlLanes / 2; h >= 1; h >>= 1) {
                if (tid < h) s_key[tid] = min(s_key[tid], s_key[tid + h]);
                __syncthreads();
            }
            const unsigned long long top = s_key[0];
            __syncthreads();                                                  // (every lane has read s_key[0] before the next round writes)
            if (top == ~0ull) dry = true;                                     // (the same for every lane: no later round finds one either)
            else {
                best_i = (int)(uint32_t)top;
                best_dist = (uint32_t)(top >> 32);
                best_shift = (int)(work[best_i] & 63u);
            }
        }
        picked[r] = best_i;
        if (best_i >= 0) n_picked++;
        if (r == par.pick) { anchor = best_i; a_shift = best_shift; a_dist = best_dist; }
        if (tid == 0) { recs[r].anchor = best_i; recs[r].shift = best_shift; recs[r].dist = best_dist; recs[r].reserved = 0u; }
    }
    __syncthreads();
    if (tid == 0) { rep->query = j; rep->n_cand = s_n; rep->n_picked = n_picked; rep->reserved = 0; }
    if (!near_rec) return;
    if (tid == 0) {
        near_rec->anchor = anchor; near_rec->query = j; near_rec->n_cand = s_n; near_rec->reserved = 0;
        near_rec->d2 = anchor >= 0 ? (double)a_dist : 0.0;
        q_pose->x = anchor >= 0 ? nodes[anchor].x : -1.0;
        q_pose->y = anchor >= 0 ? nodes[anchor].y : 0.0;
        q_pose->ang = anchor >= 0 ? pg_wrap(nodes[anchor].ang - (double)a_shift * 5.625) : 0.0;
        *q_len = has_q ? store_lens[j] : 0;
    }
    for (int k = tid; k < nodes_cap; k += kPlLanes) {
        const bool in = anchor >= 0 && abs(k - anchor) <= par.window && k <= j - par.gap;
        sel[k].x = in ? nodes[k].x : -1.0;
        sel[k].y = in ? nodes[k].y : 0.0;
        sel[k].ang = in ? nodes[k].ang : 0.0;
    }
    if (has_q) {
        const lsd_polar* src = store + (size_t)j * (size_t)store_stride;
        for (int i = tid; i < store_stride; i += kPlLanes) q_scan[i] = src[i];
    }
}

void launch_pg_describe(const lsd_pg_head* head, int nodes_cap, const lsd_polar* store, const int* store_lens, int store_stride, double range_max,
                        lsd_pg_desc* desc, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_describe, dim3(min(nodes_cap, 2048)), dim3(kPlLanes), 0, st, head, nodes_cap, store, store_lens, store_stride, range_max,
                       desc);
}

void launch_pg_recognize(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_track* track, const lsd_polar* store,
                         const int* store_lens, int store_stride, const lsd_pg_desc* desc, lsd_pg_place_par par, uint32_t* work,
                         lsd_pg_place_rec* recs, lsd_pg_place_rep* rep, lsd_pg_near_rec* near_rec, lsd_position* sel, lsd_polar* q_scan, int* q_len,
                         lsd_position* q_pose, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_place_score, dim3((nodes_cap + kPlScoreLanes - 1) / kPlScoreLanes), dim3(kPlScoreLanes), 0, st, head, nodes_cap, track, desc, par.gap,
                       par.max_dist, par.min_sectors, work);
    hipLaunchKernelGGL(k_pg_place_pick, dim3(1), dim3(kPlLanes), 0, st, head, nodes, nodes_cap, track, store, store_lens, store_stride, desc, par, work,
                       recs, rep, near_rec, sel, q_scan, q_len, q_pose);
}

}  // namespace lsdhip
