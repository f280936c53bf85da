// pgplace_dev.h -- what place recognition's kernels share (k_pgplace.hip: one query per call; k_pgloops.hip: a range of queries per
// launch): the packed byte SAD, the usability test, the staging of the query turned by 0..3 bytes, the 64 shifts of one candidate and
// the rounds that pick the best distinct places among a row of keys (pl_pick_rounds).  One text, so that the batch's keys AND its choice
// among them are the single entry's by construction (include/lsd_hip.h, "pose graph", is the rule).
#pragma once
#include "lsd_internal.h"

namespace lsdhip {

constexpr int kPlSectors = LSD_PG_DESC_SECTORS, kPlLanes = 256;    // kPlLanes: the workgroup of the rounds
constexpr uint32_t kPlNone = 0xffffffffu;                         // the key of a node that is no candidate
static_assert(sizeof(lsd_pg_desc) == 72 && offsetof(lsd_pg_desc, n_hits) == 64 && offsetof(lsd_pg_desc, n_sectors) == 68 &&
              offsetof(lsd_pg_desc, valid) == 70, "lsd_pg_desc: 64 sector bytes, the counts behind them");
static_assert(kPlSectors == 64, "a descriptor is 16 dwords");

__device__ __forceinline__ uint32_t pl_sad(uint32_t a, uint32_t b, uint32_t acc) {
#if __has_builtin(__builtin_amdgcn_sad_u8)
    return __builtin_amdgcn_sad_u8(a, b, acc);                               // four |byte - byte| added to acc
#else
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
        acc += (uint32_t)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

__device__ __forceinline__ bool pl_usable(const lsd_pg_desc* desc, int j, int n_nodes, uint32_t min_sectors) {
    return j >= 0 && j < n_nodes && desc[j].valid != 0 && desc[j].n_sectors >= min_sectors;
}

// The query sits in LDS doubled and turned by 0..3 bytes -- s_q[r][w] holds a.v[(4 w + r + 0..3) mod 64] --, so that shift s = 4 m + r
// pairs the candidate's dword k with s_q[r][k + m]: one row of 32 broadcast dwords per r, no byte shuffles, 16 packed SADs per shift.
__device__ __forceinline__ void pl_stage_query(const lsd_pg_desc* desc, int j, uint32_t (*s_q)[32], int tid, int lanes) {
    for (int t = tid; t < 128; t += lanes) {
        const int r = t >> 5, w = t & 31;
        uint32_t d = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) d |= (uint32_t)desc[j].v[(4 * w + r + b) & 63] << (8 * b);
        s_q[r][w] = d;
    }
}

// The key of node i against the staged query: (D << 6) | s of the smallest D_s -- the smallest shift wins among equal distances in one
// unsigned minimum --, kPlNone for a node that is not described, has fewer than min_sectors sectors or lies beyond max_dist.  The
// candidate's 64 bytes in 16 registers.
__device__ __forceinline__ uint32_t pl_score(const lsd_pg_desc* __restrict__ desc, int i, const uint32_t (*s_q)[32], uint32_t min_sectors,
                                             uint32_t max_dist) {
    const uint2* cw = reinterpret_cast<const uint2*>(desc + i);              // (72-byte records, 8-byte aligned)
    const uint32_t tail = cw[8].y;                                            // (n_sectors: bytes 68..69, valid: 70..71)
    if ((tail >> 16) == 0u || (tail & 0xffffu) < min_sectors) return kPlNone;
    uint32_t c[16];
#pragma unroll
    for (int k = 0; k < 8; k++) { const uint2 v = cw[k]; c[2 * k] = v.x; c[2 * k + 1] = v.y; }
    uint32_t best = kPlNone;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        uint32_t q[32];
#pragma unroll
        for (int w = 0; w < 32; w++) q[w] = s_q[r][w];
#pragma unroll
        for (int m = 0; m < 16; m++) {
            uint32_t d = 0u;
#pragma unroll
            for (int k = 0; k < 16; k++) d = pl_sad(q[k + m], c[k], d);
            best = min(best, (d << 6) | (uint32_t)(4 * m + r));
        }
    }
    return (best >> 6) <= max_dist ? best : kPlNone;
}

// The smallest of the 256 lanes' keys, in every lane, through an LDS array of kPlLanes.  Three kinds of barrier: the keys are written,
// the tree's levels, and every lane has read s_key[0] before the next call writes.
__device__ __forceinline__ unsigned long long pl_min_key(unsigned long long km, unsigned long long* s_key, int tid) {
    s_key[tid] = km;
    __syncthreads();
    for (int h = kPlLanes / 2; h >= 1; h >>= 1) {
        if (tid < h) s_key[tid] = min(s_key[tid], s_key[tid + h]);
        __syncthreads();
    }
    const unsigned long long top = s_key[0];
    __syncthreads();
    return top;
}

// The rounds of k_pg_prune with (dist, i) ascending as the order, by every lane of ONE workgroup of kPlLanes: up to par.k rounds of one
// arg-min over the keys of the nodes 0..limit (key_at(i): the row stays in the caller's address space), a node within par.spread of an
// anchor picked so far being closed.  Lane 0 writes the par.k records to out; every lane gets the number picked and, in `chosen`, the
// record of round par.pick.  A round meets barriers (pl_min_key) unless an earlier one was dry; the first one always does.
// (par by value: taken by reference, k_pg_place_pick needs 102 scalar registers in the place of 100 and loses a wave per SIMD.)
template <class KeyAt>
__device__ __forceinline__ int pl_pick_rounds(KeyAt key_at, int limit, lsd_pg_place_par par, lsd_pg_place_rec* out, unsigned long long* s_key,
                                              int tid, lsd_pg_place_rec& chosen) {
    int picked[LSD_PG_PLACE_MAX];                                             // the anchors so far: the same in every lane
    int n_picked = 0;
    bool dry = false;
    chosen = lsd_pg_place_rec{-1, 0, 0u, 0u};
#pragma unroll
    for (int r = 0; r < LSD_PG_PLACE_MAX; r++) {
        if (r >= par.k) break;
        int best_i = -1, best_shift = 0;
        uint32_t best_dist = 0u;
        if (!dry) {
            unsigned long long km = ~0ull;
            for (int i = tid; i <= limit; i += kPlLanes) {
                const uint32_t w = key_at(i);
                if (w == kPlNone) continue;
                bool open = true;
#pragma unroll
                for (int p = 0; p < LSD_PG_PLACE_MAX; p++) if (p < n_picked && abs(i - picked[p]) <= par.spread) open = false;
                if (open) km = min(km, ((unsigned long long)(w >> 6) << 32) | (unsigned long long)(uint32_t)i);
            }
            const unsigned long long top = pl_min_key(km, s_key, tid);
            if (top == ~0ull) dry = true;                                     // (the same for every lane: no later round finds one either)
            else {
                best_i = (int)(uint32_t)top;
                best_dist = (uint32_t)(top >> 32);
                best_shift = (int)(key_at(best_i) & 63u);
            }
        }
        picked[r] = best_i;
        if (best_i >= 0) n_picked++;
        if (r == par.pick) chosen = lsd_pg_place_rec{best_i, best_shift, best_dist, 0u};
        if (tid == 0) { out[r].anchor = best_i; out[r].shift = best_shift; out[r].dist = best_dist; out[r].reserved = 0u; }
    }
    return n_picked;
}

}  // namespace lsdhip
