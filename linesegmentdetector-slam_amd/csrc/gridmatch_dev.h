// gridmatch_dev.h -- what the two correlative matchers share (k_gridmatch.hip: the plain search; k_gridmatch_mr.hip: the coarse-to-fine
// one): the packed key whose maximum IS the rule's winner, the (scan, angle) slot k_grid_match_pick reads, the scan's skip test, and
// phase A -- the end cells of one (scan, angle) compacted into LDS.  One text for both, so that the two cannot round an end cell apart.
#pragma once
#include "lsd_internal.h"
#include "match_dev.h"

namespace lsdhip {

constexpr int kGmLanes = 256, kGmMaxBeams = LSD_SCAN_MAX_LEN, kBeamBatch = 8;
constexpr int kGmMaxWin = 63;                                        // wx, wy, na
// the key's fields: i^2 + j^2 <= 2 * 63^2 = 7938 < 2^13, |a| <= 63 < 2^6, the linear index < 127^3 = 2048383 < 2^21 - 1, S < 2^20
constexpr int kKeyLinBits = 21, kKeyAngBits = 6, kKeyDistBits = 13;
constexpr int kKeyAngShift = kKeyLinBits, kKeyDistShift = kKeyLinBits + kKeyAngBits, kKeyScoreShift = kKeyDistShift + kKeyDistBits;
static_assert(255ll * kGmMaxBeams < (1 << 20) && kKeyScoreShift + 20 <= 64, "the score fits its field");
static_assert((2 * kGmMaxWin + 1) * (2 * kGmMaxWin + 1) * (2 * kGmMaxWin + 1) < (1 << kKeyLinBits) - 1, "a real key is never 0");

struct GmSlot { unsigned long long key; uint32_t nb, s0; };          // per (scan, angle): the best key, the scored beams, S at (j, i) = (0, 0)
static_assert(sizeof(GmSlot) == 16, "lsd_grid.hip sizes the workspace by 16 bytes a slot");

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {      // every lane gets the maximum
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = shfl_xor_u64(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// the scan skipped whole: k_grid_integrate's test
__device__ __forceinline__ bool gm_scan_skipped(double px, double py, double pang) {
    return !(isfinite(px) && isfinite(py) && isfinite(pang)) || fabs(px + 1) < 1e-4 || fabs(px) > 1048576.0 || fabs(py) > 1048576.0;
}

// the key of the candidate (ai - na, jj - wy, ii - wx) with the score S
__device__ __forceinline__ unsigned long long gm_key(uint32_t S, int i, int j, uint32_t aa, uint32_t lin) {
    return ((unsigned long long)S << kKeyScoreShift) |
           ((unsigned long long)(((1u << kKeyDistBits) - 1) - (uint32_t)(i * i + j * j)) << kKeyDistShift) |
           ((unsigned long long)(((1u << kKeyAngBits) - 1) - aa) << kKeyAngShift) | (unsigned long long)(((1u << kKeyLinBits) - 1) - lin);
}

// Phase A, by all 256 lanes of a workgroup: one lane per beam, 256 at a time -- the integration's skip tests, sincos_g ONCE per (beam,
// angle), the rounded end cell.  `nb` gains this lane's scored beams.  The end cells of the beams whose window -- wx, wy cells to the low
// side, wx + over_x, wy + over_y to the high side -- touches the grid at all are compacted into s_end in beam order (ballot / mbcnt inside
// a wavefront, s_cnt[4] across them); the others add 0 to every candidate.  Returns the length of the list (uniform).  Ends with a barrier.
__device__ __forceinline__ int gm_end_cells(const double2* __restrict__ row, int len, double px, double py, double rot0, double rot, double resol,
                                            double range_max, int cols, int rows, int wx, int wy, int over_x, int over_y, int2* s_end, int* s_cnt,
                                            uint32_t& nb) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n_list = 0;
    for (int base = 0; base < len; base += kGmLanes) {
        const int i = base + tid;
        bool keep = false;
        int ex = 0, ey = 0;
        if (i < len) {
            const double2 b = row[i];
            const double th0 = b.y + rot0, th = b.y + rot;
            if (b.x > 0 && b.x != (double)INFINITY && isfinite(b.y) && isfinite(th0) && b.x <= range_max && isfinite(th)) {
                double s, c;
                sincos_g(th, s, c);
                ex = cvt_x86(round(px + b.x * c / resol));
                ey = cvt_x86(round(py + b.x * s / resol));
                nb++;
                // |ex|, |ey| < 2^20 + 32768: the sums below cannot wrap
                keep = ex + wx + over_x >= 0 && ex - wx < cols && ey + wy + over_y >= 0 && ey - wy < rows;
            }
        }
        const unsigned long long m = __ballot(keep);
        const int below = lanes_below(m);
        if (lane == 0) s_cnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int at = n_list, total = 0;
        for (int w = 0; w < kGmLanes / 64; w++) {
            const int cnt = s_cnt[w];
            if (w < wave) at += cnt;
            total += cnt;
        }
        if (keep) s_end[at + below] = make_int2(ex, ey);              // at + below < n_list + total <= base + 256 <= kGmMaxBeams
        n_list += total;
        __syncthreads();                                             // the next chunk rewrites s_cnt; the caller reads s_end
    }
    return n_list;
}

// S of the translation (j, i): the sum over the list of corr[ey + j][ex + i], 0 outside the grid; the loads of kBeamBatch beams are issued
// before they are accumulated.  All lanes read the same list entry: a broadcast.
__device__ __forceinline__ uint32_t gm_score(const int2* s_end, int n_list, const uint8_t* __restrict__ corr, int cols, int rows, int i, int j) {
    uint32_t S = 0;
    for (int k0 = 0; k0 < n_list; k0 += kBeamBatch) {
        uint32_t v[kBeamBatch];
#pragma unroll
        for (int u = 0; u < kBeamBatch; u++) {
            v[u] = 0;
            if (k0 + u < n_list) {
                const int2 e = s_end[k0 + u];
                const int cx = e.x + i, cy = e.y + j;
                if (cx >= 0 && cx < cols && cy >= 0 && cy < rows) v[u] = corr[(size_t)cy * cols + cx];
            }
        }
#pragma unroll
        for (int u = 0; u < kBeamBatch; u++) S += v[u];
    }
    return S;
}

// The same sum with the list dealt over the P lanes of a group (P a power of two <= 64, adjacent lanes of one wavefront; `sub` this lane's
// place in it), kBeamBatch entries at a time: a lane walks n_list / P entries, and every lane of the group gets the whole sum.  Integer
// sums have no order, so the value is gm_score's.  Every lane of the wavefront calls it (the shuffles); act == false adds nothing.
__device__ __forceinline__ uint32_t gm_score_split(const int2* s_end, int n_list, const uint8_t* __restrict__ plane, int cols, int rows, int i, int j,
                                                   int sub, int P, bool act) {
    uint32_t S = 0;
    if (act) {
        for (int k0 = sub * kBeamBatch; k0 < n_list; k0 += P * kBeamBatch) {
            uint32_t v[kBeamBatch];
#pragma unroll
            for (int u = 0; u < kBeamBatch; u++) {
                v[u] = 0;
                if (k0 + u < n_list) {
                    const int2 e = s_end[k0 + u];
                    const int cx = e.x + i, cy = e.y + j;
                    if (cx >= 0 && cx < cols && cy >= 0 && cy < rows) v[u] = plane[(size_t)cy * cols + cx];
                }
            }
#pragma unroll
            for (int u = 0; u < kBeamBatch; u++) S += v[u];
        }
    }
    for (int d = P >> 1; d >= 1; d >>= 1) S += (uint32_t)__shfl_xor((int)S, d, 64);
    return S;
}

// the lanes a group gets when n_items items share the workgroup's 256: the largest power of two P <= 64 with P * n_items <= 256, else 1
__device__ __forceinline__ int gm_split(int n_items) {
    int P = 1;
    while (P < 64 && 2 * P * n_items <= kGmLanes) P *= 2;
    return P;
}

}  // namespace lsdhip
