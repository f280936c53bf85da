// k_gridresponse.hip -- the response around a correlative match (gfx950): from the record either search wrote (k_gridmatch.hip,
// k_gridmatch_mr.hip), the scores R in a small neighbourhood of the winner, their integer moments -- a covariance in Karto's sense -- and a
// parabola through the winner and its two neighbours on each axis -- the sub-cell, sub-step pose.  No reference counterpart.  The rule
// (include/lsd_hip.h) is integer sums until one fp64 division per output, so a numpy restatement
// (tests/grid_response_cases.py) gives the same bytes.  No atomics.
//
// k_grid_response: a grid of n_scans x (2 ra + 1) workgroups of 256 lanes, one per (scan, angle offset a').  Whether the scan gets a
//   response is read from its record and is the same decision in every lane of both kernels; a scan without one gets zeros in the volume.
//   A. gm_end_cells (gridmatch_dev.h: the matchers' own text, so that no end cell can round apart) at the ORIGINAL pose and the angle
//      ang + (da + a') * ang_step, with the symmetric window |di| + rx, |dj| + ry -- a superset of the cells di + i', dj + j' can reach:
//      the list only has to hold every beam that can add something.  32 KiB of end cells plus 16 bytes of counts in LDS.
//   B. the (2 ry + 1)(2 rx + 1) <= 225 translations in ONE pass: each gets gm_split(n) adjacent lanes (4 for 49, 16 for 9) and
//      gm_score_split, because a walk of the list is a chain of dependent gathers.  R goes to the volume, i' fastest.
// k_grid_response_finish: one wavefront per scan.  The lanes stride over the at most 15^3 = 3375 values of the scan's volume and keep the
//   ten int64 moments and n_used in registers; eleven butterfly reductions by shuffles; lane 0 reads the centre and its six neighbours
//   again, does the three parabolas and the six divisions and writes the record as 24 64-bit words.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950, -O3):
//   k_grid_response          VGPRs 52   SGPRs 90   scratch 0 bytes   LDS 32784 bytes   4 waves / SIMD (the LDS: four workgroups per CU)
//   k_grid_response_finish   VGPRs 54   SGPRs 52   scratch 0 bytes   LDS     0 bytes   8 waves / SIMD
#include "lsd_internal.h"
#include "gridmatch_dev.h"

namespace lsdhip {

constexpr int kGrMaxR = 7;                                           // rx, ry, ra
static_assert((2 * kGrMaxR + 1) * (2 * kGrMaxR + 1) <= kGmLanes, "the translations of one angle are one pass of the workgroup");
// W <= 15^3 * 255 * 4096 < 2^32 and i'^2 <= 49: every moment stays below 2^38
static_assert(3375ll * 255 * kGmMaxBeams * kGrMaxR * kGrMaxR < (1ll << 38), "the moments are exact in int64 and in double");

// the record's say on whether the scan gets a response (caller memory: the range test makes noise harmless)
__device__ __forceinline__ bool gr_has_response(uint32_t flags, int di, int dj, int da) {
    return (flags & LSD_GRID_MATCH_ACCEPTED) && !(flags & LSD_GRID_MATCH_SKIPPED) && di >= -kGmMaxWin && di <= kGmMaxWin && dj >= -kGmMaxWin &&
           dj <= kGmMaxWin && da >= -kGmMaxWin && da <= kGmMaxWin;
}

__global__ __launch_bounds__(kGmLanes) void k_grid_response(const double2* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                            const uint8_t* __restrict__ poses, size_t pose_pitch,
                                                            const lsd_grid_match_rec* __restrict__ recs, int cols, int rows, double resol,
                                                            double range_max, const uint8_t* __restrict__ corr, double ang_step, int rx, int ry,
                                                            int ra, uint32_t* __restrict__ volume) {
    __shared__ int2 s_end[kGmMaxBeams];
    __shared__ int s_cnt[kGmLanes / 64];
    const int scan = blockIdx.x, ai = blockIdx.y, tid = threadIdx.x;
    const int nx = 2 * rx + 1, n_tr = nx * (2 * ry + 1);
    uint32_t* mine = volume + ((size_t)scan * (2 * ra + 1) + ai) * n_tr;
    const lsd_grid_match_rec* rec = recs + scan;
    const int di = rec->di, dj = rec->dj, da = rec->da;
    if (!gr_has_response(rec->flags, di, dj, da)) {
        if (tid < n_tr) mine[tid] = 0;
        return;
    }
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    // A. the end cells of this angle (gridmatch_dev.h); a pose the scan test skips (no authentic record has one) scores no beam
    int n_list = 0;
    if (!gm_scan_skipped(px, py, pang)) {
        const int len = min(max(lens[scan], 0), stride);             // (stride <= kGmMaxBeams: the entry refuses more)
        const double rot0 = deg2rad_ref(pang), rot = deg2rad_ref(pang + (double)(da + ai - ra) * ang_step);
        uint32_t nb = 0;
        n_list = gm_end_cells(scans + (size_t)scan * stride, len, px, py, rot0, rot, resol, range_max, cols, rows, (di < 0 ? -di : di) + rx,
                              (dj < 0 ? -dj : dj) + ry, 0, 0, s_end, s_cnt, nb);
    }
    // B. the translations, P lanes each
    const int P = gm_split(n_tr), t = tid / P, sub = tid & (P - 1);
    const bool act = t < n_tr;
    const int jj = t / nx, ii = t - jj * nx;
    const uint32_t R = gm_score_split(s_end, n_list, corr, cols, rows, di + ii - rx, dj + jj - ry, sub, P, act);
    if (act && sub == 0) mine[t] = R;
}

// the offset of the parabola's peak through (-1, m), (0, c), (1, p); not a peak: +0.0 and the axis's bit
__device__ __forceinline__ double gr_parabola(long long m, long long c, long long p, uint32_t bit, uint32_t& flags) {
    const long long num = m - p, den = 2 * (m - 2 * c + p);
    if (m > c || p > c || den >= 0) {
        flags |= bit;
        return 0.0;
    }
    if (num == 0) return 0.0;                                        // (0 / den is -0.0)
    return (double)num / (double)den;
}

__global__ __launch_bounds__(64) void k_grid_response_finish(const unsigned long long* __restrict__ recs, const uint32_t* __restrict__ volume,
                                                             double ang_step, int rx, int ry, int ra, uint32_t keep_num, uint32_t keep_den,
                                                             unsigned long long* __restrict__ out) {
    const int scan = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* rw = recs + (size_t)scan * (sizeof(lsd_grid_match_rec) / 8);
    const unsigned long long w0 = rw[0], w1 = rw[1], w2 = rw[2], w3 = rw[3], w4 = rw[4], w5 = rw[5];
    const uint32_t score = (uint32_t)w3, mflags = (uint32_t)(w5 >> 32);
    const int di = (int)(uint32_t)w4, dj = (int)(uint32_t)(w4 >> 32), da = (int)(uint32_t)w5;
    unsigned long long* o = out + (size_t)scan * (sizeof(lsd_grid_response_rec) / 8);
    if (!gr_has_response(mflags, di, dj, da)) {
        if (lane == 0) {
            o[0] = w0; o[1] = w1; o[2] = w2;                         // the pose as bits: what is copied is copied exactly
            for (int k = 3; k < 23; k++) o[k] = 0;
            o[23] = (unsigned long long)LSD_GRID_RESPONSE_NONE;
        }
        return;
    }
    const int nx = 2 * rx + 1, ny = 2 * ry + 1, n_tr = nx * ny, n_vol = n_tr * (2 * ra + 1);
    const uint32_t* vol = volume + (size_t)scan * n_vol;
    const unsigned long long thr = (unsigned long long)score * keep_num;
    long long m[10];
#pragma unroll
    for (int k = 0; k < 10; k++) m[k] = 0;
    uint32_t n_used = 0;
    for (int idx = lane; idx < n_vol; idx += 64) {
        const uint32_t R = vol[idx];
        if ((unsigned long long)R * keep_den >= thr) {
            const int aa = idx / n_tr, rem = idx - aa * n_tr, jj = rem / nx;
            const long long i = rem - jj * nx - rx, j = jj - ry, a = aa - ra, w = R;
            n_used++;
            m[0] += w; m[1] += w * i; m[2] += w * j; m[3] += w * a;
            m[4] += w * i * i; m[5] += w * i * j; m[6] += w * j * j;
            m[7] += w * i * a; m[8] += w * j * a; m[9] += w * a * a;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 10; k++) m[k] += (long long)shfl_xor_u64((unsigned long long)m[k], d);
        n_used += (uint32_t)__shfl_xor((int)n_used, d, 64);
    }
    if (lane != 0) return;
    const int at = (ra * ny + ry) * nx + rx;                         // the winner's place in the volume
    const long long c = vol[at];
    uint32_t flags = LSD_GRID_RESPONSE_VALID | ((uint32_t)c != score ? LSD_GRID_RESPONSE_MISMATCH : 0u);
    double sub[3];
    sub[0] = gr_parabola(vol[at - 1], c, vol[at + 1], LSD_GRID_RESPONSE_X_NOT_PEAK, flags);
    sub[1] = gr_parabola(vol[at - nx], c, vol[at + nx], LSD_GRID_RESPONSE_Y_NOT_PEAK, flags);
    sub[2] = ra > 0 ? gr_parabola(vol[at - n_tr], c, vol[at + n_tr], LSD_GRID_RESPONSE_A_NOT_PEAK, flags) : 0.0;
    double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m[0] > 0) {
        const double W = (double)m[0];
        cov[0] = (double)m[4] / W;
        cov[1] = (double)m[5] / W;
        cov[2] = (double)m[6] / W;
        cov[3] = ((double)m[7] / W) * ang_step;
        cov[4] = ((double)m[8] / W) * ang_step;
        cov[5] = ((double)m[9] / W) * (ang_step * ang_step);
    } else {
        flags |= LSD_GRID_RESPONSE_EMPTY;
    }
    const double x = __longlong_as_double((long long)w0) + sub[0], y = __longlong_as_double((long long)w1) + sub[1];
    const double ang = __longlong_as_double((long long)w2) + sub[2] * ang_step;
    o[0] = (unsigned long long)__double_as_longlong(x);
    o[1] = (unsigned long long)__double_as_longlong(y);
    o[2] = (unsigned long long)__double_as_longlong(ang);
#pragma unroll
    for (int k = 0; k < 6; k++) o[3 + k] = (unsigned long long)__double_as_longlong(cov[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) o[9 + k] = (unsigned long long)__double_as_longlong(sub[k]);
#pragma unroll
    for (int k = 0; k < 10; k++) o[12 + k] = (unsigned long long)m[k];
    o[22] = (unsigned long long)(uint32_t)c | ((unsigned long long)n_used << 32);
    o[23] = (unsigned long long)flags;
}

static_assert(sizeof(lsd_grid_response_rec) == 192 && offsetof(lsd_grid_response_rec, cov) == 24 && offsetof(lsd_grid_response_rec, sub) == 72 &&
              offsetof(lsd_grid_response_rec, m) == 96 && offsetof(lsd_grid_response_rec, score_centre) == 176 &&
              offsetof(lsd_grid_response_rec, n_used) == 180 && offsetof(lsd_grid_response_rec, flags) == 184 &&
              offsetof(lsd_grid_response_rec, reserved) == 188,
              "k_grid_response_finish writes the record as 24 64-bit words");
static_assert(sizeof(lsd_grid_match_rec) == 56 && offsetof(lsd_grid_match_rec, score) == 24 && offsetof(lsd_grid_match_rec, di) == 32 &&
              offsetof(lsd_grid_match_rec, dj) == 36 && offsetof(lsd_grid_match_rec, da) == 40 && offsetof(lsd_grid_match_rec, flags) == 44,
              "k_grid_response_finish reads the match record as 64-bit words");

size_t grid_response_volume_bytes(int n_scans, const lsd_grid_response_par& rp) {
    return (size_t)n_scans * (2 * rp.ra + 1) * (2 * rp.ry + 1) * (2 * rp.rx + 1) * sizeof(uint32_t);
}

void launch_grid_response(const GridScans& g, const lsd_grid_match_rec* records, const uint8_t* corr, double ang_step, const lsd_grid_response_par& rp,
                          uint32_t* volume, lsd_grid_response_rec* out, hipStream_t s) {
    hipLaunchKernelGGL(k_grid_response, dim3(g.n_scans, 2 * rp.ra + 1), dim3(kGmLanes), 0, s, reinterpret_cast<const double2*>(g.scans), g.lens,
                       g.stride, static_cast<const uint8_t*>(g.poses), g.pose_pitch, records, g.cols, g.rows, g.resol, g.range_max, corr, ang_step,
                       rp.rx, rp.ry, rp.ra, volume);
    hipLaunchKernelGGL(k_grid_response_finish, dim3(g.n_scans), dim3(64), 0, s, reinterpret_cast<const unsigned long long*>(records), volume, ang_step,
                       rp.rx, rp.ry, rp.ra, rp.keep_num, rp.keep_den, reinterpret_cast<unsigned long long*>(out));
}

}  // namespace lsdhip
