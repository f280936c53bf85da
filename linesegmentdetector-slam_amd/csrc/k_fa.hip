// k_fa.hip -- FeatureAssociation on the device: pair list, candidates, selection, fusion and the UKF update, gfx950, fp64.
//
// Replaces myfa::FeatureAssociation (LSD/myFA.cpp:13-184), myfa::ukf (:404-536) and the bookkeeping of the replay driver's frame loop
// (LSD/main_on_windows.cpp:125-183) for n_seq independent sequences at once (grid.y = sequence).  Three launches per frame index:
//   k_fa_prepare  one workgroup per sequence: ScanPose (from the odometry, or given), the rounded lidarPose, lastPose, and the
//                 pair list in the reference's loop order (scan line outer, map line inner) by ordered compaction
//   k_fa_match    one lane per candidate, a grid-stride loop over a small grid; reads the pair count from the device (match_dev.h)
//   k_fa_fuse     one workgroup per sequence: ordered compaction of score < 3, stable sort on (score, candidate index), the
//                 weighted mean on one lane, the UKF with one lane per matrix entry and sequential sums, state + report + the
//                 frame loop's angle bookkeeping (and, in the resumable loop, the carry after a sequence's last frame)
// Arithmetic order (the build has -ffp-contract=off): plain ascending sums from 0 for every dot product; LLT as Eigen's unblocked
// algorithm (size < 32); Xdiv * diag(Wc) rounded entry by entry before the product with Xdiv^T; the 3x3 inverse as Eigen's
// compute_inverse_size3 (cyclic cofactors, det = (c00 m00 + c10 m10) + c20 m20, inv(j, i) = cof(i, j) / det as a product with
// 1/det).  tests/fa_restatement.py states the same in Python; agreement with an Eigen build is not verified (no Eigen here).
#include "match_dev.h"

namespace lsdhip {

constexpr int kFaThreads = 256;
constexpr int kFaMatchBlocks = 8;                                  // wavefronts of k_fa_match per sequence

// Block-wide exclusive prefix of `flag` over the 256 lanes (four wavefronts); *total = the block's count.
__device__ __forceinline__ int fa_block_scan(bool flag, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
    for (int k = 0; k < kFaThreads / 64; k++) {
        const int v = s_w[k];
        if (k < w) off += v;
        total += v;
    }
    __syncthreads();
    return off + before;
}

__device__ __forceinline__ double fa_atand(double v) { return atan_g(v) * 180.0 / kPi; }    // baseFunc.cpp:14-16

// previous state of sequence s at frame t: the initial state (the carry's) at t = 0
__device__ __forceinline__ const lsd_fa_state* fa_prev(const FaArgs& a, int s) {
    if (a.t == 0) return a.carry ? &a.carry[s].state : a.init + s;
    return a.states + (size_t)s * a.frames_pitch + a.t - 1;
}

// Odom[cnt_frame - 1] and Odom[cnt_frame] of frame t
__device__ __forceinline__ void fa_odom(const FaArgs& a, int s, lsd_position& o0, lsd_position& o1) {
    if (a.carry) {
        const lsd_position* r = a.odom + (size_t)s * a.frames_pitch;
        o1 = r[a.t];
        o0 = a.t == 0 ? a.carry[s].odom : r[a.t - 1];
    } else {
        const lsd_position* r = a.odom + (size_t)s * (a.frames_pitch + 1);
        o0 = r[a.t];
        o1 = r[a.t + 1];
    }
}

// the loop's bookkeeping before frame t: the sum and length of angRotate, isOffset, and cnt_frame - 1 (empty before the first frame)
struct FaBook { double sum, cnt; bool offset; int frame; };
__device__ __forceinline__ FaBook fa_book(const FaArgs& a, int s) {
    if (a.t > 0) {
        const double* aux = a.aux + (size_t)s * kFaAux;
        return {aux[0], aux[1], aux[2] != 0, (int)aux[3]};
    }
    if (a.carry) {
        const lsd_fa_carry& c = a.carry[s];
        return {c.ang_sum, c.ang_count, c.is_offset != 0, c.frames};
    }
    return {0.0, 0.0, false, 0};
}

// The map of sequence s: the single map of the arguments (kMaps false: the entries that take one map), or record map_of[s] of the table
// (the fleet entries).  `live` false: the id is outside the table and the sequence sits the call out.  The sequence is the workgroup's
// (blockIdx.y), so the id and the record are uniform: plain loads through a const __restrict__ pointer, which the compiler keeps scalar.
// n_map is the count the pair list uses: the host's, or the device's (a map update still in flight when the tick was enqueued) held to
// its capacity -- an overflowed detector count leaves the first n_map records valid, a given-up image (-1) none.
struct FaMap { const double* cache; const lsd_line* lines; int cols, rows, n_map; double resol; bool live; };
template <bool kMaps>
__device__ __forceinline__ FaMap fa_map(const FaArgs& a, int s) {
    if constexpr (!kMaps) {
        return {a.map_cache, a.map_lines, a.cols, a.rows, a.d_n_map ? min(max(*a.d_n_map, 0), a.n_map) : a.n_map, a.map_resol, true};
    } else {
        const int32_t* __restrict__ of = a.map_of;
        const int id = of[s];
        if ((unsigned)id >= (unsigned)a.n_maps) return {nullptr, nullptr, 0, 0, 0, 1.0, false};
        const lsd_map_ref* __restrict__ m = a.maps + id;
        const int32_t* dn = m->d_n_map;
        const int cap = m->n_map;
        return {m->d_map_cache, m->d_map_lines, m->cols, m->rows, dn ? min(max(*dn, 0), cap) : cap, m->mapResol, true};
    }
}

template <bool kMaps>
__global__ __launch_bounds__(kFaThreads) void k_fa_prepare(FaArgs a) {
    const int s = blockIdx.y, tid = threadIdx.x;
    __shared__ int s_w[kFaThreads / 64];
    const FaMap mp = fa_map<kMaps>(a, s);
    const bool live = (!a.n_frames || a.t < a.n_frames[s]) && mp.live;
    if (!live) {                                                   // past the end of this sequence, or sitting out: k_fa_match scores nothing
        if (tid == 0) { a.n_pairs[s] = 0; a.n_cand[s] = 0; }
        return;
    }
    const size_t slot = (size_t)s * a.frames_pitch + a.t;
    const lsd_fa_state* prev = fa_prev(a, s);
    double* ctl = a.ctl + (size_t)s * kFaCtl;
    if (tid == 0) {
        const double* lp = a.lidar_pos + 2 * slot;
        ctl[0] = (double)cvt_x86(round(lp[0]));                    // trans2FA: (int)round(FS.lidarPos.x), main_on_windows.cpp:228-229
        ctl[1] = (double)cvt_x86(round(lp[1]));
        if (a.given) {                                             // one frame of lsd_feature_association: lastPose, ScanPose given
            for (int k = 0; k < 6; k++) ctl[2 + k] = a.given[6 * s + k];
        } else {
            ctl[2] = prev->x[0]; ctl[3] = prev->x[1]; ctl[4] = prev->x[2];      // lastPose = the last state's x[0..2] (:169-171)
            double spx = 0, spy = 0, spa = 0;
            if (!(fabs(prev->x[0] + 1) < 0.0001)) {                // :125-140
                const FaBook bk = fa_book(a, s);
                const double theta = bk.sum / bk.cnt;              // the mean of angRotate (0/0 if it is empty)
                lsd_position o0, o1;
                fa_odom(a, s, o0, o1);
                const double tx = (o1.x - o0.x) / mp.resol, ty = (o1.y - o0.y) / mp.resol, ta = fa_atand(o1.ang - o0.ang);
                double sd, cd;
                sincos_g(deg2rad_ref(theta), sd, cd);
                spx = tx * cd - ty * sd;
                spy = ty * sd + ty * cd;                           // (sic: ty twice, :137)
                spa = ta;
            }
            ctl[5] = spx; ctl[6] = spy; ctl[7] = spa;
        }
    }
    // the pair list of :28-58 in its loop order
    const int n_scan = min(a.n_lines ? a.n_lines[slot] : a.n_scan_given, a.line_pitch);
    const lsd_line* sl = a.scan_lines + slot * a.line_pitch;
    const int n_map = mp.n_map;
    const long long total = (long long)max(n_scan, 0) * n_map;
    int* pairs = a.pairs + (size_t)s * a.pair_cap * 2;
    int base = 0;
    for (long long b = 0; b < total; b += kFaThreads) {
        const long long q = b + tid;
        bool take = false;
        int cs = 0, cm = 0;
        if (q < total) {
            cs = (int)(q / n_map); cm = (int)(q % n_map);
            const double ls = sl[cs].len, lm = mp.lines[cm].len, ld = ls * 0.35;   // ignoreScanLength, scanToMapDiff (baseFunc.h:80-82)
            take = !(ls < 40) && !(lm < ls - ld || lm > ls + ld);
        }
        int cnt;
        const int pos = base + fa_block_scan(take, s_w, cnt);
        if (take) { pairs[2 * pos] = cm; pairs[2 * pos + 1] = cs; }   // pos < pair_cap: the capacity is n_map x line_pitch
        base += cnt;
    }
    if (tid == 0) { a.n_pairs[s] = base; a.n_cand[s] = 4 * base; }
}

template <bool kMaps>
__global__ __launch_bounds__(64) void k_fa_match(FaArgs a) {
    const int s = blockIdx.y;
    const int n_cand = a.n_cand[s];                                // the count is the device's: a grid-stride loop over a small grid
    const FaMap mp = fa_map<kMaps>(a, s);
    if (!mp.live) return;                                          // (sitting out: k_fa_prepare left n_cand 0 as well)
    const size_t slot = (size_t)s * a.frames_pitch + a.t;
    const double* ctl = a.ctl + (size_t)s * kFaCtl;
    const int n_points = min(a.n_pts ? a.n_pts[slot] : a.n_pts_given, a.pts_pitch);
    for (int b = blockIdx.x * 64; b < n_cand; b += gridDim.x * 64) {     // uniform per workgroup (one wavefront)
        const int cidx = b + threadIdx.x;
        match_candidate(cidx < n_cand, cidx, mp.cache, mp.cols, mp.rows, mp.lines, a.scan_lines + slot * a.line_pitch,
                        a.pts + slot * a.pts_pitch * 3, n_points, ctl[0], ctl[1], ctl[2], ctl[3], a.pairs + (size_t)s * a.pair_cap * 2,
                        1.0 /* z_occ_max_dis, baseFunc.h:60 */, 60.0 /* maxEstiDist, :86 */, a.cand + (size_t)s * a.pair_cap * 16);
    }
}

template <bool kMaps>
__global__ __launch_bounds__(kFaThreads) void k_fa_fuse(FaArgs a) {
    const int s = blockIdx.y, tid = threadIdx.x;
    if (a.n_frames && a.t >= a.n_frames[s]) return;
    if constexpr (kMaps) {                                         // sitting out: the carry, the state and the report keep their bytes
        if ((unsigned)a.map_of[s] >= (unsigned)a.n_maps) return;
    }
    const size_t slot = (size_t)s * a.frames_pitch + a.t;
    const lsd_fa_state* in = fa_prev(a, s);
    if (a.state_in) in = a.state_in + s;
    lsd_fa_state* out = a.states + slot;
    lsd_fa_report* rep = a.reports + slot;
    const double* ctl = a.ctl + (size_t)s * kFaCtl;
    const int n_cand = a.n_cand[s];
    const size_t ccap = (size_t)a.pair_cap * 4;
    const double* cand = a.cand + (size_t)s * ccap * 4;
    int* g_idx = a.scratch + (size_t)s * ccap * 2;                 // the global path: kept indices, then their sorted order
    int* g_sorted = g_idx + ccap;

    __shared__ double s_key[kFaLdsMax];
    __shared__ int s_idx[kFaLdsMax], s_sorted[kFaLdsMax];
    __shared__ int s_w[kFaThreads / 64];
    __shared__ double s_est[4];
    __shared__ int s_branch;

    // 1. keep score < 3 (:261) in single-thread order: count, then place
    int n_kept = 0;
    for (int b = 0; b < n_cand; b += kFaThreads) {
        const int i = b + tid;
        int cnt;
        fa_block_scan(i < n_cand && cand[4 * (size_t)i + 3] < 3, s_w, cnt);
        n_kept += cnt;
    }
    const bool in_lds = n_kept <= a.lds_bound;
    int base = 0;
    for (int b = 0; b < n_cand; b += kFaThreads) {
        const int i = b + tid;
        const double sc = i < n_cand ? cand[4 * (size_t)i + 3] : 3.0;
        const bool take = sc < 3;
        int cnt;
        const int pos = base + fa_block_scan(take, s_w, cnt);
        if (take) {
            if (in_lds) { s_key[pos] = sc; s_idx[pos] = i; }
            else g_idx[pos] = i;
        }
        base += cnt;
    }
    __syncthreads();
    // 2. stable ascending sort by score (qsort with CompScore, :98 -- glibc's merge sort keeps equal scores in input order):
    //    the rank of (score, position) among the kept ones.  O(n^2 / 256) comparisons: 24-87 kept per frame on the reference's log
    //    (LDS); the global path is exact at any count, only slower.
    for (int i = tid; i < n_kept; i += kFaThreads) {
        const int ii = in_lds ? s_idx[i] : g_idx[i];
        const double ki = in_lds ? s_key[i] : cand[4 * (size_t)ii + 3];
        int r = 0;
        for (int j = 0; j < n_kept; j++) {
            const double kj = in_lds ? s_key[j] : cand[4 * (size_t)g_idx[j] + 3];
            r += (kj < ki) || (kj == ki && j < i);
        }
        if (in_lds) s_sorted[r] = ii;
        else g_sorted[r] = ii;
    }
    __syncthreads();
    const int* sorted = in_lds ? s_sorted : g_sorted;

    // 3. the branch, and the fusion on one lane (:140-156)
    if (tid == 0) {
        int br;
        double ex = -1, ey = -1, ea = 0, es = HUGE_VAL;
        if (n_kept == 0) br = LSD_FA_RESET;
        else if (fabs(ctl[2] + 1) < 0.0001) {
            br = LSD_FA_FIRST;
            const double* c0 = cand + 4 * (size_t)sorted[0];
            ex = c0[0]; ey = c0[1]; ea = c0[2]; es = c0[3];
        } else {
            br = LSD_FA_UKF;
            double sumX = 0, sumY = 0, sumAngle = 0, sumScore = 0;
            for (int k = 0; k < n_kept; k++) {
                const double* c = cand + 4 * (size_t)sorted[k];
                const double w = 1 / (c[3] * c[3]);                // 1 / pow(score, 2)
                sumX += c[0] * w;
                sumY += c[1] * w;
                sumAngle += c[2] * w;
                sumScore += w;
            }
            ex = sumX / sumScore; ey = sumY / sumScore; ea = sumAngle / sumScore;
            es = 1 / sqrt(sumScore / (double)n_kept);
        }
        s_branch = br;
        s_est[0] = ex; s_est[1] = ey; s_est[2] = ea; s_est[3] = es;
        rep->estimate.x = ex; rep->estimate.y = ey; rep->estimate.ang = ea; rep->score = es;
        rep->scan_pose.x = ctl[5]; rep->scan_pose.y = ctl[6]; rep->scan_pose.ang = ctl[7];
        rep->n_pairs = a.n_pairs[s]; rep->n_kept = n_kept; rep->branch = br; rep->llt = -2;
    }
    __syncthreads();
    const int branch = s_branch;
    if (branch == LSD_FA_RESET) {                                  // :62-83
        if (tid < 9) out->x[tid] = tid == 0 || tid == 1 ? -1.0 : 0.0;
        if (tid < 81) out->P[tid] = tid % 10 ? 0.0 : (tid < 30 ? 100.0 : tid < 60 ? 1.0 : 0.1);
    } else if (branch == LSD_FA_FIRST) {                           // :86-95
        if (tid < 9) out->x[tid] = tid < 3 ? s_est[tid] : in->x[tid];
        if (tid < 81) out->P[tid] = in->P[tid];
    } else {
        // 4. myfa::ukf (:404-536).  m: the LLT's working copy, row-major m[i * 9 + j]
        __shared__ double x[9], m[81], Xs[9 * 19], Xm[9], Xd[9 * 19], T[9 * 19], G[81], inv[9], K[27], Zd[3];
        __shared__ double s_xk;
        __shared__ int s_fail;
        if (tid < 9) x[tid] = tid < 3 ? in->x[tid] + ctl[5 + tid] : in->x[tid];   // kalman_x(0..2) += ScanPose (:430-432)
        if (tid < 81) m[tid] = in->P[(tid % 9) * 9 + tid / 9];
        if (tid == 0) s_fail = -1;
        __syncthreads();
        // kalman_P.llt() (Eigen's llt_inplace::unblocked): returns at the first column whose pivot is not positive
        for (int k = 0; k < 9; k++) {
            if (tid == 0) {
                double xk = m[k * 9 + k];
                if (k > 0) {
                    double sq = 0;
                    for (int j = 0; j < k; j++) sq += m[k * 9 + j] * m[k * 9 + j];
                    xk -= sq;
                }
                if (xk <= 0) s_fail = k;
                else { xk = sqrt(xk); m[k * 9 + k] = xk; }
                s_xk = xk;
            }
            __syncthreads();
            if (s_fail >= 0) break;
            if (tid > k && tid < 9) {
                double v = m[tid * 9 + k];
                if (k > 0) {
                    double t = 0;
                    for (int j = 0; j < k; j++) t += m[tid * 9 + j] * m[k * 9 + j];
                    v -= t;
                }
                m[tid * 9 + k] = v / s_xk;
            }
            __syncthreads();
        }
        const int L = 9;
        const double alpha = 1e-2, ki = 0, beta = 2;
        const double lambda = alpha * alpha * (L + ki) - L;
        double c = L + lambda;
        const double wm0 = lambda / c, wmi = 0.5 / c;
        const double wc0 = lambda / c + (1 - alpha * alpha + beta);
        c = sqrt(c);
        // sigma points (:446-450): column j + 1 = x + c * L^T[:, j] -- row j of L; prediction with t = 1 (:460-477)
        if (tid < 19) {
            const int col = tid;
            double X[9];
            for (int i = 0; i < 9; i++) {
                if (col == 0) X[i] = x[i];
                else {
                    const int j = (col - 1) % 9;
                    const double lji = j >= i ? m[j * 9 + i] : 0.0;      // matrixL(): the upper triangle reads 0
                    const double A = c * lji;
                    X[i] = col <= 9 ? x[i] + A : x[i] - A;
                }
            }
            const double kt = 1;
            Xs[0 * 19 + col] = X[0] + kt * X[3] + 0.5 * kt * kt * X[6];
            Xs[1 * 19 + col] = X[1] + kt * X[4] + 0.5 * kt * kt * X[7];
            Xs[2 * 19 + col] = X[2] + kt * X[5] + 0.5 * kt * kt * X[8];
            Xs[3 * 19 + col] = X[3] + kt * X[6];
            Xs[4 * 19 + col] = X[4] + kt * X[7];
            Xs[5 * 19 + col] = X[5] + kt * X[8];
            Xs[6 * 19 + col] = X[6];
            Xs[7 * 19 + col] = X[7];
            Xs[8 * 19 + col] = X[8];
        }
        __syncthreads();
        if (tid < 9) {                                             // Xmeans (= Zmeans for rows 0..2)
            double acc = 0;
            for (int col = 0; col < 19; col++) acc += (col == 0 ? wm0 : wmi) * Xs[tid * 19 + col];
            Xm[tid] = acc;
        }
        __syncthreads();
        if (tid < 9 * 19) {                                        // Xdiv (Zdiv = its rows 0..2) and Xdiv * diag(Wc)
            const int col = tid % 19;
            const double d = Xs[tid] - Xm[tid / 19];
            Xd[tid] = d;
            T[tid] = d * (col == 0 ? wc0 : wmi);
        }
        __syncthreads();
        if (tid < 81) {                                            // G = Xdiv diag(Wc) Xdiv^T
            const int i = tid / 9, j = tid % 9;
            double acc = 0;
            for (int col = 0; col < 19; col++) acc += T[i * 19 + col] * Xd[j * 19 + col];
            G[tid] = acc;
        }
        __syncthreads();
        // Pzz = G[0..2][0..2] + R (R = I); Pxz = G[:, 0..2]; Pzz.inverse() (Eigen's compute_inverse_size3)
        if (tid < 9) {
            const int i = tid / 3, j = tid % 3;
            auto pz = [&](int r, int q) { return G[r * 9 + q] + (r == q ? 1.0 : 0.0); };
            auto cof = [&](int r, int q) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, q1 = (q + 1) % 3, q2 = (q + 2) % 3;
                return pz(r1, q1) * pz(r2, q2) - pz(r1, q2) * pz(r2, q1);
            };
            const double det = (cof(0, 0) * pz(0, 0) + cof(1, 0) * pz(1, 0)) + cof(2, 0) * pz(2, 0);
            const double invdet = 1 / det;
            inv[j * 3 + i] = cof(i, j) * invdet;
        }
        __syncthreads();
        if (tid < 27) {                                            // K = Pxz Pzz^-1
            const int i = tid / 3, q = tid % 3;
            double acc = 0;
            for (int r = 0; r < 3; r++) acc += G[i * 9 + r] * inv[r * 3 + q];
            K[tid] = acc;
        }
        if (tid < 3) Zd[tid] = s_est[tid] - Xm[tid];               // Zdiff
        __syncthreads();
        if (tid < 9) {                                             // x = Xmeans + K Zdiff
            double acc = 0;
            for (int q = 0; q < 3; q++) acc += K[tid * 3 + q] * Zd[q];
            out->x[tid] = Xm[tid] + acc;
        }
        if (tid < 81) {                                            // P = P1 - K Pxz^T, P1 = G + Q; stored column-major
            const int i = tid / 9, j = tid % 9;
            const double q = i != j ? 0.0 : i < 3 ? 1.0 : i < 6 ? 0.01 : 0.0001;
            double acc = 0;
            for (int r = 0; r < 3; r++) acc += K[i * 3 + r] * G[j * 9 + r];
            out->P[j * 9 + i] = (G[tid] + q) - acc;
        }
        if (tid == 0) rep->llt = s_fail;
    }
    // 5. the frame loop's angle bookkeeping (main_on_windows.cpp:172-180)
    if (!a.odom) return;
    __syncthreads();                                               // out->x[2] was written by lane 2; every read of `in` is done
    const bool last = a.carry && a.t == a.n_frames[s] - 1;         // the resumable loop: write the loop's variables back to the carry
    lsd_fa_carry* cy = last ? a.carry + s : nullptr;               // (at t = 0, `in` IS the carry's state: written only past the barrier)
    if (tid == 0) {
        double* aux = a.aux + (size_t)s * kFaAux;
        const FaBook bk = fa_book(a, s);
        lsd_position o0, o1;
        fa_odom(a, s, o0, o1);
        bool offset = bk.offset;
        double angDiff = out->x[2] - fa_atand(o1.ang);
        if (fabs(angDiff) > 90 && bk.frame == 0) offset = true;   // cnt_frame == 1
        if (offset && angDiff < 0) angDiff += 360;
        const double sum = bk.sum + angDiff, cnt = bk.cnt + 1;     // angRotate.push_back, summed from 0 in push order by the next frame
        aux[0] = sum;
        aux[1] = cnt;
        aux[2] = offset ? 1.0 : 0.0;
        aux[3] = (double)(bk.frame + 1);
        if (cy) {
            cy->odom = o1;
            cy->ang_sum = sum;
            cy->ang_count = cnt;
            cy->frames = bk.frame + 1;
            cy->is_offset = offset ? 1 : 0;
        }
    }
    if (cy) {
        if (tid < 9) cy->state.x[tid] = out->x[tid];
        if (tid < 81) cy->state.P[tid] = out->P[tid];
    }
}

template <bool kMaps>
static void fa_frame(const FaArgs& a, int n_seq, bool prepare, hipStream_t st) {
    if (prepare) {
        hipLaunchKernelGGL(k_fa_prepare<kMaps>, dim3(1, n_seq), dim3(kFaThreads), 0, st, a);
        // 50-120 pairs (200-480 candidates) per frame on the reference's logs: 8 wavefronts per sequence cover them in one pass; more
        // loop.  (The capacity, n_map x 360 pairs, would be ~900 workgroups per sequence and frame, nearly all of them empty.)
        const long long cap_blocks = ((long long)a.pair_cap * 4 + 63) / 64;
        const int blocks = (int)(cap_blocks < kFaMatchBlocks ? cap_blocks : kFaMatchBlocks);
        hipLaunchKernelGGL(k_fa_match<kMaps>, dim3(blocks > 0 ? blocks : 1, n_seq), dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(k_fa_fuse<kMaps>, dim3(1, n_seq), dim3(kFaThreads), 0, st, a);
}

// the single-map entries launch the kMaps = false instantiation: the same registers and no scratch gained; FaArgs is 24 bytes larger
void launch_fa_frame(const FaArgs& a, int n_seq, bool prepare, hipStream_t st) {
    if (a.maps) fa_frame<true>(a, n_seq, prepare, st);
    else fa_frame<false>(a, n_seq, prepare, st);
}

// Carries from one map frame to another, in place (lsd_enqueue_fa_carry_rebase_device): one lane per (sequence,
// entry), entries 0..8 = state.x, 9..89 = state.P; sc = from.mapResol / to.mapResol, tx / ty = the origin's move in pixels of `to`.
// A sequence moves iff key_of is null or key_of[s] == key, read here, when the kernel runs.  The carry's "no pose" test (x[0] read by
// every lane of the sequence) must see the value from before lane 0's write: the barrier between the read and the writes orders them
// (a workgroup holds kFaRebaseSeqs whole sequences, so every lane that reads a sequence's x[0] shares the barrier with its writer).
constexpr int kFaRebaseEntries = 90, kFaRebaseSeqs = 2;
__global__ __launch_bounds__(kFaRebaseEntries * kFaRebaseSeqs) void k_fa_rebase(lsd_fa_carry* carry, int n_seq, const int32_t* key_of, int32_t key,
                                                                                 double sc, double tx, double ty) {
    const int s = blockIdx.x * kFaRebaseSeqs + (int)threadIdx.x / kFaRebaseEntries, e = (int)threadIdx.x % kFaRebaseEntries;
    bool move = s < n_seq && (!key_of || key_of[s] == key);
    double x0 = 0;
    if (move) x0 = carry[s].state.x[0];
    __syncthreads();
    if (!move || fabs(x0 + 1) < 0.0001) return;                    // no pose yet / just reset (myFA.cpp:99): the sentinel keeps its bytes
    lsd_fa_state* st = &carry[s].state;
    if (e < 9) {
        if (e % 3 == 2) return;                                    // degrees
        const double v = st->x[e] * sc;
        st->x[e] = e == 0 ? v + tx : e == 1 ? v + ty : v;
    } else {
        const int q = e - 9, i = q % 9, j = q / 9;                 // column-major; the scaling is symmetric in (i, j) up to its order
        const double di = i % 3 != 2 ? sc : 1.0, dj = j % 3 != 2 ? sc : 1.0;
        st->P[q] = (st->P[q] * di) * dj;
    }
}

void launch_fa_rebase(lsd_fa_carry* carry, int n_seq, const int32_t* key_of, int32_t key, double sc, double tx, double ty, hipStream_t st) {
    hipLaunchKernelGGL(k_fa_rebase, dim3((n_seq + kFaRebaseSeqs - 1) / kFaRebaseSeqs), dim3(kFaRebaseEntries * kFaRebaseSeqs), 0, st, carry,
                       n_seq, key_of, key, sc, tx, ty);
}

}  // namespace lsdhip
