// k_facorrect.hip -- the grid match response fused into the localiser's carry (lsd_enqueue_fa_carry_correct_device; include/lsd_hip.h;
// DESIGN.md 8.1.10; restated in tests/fa_correct_cases.py): a measurement update of the carry's 9-state filter with the response record
// as the measurement, H = [I3 0] -- the closing lines of k_fa_fuse (K = Pxz Pzz^-1, x += K Zdiff, P = P1 - K Pxz^T) with the filter's own
// P in the place of the sigma points' G.  fp64 without FMA, every sum ascending from 0.0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lsd_internal.h"

namespace lsdhip {

// One lane per (sequence, entry of the state), entries 0..8 = state.x, 9..89 = state.P, as k_fa_rebase; a workgroup holds kFaCorrectSeqs
// whole sequences.  In front of the first barrier a lane reads its entry of the carry (to LDS), the carry's pose bytes and the original
// poses of the slots t = e, e + 90, ..; behind the second barrier every lane of a sequence holds the slot (a max-reduction in two levels:
// 90 -> 10 -> 1) and decides the outcome for itself, from LDS and from the one response record -- the same arithmetic in every lane,
// so no lane waits for another again, and the carry, read only in front of the first barrier, is written only past the second.
constexpr int kFaCorrectEntries = 90, kFaCorrectSeqs = 2, kFaCorrectFold = 10;      // 90 = 10 x 9: the first level folds nine lanes each
constexpr int kFaCorrectNotFinite = 1 << 30;                                       // above every slot + 1 (frames_pitch <= 4096)
static_assert(sizeof(lsd_fa_state) == kFaCorrectEntries * sizeof(double) && offsetof(lsd_fa_carry, state) == 0, "the state is the carry's first 90 doubles");
static_assert(sizeof(lsd_fa_correct_rep) == 48 && sizeof(lsd_fa_correct_par) == 32, "the records the Python mirror assumes");

__global__ __launch_bounds__(kFaCorrectEntries * kFaCorrectSeqs) void k_fa_correct(lsd_fa_carry* carry, int n_seq, int frames_pitch,
                                                                                   const unsigned char* poses, size_t pose_pitch,
                                                                                   const lsd_grid_response_rec* resp, const int32_t* key_of,
                                                                                   int32_t key, lsd_fa_correct_par par, lsd_fa_correct_rep* rep) {
    __shared__ double s_st[kFaCorrectSeqs][kFaCorrectEntries];
    __shared__ int s_red[kFaCorrectSeqs][kFaCorrectEntries];
    __shared__ int s_fold[kFaCorrectSeqs][kFaCorrectFold];
    const int sl = (int)threadIdx.x / kFaCorrectEntries, e = (int)threadIdx.x % kFaCorrectEntries;
    const int s = blockIdx.x * kFaCorrectSeqs + sl;
    const bool active = s < n_seq && (!key_of || key_of[s] == key);
    double v = 0;
    int mine = 0;                                                  // slot + 1 of the last matching slot this lane saw; 0: none
    if (active) {
        const double* st = reinterpret_cast<const double*>(&carry[s].state);
        v = st[e];
        const long long k0 = __double_as_longlong(st[0]), k1 = __double_as_longlong(st[1]), k2 = __double_as_longlong(st[2]);
        const unsigned char* base = poses + (size_t)s * (size_t)frames_pitch * pose_pitch;
        for (int t = e; t < frames_pitch; t += kFaCorrectEntries) {          // bytes, not values: -0.0 is not +0.0, a NaN equals itself
            const long long* p = reinterpret_cast<const long long*>(base + (size_t)t * pose_pitch);
            if (p[0] == k0 && p[1] == k1 && p[2] == k2) mine = t + 1;
        }
        if (!isfinite(v)) mine |= kFaCorrectNotFinite;                       // (step 2 comes before the slot: its bit outbids every slot)
    }
    s_st[sl][e] = v;
    s_red[sl][e] = mine;
    __syncthreads();
    if (e < kFaCorrectFold) {
        int m = 0;
        for (int i = 0; i < kFaCorrectEntries / kFaCorrectFold; i++) m = max(m, s_red[sl][e * (kFaCorrectEntries / kFaCorrectFold) + i]);
        s_fold[sl][e] = m;
    }
    __syncthreads();
    if (!active) return;                                           // step 0: nothing of s is written
    int found = 0;
    for (int i = 0; i < kFaCorrectFold; i++) found = max(found, s_fold[sl][i]);

    const double* x = s_st[sl];
    const double* P = s_st[sl] + 9;                                // P(i, j) = P[j * 9 + i]
    double innov[3] = {0.0, 0.0, 0.0}, Sinv[9], d2 = 0.0, det = 0.0;
    int slot = -1;
    uint32_t flags;
    if (fabs(x[0] + 1) < 0.0001) flags = LSD_FA_CORRECT_NO_POSE;   // the reference's "no pose yet" test (myFA.cpp:99), as k_fa_rebase
    else if (found & kFaCorrectNotFinite) flags = LSD_FA_CORRECT_NOT_FINITE;
    else if (found == 0) flags = LSD_FA_CORRECT_STALE;
    else {
        slot = found - 1;
        const lsd_grid_response_rec* r = resp + ((size_t)s * (size_t)frames_pitch + (size_t)slot);
        const uint32_t rf = r->flags;
        const double z[3] = {r->x, r->y, r->ang};
        const double c[6] = {r->cov[0], r->cov[1], r->cov[2], r->cov[3], r->cov[4], r->cov[5]};
        bool fin = isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]);
#pragma unroll
        for (int i = 0; i < 6; i++) fin = fin && isfinite(c[i]);
        if (!(rf & LSD_GRID_RESPONSE_VALID) || (rf & (LSD_GRID_RESPONSE_NONE | LSD_GRID_RESPONSE_EMPTY | LSD_GRID_RESPONSE_MISMATCH)))
            flags = LSD_FA_CORRECT_NO_RESPONSE;
        else if (!fin) flags = LSD_FA_CORRECT_NOT_FINITE;
        else {
            // S = P[0..2][0..2] + R, R = cov * cov_scale + the floors on the diagonal; S.inverse() as k_fa_fuse takes Pzz's
            const double R[9] = {c[0] * par.cov_scale + par.floor_xy, c[1] * par.cov_scale, c[3] * par.cov_scale,
                                 c[1] * par.cov_scale, c[2] * par.cov_scale + par.floor_xy, c[4] * par.cov_scale,
                                 c[3] * par.cov_scale, c[4] * par.cov_scale, c[5] * par.cov_scale + par.floor_ang};
            double S[9];
#pragma unroll
            for (int q = 0; q < 9; q++) S[q] = P[(q % 3) * 9 + q / 3] + R[q];          // S[r * 3 + q] = P(r, q) + R(r, q)
            auto cof = [&](int a, int b) {
                const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
                return S[a1 * 3 + b1] * S[a2 * 3 + b2] - S[a1 * 3 + b2] * S[a2 * 3 + b1];
            };
            det = (cof(0, 0) * S[0] + cof(1, 0) * S[3]) + cof(2, 0) * S[6];
            const double invdet = 1 / det;
            if (!(det > 0) || !isfinite(invdet)) flags = LSD_FA_CORRECT_SINGULAR;
            else {
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) Sinv[j * 3 + i] = cof(i, j) * invdet;
#pragma unroll
                for (int q = 0; q < 3; q++) innov[q] = z[q] - x[q];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    double t = 0;
#pragma unroll
                    for (int j = 0; j < 3; j++) t += Sinv[i * 3 + j] * innov[j];
                    d2 += innov[i] * t;
                }
                flags = par.gate > 0 && !(d2 <= par.gate) ? LSD_FA_CORRECT_GATED : LSD_FA_CORRECT_APPLIED;
            }
        }
    }
    if (e == 0 && rep) {
        lsd_fa_correct_rep* o = rep + s;
        o->innov[0] = innov[0]; o->innov[1] = innov[1]; o->innov[2] = innov[2];
        o->d2 = d2; o->det = det; o->slot = slot; o->flags = flags;
    }
    if (flags != LSD_FA_CORRECT_APPLIED) return;                   // the carry keeps every byte
    // K = Pxz S^-1 with Pxz = P[:, 0..2]; x += K innov; P = P - K Pxz^T: row i of K, recomputed by every lane that needs it
    const int q = e < 9 ? 0 : e - 9, i = e < 9 ? e : q % 9, j = q / 9;
    double K[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) acc += P[r * 9 + i] * Sinv[r * 3 + b];
        K[b] = acc;
    }
    lsd_fa_state* out = &carry[s].state;
    if (e < 9) {
        double acc = 0;
#pragma unroll
        for (int b = 0; b < 3; b++) acc += K[b] * innov[b];
        out->x[i] = x[i] + acc;
    } else {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) acc += K[r] * P[r * 9 + j];
        out->P[q] = P[q] - acc;
    }
}

void launch_fa_correct(lsd_fa_carry* carry, int n_seq, int frames_pitch, const void* poses, size_t pose_pitch, const lsd_grid_response_rec* resp,
                       const int32_t* key_of, int32_t key, lsd_fa_correct_par par, lsd_fa_correct_rep* rep, hipStream_t st) {
    hipLaunchKernelGGL(k_fa_correct, dim3((n_seq + kFaCorrectSeqs - 1) / kFaCorrectSeqs), dim3(kFaCorrectEntries * kFaCorrectSeqs), 0, st, carry,
                       n_seq, frames_pitch, static_cast<const unsigned char*>(poses), pose_pitch, resp, key_of, key, par, rep);
}

}  // namespace lsdhip
