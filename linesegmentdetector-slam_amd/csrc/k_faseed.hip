// k_faseed.hip -- a located pose written into a carry that has none (lsd_enqueue_fa_carry_seed_device; include/lsd_hip.h; DESIGN.md
// 8.1.13; restated in tests/fa_relocate_cases.py): the neighbour of k_facorrect.hip for the robots the loop itself cannot find.  The state
// becomes the located pose at rest with a stated covariance, and the loop's angle bookkeeping is REPLACED by the one offset a first frame
// at that pose would have pushed, so the next frame's theta is that offset and not 0 / 0.  fp64 without FMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "devmath.h"
#include "lsd_internal.h"

namespace lsdhip {

// One lane per (pick, entry of the state), entries 0..8 = state.x, 9..89 = state.P, as k_fa_correct; a workgroup holds kFaSeedPicks whole
// picks.  Every lane of a pick decides the outcome for itself from the same few loads -- the same arithmetic in every lane, so none waits
// for another --; the one barrier stands between the read of the carry's x[0] (the "no pose" test) and lane 0's write of it.
constexpr int kFaSeedEntries = 90, kFaSeedPicks = 2;
static_assert(sizeof(lsd_fa_seed_rep) == 48 && sizeof(lsd_fa_seed_par) == 48, "the records the Python mirror assumes");
static_assert(sizeof(lsd_grid_locate_rec) == 64 && sizeof(lsd_grid_response_rec) == 192, "the records the seed reads");

__device__ __forceinline__ double seed_atand(double v) { return atan_g(v) * 180.0 / kPi; }   // the loop's atand (k_fa.hip: fa_atand; baseFunc.cpp:14-16)

__global__ __launch_bounds__(kFaSeedEntries * kFaSeedPicks) void k_fa_seed(lsd_fa_carry* carry, int n_seq, int frames_pitch, const int32_t* pick,
                                                                            int n_pick, const lsd_grid_locate_rec* loc,
                                                                            const lsd_grid_response_rec* resp, lsd_fa_seed_par par,
                                                                            lsd_fa_seed_rep* rep) {
    const int j = blockIdx.x * kFaSeedPicks + (int)threadIdx.x / kFaSeedEntries, e = (int)threadIdx.x % kFaSeedEntries;
    const int pk = j < n_pick ? pick[j] : -1;
    const int s = pk >= 0 ? pk / frames_pitch : -1, slot = pk >= 0 ? pk % frames_pitch : -1;
    const bool in_range = pk >= 0 && s < n_seq;
    double x0 = 0;
    if (in_range) x0 = carry[s].state.x[0];
    __syncthreads();
    if (j >= n_pick) return;

    double z[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, d = 0.0;
    uint32_t flags, loc_flags = 0;
    bool off = false;
    if (pk < 0) flags = LSD_FA_SEED_UNUSED;
    else if (!in_range) flags = LSD_FA_SEED_BAD_PICK;
    else if (!(fabs(x0 + 1) < 0.0001)) flags = LSD_FA_SEED_HAS_POSE;
    else {
        const lsd_grid_locate_rec* l = loc + j;
        loc_flags = l->flags;
        if (loc_flags != LSD_GRID_LOCATE_ACCEPTED) flags = LSD_FA_SEED_NOT_LOCATED;
        else if (l->n_best > par.max_best) flags = LSD_FA_SEED_AMBIGUOUS;
        else {
            bool fin;
            flags = LSD_FA_SEED_SEEDED;
            if (resp) {
                const lsd_grid_response_rec* r = resp + j;
                const uint32_t rf = r->flags;
                const double c[6] = {r->cov[0], r->cov[1], r->cov[2], r->cov[3], r->cov[4], r->cov[5]};
                z[0] = r->x; z[1] = r->y; z[2] = r->ang;
                fin = isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]);
#pragma unroll
                for (int i = 0; i < 6; i++) fin = fin && isfinite(c[i]);
                if (!(rf & LSD_GRID_RESPONSE_VALID) || (rf & (LSD_GRID_RESPONSE_NONE | LSD_GRID_RESPONSE_EMPTY | LSD_GRID_RESPONSE_MISMATCH)))
                    flags = LSD_FA_SEED_NO_RESPONSE;
                // R of the correction's step 5, row-major and symmetric
                R[0] = c[0] * par.cov_scale + par.floor_xy; R[1] = c[1] * par.cov_scale; R[2] = c[3] * par.cov_scale;
                R[3] = R[1]; R[4] = c[2] * par.cov_scale + par.floor_xy; R[5] = c[4] * par.cov_scale;
                R[6] = R[2]; R[7] = R[5]; R[8] = c[5] * par.cov_scale + par.floor_ang;
            } else {
                z[0] = l->x; z[1] = l->y; z[2] = l->ang;
                fin = isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]);
                R[0] = par.var_xy; R[4] = par.var_xy; R[8] = par.var_ang;
            }
            if (flags == LSD_FA_SEED_SEEDED && !fin) flags = LSD_FA_SEED_NOT_FINITE;
        }
    }
    const bool seeded = flags == LSD_FA_SEED_SEEDED;
    if (seeded && e == 0) {                                        // the loop's own lines (k_fa_fuse, 5.), as of a first frame
        d = z[2] - seed_atand(carry[s].odom.ang);
        off = fabs(d) > 90;
        if (off && d < 0) d += 360;
    }
    if (e == 0 && rep) {
        lsd_fa_seed_rep* o = rep + j;
        o->pose[0] = seeded ? z[0] : 0.0; o->pose[1] = seeded ? z[1] : 0.0; o->pose[2] = seeded ? z[2] : 0.0;
        o->ang_diff = d; o->seq = s; o->slot = slot; o->flags = flags; o->loc_flags = loc_flags;
    }
    if (!seeded) return;                                           // the carry keeps every byte
    lsd_fa_carry* cy = carry + s;
    if (e < 9) cy->state.x[e] = e < 3 ? z[e] : 0.0;
    else {
        const int q = e - 9, i = q % 9, jj = q / 9;                // column-major; the block is symmetric
        cy->state.P[q] = i < 3 && jj < 3 ? R[i * 3 + jj] : i != jj ? 0.0 : i < 6 ? 1.0 : 0.1;
    }
    if (e == 0) {
        cy->ang_sum = 0.0 + d;
        cy->ang_count = 1.0;
        cy->is_offset = off ? 1 : 0;                               // odom and frames keep their bytes
    }
}

void launch_fa_seed(lsd_fa_carry* carry, int n_seq, int frames_pitch, const int32_t* pick, int n_pick, const lsd_grid_locate_rec* loc,
                    const lsd_grid_response_rec* resp, lsd_fa_seed_par par, lsd_fa_seed_rep* rep, hipStream_t st) {
    hipLaunchKernelGGL(k_fa_seed, dim3((n_pick + kFaSeedPicks - 1) / kFaSeedPicks), dim3(kFaSeedEntries * kFaSeedPicks), 0, st, carry, n_seq,
                       frames_pitch, pick, n_pick, loc, resp, par, rep);
}

}  // namespace lsdhip
