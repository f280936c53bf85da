// k_gridlocate_tight.hip -- the global localisation of k_gridlocate.hip with the other half of branch and bound (gfx950): the lower bound
// is raised after every level from one probe per heading, and a level whose frontier does not fit max_nodes is rebuilt once under the
// raised bound before the search gives up.  The rule (include/lsd_hip.h) keeps every bound the score of a real candidate,
// so the records are the exhaustive search's; tests/grid_locate_tight_cases.py restates it.  The offsets, the top level, the first bound
// and the seed are k_gridlocate.hip's kernels as they are; the expansion, the descent and the pick are loc_expand, loc_descend and loc_pick
// of gridlocate_dev.h.
//
// k_grid_locate_tight_level: one workgroup per scan, between the levels.  At first (level = H) it clears the scan's kLocTight words and the
//   heading keys and states L_H.  For a level l = h - 1 >= 1 it folds the probes' maximum into L, states L_l, and where |G_l| > max_nodes
//   and the retry is on it keeps the first count, sets the level's bit, zeroes the level's counter and arms the retry.  A level below an
//   overflow is dead: its words stay 0 and nothing is armed.  It clears the heading keys and the probes' word for the next level.
// k_grid_locate_tight_expand: k_grid_locate_expand's text, and every surviving child enters its heading's key (U << 32 | 0xFFFFFFFF -
//   (Q nbx + P)) with atomicMax: reduced inside the wavefront over the children of consecutive parents of one heading, and the atomic
//   skipped when a plain load already shows a key as large (the keys only grow).  As the retry (retry = 1) it returns at once unless the
//   scan's level is armed, and it leaves the keys alone.
// k_grid_locate_tight_probe: n_scans x n_ang workgroups; a heading without a key returns.  The heading's offsets are staged in LDS and
//   the descent of k_grid_locate_top runs from the key's node of level l down to a candidate; its S enters the scan's word by atomicMax.
// k_grid_locate_tight_pick: the pick with the 128-byte statistics.
// No spin-waits, no hand-shakes between workgroups: all ordering comes from launch boundaries.  Every loop bound read from device memory is
// clamped (a count above max_nodes runs nothing, a heading index is at most n_ang - 1, a key's node is taken inside its level).
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950, -O3): DESIGN.md 8.1.14.
#include <algorithm>

#include "lsd_internal.h"
#include "gridmatch_dev.h"
#include "gridlocate_dev.h"

namespace lsdhip {

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_tight_level(LocBox g, int level, int first, uint32_t retry, uint32_t* __restrict__ ctl,
                                                                      uint32_t* __restrict__ tight, unsigned long long* __restrict__ heads) {
    const int scan = blockIdx.x, tid = threadIdx.x;
    uint32_t* myctl = ctl + (size_t)scan * kLocCtl;
    uint32_t* mine = tight + (size_t)scan * kLocTight;
    unsigned long long* myheads = heads + (size_t)scan * g.n_ang;
    for (int a = tid; a < g.n_ang; a += kGmLanes) myheads[a] = 0;
    if (first) {
        // (an empty scan's L is 0xFFFFFFFF: no U reaches it, and the pick reports zeros)
        if (tid < kLocTight) mine[tid] = tid == kLtBound + level ? myctl[kLcBound] : 0u;
        return;
    }
    if (tid != 0) return;
    const uint32_t probe = mine[kLtProbe];
    mine[kLtProbe] = 0;
    mine[kLtArmed] = 0;
    bool dead = false;                                               // an overflow above: this level was not run
    for (int j = level + 1; j <= g.H; j++) dead |= myctl[j] > g.max_nodes;
    if (dead) return;
    const uint32_t L = max(myctl[kLcBound], probe);
    myctl[kLcBound] = L;
    mine[kLtBound + level] = L;
    const uint32_t count = myctl[level];
    if (retry && count > g.max_nodes) {
        mine[kLtFirst + level] = count;
        mine[kLtRetried] |= 1u << level;
        myctl[level] = 0;
        mine[kLtArmed] = 1;
    }
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_tight_expand(LocBox g, int h, int retry, const uint8_t* __restrict__ plane,
                                                                       const short2* __restrict__ offs, const uint32_t* __restrict__ nbs,
                                                                       uint32_t* __restrict__ ctl, const uint32_t* __restrict__ tight,
                                                                       const uint2* __restrict__ in, uint2* __restrict__ out,
                                                                       LocSlot* __restrict__ slots, unsigned long long* __restrict__ heads) {
    __shared__ unsigned long long s_key[kLocWaves];
    __shared__ uint32_t s_c[kLocWaves];
    if (retry && tight[(size_t)blockIdx.x * kLocTight + kLtArmed] == 0) return;     // (uniform in the workgroup)
    // the keys serve the probe of level h - 1 >= 1; the retry appends nothing to them
    unsigned long long* myheads = (retry || h == 1 || !heads) ? nullptr : heads + (size_t)blockIdx.x * g.n_ang;
    loc_expand(g, h, plane, offs, nbs, ctl, in, out, slots, myheads, s_key, s_c);
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_tight_probe(LocBox g, LocPlanes pl, int level, const uint8_t* __restrict__ pyr,
                                                                      const short2* __restrict__ offs, const uint32_t* __restrict__ nbs,
                                                                      const unsigned long long* __restrict__ heads, uint32_t* __restrict__ tight) {
    __shared__ short2 s_off[kGmMaxBeams];
    __shared__ uint32_t s_u[kLocWaves];
    const int scan = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    const size_t sa = (size_t)scan * g.n_ang + a;
    const unsigned long long key = heads[sa];
    if (key == 0) return;                                            // no node of this heading survived: no probe (uniform in the workgroup)
    const int n = (int)min(nbs[sa], (uint32_t)g.stride);
    const short2* mine = offs + sa * g.stride;
    for (int k = tid; k < n; k += kGmLanes) s_off[k] = mine[k];
    __syncthreads();
    const uint32_t nbx = (uint32_t)((g.nx + (1 << level) - 1) >> level), nby = (uint32_t)((g.ny + (1 << level) - 1) >> level);
    const uint32_t idx = 0xFFFFFFFFu - (uint32_t)key;
    const int Q = (int)min(idx / nbx, nby - 1), P = (int)(idx % nbx);
    const uint32_t S = loc_descend(g, pl, pyr, s_off, n, level, Q, P, (uint32_t)(key >> 32), s_u);
    if (tid == 0) atomicMax(&tight[(size_t)scan * kLocTight + kLtProbe], S);
}

__global__ __launch_bounds__(64) void k_grid_locate_tight_pick(LocBox g, int n_slots, double ang0, double ang_step, uint32_t min_beams, uint32_t min_num,
                                                               uint32_t min_den, const uint32_t* __restrict__ nbs, const uint32_t* __restrict__ ctl,
                                                               const uint32_t* __restrict__ tight, const LocSlot* __restrict__ slots,
                                                               unsigned long long* __restrict__ out, uint32_t* __restrict__ stats) {
    loc_pick(g, n_slots, ang0, ang_step, min_beams, min_num, min_den, nbs, ctl, tight, slots, out, stats);
}

void grid_locate_tight_ws(int n_scans, int stride, const lsd_grid_locate_par& par, size_t bytes[kGridLocateTightRegions]) {
    grid_locate_ws(n_scans, stride, par, bytes);
    bytes[kGridLocateRegions] = (size_t)n_scans * kLocTight * sizeof(uint32_t);
    bytes[kGridLocateRegions + 1] = (size_t)n_scans * par.n_ang * sizeof(unsigned long long);
}

// levels + 6 + max(levels - 1, 0) * (1 + probe + retry) launches: a number fixed by par and tight, never by the data
void launch_grid_locate_tight(const lsd_polar* scans, const int* lens, int n_scans, int stride, int cols, int rows, double resol, double range_max,
                              const uint8_t* pyramid, const lsd_grid_locate_par& par, uint32_t tight, void* const ws[kGridLocateTightRegions],
                              lsd_grid_locate_rec* out, lsd_grid_locate_tight_stats* stats, hipStream_t s) {
    const LocGeom q = launch_grid_locate_head(scans, lens, n_scans, stride, cols, rows, resol, range_max, pyramid, par, ws, s);
    const short2* offs = static_cast<const short2*>(ws[0]);
    const uint32_t* nbs = static_cast<const uint32_t*>(ws[1]);
    uint2* lists[2] = {static_cast<uint2*>(ws[4]), static_cast<uint2*>(ws[5])};
    uint32_t* ctl = static_cast<uint32_t*>(ws[6]);
    LocSlot* slots = static_cast<LocSlot*>(ws[7]);
    uint32_t* tw = static_cast<uint32_t*>(ws[kGridLocateRegions]);
    unsigned long long* heads = static_cast<unsigned long long*>(ws[kGridLocateRegions + 1]);
    const int H = par.levels;
    const bool probe = tight & LSD_GRID_LOCATE_TIGHT_PROBE, retry = tight & LSD_GRID_LOCATE_TIGHT_RETRY;
    const dim3 per_scan(n_scans), per_heading(n_scans, par.n_ang), wide(n_scans, q.g_exp), lanes(kGmLanes);
    hipLaunchKernelGGL(k_grid_locate_tight_level, per_scan, lanes, 0, s, q.g, H, 1, 0u, ctl, tw, heads);
    int cur = 0;
    for (int h = H; h >= 1; h--, cur ^= 1) {
        const uint8_t* plane = pyramid + q.pl.off[h - 1];
        hipLaunchKernelGGL(k_grid_locate_tight_expand, wide, lanes, 0, s, q.g, h, 0, plane, offs, nbs, ctl, tw, lists[cur], lists[cur ^ 1], slots,
                           probe ? heads : nullptr);
        if (h == 1) break;
        if (probe) hipLaunchKernelGGL(k_grid_locate_tight_probe, per_heading, lanes, 0, s, q.g, q.pl, h - 1, pyramid, offs, nbs, heads, tw);
        hipLaunchKernelGGL(k_grid_locate_tight_level, per_scan, lanes, 0, s, q.g, h - 1, 0, retry ? 1u : 0u, ctl, tw, heads);
        if (retry)
            hipLaunchKernelGGL(k_grid_locate_tight_expand, wide, lanes, 0, s, q.g, h, 1, plane, offs, nbs, ctl, tw, lists[cur], lists[cur ^ 1], slots,
                               nullptr);
    }
    hipLaunchKernelGGL(k_grid_locate_tight_pick, per_scan, dim3(64), 0, s, q.g, H ? q.g_exp : q.g_seed, par.ang0, par.ang_step, par.min_beams,
                       par.min_num, par.min_den, nbs, ctl, tw, slots, reinterpret_cast<unsigned long long*>(out), reinterpret_cast<uint32_t*>(stats));
}

}  // namespace lsdhip
