// k_gridlocate.hip -- global scan-to-grid localisation (gfx950): the correlative score of k_gridmatch.hip searched over a whole box of
// lidar cells and a whole fan of headings, without a prior, by branch and bound over a pyramid of block maxima (Olson; Cartographer's
// fast correlative matcher), held to the exhaustive search byte for byte.  The rule (include/lsd_hip.h) is made of
// integers behind the beam offsets and tests/grid_locate_cases.py restates it.
//
// k_grid_pyramid_level: one launch per level.  Level 0 copies the lookup plane; level h takes, per output cell, the maximum of four cells
//   of level h - 1 at stride 2^(h-1) (cells outside that plane as 0).  One byte per cell out, four in: a bandwidth kernel.
// k_grid_locate_offsets: n_scans x n_ang workgroups of 256 lanes.  Phase A of k_grid_match (gridmatch_dev.h: the same text) at the pose
//   (0, 0, theta_a), every scored beam kept; the offsets go to workspace as an int16 pair per scored beam, with nb(a).
// k_grid_locate_top: n_scans x n_ang workgroups.  The heading's offsets are staged in LDS; one lane per top node sums U_H into the dense
//   array (neighbouring lanes read neighbouring plane cells, the list entry is a broadcast); a key maximum finds the node the greedy descent
//   starts from; the descent scores the four children of a node one per wavefront, the beams dealt over its lanes, down to L_a.
// k_grid_locate_bound: one workgroup per scan: L = max(max_a L_a, score_floor), the sum of nb(a), and the scan's counters cleared.
// k_grid_locate_seed: the dense U_H compacted into F_H (ballot / mbcnt, one atomic per wavefront); with levels = 0 the top nodes ARE the
//   candidates and the kernel takes their key maximum instead.
// k_grid_locate_expand: one launch per level h = H .. 1, a fixed geometry.  The parent count is read on the device and clamped to
//   max_nodes (a count above it is the overflow: the level is not run).  A wavefront takes a parent: its lanes split the heading's beams,
//   read the four children's cells of plane h - 1 and reduce four sums; lane 0 appends the survivors with one atomic for the wavefront.
//   List order is free.  At h = 1 the children are candidates: they enter the key maximum and the count of equals instead of a list.
// k_grid_locate_pick: one wavefront per scan: the key maximum over the workgroups' slots (S, then 2^44 - 1 - lin), n_best, the outcome,
//   the record and the statistics.
//
// gridlocate_dev.h holds what k_gridlocate_tight.hip shares with this file: the workspace's records, loc_cell, the wave reductions, the slot
// merge; launch_grid_locate_head is the four launches both searches begin with.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950, -O3): DESIGN.md 8.1.12.
#include <algorithm>

#include "lsd_internal.h"
#include "gridmatch_dev.h"
#include "gridlocate_dev.h"

namespace lsdhip {

__global__ __launch_bounds__(256) void k_grid_pyramid_level(const uint8_t* __restrict__ prev, int cols, int rows, int h, uint8_t* __restrict__ out) {
    const int m = (1 << h) - 1, pc = cols + m, pr = rows + m;
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= pc || oy >= pr) return;
    uint32_t v;
    if (h == 0) {
        v = prev[(size_t)oy * cols + ox];
    } else {
        const int x = ox - m, y = oy - m, half = 1 << (h - 1);
        v = max(max(loc_cell(prev, cols, rows, h - 1, x, y), loc_cell(prev, cols, rows, h - 1, x + half, y)),
                max(loc_cell(prev, cols, rows, h - 1, x, y + half), loc_cell(prev, cols, rows, h - 1, x + half, y + half)));
    }
    out[(size_t)oy * pc + ox] = (uint8_t)v;
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_offsets(const double2* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                                  double resol, double range_max, double ang0, double ang_step, int n_ang,
                                                                  short2* __restrict__ offs, uint32_t* __restrict__ nbs) {
    __shared__ int2 s_end[kGmMaxBeams];
    __shared__ int s_cnt[kLocWaves];
    const int scan = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    const int len = min(max(lens[scan], 0), stride);
    const double rot = deg2rad_ref(ang0 + (double)a * ang_step);
    // the end cell at the pose (0, 0, theta_a) IS the offset (0.0 + d is d); a window this wide keeps every scored beam in the list
    uint32_t nb_unused = 0;
    const int n = gm_end_cells(scans + (size_t)scan * stride, len, 0.0, 0.0, rot, rot, resol, range_max, 1, 1, 1 << 22, 1 << 22, 0, 0, s_end, s_cnt,
                               nb_unused);
    __syncthreads();                                                 // (a scan of no readings runs no barrier in phase A)
    short2* mine = offs + ((size_t)scan * n_ang + a) * stride;
    for (int k = tid; k < n; k += kGmLanes) mine[k] = make_short2((short)s_end[k].x, (short)s_end[k].y);      // n <= len <= stride; |offset| < 32767
    if (tid == 0) nbs[(size_t)scan * n_ang + a] = (uint32_t)n;
}

// U of the node whose low corner is the lidar cell (X, Y), by one lane: the list is a broadcast, kBeamBatch loads in flight
__device__ __forceinline__ uint32_t loc_score_lane(const short2* s_off, int n, const uint8_t* __restrict__ plane, int cols, int rows, int h, int X, int Y) {
    uint32_t S = 0;
    for (int k0 = 0; k0 < n; k0 += kBeamBatch) {
        uint32_t v[kBeamBatch];
#pragma unroll
        for (int u = 0; u < kBeamBatch; u++) {
            v[u] = 0;
            if (k0 + u < n) {
                const short2 o = s_off[k0 + u];
                v[u] = loc_cell(plane, cols, rows, h, X + o.x, Y + o.y);
            }
        }
#pragma unroll
        for (int u = 0; u < kBeamBatch; u++) S += v[u];
    }
    return S;
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_top(LocBox g, LocPlanes pl, const uint8_t* __restrict__ pyr, const short2* __restrict__ offs,
                                                              const uint32_t* __restrict__ nbs, uint32_t* __restrict__ U, uint32_t* __restrict__ la) {
    __shared__ short2 s_off[kGmMaxBeams];
    __shared__ unsigned long long s_key[kLocWaves];
    __shared__ uint32_t s_u[kLocWaves];
    const int scan = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t sa = (size_t)scan * g.n_ang + a;
    const int n = (int)min(nbs[sa], (uint32_t)g.stride);
    const short2* mine = offs + sa * g.stride;
    for (int k = tid; k < n; k += kGmLanes) s_off[k] = mine[k];
    __syncthreads();
    const int H = g.H, nbx = (g.nx + (1 << H) - 1) >> H, nby = (g.ny + (1 << H) - 1) >> H, nblk = nbx * nby;
    uint32_t* myU = U + sa * nblk;
    const uint8_t* top = pyr + pl.off[H];
    unsigned long long best = 0;
    for (int base = 0; base < nblk; base += kGmLanes) {
        const int t = base + tid;
        if (t < nblk) {
            const int Q = t / nbx, P = t - Q * nbx;
            const uint32_t u = loc_score_lane(s_off, n, top, g.cols, g.rows, H, g.x0 + (P << H), g.y0 + (Q << H));
            myU[t] = u;
            const unsigned long long key = ((unsigned long long)u << 32) | (0xFFFFFFFFu - (uint32_t)t);
            best = key > best ? key : best;
        }
    }
    best = wave_max_u64(best);
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    for (int w = 0; w < kLocWaves; w++) best = s_key[w] > best ? s_key[w] : best;
    const int seed = (int)(0xFFFFFFFFu - (uint32_t)best);            // (nblk >= 1: some lane made a key)
    int Q = seed / nbx, P = seed - Q * nbx;
    uint32_t val = (uint32_t)(best >> 32);
    // the greedy descent: child `wave` of the node, the beams dealt over the wavefront's lanes
    for (int h = H; h >= 1; h--) {
        const int side = 1 << (h - 1), cq = 2 * Q + (wave >> 1), cp = 2 * P + (wave & 1);
        const bool exists = cp * side < g.nx && cq * side < g.ny;
        uint32_t u = 0;
        if (exists) {
            const uint8_t* plane = pyr + pl.off[h - 1];
            for (int k = lane; k < n; k += 64) {
                const short2 o = s_off[k];
                u += loc_cell(plane, g.cols, g.rows, h - 1, g.x0 + cp * side + o.x, g.y0 + cq * side + o.y);
            }
        }
        u = loc_wave_sum(u);
        __syncthreads();                                             // (s_u: the reads of the level before)
        if (lane == 0) s_u[wave] = u;
        __syncthreads();
        int c = 0;
        val = s_u[0];                                                // (child 0 always exists)
        for (int w = 1; w < kLocWaves; w++) {
            const bool ex = (2 * P + (w & 1)) * side < g.nx && (2 * Q + (w >> 1)) * side < g.ny;
            if (ex && s_u[w] > val) { val = s_u[w]; c = w; }
        }
        Q = 2 * Q + (c >> 1);
        P = 2 * P + (c & 1);
    }
    if (tid == 0) la[sa] = val;
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_bound(int n_ang, uint32_t score_floor, const uint32_t* __restrict__ nbs,
                                                                const uint32_t* __restrict__ la, uint32_t* __restrict__ ctl) {
    __shared__ uint32_t s_l[kLocWaves], s_n[kLocWaves];
    const int scan = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t L = 0, beams = 0;
    for (int a = tid; a < n_ang; a += kGmLanes) {
        L = max(L, la[(size_t)scan * n_ang + a]);
        beams += nbs[(size_t)scan * n_ang + a];                      // (at most 4096 * 4096: no wrap)
    }
    for (int d = 32; d >= 1; d >>= 1) L = max(L, (uint32_t)__shfl_xor((int)L, d, 64));
    beams = loc_wave_sum(beams);
    if (lane == 0) { s_l[wave] = L; s_n[wave] = beams; }
    __syncthreads();
    if (tid < kLocCtl) {
        L = max(max(max(s_l[0], s_l[1]), max(s_l[2], s_l[3])), score_floor);
        beams = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        // no beam scored at any heading: nothing is searched (no U reaches this bound)
        ctl[(size_t)scan * kLocCtl + tid] = tid == kLcBound ? (beams ? L : 0xFFFFFFFFu) : tid == kLcBeams ? beams : 0u;
    }
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_seed(LocBox g, const uint32_t* __restrict__ U, uint32_t* __restrict__ ctl,
                                                               uint2* __restrict__ list, LocSlot* __restrict__ slots) {
    __shared__ unsigned long long s_key[kLocWaves];
    __shared__ uint32_t s_c[kLocWaves];
    const int scan = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int H = g.H, nbx = (g.nx + (1 << H) - 1) >> H, nby = (g.ny + (1 << H) - 1) >> H, nblk = nbx * nby;
    const uint32_t total = (uint32_t)g.n_ang * (uint32_t)nblk;      // <= 2^28
    uint32_t* myctl = ctl + (size_t)scan * kLocCtl;
    const uint32_t L = myctl[kLcBound];
    const uint32_t* myU = U + (size_t)scan * total;
    uint2* mylist = list + (size_t)scan * g.max_nodes;
    unsigned long long key = 0;
    uint32_t cnt = 0;
    for (uint32_t base = blockIdx.y * kGmLanes; base < total; base += gridDim.y * kGmLanes) {      // (uniform in the wavefront)
        const uint32_t t = base + tid;
        uint32_t u = 0;
        const bool keep = t < total && (u = myU[t]) >= L;
        const unsigned long long m = __ballot(keep);
        if (m == 0) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&myctl[H], (uint32_t)__builtin_popcountll(m));
        at = (uint32_t)__shfl((int)at, 0, 64) + (uint32_t)lanes_below(m);
        if (keep && H == 0) {                                        // the top nodes are the candidates: lin = t
            loc_merge(key, cnt, ((unsigned long long)u << kLocLinBits) | (kLocLinMask - t), 1u);
        } else if (keep && at < g.max_nodes) {
            const uint32_t a = t / (uint32_t)nblk, r = t - a * (uint32_t)nblk, Q = r / (uint32_t)nbx, P = r - Q * (uint32_t)nbx;
            mylist[at] = make_uint2((Q << 16) | P, a);               // (H >= 1: Q, P < 2^15)
        }
    }
    if (H == 0) loc_store_slot(key, cnt, slots + (size_t)scan * kLocSlots + blockIdx.y, s_key, s_c);
}

__global__ __launch_bounds__(kGmLanes) void k_grid_locate_expand(LocBox g, int h, const uint8_t* __restrict__ plane, const short2* __restrict__ offs,
                                                                 const uint32_t* __restrict__ nbs, uint32_t* __restrict__ ctl,
                                                                 const uint2* __restrict__ in, uint2* __restrict__ out, LocSlot* __restrict__ slots) {
    __shared__ unsigned long long s_key[kLocWaves];
    __shared__ uint32_t s_c[kLocWaves];
    const int scan = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool last = h == 1;
    uint32_t* myctl = ctl + (size_t)scan * kLocCtl;
    uint32_t count = myctl[h];
    if (count > g.max_nodes) count = 0;                              // the overflow: this level and those below are not run
    count = min(count, g.max_nodes);
    const uint32_t L = myctl[kLcBound];
    const uint2* myin = in + (size_t)scan * g.max_nodes;
    uint2* myout = out + (size_t)scan * g.max_nodes;
    const int side = 1 << (h - 1);
    unsigned long long key = 0;
    uint32_t cnt = 0, scored = 0, front0 = 0;
    for (uint32_t p = blockIdx.y * kLocWaves + wave; p < count; p += gridDim.y * kLocWaves) {      // a parent per wavefront
        const uint2 e = myin[p];
        const int a = (int)min(e.y, (uint32_t)(g.n_ang - 1)), Q = (int)(e.x >> 16), P = (int)(e.x & 0xFFFFu);
        const size_t sa = (size_t)scan * g.n_ang + a;
        const int n = (int)min(nbs[sa], (uint32_t)g.stride);
        const short2* mine = offs + sa * g.stride;
        const int cp = 2 * P, cq = 2 * Q;
        const bool ex1 = (cp + 1) * side < g.nx, ex2 = (cq + 1) * side < g.ny;     // (child 0 exists: its parent does)
        const int X = g.x0 + cp * side, Y = g.y0 + cq * side;
        uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0;
        for (int k = lane; k < n; k += 64) {
            const short2 o = mine[k];
            const int x = X + o.x, y = Y + o.y;
            u0 += loc_cell(plane, g.cols, g.rows, h - 1, x, y);
            if (ex1) u1 += loc_cell(plane, g.cols, g.rows, h - 1, x + side, y);
            if (ex2) u2 += loc_cell(plane, g.cols, g.rows, h - 1, x, y + side);
            if (ex1 && ex2) u3 += loc_cell(plane, g.cols, g.rows, h - 1, x + side, y + side);
        }
        u0 = loc_wave_sum(u0); u1 = loc_wave_sum(u1); u2 = loc_wave_sum(u2); u3 = loc_wave_sum(u3);
        if (lane == 0) {
            const uint32_t u[4] = {u0, u1, u2, u3};
            const bool ex[4] = {true, ex1, ex2, ex1 && ex2};
            uint32_t ns = 0;
            for (int c = 0; c < 4; c++) {
                scored += ex[c];
                ns += ex[c] && u[c] >= L;
            }
            uint32_t at = 0;
            if (last) front0 += ns;
            else if (ns) at = atomicAdd(&myctl[h - 1], ns);          // one atomic for the wavefront
            for (int c = 0; c < 4; c++) {
                if (!(ex[c] && u[c] >= L)) continue;
                const uint32_t q = (uint32_t)(cq + (c >> 1)), pp = (uint32_t)(cp + (c & 1));
                if (last) {
                    const unsigned long long lin = ((unsigned long long)a * g.ny + q) * g.nx + pp;
                    loc_merge(key, cnt, ((unsigned long long)u[c] << kLocLinBits) | (kLocLinMask - lin), 1u);
                } else {
                    if (at < g.max_nodes) myout[at] = make_uint2((q << 16) | pp, (uint32_t)a);
                    at++;
                }
            }
        }
    }
    if (lane == 0) {
        if (scored) atomicAdd(&myctl[kLcScored], scored);
        if (front0) atomicAdd(&myctl[0], front0);
    }
    if (last) loc_store_slot(key, cnt, slots + (size_t)scan * kLocSlots + blockIdx.y, s_key, s_c);
}

__global__ __launch_bounds__(64) void k_grid_locate_pick(LocBox g, int n_slots, double ang0, double ang_step, uint32_t min_beams, uint32_t min_num,
                                                         uint32_t min_den, const uint32_t* __restrict__ nbs, const uint32_t* __restrict__ ctl,
                                                         const LocSlot* __restrict__ slots, unsigned long long* __restrict__ out,
                                                         uint32_t* __restrict__ stats) {
    const int scan = blockIdx.x, lane = threadIdx.x, H = g.H;
    const uint32_t* myctl = ctl + (size_t)scan * kLocCtl;
    unsigned long long key = 0;
    uint32_t cnt = 0;
    for (int i = lane; i < n_slots; i += 64) {
        const LocSlot s = slots[(size_t)scan * kLocSlots + i];
        loc_merge(key, cnt, s.key, s.cnt);
    }
    loc_wave_merge(key, cnt);
    if (lane != 0) return;
    const unsigned long long sentinel_xy = (unsigned long long)__double_as_longlong(-1.0);
    unsigned long long w[8] = {sentinel_xy, sentinel_xy, 0, 0, 0, 0, 0, 0};
    uint32_t st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t beams = myctl[kLcBeams];
    uint32_t flags, L = 0;
    if (beams == 0) {
        flags = LSD_GRID_LOCATE_EMPTY;
    } else {
        L = myctl[kLcBound];
        const int nbx = (g.nx + (1 << H) - 1) >> H, nby = (g.ny + (1 << H) - 1) >> H;
        st[0] = (uint32_t)g.n_ang * (uint32_t)(nbx * nby);
        bool overflow = false;
        for (int h = H; h >= 0; h--) {
            st[1 + h] = myctl[h];
            if (h >= 1 && myctl[h] > g.max_nodes) { overflow = true; break; }     // (the levels below were not run: their counts are 0)
        }
        st[10] = st[0] + myctl[kLcScored];
        if (overflow) {
            flags = LSD_GRID_LOCATE_OVERFLOW;
        } else if (myctl[0] == 0 || cnt == 0) {
            flags = LSD_GRID_LOCATE_NOT_FOUND;
        } else {
            const uint32_t S = (uint32_t)(key >> kLocLinBits);
            const unsigned long long lin = kLocLinMask - (key & kLocLinMask), per = (unsigned long long)g.nx * g.ny;
            const int a = (int)min(lin / per, (unsigned long long)(g.n_ang - 1));
            const unsigned long long rem = lin - (unsigned long long)a * per;
            const int q = (int)(rem / g.nx), p = (int)(rem - (unsigned long long)q * g.nx);
            const uint32_t nb = nbs[(size_t)scan * g.n_ang + a];
            const int cx = g.x0 + p, cy = g.y0 + q;
            const bool ok = nb >= min_beams && (unsigned long long)S * min_den >= 255ull * nb * min_num;
            flags = ok ? LSD_GRID_LOCATE_ACCEPTED : LSD_GRID_LOCATE_REJECTED;
            if (ok) {
                w[0] = (unsigned long long)__double_as_longlong((double)cx);
                w[1] = (unsigned long long)__double_as_longlong((double)cy);
                w[2] = (unsigned long long)__double_as_longlong(ang0 + (double)a * ang_step);
            }
            w[3] = (unsigned long long)S | ((unsigned long long)nb << 32);
            w[4] = (unsigned long long)(uint32_t)cx | ((unsigned long long)(uint32_t)cy << 32);
            w[5] = (unsigned long long)(uint32_t)a;
            w[6] = (unsigned long long)cnt;
        }
    }
    w[5] |= (unsigned long long)flags << 32;
    w[6] |= (unsigned long long)L << 32;
    for (int i = 0; i < 8; i++) out[(size_t)scan * 8 + i] = w[i];
    if (stats)
        for (int i = 0; i < 12; i++) stats[(size_t)scan * 12 + i] = st[i];
}

size_t grid_pyramid_offset(int cols, int rows, int h) {
    size_t at = 0;
    for (int l = 0; l < h; l++) at += (size_t)(cols + (1 << l) - 1) * (rows + (1 << l) - 1);
    return at;
}

void launch_grid_pyramid(const uint8_t* corr, int cols, int rows, int levels, uint8_t* pyramid, hipStream_t s) {
    for (int h = 0; h <= levels; h++) {
        const int m = (1 << h) - 1;
        const dim3 grid((cols + m + 63) / 64, (rows + m + 3) / 4);
        const uint8_t* prev = h == 0 ? corr : pyramid + grid_pyramid_offset(cols, rows, h - 1);
        hipLaunchKernelGGL(k_grid_pyramid_level, grid, dim3(256), 0, s, prev, cols, rows, h, pyramid + grid_pyramid_offset(cols, rows, h));
    }
}

size_t grid_locate_top_nodes(const lsd_grid_locate_par& par) {
    const size_t b = (size_t)1 << par.levels;
    return (size_t)par.n_ang * ((par.nx + b - 1) / b) * ((par.ny + b - 1) / b);
}

void grid_locate_ws(int n_scans, int stride, const lsd_grid_locate_par& par, size_t bytes[kGridLocateRegions]) {
    const size_t ns = (size_t)n_scans, sa = ns * par.n_ang, list = par.levels ? ns * par.max_nodes * sizeof(uint2) : 0;
    bytes[0] = sa * stride * sizeof(short2);
    bytes[1] = sa * sizeof(uint32_t);
    bytes[2] = sa * sizeof(uint32_t);
    bytes[3] = ns * grid_locate_top_nodes(par) * sizeof(uint32_t);
    bytes[4] = list;
    bytes[5] = list;
    bytes[6] = ns * kLocCtl * sizeof(uint32_t);
    bytes[7] = ns * kLocSlots * sizeof(LocSlot);
}

// the launches both searches begin with: the offsets, the top level with the descent of every heading, the bound, the seed of F_H
LocGeom launch_grid_locate_head(const lsd_polar* scans, const int* lens, int n_scans, int stride, int cols, int rows, double resol, double range_max,
                                const uint8_t* pyramid, const lsd_grid_locate_par& par, void* const ws[kGridLocateRegions], hipStream_t s) {
    short2* offs = static_cast<short2*>(ws[0]);
    uint32_t *nbs = static_cast<uint32_t*>(ws[1]), *la = static_cast<uint32_t*>(ws[2]), *U = static_cast<uint32_t*>(ws[3]);
    uint32_t* ctl = static_cast<uint32_t*>(ws[6]);
    LocSlot* slots = static_cast<LocSlot*>(ws[7]);
    LocGeom q;
    q.g = LocBox{cols, rows, par.x0, par.y0, par.nx, par.ny, par.n_ang, stride, par.levels, par.max_nodes};
    for (int h = 0; h <= LSD_GRID_LOCATE_MAX_LEVELS; h++) q.pl.off[h] = grid_pyramid_offset(cols, rows, h);
    const dim3 per_heading(n_scans, par.n_ang);
    hipLaunchKernelGGL(k_grid_locate_offsets, per_heading, dim3(kGmLanes), 0, s, reinterpret_cast<const double2*>(scans), lens, stride, resol,
                       range_max, par.ang0, par.ang_step, par.n_ang, offs, nbs);
    hipLaunchKernelGGL(k_grid_locate_top, per_heading, dim3(kGmLanes), 0, s, q.g, q.pl, pyramid, offs, nbs, U, la);
    hipLaunchKernelGGL(k_grid_locate_bound, dim3(n_scans), dim3(kGmLanes), 0, s, par.n_ang, par.score_floor, nbs, la, ctl);
    // the geometry of the seed and the expansions comes from the parameters, never from the data
    const size_t top = grid_locate_top_nodes(par);
    q.g_seed = (int)std::min<size_t>((top + kGmLanes - 1) / kGmLanes, kLocSlots);
    q.g_exp = (int)std::min<size_t>(((size_t)par.max_nodes + kLocWaves - 1) / kLocWaves, kLocSlots);
    hipLaunchKernelGGL(k_grid_locate_seed, dim3(n_scans, q.g_seed), dim3(kGmLanes), 0, s, q.g, U, ctl, static_cast<uint2*>(ws[4]), slots);
    return q;
}

void launch_grid_locate(const lsd_polar* scans, const int* lens, int n_scans, int stride, int cols, int rows, double resol, double range_max,
                        const uint8_t* pyramid, const lsd_grid_locate_par& par, void* const ws[kGridLocateRegions], lsd_grid_locate_rec* out,
                        lsd_grid_locate_stats* stats, hipStream_t s) {
    const LocGeom q = launch_grid_locate_head(scans, lens, n_scans, stride, cols, rows, resol, range_max, pyramid, par, ws, s);
    const short2* offs = static_cast<const short2*>(ws[0]);
    const uint32_t* nbs = static_cast<const uint32_t*>(ws[1]);
    uint2* lists[2] = {static_cast<uint2*>(ws[4]), static_cast<uint2*>(ws[5])};
    uint32_t* ctl = static_cast<uint32_t*>(ws[6]);
    LocSlot* slots = static_cast<LocSlot*>(ws[7]);
    const int H = par.levels;
    int cur = 0;
    for (int h = H; h >= 1; h--, cur ^= 1)
        hipLaunchKernelGGL(k_grid_locate_expand, dim3(n_scans, q.g_exp), dim3(kGmLanes), 0, s, q.g, h, pyramid + q.pl.off[h - 1], offs, nbs, ctl,
                           lists[cur], lists[cur ^ 1], slots);
    hipLaunchKernelGGL(k_grid_locate_pick, dim3(n_scans), dim3(64), 0, s, q.g, H ? q.g_exp : q.g_seed, par.ang0, par.ang_step, par.min_beams,
                       par.min_num, par.min_den, nbs, ctl, slots, reinterpret_cast<unsigned long long*>(out), reinterpret_cast<uint32_t*>(stats));
}

}  // namespace lsdhip
