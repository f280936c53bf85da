// gridlocate_dev.h -- what k_gridlocate.hip and k_gridlocate_tight.hip share (gfx950): the workspace's records and counters, a cell of a
// pyramid plane, the wave reductions, the slot merge and the launches both searches begin with; and the tight search's own descent,
// expansion and pick (loc_descend, loc_expand, loc_pick).  Those three restate the loops of k_grid_locate_top, k_grid_locate_expand and
// k_grid_locate_pick, which keep their own text in k_gridlocate.hip: calling these from there changed the existing kernels' register
// allocation and instruction order, and the existing search's programs stay what they were.  The rule is
// include/lsd_hip.h's and DESIGN.md 8.1.12 / 8.1.14's.
#pragma once
#include "lsd_internal.h"
#include "gridmatch_dev.h"

namespace lsdhip {

constexpr int kLocWaves = kGmLanes / 64;
constexpr int kLocCtl = 16;                                          // words per scan: |F_h| for h = 0..8, then ...
constexpr int kLcScored = 9, kLcBound = 10, kLcBeams = 11;           // ... the children evaluated, L, the sum of nb(a)
constexpr int kLocSlots = 1024;                                      // the most workgroups per scan the seed and expansion kernels get
constexpr int kLocLinBits = 44;                                      // lin < 4096 * 65535^2 < 2^44 - 1; S < 2^20
constexpr unsigned long long kLocLinMask = (1ull << kLocLinBits) - 1;
static_assert(4096ull * 65535 * 65535 < kLocLinMask && kLocLinBits + 20 <= 64, "the key holds the score and the index");

// the tight search's words per scan: L_h for h = 0..8, the first count of a retried level h = 0..8, then ...
constexpr int kLocTight = 32;
constexpr int kLtBound = 0, kLtFirst = 9, kLtRetried = 18, kLtArmed = 19, kLtProbe = 20;   // ... the retried levels' bits, "the retry runs", max_a S_a

struct LocSlot { unsigned long long key; uint32_t cnt, pad; };       // per (scan, workgroup): the best key and the candidates with its S
static_assert(sizeof(LocSlot) == 16, "grid_locate_ws sizes the workspace by 16 bytes a slot");

struct LocBox { int cols, rows, x0, y0, nx, ny, n_ang, stride, H; uint32_t max_nodes; };
struct LocPlanes { size_t off[LSD_GRID_LOCATE_MAX_LEVELS + 1]; };    // the levels' offsets in the pyramid buffer
struct LocGeom { LocBox g; LocPlanes pl; int g_seed, g_exp; };      // what launch_grid_locate_head fixed: the box, the planes, the seed's and the expansions' workgroups per scan
LocGeom launch_grid_locate_head(const lsd_polar* scans, const int* lens, int n_scans, int stride, int cols, int rows, double resol, double range_max,
                                const uint8_t* pyramid, const lsd_grid_locate_par& par, void* const ws[kGridLocateRegions], hipStream_t s);

// plane_h at the cell (x, y) of the grid's frame, x = -(2^h - 1) .. cols - 1 and y likewise; 0 outside the plane
__device__ __forceinline__ uint32_t loc_cell(const uint8_t* __restrict__ plane, int cols, int rows, int h, int x, int y) {
    const int m = (1 << h) - 1, cx = x + m, cy = y + m, pc = cols + m;
    return (cx >= 0 && cx < pc && cy >= 0 && cy < rows + m) ? plane[(size_t)cy * pc + cx] : 0u;
}

__device__ __forceinline__ uint32_t loc_wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// (key, cnt): the largest key and the number of candidates whose S is its S; cnt == 0: none yet
__device__ __forceinline__ void loc_merge(unsigned long long& key, uint32_t& cnt, unsigned long long k2, uint32_t c2) {
    if (c2 == 0) return;
    if (cnt == 0) { key = k2; cnt = c2; return; }
    const unsigned long long s1 = key >> kLocLinBits, s2 = k2 >> kLocLinBits;
    if (s1 == s2) { cnt += c2; key = k2 > key ? k2 : key; }
    else if (s2 > s1) { key = k2; cnt = c2; }
}

__device__ __forceinline__ void loc_wave_merge(unsigned long long& key, uint32_t& cnt) {      // every lane gets the result
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long k2 = shfl_xor_u64(key, d);
        const uint32_t c2 = (uint32_t)__shfl_xor((int)cnt, d, 64);
        loc_merge(key, cnt, k2, c2);
    }
}

// the workgroup's (key, cnt) into its slot; every lane calls it
__device__ __forceinline__ void loc_store_slot(unsigned long long key, uint32_t cnt, LocSlot* slot, unsigned long long* s_key, uint32_t* s_c) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    loc_wave_merge(key, cnt);
    if (lane == 0) { s_key[wave] = key; s_c[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kLocWaves; w++) loc_merge(key, cnt, s_key[w], s_c[w]);
        LocSlot out;
        out.key = cnt ? key : 0; out.cnt = cnt; out.pad = 0;
        *slot = out;
    }
}

// the greedy descent from the node (Q, P) of level h0 >= 1 by a workgroup of kLocWaves wavefronts whose heading's n offsets are staged in
// s_off: child `wave` of the node, the beams dealt over the wavefront's lanes; the largest U, among equals the smallest (Q, P).  Every
// lane gets the S of the candidate it ends at.
__device__ __forceinline__ uint32_t loc_descend(const LocBox& g, const LocPlanes& pl, const uint8_t* __restrict__ pyr, const short2* s_off, int n, int h0,
                                                int Q, int P, uint32_t val, uint32_t* s_u) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h = h0; h >= 1; h--) {
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
    return val;
}

// what a wavefront of the tight expansion holds back for one heading before it goes to the heading's key: U << 32 | 0xFFFFFFFF - (Q nbx + P)
struct LocHeadKey { unsigned long long key; int a; };

// the heading's key only grows, so a plain load that already shows a key as large spares the atomic (a stale load costs one atomic more)
__device__ __forceinline__ void loc_flush_head(const LocHeadKey& k, unsigned long long* __restrict__ heads) {
    if (k.key == 0) return;
    unsigned long long* at = heads + k.a;
    if (*(volatile unsigned long long*)at < k.key) atomicMax(at, k.key);
}

// One level h of the search for the workgroup (blockIdx.x = the scan, blockIdx.y of gridDim.y workgroups): the parents of `in` -- their
// count read on the device and clamped to max_nodes (a count above it is the overflow: the level is not run) -- a parent per wavefront, its
// lanes splitting the heading's beams; lane 0 appends the survivors with one atomic for the wavefront; at h = 1 the children are candidates
// and enter the key maximum and the count of equals.  heads (may be null) points at the scan's n_ang keys, which receive the best
// surviving child of every heading.
__device__ __forceinline__ void loc_expand(const LocBox& g, int h, const uint8_t* __restrict__ plane, const short2* __restrict__ offs,
                                           const uint32_t* __restrict__ nbs, uint32_t* __restrict__ ctl, const uint2* __restrict__ in,
                                           uint2* __restrict__ out, LocSlot* __restrict__ slots, unsigned long long* __restrict__ heads,
                                           unsigned long long* s_key, uint32_t* s_c) {
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
    LocHeadKey held{0, 0};
    const uint32_t nbx_c = (uint32_t)((g.nx + side - 1) >> (h - 1));  // the children's nodes per row
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
                    if (heads) {                                 // every survivor, listed or not; q nbx + p <= 2^30 at level 1
                        const unsigned long long hk = ((unsigned long long)u[c] << 32) | (0xFFFFFFFFu - (q * nbx_c + pp));
                        if (held.a != a) { loc_flush_head(held, heads); held.key = 0; held.a = a; }
                        held.key = hk > held.key ? hk : held.key;
                    }
                }
            }
        }
    }
    if (lane == 0) {
        if (scored) atomicAdd(&myctl[kLcScored], scored);
        if (front0) atomicAdd(&myctl[0], front0);
        if (heads) loc_flush_head(held, heads);
    }
    if (last) loc_store_slot(key, cnt, slots + (size_t)scan * kLocSlots + blockIdx.y, s_key, s_c);
}

// One wavefront per scan: the key maximum over the workgroups' slots (S, then 2^44 - 1 - lin), n_best, the outcome, the record and the
// statistics: thirty-two words, the first twelve k_grid_locate_pick's -- then the retried levels, L_h and the first counts from the scan's kLocTight words.
__device__ __forceinline__ void loc_pick(const LocBox& g, int n_slots, double ang0, double ang_step, uint32_t min_beams, uint32_t min_num,
                                         uint32_t min_den, const uint32_t* __restrict__ nbs, const uint32_t* __restrict__ ctl,
                                         const uint32_t* __restrict__ tight, const LocSlot* __restrict__ slots, unsigned long long* __restrict__ out,
                                         uint32_t* __restrict__ stats) {
    constexpr int kWords = 32;
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
    uint32_t st[kWords] = {};
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
        const uint32_t* mine = tight + (size_t)scan * kLocTight;      // (the words of a level that was not run are 0: k_grid_locate_tight_level)
        st[11] = mine[kLtRetried];
        for (int h = 1; h <= LSD_GRID_LOCATE_MAX_LEVELS; h++) { st[12 + h] = mine[kLtBound + h]; st[21 + h] = mine[kLtFirst + h]; }
        st[12] = overflow ? 0u : L;                                  // L_0 = L_1: no probe follows the last expansion
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
        for (int i = 0; i < kWords; i++) stats[(size_t)scan * kWords + i] = st[i];
}

static_assert(sizeof(lsd_grid_locate_rec) == 64 && offsetof(lsd_grid_locate_rec, score) == 24 && offsetof(lsd_grid_locate_rec, cx) == 32 &&
              offsetof(lsd_grid_locate_rec, a) == 40 && offsetof(lsd_grid_locate_rec, flags) == 44 && offsetof(lsd_grid_locate_rec, n_best) == 48 &&
              offsetof(lsd_grid_locate_rec, lower_bound) == 52, "the picks write the record as eight 64-bit words");
static_assert(sizeof(lsd_grid_locate_stats) == 48 && offsetof(lsd_grid_locate_stats, frontier) == 4 && offsetof(lsd_grid_locate_stats, scored) == 40,
              "k_grid_locate_pick writes the statistics as twelve words");
static_assert(sizeof(lsd_grid_locate_tight_stats) == 128 && offsetof(lsd_grid_locate_tight_stats, frontier) == 4 &&
              offsetof(lsd_grid_locate_tight_stats, scored) == 40 && offsetof(lsd_grid_locate_tight_stats, retried) == 44 &&
              offsetof(lsd_grid_locate_tight_stats, bound) == 48 && offsetof(lsd_grid_locate_tight_stats, first_count) == 84,
              "loc_pick writes the tight statistics as thirty-two words whose first twelve are lsd_grid_locate_stats");

}  // namespace lsdhip
