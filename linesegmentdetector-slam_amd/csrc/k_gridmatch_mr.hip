// k_gridmatch_mr.hip -- the correlative match of k_gridmatch.hip as a two-level (coarse-to-fine) search (gfx950): Olson's multi-resolution
// form, held to the plain search byte for byte.  A plane of block maxima bounds the score of a whole b x b block of translations from
// above; a block whose bound is below a score already reached cannot hold the winner and is never scored.  The rule (DESIGN.md 8.1.8,
// include/lsd_hip.h) is made of integers and tests/grid_match_mr_cases.py restates it.  No atomics.
//
// k_grid_coarse: coarse[y + b - 1][x + b - 1] = the maximum of corr over the b x b cells from (x, y) up, cells outside the grid as 0, for
//   x = -(b - 1) .. cols - 1 and y likewise.  A workgroup of 256 lanes owns a tile of 32 x 8 outputs; it stages the (32 + b - 1) x
//   (8 + b - 1) cells they cover in LDS (at most 47 x 23 at a pitch of 48), takes the row maxima in LDS (23 x 32), then every lane the
//   column maximum of its own output.  One byte per cell in and out: a bandwidth kernel.
// k_grid_match_coarse: n_scans x (2 na + 1) workgroups of 256 lanes.  Phase A of k_grid_match (gridmatch_dev.h: the same text) with
//   the window widened on the high side to the whole block grid -- the last block may overhang the window, and a beam that only its
//   overhang reaches still counts in U.  Then one lane per block -- a group of up to 64 lanes where the blocks are few, the list dealt over
//   them (gm_score_split) -- sums U over the list and writes it to workspace; the workgroup finds
//   the seed, the largest (U, smaller index) by a key maximum; the seed's b^2 <= 256 candidates are scored one per lane; L_a, nb, S at the
//   zero offset and the seed go to a 16-byte slot.
// k_grid_match_fine: n_scans x (2 na + 1) workgroups.  L = the maximum of the scan's L_a (at most 127 words, read by every workgroup).
//   Phase A once more (recomputed, not read back: see DESIGN.md 8.1.8).  The blocks of this angle with U >= L are compacted into LDS
//   (ballot / mbcnt, as phase A compacts beams), and their candidates are dealt to the lanes as items in order, item t to lane t mod 256:
//   item t is cell t mod b^2 of survivor t / b^2 (a cell beyond the window idles its lane for that item); fewer than 129 items get groups
//   of lanes, as the blocks of the coarse kernel do.  The key maximum, nb and s0 go
//   to a GmSlot exactly as k_grid_match writes it -- key 0 where nothing survived --, and k_grid_match_pick finishes unchanged.
// k_grid_match_mr_stats: one wavefront per scan sums the per-angle counts into the 16-byte statistics record; launched only when asked for.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950, -O3):
//   k_grid_coarse           VGPRs 37   SGPRs  35   scratch 0 bytes   LDS  1840 bytes   8 waves / SIMD
//   k_grid_match_coarse     VGPRs 55   SGPRs  95   scratch 0 bytes   LDS 32864 bytes   4 waves / SIMD (the LDS: four workgroups per CU)
//   k_grid_match_fine       VGPRs 61   SGPRs 105   scratch 0 bytes   LDS 41040 bytes   3 waves / SIMD (the LDS: three workgroups per CU)
//   k_grid_match_mr_stats   VGPRs 27   SGPRs  31   scratch 0 bytes   LDS     0 bytes   8 waves / SIMD
#include "lsd_internal.h"
#include "gridmatch_dev.h"

namespace lsdhip {

constexpr int kCoTileW = 32, kCoTileH = 8, kCoMaxBlock = 16;
constexpr int kCoPitch = 48, kCoRows = kCoTileH + kCoMaxBlock - 1;       // the staged cells: (32 + 15) x (8 + 15)
static_assert(kCoPitch >= kCoTileW + kCoMaxBlock - 1 && kCoTileW * kCoTileH == 256 && kCoMaxBlock * kCoMaxBlock <= kGmLanes, "one workgroup");
constexpr int kMrMaxBlocks = ((2 * kGmMaxWin + 1 + 1) / 2) * ((2 * kGmMaxWin + 1 + 1) / 2);     // b = 2 at the widest window: 64 x 64
static_assert(kMrMaxBlocks == 4096, "s_blk holds every block of an angle");

struct MrSlot { uint32_t la, nb, s0, seed; };                        // per (scan, angle), written by k_grid_match_coarse
struct MrCount { uint32_t refined, fine; };                          // per (scan, angle), written by k_grid_match_fine
static_assert(sizeof(MrSlot) == 16 && sizeof(MrCount) == 8, "grid_match_mr_ws sizes the workspace by these");

__global__ __launch_bounds__(256) void k_grid_coarse(const uint8_t* __restrict__ corr, int cols, int rows, int b, uint8_t* __restrict__ coarse) {
    __shared__ uint8_t s_in[kCoRows * kCoPitch];
    __shared__ uint8_t s_row[kCoRows * kCoTileW];
    const int tid = threadIdx.x, h = b - 1;
    const int ccols = cols + h, crows = rows + h;
    const int tx0 = blockIdx.x * kCoTileW, ty0 = blockIdx.y * kCoTileH;            // in coarse coordinates
    const int lw = kCoTileW + h, lh = kCoTileH + h;
    for (int t = tid; t < lw * lh; t += 256) {
        const int ly = t / lw, lx = t - ly * lw;
        const int gx = tx0 - h + lx, gy = ty0 - h + ly;                             // output (ox, oy) covers the cells from (ox - h, oy - h) up
        uint8_t v = 0;
        if (gx >= 0 && gx < cols && gy >= 0 && gy < rows) v = corr[(size_t)gy * cols + gx];
        s_in[ly * kCoPitch + lx] = v;
    }
    __syncthreads();
    for (int t = tid; t < lh * kCoTileW; t += 256) {
        const int ly = t / kCoTileW, lx = t & (kCoTileW - 1);
        const uint8_t* p = s_in + ly * kCoPitch + lx;
        uint32_t m = 0;
        for (int u = 0; u < b; u++) m = max(m, (uint32_t)p[u]);
        s_row[t] = (uint8_t)m;
    }
    __syncthreads();
    const int lx = tid & (kCoTileW - 1), ly = tid / kCoTileW;
    const int ox = tx0 + lx, oy = ty0 + ly;
    if (ox >= ccols || oy >= crows) return;
    uint32_t m = 0;
    for (int v = 0; v < b; v++) m = max(m, (uint32_t)s_row[(ly + v) * kCoTileW + lx]);
    coarse[(size_t)oy * ccols + ox] = (uint8_t)m;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__global__ __launch_bounds__(kGmLanes) void k_grid_match_coarse(const double2* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                                const uint8_t* __restrict__ poses, size_t pose_pitch, int cols, int rows,
                                                                double resol, double range_max, const uint8_t* __restrict__ corr,
                                                                const uint8_t* __restrict__ coarse, int b, int wx, int wy, int na,
                                                                double ang_step, uint32_t* __restrict__ U, MrSlot* __restrict__ mslots) {
    __shared__ int2 s_end[kGmMaxBeams];
    __shared__ unsigned long long s_key[kGmLanes / 64];
    __shared__ int s_cnt[kGmLanes / 64];
    __shared__ uint32_t s_nb[kGmLanes / 64], s_la[kGmLanes / 64], s_z[kGmLanes / 64];
    const int scan = blockIdx.x, ai = blockIdx.y, a = ai - na, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    if (gm_scan_skipped(px, py, pang)) return;
    const int len = min(max(lens[scan], 0), stride);
    const double rot0 = deg2rad_ref(pang), rot = deg2rad_ref(pang + (double)a * ang_step);
    const int nx = 2 * wx + 1, ny = 2 * wy + 1, nbx = (nx + b - 1) / b, nby = (ny + b - 1) / b, nblk = nbx * nby;
    // A. the end cells of this angle; the window reaches to the end of the last block
    uint32_t nb = 0;
    const int n_list = gm_end_cells(scans + (size_t)scan * stride, len, px, py, rot0, rot, resol, range_max, cols, rows, wx, wy, nbx * b - nx,
                                    nby * b - ny, s_end, s_cnt, nb);
    // B. U of every block, one lane per block; the seed: the largest U, among equals the smallest index
    const int h = b - 1, ccols = cols + h, crows = rows + h;
    uint32_t* myU = U + ((size_t)scan * (2 * na + 1) + ai) * nblk;
    unsigned long long best = 0;
    const int Pu = gm_split(nblk);                                   // few blocks: the list is dealt over Pu lanes a block
    for (int base = 0; base < nblk; base += kGmLanes / Pu) {
        const int blk = base + tid / Pu;
        const bool act = blk < nblk;
        const int J = blk / nbx, I = blk - J * nbx;
        // the coarse cell of the end cell (ex, ey) for the block whose low corner is the translation (-wx + I b, -wy + J b)
        const uint32_t u = gm_score_split(s_end, n_list, coarse, ccols, crows, -wx + I * b + h, -wy + J * b + h, tid & (Pu - 1), Pu, act);
        if (act && (tid & (Pu - 1)) == 0) {
            myU[blk] = u;
            const unsigned long long key = ((unsigned long long)u << 32) | (0xFFFFFFFFu - (uint32_t)blk);
            best = key > best ? key : best;
        }
    }
    best = wave_max_u64(best);
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    for (int w = 0; w < kGmLanes / 64; w++) best = s_key[w] > best ? s_key[w] : best;
    const int seed = (int)(0xFFFFFFFFu - (uint32_t)best);            // (nblk >= 1: some lane made a key)
    // C. the seed's candidates, one per lane: L_a; and S at the zero offset, the list dealt to the lanes
    uint32_t la = 0;
    {
        const int Ps = gm_split(b * b), cell = tid / Ps;
        const int J = seed / nbx, I = seed - J * nbx, v = cell / b, u = cell - v * b;
        const int i = -wx + I * b + u, j = -wy + J * b + v;
        la = gm_score_split(s_end, n_list, corr, cols, rows, i, j, tid & (Ps - 1), Ps, v < b && i <= wx && j <= wy);
    }
    uint32_t z = 0;
    for (int k = tid; k < n_list; k += kGmLanes) {
        const int2 e = s_end[k];
        if (e.x >= 0 && e.x < cols && e.y >= 0 && e.y < rows) z += corr[(size_t)e.y * cols + e.x];
    }
    la = wave_max_u32(la);
    z = wave_sum_u32(z);
    nb = wave_sum_u32(nb);
    if (lane == 0) { s_la[wave] = la; s_z[wave] = z; s_nb[wave] = nb; }
    __syncthreads();
    if (tid == 0) {
        MrSlot out;
        out.la = max(max(s_la[0], s_la[1]), max(s_la[2], s_la[3]));
        out.nb = s_nb[0] + s_nb[1] + s_nb[2] + s_nb[3];
        out.s0 = s_z[0] + s_z[1] + s_z[2] + s_z[3];
        out.seed = (uint32_t)seed;
        mslots[(size_t)scan * (2 * na + 1) + ai] = out;
    }
}

__global__ __launch_bounds__(kGmLanes) void k_grid_match_fine(const double2* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                              const uint8_t* __restrict__ poses, size_t pose_pitch, int cols, int rows,
                                                              double resol, double range_max, const uint8_t* __restrict__ corr, int b, int wx,
                                                              int wy, int na, double ang_step, const uint32_t* __restrict__ U,
                                                              const MrSlot* __restrict__ mslots, GmSlot* __restrict__ slots,
                                                              MrCount* __restrict__ counts) {
    __shared__ int2 s_end[kGmMaxBeams];
    __shared__ uint16_t s_blk[kMrMaxBlocks];
    __shared__ unsigned long long s_key[kGmLanes / 64];
    __shared__ int s_cnt[kGmLanes / 64];
    __shared__ uint32_t s_l[kGmLanes / 64], s_fine[kGmLanes / 64];
    const int scan = blockIdx.x, ai = blockIdx.y, a = ai - na, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_ang = 2 * na + 1;
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    if (gm_scan_skipped(px, py, pang)) return;
    const int len = min(max(lens[scan], 0), stride);
    const double rot0 = deg2rad_ref(pang), rot = deg2rad_ref(pang + (double)a * ang_step);
    const int nx = 2 * wx + 1, ny = 2 * wy + 1, nbx = (nx + b - 1) / b, nby = (ny + b - 1) / b, nblk = nbx * nby;
    // L: the best score any angle's seed has reached
    const MrSlot* ms = mslots + (size_t)scan * n_ang;
    uint32_t L = tid < n_ang ? ms[tid].la : 0;                       // n_ang <= 127 < 256
    L = wave_max_u32(L);
    if (lane == 0) s_l[wave] = L;
    // A. the end cells once more: only the window itself is scored from here on
    uint32_t nb_unused = 0;
    const int n_list = gm_end_cells(scans + (size_t)scan * stride, len, px, py, rot0, rot, resol, range_max, cols, rows, wx, wy, 0, 0, s_end, s_cnt,
                                    nb_unused);
    __syncthreads();                                                 // (a scan of no readings runs no barrier in phase A)
    L = max(max(s_l[0], s_l[1]), max(s_l[2], s_l[3]));
    // B. the survivors of this angle, in block order
    const uint32_t* myU = U + ((size_t)scan * n_ang + ai) * nblk;
    int n_surv = 0;
    uint32_t fine = 0;
    for (int base = 0; base < nblk; base += kGmLanes) {
        const int blk = base + tid;
        const bool keep = blk < nblk && myU[blk] >= L;
        if (keep) {
            const int J = blk / nbx, I = blk - J * nbx;
            fine += (uint32_t)(min(b, nx - I * b) * min(b, ny - J * b));
        }
        const unsigned long long m = __ballot(keep);
        const int below = lanes_below(m);
        __syncthreads();                                             // (s_cnt: the last reads of the round before)
        if (lane == 0) s_cnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int at = n_surv, total = 0;
        for (int w = 0; w < kGmLanes / 64; w++) {
            const int cnt = s_cnt[w];
            if (w < wave) at += cnt;
            total += cnt;
        }
        if (keep) s_blk[at + below] = (uint16_t)blk;                 // at + below < n_surv + total <= nblk <= kMrMaxBlocks
        n_surv += total;
    }
    __syncthreads();
    // C. their candidates as items: item t is cell t mod b^2 of survivor t / b^2
    const int bb = b * b, n_items = n_surv * bb;
    const uint32_t aa = (uint32_t)(a < 0 ? -a : a);
    unsigned long long best = 0;
    const int Pf = gm_split(n_items);                                // few items: the list is dealt over Pf lanes an item
    for (int base = 0; base < n_items; base += kGmLanes / Pf) {
        const int t = base + tid / Pf;
        const bool in_list = t < n_items;
        const int sv = in_list ? t / bb : 0, cell = t - sv * bb, blk = s_blk[sv];
        const int J = blk / nbx, I = blk - J * nbx, v = cell / b, u = cell - v * b;
        const int ii = I * b + u, jj = J * b + v, i = ii - wx, j = jj - wy;
        const bool act = in_list && ii < nx && jj < ny;
        const uint32_t S = gm_score_split(s_end, n_list, corr, cols, rows, i, j, tid & (Pf - 1), Pf, act);
        if (act) {
            const unsigned long long key = gm_key(S, i, j, aa, (uint32_t)((ai * ny + jj) * nx + ii));
            best = key > best ? key : best;
        }
    }
    // D. the best of this angle, as k_grid_match writes it
    best = wave_max_u64(best);
    fine = wave_sum_u32(fine);
    if (lane == 0) { s_key[wave] = best; s_fine[wave] = fine; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long k = s_key[0];
        for (int w = 1; w < kGmLanes / 64; w++) k = s_key[w] > k ? s_key[w] : k;
        GmSlot out;
        out.key = k; out.nb = ms[ai].nb; out.s0 = ms[ai].s0;
        slots[(size_t)scan * n_ang + ai] = out;
        MrCount c;
        c.refined = (uint32_t)n_surv; c.fine = s_fine[0] + s_fine[1] + s_fine[2] + s_fine[3];
        counts[(size_t)scan * n_ang + ai] = c;
    }
}

__global__ __launch_bounds__(64) void k_grid_match_mr_stats(const uint8_t* __restrict__ poses, size_t pose_pitch, int b, int wx, int wy, int na,
                                                            const MrSlot* __restrict__ mslots, const MrCount* __restrict__ counts,
                                                            uint32_t* __restrict__ stats) {
    const int scan = blockIdx.x, lane = threadIdx.x, n_ang = 2 * na + 1;
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    uint32_t* out = stats + (size_t)scan * 4;
    if (gm_scan_skipped(pose[0], pose[1], pose[2])) {
        if (lane < 4) out[lane] = 0;
        return;
    }
    uint32_t refined = 0, fine = 0, L = 0;
    for (int ai = lane; ai < n_ang; ai += 64) {
        const MrCount c = counts[(size_t)scan * n_ang + ai];
        refined += c.refined;
        fine += c.fine;
        L = max(L, mslots[(size_t)scan * n_ang + ai].la);
    }
    refined = wave_sum_u32(refined);
    fine = wave_sum_u32(fine);
    L = wave_max_u32(L);
    if (lane == 0) {
        out[0] = (uint32_t)(n_ang * ((2 * wx + b) / b) * ((2 * wy + b) / b));
        out[1] = refined; out[2] = fine; out[3] = L;
    }
}

static_assert(sizeof(lsd_grid_match_mr_stats) == 16, "k_grid_match_mr_stats writes four words");

void launch_grid_coarse(const uint8_t* corr, int cols, int rows, int block, uint8_t* coarse, hipStream_t s) {
    const dim3 grid((cols + block - 1 + kCoTileW - 1) / kCoTileW, (rows + block - 1 + kCoTileH - 1) / kCoTileH);
    hipLaunchKernelGGL(k_grid_coarse, grid, dim3(256), 0, s, corr, cols, rows, block, coarse);
}

static inline size_t mr_blocks(const lsd_grid_search& se, int block) {
    return (size_t)((2 * se.wx + block) / block) * ((2 * se.wy + block) / block);
}

void grid_match_mr_ws(int n_scans, const lsd_grid_search& se, int block, size_t bytes[4]) {
    const size_t sa = (size_t)n_scans * (2 * se.na + 1);
    bytes[0] = sa * mr_blocks(se, block) * sizeof(uint32_t);
    bytes[1] = sa * sizeof(MrSlot);
    bytes[2] = sa * sizeof(MrCount);
    bytes[3] = sa * sizeof(GmSlot);
}

void launch_grid_match_mr(const GridScans& g, const uint8_t* corr, const uint8_t* coarse, int block, const lsd_grid_search& se, void* const ws[4],
                          lsd_grid_match_rec* out, lsd_grid_match_mr_stats* stats, hipStream_t s) {
    const dim3 grid(g.n_scans, 2 * se.na + 1);
    const double2* sc = reinterpret_cast<const double2*>(g.scans);
    const uint8_t* po = static_cast<const uint8_t*>(g.poses);
    uint32_t* U = static_cast<uint32_t*>(ws[0]);
    MrSlot* ms = static_cast<MrSlot*>(ws[1]);
    MrCount* mc = static_cast<MrCount*>(ws[2]);
    hipLaunchKernelGGL(k_grid_match_coarse, grid, dim3(kGmLanes), 0, s, sc, g.lens, g.stride, po, g.pose_pitch, g.cols, g.rows, g.resol, g.range_max,
                       corr, coarse, block, se.wx, se.wy, se.na, se.ang_step, U, ms);
    hipLaunchKernelGGL(k_grid_match_fine, grid, dim3(kGmLanes), 0, s, sc, g.lens, g.stride, po, g.pose_pitch, g.cols, g.rows, g.resol, g.range_max,
                       corr, block, se.wx, se.wy, se.na, se.ang_step, U, ms, static_cast<GmSlot*>(ws[3]), mc);
    launch_grid_match_pick(g.n_scans, g.poses, g.pose_pitch, se, ws[3], out, s);
    if (stats)
        hipLaunchKernelGGL(k_grid_match_mr_stats, dim3(g.n_scans), dim3(64), 0, s, po, g.pose_pitch, block, se.wx, se.wy, se.na, ms, mc,
                           reinterpret_cast<uint32_t*>(stats));
}

}  // namespace lsdhip
