// k_gridmatch.hip -- correlative scan-to-grid matching (gfx950): a scan's pose is corrected against the growing grid before the scan is
// integrated into it (Olson's / Karto's matcher in its plain form).  No reference counterpart.  Both rules (DESIGN.md 8.1.7,
// include/lsd_hip.h) are made of integers once the end cells are rounded and have no iteration order, so a numpy restatement
// (tests/grid_match_cases.py) gives the same bytes.
//
// k_grid_likelihood: the lookup plane.  A workgroup of 256 lanes owns a tile of 32 x 8 cells; it stages the OCCUPANCY (one byte per cell,
//   the publish rule's "100") of the tile and a halo of `radius` cells in LDS -- at most (32 + 14) x (8 + 14) cells at a pitch of 48 bytes:
//   1056 bytes --, cells outside the grid as free, then every lane takes the maximum of w[|v|][|u|] over the occupied cells of its
//   (2 r + 1)^2 window.  The table is read from the kernel argument (uniform indices: scalar loads).
// k_grid_match: a grid of n_scans x (2 na + 1) workgroups of 256 lanes, one per (scan, angle a).
//   A. one lane per beam, 256 at a time: the integration's skip tests, th = angle + deg2rad_ref(ang + a * ang_step), sincos_g ONCE per
//      (beam, angle), the rounded end cell.  nb counts the scored beams; the end cells of those whose window touches the grid at all (the
//      others add 0 to every candidate) are compacted into LDS by ballot / mbcnt inside a wavefront and four counts across them:
//      4096 x 2 int32 = 32 KiB, plus 64 bytes of reduction cells.
//   B. one lane per translation (j, i), 256 at a time, i fastest, so neighbouring lanes read neighbouring bytes of the plane.  Every lane
//      walks the LDS list (all lanes read the same entry: a broadcast, no bank conflict) and sums; the loads of kBeamBatch beams are issued
//      before they are accumulated, as match_candidate does with kPtBatch.
//   C. the best of this angle: the maximum of a packed 64-bit key -- S in bits 40..59, then 8191 - (i^2 + j^2), 63 - |a|, and
//      2^21 - 1 - the linear index, so the largest key IS the rule's winner -- by shuffles inside a wavefront and LDS across the four.
//      Key, nb and S at the zero offset go to the (scan, angle) slot.  No atomics.
// k_grid_match_pick: one wavefront per scan: the maximum over the 2 na + 1 slots, the acceptance test, the 56-byte record.
// A skipped scan (the same decision in every lane of both kernels) leaves its slots unwritten and unread.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950, -O3):
//   k_grid_likelihood   VGPRs 23   SGPRs 44   scratch 0 bytes   LDS  1056 bytes   8 waves / SIMD
//   k_grid_match        VGPRs 54   SGPRs 86   scratch 0 bytes   LDS 32840 bytes   4 waves / SIMD (the LDS: four workgroups per CU)
//   k_grid_match_pick   VGPRs 14   SGPRs 36   scratch 0 bytes   LDS     0 bytes   8 waves / SIMD
//
// The key, the slot and phase A live in gridmatch_dev.h, shared with the coarse-to-fine search of k_gridmatch_mr.hip, which ends in this
// file's k_grid_match_pick; k_gridresponse.hip reads the records for a sub-cell pose and a covariance of the response.  NOT in any of
// them: loop closure, the fleet classes.
#include "lsd_internal.h"
#include "gridmatch_dev.h"

namespace lsdhip {

constexpr int kLikeTileW = 32, kLikeTileH = 8, kLikeHalo = 7;
constexpr int kLikePitch = 48;                                       // >= kLikeTileW + 2 * kLikeHalo
constexpr int kLikeRows = kLikeTileH + 2 * kLikeHalo;
static_assert(kLikePitch >= kLikeTileW + 2 * kLikeHalo && kLikeTileW * kLikeTileH == 256, "the tile is one workgroup");

__global__ __launch_bounds__(256) void k_grid_likelihood(const uint32_t* __restrict__ pass, const uint32_t* __restrict__ hit, int cols, int rows,
                                                         uint32_t min_pass, uint32_t occ_num, uint32_t occ_den, lsd_grid_smear sm,
                                                         uint8_t* __restrict__ corr) {
    __shared__ uint8_t s_occ[kLikeRows * kLikePitch];
    const int tid = threadIdx.x, r = sm.radius;
    const int tx0 = blockIdx.x * kLikeTileW, ty0 = blockIdx.y * kLikeTileH;
    const int lw = kLikeTileW + 2 * r, lh = kLikeTileH + 2 * r;
    for (int t = tid; t < lw * lh; t += 256) {
        const int ly = t / lw, lx = t - ly * lw;
        const int gx = tx0 - r + lx, gy = ty0 - r + ly;
        uint8_t occ = 0;
        if (gx >= 0 && gx < cols && gy >= 0 && gy < rows) {
            const size_t at = (size_t)gy * cols + gx;
            const uint32_t p = pass[at], h = hit[at];
            occ = p >= min_pass && (unsigned long long)h * occ_den >= (unsigned long long)p * occ_num;
        }
        s_occ[ly * kLikePitch + lx] = occ;
    }
    __syncthreads();
    const int lx = tid & (kLikeTileW - 1), ly = tid / kLikeTileW;
    const int x = tx0 + lx, y = ty0 + ly;
    if (x >= cols || y >= rows) return;
    uint32_t best = 0;
    for (int v = -r; v <= r; v++) {
        const uint8_t* row = s_occ + (ly + r + v) * kLikePitch + lx + r;
        const int av = v < 0 ? -v : v;
        for (int u = -r; u <= r; u++) {
            const uint32_t w = sm.w[av][u < 0 ? -u : u];
            if (row[u] && w > best) best = w;
        }
    }
    corr[(size_t)y * cols + x] = (uint8_t)best;
}

__global__ __launch_bounds__(kGmLanes) void k_grid_match(const double2* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                         const uint8_t* __restrict__ poses, size_t pose_pitch, int cols, int rows, double resol,
                                                         double range_max, const uint8_t* __restrict__ corr, int wx, int wy, int na,
                                                         double ang_step, GmSlot* __restrict__ slots) {
    __shared__ int2 s_end[kGmMaxBeams];
    __shared__ unsigned long long s_key[kGmLanes / 64];
    __shared__ int s_cnt[kGmLanes / 64];
    __shared__ uint32_t s_nb[kGmLanes / 64];
    __shared__ uint32_t s_s0;
    const int scan = blockIdx.x, ai = blockIdx.y, a = ai - na, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    if (gm_scan_skipped(px, py, pang)) return;
    const int len = min(max(lens[scan], 0), stride);                 // (stride <= kGmMaxBeams: the entry refuses more)
    const double rot0 = deg2rad_ref(pang), rot = deg2rad_ref(pang + (double)a * ang_step);
    const double2* row = scans + (size_t)scan * stride;
    // A. the end cells of this angle (gridmatch_dev.h)
    uint32_t nb = 0;
    const int n_list = gm_end_cells(row, len, px, py, rot0, rot, resol, range_max, cols, rows, wx, wy, 0, 0, s_end, s_cnt, nb);
    // B. the translations
    const int nx = 2 * wx + 1, ny = 2 * wy + 1, n_tr = nx * ny;
    unsigned long long best = 0;
    const uint32_t aa = (uint32_t)(a < 0 ? -a : a);
    for (int t0 = 0; t0 < n_tr; t0 += kGmLanes) {
        const int t = t0 + tid;
        if (t < n_tr) {
            const int jj = t / nx, ii = t - jj * nx;
            const int i = ii - wx, j = jj - wy;
            const uint32_t S = gm_score(s_end, n_list, corr, cols, rows, i, j);
            const uint32_t lin = (uint32_t)((ai * ny + jj) * nx + ii);
            const unsigned long long key = gm_key(S, i, j, aa, lin);
            best = key > best ? key : best;
            if (i == 0 && j == 0) s_s0 = S;
        }
    }
    // C. the best of this angle
    best = wave_max_u64(best);
    for (int d = 32; d >= 1; d >>= 1) nb += (uint32_t)__shfl_xor((int)nb, d, 64);
    if (lane == 0) { s_key[wave] = best; s_nb[wave] = nb; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long k = s_key[0];
        uint32_t n = s_nb[0];
        for (int w = 1; w < kGmLanes / 64; w++) {
            k = s_key[w] > k ? s_key[w] : k;
            n += s_nb[w];
        }
        GmSlot out;
        out.key = k; out.nb = n; out.s0 = s_s0;
        slots[(size_t)scan * (2 * na + 1) + ai] = out;
    }
}

__global__ __launch_bounds__(64) void k_grid_match_pick(const uint8_t* __restrict__ poses, size_t pose_pitch, int wx, int wy, int na,
                                                        double ang_step, uint32_t min_beams, uint32_t min_num, uint32_t min_den,
                                                        const GmSlot* __restrict__ slots, unsigned long long* __restrict__ out) {
    const int scan = blockIdx.x, lane = threadIdx.x, n_ang = 2 * na + 1;
    const unsigned long long* pw = reinterpret_cast<const unsigned long long*>(poses + (size_t)scan * pose_pitch);
    const unsigned long long w0 = pw[0], w1 = pw[1], w2 = pw[2];     // the pose as bits: what is copied is copied exactly
    const double px = __longlong_as_double((long long)w0), py = __longlong_as_double((long long)w1), pang = __longlong_as_double((long long)w2);
    unsigned long long* rec = out + (size_t)scan * (sizeof(lsd_grid_match_rec) / 8);
    if (gm_scan_skipped(px, py, pang)) {
        if (lane == 0) {
            rec[0] = w0; rec[1] = w1; rec[2] = w2;
            rec[3] = 0; rec[4] = 0;
            rec[5] = (unsigned long long)LSD_GRID_MATCH_SKIPPED << 32;
            rec[6] = 0;
        }
        return;
    }
    const GmSlot* mine = slots + (size_t)scan * n_ang;
    unsigned long long best = 0;
    for (int ai = lane; ai < n_ang; ai += 64) {
        const unsigned long long k = mine[ai].key;
        best = k > best ? k : best;
    }
    best = wave_max_u64(best);
    if (lane != 0) return;
    const uint32_t S = (uint32_t)(best >> kKeyScoreShift);
    const int lin = (int)(((1u << kKeyLinBits) - 1) - (uint32_t)(best & ((1u << kKeyLinBits) - 1)));
    const int nx = 2 * wx + 1, ny = 2 * wy + 1;
    const int ai = lin / (nx * ny), rem = lin - ai * (nx * ny), jj = rem / nx, ii = rem - jj * nx;
    const int di = ii - wx, dj = jj - wy, da = ai - na;
    const uint32_t nb = mine[ai].nb, prior = mine[na].s0;
    const bool ok = nb >= min_beams && (unsigned long long)S * min_den >= 255ull * nb * min_num;
    if (ok) {
        rec[0] = (unsigned long long)__double_as_longlong(px + (double)di);
        rec[1] = (unsigned long long)__double_as_longlong(py + (double)dj);
        rec[2] = (unsigned long long)__double_as_longlong(pang + (double)da * ang_step);
    } else {
        rec[0] = w0; rec[1] = w1; rec[2] = w2;
    }
    rec[3] = (unsigned long long)S | ((unsigned long long)nb << 32);
    rec[4] = (unsigned long long)(uint32_t)di | ((unsigned long long)(uint32_t)dj << 32);
    rec[5] = (unsigned long long)(uint32_t)da | ((unsigned long long)(ok ? LSD_GRID_MATCH_ACCEPTED : 0u) << 32);
    rec[6] = (unsigned long long)prior;
}

static_assert(sizeof(lsd_grid_match_rec) == 56 && offsetof(lsd_grid_match_rec, score) == 24 && offsetof(lsd_grid_match_rec, di) == 32 &&
              offsetof(lsd_grid_match_rec, da) == 40 && offsetof(lsd_grid_match_rec, flags) == 44 && offsetof(lsd_grid_match_rec, score_prior) == 48,
              "k_grid_match_pick writes the record as seven 64-bit words");

void launch_grid_likelihood(const uint32_t* pass, const uint32_t* hit, int cols, int rows, uint32_t min_pass, uint32_t occ_num, uint32_t occ_den,
                            const lsd_grid_smear& smear, uint8_t* corr, hipStream_t s) {
    const dim3 grid((cols + kLikeTileW - 1) / kLikeTileW, (rows + kLikeTileH - 1) / kLikeTileH);
    hipLaunchKernelGGL(k_grid_likelihood, grid, dim3(256), 0, s, pass, hit, cols, rows, min_pass, occ_num, occ_den, smear, corr);
}

void launch_grid_match_pick(int n_scans, const void* poses, size_t pose_pitch, const lsd_grid_search& se, const void* slots, lsd_grid_match_rec* out,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_grid_match_pick, dim3(n_scans), dim3(64), 0, s, static_cast<const uint8_t*>(poses), pose_pitch, se.wx, se.wy, se.na,
                       se.ang_step, se.min_beams, se.min_num, se.min_den, static_cast<const GmSlot*>(slots),
                       reinterpret_cast<unsigned long long*>(out));
}

size_t grid_match_slot_bytes(int n_scans, int na) { return (size_t)n_scans * (2 * na + 1) * sizeof(GmSlot); }

void launch_grid_match(const GridScans& g, const uint8_t* corr, const lsd_grid_search& se, void* slots, lsd_grid_match_rec* out, hipStream_t s) {
    hipLaunchKernelGGL(k_grid_match, dim3(g.n_scans, 2 * se.na + 1), dim3(kGmLanes), 0, s, reinterpret_cast<const double2*>(g.scans), g.lens,
                       g.stride, static_cast<const uint8_t*>(g.poses), g.pose_pitch, g.cols, g.rows, g.resol, g.range_max, corr, se.wx, se.wy, se.na,
                       se.ang_step, static_cast<GmSlot*>(slots));
    launch_grid_match_pick(g.n_scans, g.poses, g.pose_pitch, se, slots, out, s);
}

}  // namespace lsdhip
