// k_gridray.hip -- ray casting on the grid (gfx950): what a scan should look like from a pose, beam by beam, against an int8
// OccupancyGrid (the layout k_grid_publish writes and the map update reads), the class of every beam (agrees with the map, ends in
// front of it, goes through it, ...), a summary per scan with an optional gate, and an optional screened copy of the scans.  No
// reference counterpart.  The rule is exact and has no iteration order, so a numpy restatement
// (tests/grid_ray_cases.py) gives the same bytes.
//
// k_grid_raycast: one workgroup of 256 lanes per (scan, chunk of 64 beams), so a scan of 4096 beams is spread over 64 workgroups.
//   A. one lane per beam (the first wavefront): the cast test, th = angle + deg2rad_ref(ang), sincos_g(th) ONCE per beam, the range_max
//      end cell (x1, y1) = cvt_x86(round(pose + range_max * (c, s) / mapResol)), n = max(|dx|, |dy|), into LDS;
//   B. a group of kRayP = 16 adjacent lanes of one wavefront per beam (16 groups, 4 rounds for a full chunk): the group tests the cells
//      k = base + 16 u + sub, u = 0 .. 3, of the ray's closed form (k_gridmap.hip's), base += 64 -- neighbouring lanes read neighbouring
//      bytes of an x-major ray, and a lane's four loads are in flight together: the walk is a chain of dependent round trips to
//      memory, one per 64 cells --, finds the first occupied and the first unknown cell by ballot on its own 16 bits, and is done at
//      the first occupied cell: a ray costs its length to the wall (rounded up to 64 cells), not range_max's.  The loop is kept
//      wavefront-uniform (it runs while any of the wavefront's four groups still walks), so every ballot is executed by all 64 lanes;
//   C. one lane per beam again: the two distances, the class, the 32-byte record and the screened reading.
// A cell is read as k_occ.hip reads it: byte 255 unknown, 0 free, anything else occupied; outside the grid: unknown, and not loaded.
// 2 k m + n stays below 2^32: the entry refuses range_max / mapResol >= 32767, hence n <= 32768.
// k_grid_ray_sum: one wavefront per scan counts the class words and writes the 64-byte record and the gate.  No atomics, nothing to
// zero, no workspace.
#include "gridmatch_dev.h"

namespace lsdhip {

constexpr int kRayLanes = 256, kRayChunk = 64, kRayP = 16, kRayGroups = kRayLanes / kRayP, kRayU = 4;
static_assert(64 % kRayP == 0, "a group is adjacent lanes of one wavefront");

// the cell k of the ray from (x0, y0) over (dx, dy): k_grid_integrate's closed form
__device__ __forceinline__ int2 ray_cell(int x0, int y0, int dx, int dy, uint32_t k) {
    const uint32_t adx = (uint32_t)abs(dx), ady = (uint32_t)abs(dy);
    const bool xmajor = adx >= ady;
    const uint32_t nn = xmajor ? adx : ady, m = xmajor ? ady : adx;
    const int minor = nn ? (int)((2u * k * m + nn) / (2u * nn)) : 0;
    const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    return xmajor ? make_int2(x0 + sx * (int)k, y0 + sy * minor) : make_int2(x0 + sx * minor, y0 + sy * (int)k);
}

__device__ __forceinline__ double ray_dist(int2 cell, double px, double py, double resol) {
    const double ddx = (double)cell.x - px, ddy = (double)cell.y - py;
    return sqrt(ddx * ddx + ddy * ddy) * resol;
}

// (scans and scans_out may be the same array: each reading is read and written by the same lane, so neither is __restrict__)
__global__ __launch_bounds__(kRayLanes) void k_grid_raycast(const double2* scans, const int* __restrict__ lens, int stride,
                                                            const uint8_t* __restrict__ poses, size_t pose_pitch, int cols, int rows,
                                                            double resol, double range_max, const uint8_t* __restrict__ grid, double tol,
                                                            uint32_t drop_mask, lsd_grid_ray* __restrict__ out, double2* scans_out) {
    __shared__ int s_x1[kRayChunk], s_y1[kRayChunk], s_n[kRayChunk];           // s_n: the ray's steps, -1 for a beam that is not cast
    __shared__ int s_hit[kRayChunk], s_unk[kRayChunk];
    const int scan = blockIdx.x, tid = threadIdx.x;
    const int len = min(max(lens[scan], 0), stride);
    const int first = blockIdx.y * kRayChunk;
    if (first >= len) return;
    const int nb = min(kRayChunk, len - first);                                // the chunk's beams
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    const bool skipped = gm_scan_skipped(px, py, pang);                        // (the same decision in every lane)
    const int x0 = skipped ? 0 : cvt_x86(round(px)), y0 = skipped ? 0 : cvt_x86(round(py));
    const size_t at = (size_t)scan * stride + first + tid;
    // A. the end cell
    double2 b = make_double2(0.0, 0.0);
    bool cast = false;
    if (tid < nb) {
        b = scans[at];
        int x1 = x0, y1 = y0, n = -1;
        if (!skipped) {
            const double th = b.y + deg2rad_ref(pang);
            if (isfinite(b.y) && isfinite(th)) {
                double s, c;
                sincos_g(th, s, c);
                x1 = cvt_x86(round(px + range_max * c / resol));
                y1 = cvt_x86(round(py + range_max * s / resol));
                n = max(abs(x1 - x0), abs(y1 - y0));
                cast = true;
            }
        }
        s_x1[tid] = x1;
        s_y1[tid] = y1;
        s_n[tid] = n;
    }
    __syncthreads();
    // B. the walk: group g takes the beams g, g + 16, ...
    if (!skipped) {
        const int sub = tid & (kRayP - 1), grp = tid / kRayP, shift = tid & 63 & ~(kRayP - 1);
        for (int beam = grp; beam - grp < nb; beam += kRayGroups) {           // (workgroup-uniform trip count)
            const int n = beam < nb ? s_n[beam] : -1;
            const int dx = n >= 0 ? s_x1[beam] - x0 : 0, dy = n >= 0 ? s_y1[beam] - y0 : 0;
            int k_hit = -1, k_unk = -1, base = 0;
            bool walking = n >= 0;
            while (__any(walking)) {
                uint8_t v[kRayU];                                              // the loads of kRayU cells are issued before any is looked at
#pragma unroll
                for (int u = 0; u < kRayU; u++) {
                    const int k = base + u * kRayP + sub;
                    v[u] = 0;                                                  // (a lane past the ray's end reports nothing)
                    if (walking && k <= n) {
                        const int2 cell = ray_cell(x0, y0, dx, dy, (uint32_t)k);
                        v[u] = 255;                                            // outside the grid: unknown
                        if (cell.x >= 0 && cell.x < cols && cell.y >= 0 && cell.y < rows) v[u] = grid[(size_t)cell.y * cols + cell.x];
                    }
                }
                bool found = false;
#pragma unroll
                for (int u = 0; u < kRayU; u++) {
                    const uint32_t mo = (uint32_t)(__ballot(v[u] != 0 && v[u] != 255) >> shift) & ((1u << kRayP) - 1);
                    uint32_t mu = (uint32_t)(__ballot(v[u] == 255) >> shift) & ((1u << kRayP) - 1);
                    if (walking && !found) {
                        if (mo) {
                            const int f = __builtin_ctz(mo);
                            k_hit = base + u * kRayP + f;
                            mu &= (1u << f) - 1;                               // an unknown cell behind the first occupied one is not reported
                            found = true;
                        }
                        if (k_unk < 0 && mu) k_unk = base + u * kRayP + __builtin_ctz(mu);
                    }
                }
                if (walking) {
                    base += kRayU * kRayP;
                    walking = !found && base <= n;
                }
            }
            if (sub == 0 && beam < nb) {
                s_hit[beam] = k_hit;
                s_unk[beam] = k_unk;
            }
        }
        __syncthreads();
    }
    // C. the record and the screened reading
    if (tid >= nb) return;
    lsd_grid_ray r;
    r.r_exp = 0.0; r.r_unk = 0.0; r.cx = 0; r.cy = 0; r.k_hit = 0; r.cls = LSD_GRID_RAY_NOT_CAST;
    if (cast) {
        const int k_hit = s_hit[tid], k_unk = s_unk[tid];
        const int dx = s_x1[tid] - x0, dy = s_y1[tid] - y0;
        const double inf = (double)INFINITY;
        int2 end = make_int2(s_x1[tid], s_y1[tid]);
        r.r_exp = inf;
        if (k_hit >= 0) {
            end = ray_cell(x0, y0, dx, dy, (uint32_t)k_hit);
            r.r_exp = ray_dist(end, px, py, resol);
        }
        r.r_unk = k_unk >= 0 ? ray_dist(ray_cell(x0, y0, dx, dy, (uint32_t)k_unk), px, py, resol) : inf;
        r.cx = end.x; r.cy = end.y; r.k_hit = k_hit;
        const double m = b.x;
        if (!(m > 0)) r.cls = LSD_GRID_RAY_NO_MEASUREMENT;                     // (NaN > 0 is false)
        else if (m == inf || m > range_max) r.cls = k_hit >= 0 ? LSD_GRID_RAY_LONG : (k_unk >= 0 ? LSD_GRID_RAY_UNEXPLORED : LSD_GRID_RAY_AGREE_FREE);
        else {
            const double d = m - r.r_exp;
            if (fabs(d) <= tol) r.cls = LSD_GRID_RAY_AGREE;
            else if (d > tol) r.cls = LSD_GRID_RAY_LONG;
            else r.cls = r.r_unk <= m ? LSD_GRID_RAY_UNEXPLORED : LSD_GRID_RAY_SHORT;
        }
    }
    out[at] = r;
    if (scans_out) {
        if ((drop_mask >> r.cls) & 1u) b.x = __longlong_as_double(0x7FF8000000000000ll);
        scans_out[at] = b;                                                     // (the bits as they were read: in place is allowed)
    }
}

__global__ __launch_bounds__(64) void k_grid_ray_sum(const int* __restrict__ lens, int stride, const uint8_t* __restrict__ poses, size_t pose_pitch,
                                                     const lsd_grid_ray* __restrict__ rays, uint32_t min_beams, uint32_t ok_num, uint32_t ok_den,
                                                     int gate, lsd_grid_ray_sum* __restrict__ sum) {
    const int scan = blockIdx.x, lane = threadIdx.x;
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    const bool skipped = gm_scan_skipped(px, py, pang);
    const int len = min(max(lens[scan], 0), stride);
    uint32_t n[7] = {0, 0, 0, 0, 0, 0, 0};
    if (!skipped) {
        const lsd_grid_ray* row = rays + (size_t)scan * stride;
        for (int i = lane; i < len; i += 64) {
            const uint32_t cls = row[i].cls;
#pragma unroll
            for (int c = 0; c < 7; c++) n[c] += cls == (uint32_t)c;
        }
#pragma unroll
        for (int c = 0; c < 7; c++)
            for (int d = 32; d >= 1; d >>= 1) n[c] += (uint32_t)__shfl_xor((int)n[c], d, 64);
    }
    if (lane != 0) return;
    lsd_grid_ray_sum r;
    const uint32_t judged = n[2] + n[3] + n[4] + n[5];
    const bool consistent = !skipped && judged >= min_beams &&
                            (unsigned long long)(n[2] + n[3]) * ok_den >= (unsigned long long)judged * ok_num;
    r.x = gate && !skipped && !consistent ? -1.0 : px;                         // the "no pose" sentinel: every grid entry skips the scan
    r.y = py; r.ang = pang;
#pragma unroll
    for (int c = 0; c < 7; c++) r.n[c] = n[c];
    r.judged = judged;
    r.flags = (consistent ? LSD_GRID_RAY_CONSISTENT : 0u) | (skipped ? LSD_GRID_RAY_SKIPPED : 0u);
    r.pad = 0;
    sum[scan] = r;
}

void launch_grid_raycast(const GridScans& g, const int8_t* grid, const lsd_grid_ray_par& par, lsd_grid_ray* out, lsd_grid_ray_sum* sum,
                         lsd_polar* scans_out, hipStream_t s) {
    const unsigned chunks = (unsigned)((g.stride + kRayChunk - 1) / kRayChunk);
    hipLaunchKernelGGL(k_grid_raycast, dim3(g.n_scans, chunks), dim3(kRayLanes), 0, s, reinterpret_cast<const double2*>(g.scans), g.lens, g.stride,
                       static_cast<const uint8_t*>(g.poses), g.pose_pitch, g.cols, g.rows, g.resol, g.range_max,
                       reinterpret_cast<const uint8_t*>(grid), par.tol, par.drop_mask, out, reinterpret_cast<double2*>(scans_out));
    hipLaunchKernelGGL(k_grid_ray_sum, dim3(g.n_scans), dim3(64), 0, s, g.lens, g.stride, static_cast<const uint8_t*>(g.poses), g.pose_pitch, out,
                       par.min_beams, par.ok_num, par.ok_den, par.gate, sum);
}

}  // namespace lsdhip
