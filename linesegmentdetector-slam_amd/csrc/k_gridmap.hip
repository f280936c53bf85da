// k_gridmap.hip -- mapping with known poses (gfx950): localised scans are integrated into two counter planes, pass[] and hit[] (Karto's
// counting model), and a pair of planes is published as the int8 OccupancyGrid the map update reads.  No reference counterpart: the
// reference takes its maps from an outside SLAM.  The rule is exact and has no iteration order, so a numpy restatement
// (tests/grid_cases.py) gives the same bytes.
//
// k_grid_integrate: one workgroup of 256 lanes per scan.  The pose (the first three doubles of a record at a byte pitch: lsd_position,
// lsd_fa_state, lsd_fa_carry) decides for the whole workgroup whether the scan is skipped.  The beams are taken 256 at a time:
//   A. one lane per beam: the skip tests, rr = min(range, range_max), th = angle + deg2rad_ref(ang), sincos_g(th) ONCE per beam, the end
//      cell (x1, y1) = cvt_x86(round(pose + rr * (c, s) / mapResol)), n = max(|dx|, |dy|); the beam's hit, one atomic at its end cell;
//   B. an inclusive scan of n over the workgroup (shuffles inside a wavefront, LDS across the four);
//   C. the sum of n many (beam, step k = 1..n) items dealt out to the lanes in order, item j to lane j % 256: a lane finds its beam by
//      bisecting the prefix sums in LDS (8 reads) and evaluates the ray's closed form,
//          major = start + k * sgn,   minor = start + sgn_minor * ((2 k m + n) / (2 n)),
//      so rays of 3 and of 300 cells cost their lengths, not the longest's, and neighbouring lanes add to neighbouring cells.
// Step k = 0 is the start cell, the same for every beam of the scan: its passes are counted per lane, summed over the workgroup and added
// once.  2 k m + n stays below 2^32: the entry refuses range_max / mapResol >= 32767, hence n <= 32768.  Cells outside the grid are
// skipped, nothing else is clipped.  Counters are uint32 and wrap at 2^32.
// k_grid_publish: one lane per cell, integer comparisons only.
#include "lsd_internal.h"
#include "match_dev.h"

namespace lsdhip {

constexpr int kGridLanes = 256;

__global__ __launch_bounds__(kGridLanes) void k_grid_integrate(const double2* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                               const uint8_t* __restrict__ poses, size_t pose_pitch, int cols, int rows,
                                                               double resol, double range_max, uint32_t* __restrict__ pass,
                                                               uint32_t* __restrict__ hit) {
    __shared__ int s_x1[kGridLanes], s_y1[kGridLanes];
    __shared__ uint32_t s_pre[kGridLanes + 1];             // s_pre[b] = steps of the chunk's beams below b
    __shared__ uint32_t s_wave[kGridLanes / 64];
    const int scan = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* pose = reinterpret_cast<const double*>(poses + (size_t)scan * pose_pitch);
    const double px = pose[0], py = pose[1], pang = pose[2];
    // the scan skipped whole (the same decision in every lane): no pose, the reference's "no pose" test (myFA.cpp:99), or a pose far outside
    if (!(isfinite(px) && isfinite(py) && isfinite(pang)) || fabs(px + 1) < 1e-4 || fabs(px) > 1048576.0 || fabs(py) > 1048576.0) return;
    const int len = min(max(lens[scan], 0), stride);
    const int x0 = cvt_x86(round(px)), y0 = cvt_x86(round(py));
    const double rot = deg2rad_ref(pang);
    const double2* row = scans + (size_t)scan * stride;
    uint32_t starts = 0;                                   // beams of this lane that pass through the start cell
    for (int base = 0; base < len; base += kGridLanes) {
        const int i = base + tid;
        uint32_t n = 0;
        int x1 = x0, y1 = y0;
        if (i < len) {
            const double2 b = row[i];
            const double th = b.y + rot;
            if (b.x > 0 && b.x != (double)INFINITY && isfinite(b.y) && isfinite(th)) {      // (NaN > 0 is false)
                const double rr = b.x < range_max ? b.x : range_max;
                double s, c;
                sincos_g(th, s, c);
                x1 = cvt_x86(round(px + rr * c / resol));
                y1 = cvt_x86(round(py + rr * s / resol));
                const uint32_t adx = (uint32_t)abs(x1 - x0), ady = (uint32_t)abs(y1 - y0);
                n = adx > ady ? adx : ady;
                starts++;
                if (b.x <= range_max && x1 >= 0 && x1 < cols && y1 >= 0 && y1 < rows) atomicAdd(&hit[(size_t)y1 * cols + x1], 1u);
            }
        }
        s_x1[tid] = x1;
        s_y1[tid] = y1;
        uint32_t inc = n;                                  // inclusive scan: the wavefront, then the four totals
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t below = 0;
        for (int w = 0; w < wave; w++) below += s_wave[w];
        s_pre[tid + 1] = below + inc;
        if (tid == 0) s_pre[0] = 0;
        __syncthreads();
        const uint32_t total = s_pre[kGridLanes];
        for (uint32_t j = tid; j < total; j += kGridLanes) {
            int lo = 0, hi = kGridLanes;                   // s_pre[lo] <= j < s_pre[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid] <= j) lo = mid; else hi = mid;
            }
            const uint32_t k = j - s_pre[lo] + 1;          // 1 .. n of beam lo
            const int dx = s_x1[lo] - x0, dy = s_y1[lo] - y0;
            const uint32_t adx = (uint32_t)abs(dx), ady = (uint32_t)abs(dy);
            const bool xmajor = adx >= ady;
            const uint32_t nn = xmajor ? adx : ady, m = xmajor ? ady : adx;
            const int minor = (int)((2u * k * m + nn) / (2u * nn));
            const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
            const int cx = xmajor ? x0 + sx * (int)k : x0 + sx * minor;
            const int cy = xmajor ? y0 + sy * minor : y0 + sy * (int)k;
            if (cx >= 0 && cx < cols && cy >= 0 && cy < rows) atomicAdd(&pass[(size_t)cy * cols + cx], 1u);
        }
        __syncthreads();                                   // the next chunk rewrites the LDS arrays
    }
    // the start cell: one add per scan
    for (int d = 32; d >= 1; d >>= 1) starts += __shfl_down(starts, d, 64);
    if (lane == 0) s_wave[wave] = starts;
    __syncthreads();
    if (tid == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kGridLanes / 64; w++) sum += s_wave[w];
        if (sum && x0 >= 0 && x0 < cols && y0 >= 0 && y0 < rows) atomicAdd(&pass[(size_t)y0 * cols + x0], sum);
    }
}

__global__ __launch_bounds__(256) void k_grid_publish(const uint32_t* __restrict__ pass, const uint32_t* __restrict__ hit, size_t n_cells,
                                                      uint32_t min_pass, uint32_t occ_num, uint32_t occ_den, int8_t* __restrict__ grid) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cells) return;
    const uint32_t p = pass[i], h = hit[i];
    grid[i] = p < min_pass ? -1 : ((unsigned long long)h * occ_den >= (unsigned long long)p * occ_num ? 100 : 0);
}

void launch_grid_integrate(const GridScans& g, uint32_t* pass, uint32_t* hit, hipStream_t s) {
    hipLaunchKernelGGL(k_grid_integrate, dim3(g.n_scans), dim3(kGridLanes), 0, s, reinterpret_cast<const double2*>(g.scans), g.lens, g.stride,
                       static_cast<const uint8_t*>(g.poses), g.pose_pitch, g.cols, g.rows, g.resol, g.range_max, pass, hit);
}

void launch_grid_publish(const uint32_t* pass, const uint32_t* hit, size_t n_cells, uint32_t min_pass, uint32_t occ_num, uint32_t occ_den,
                         int8_t* grid, hipStream_t s) {
    hipLaunchKernelGGL(k_grid_publish, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, s, pass, hit, n_cells, min_pass, occ_num, occ_den,
                       grid);
}

}  // namespace lsdhip
