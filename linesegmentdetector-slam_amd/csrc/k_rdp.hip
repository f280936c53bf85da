// k_rdp.hip -- myrdp::FeatureScan for a BATCH of lidar scans (gfx950): one wavefront per scan.
//
// Replaces LSD/myRDP.cpp:9-185 (FeatureScan) with its callees RegionSegmentation (:274-345), SplitMerge (:187-217),
// SplitMergeAssistant (:219-272) and getThresholdDeltaDist (:347-368), SURVEY 8f #4.  The reference handles one scan of at most
// 360 readings per frame on the host (LSD/main_on_windows.cpp:127); this is the batched form: N scans of len[i] readings each,
// results at fixed strides.  The phases of a scan and the IEEE corner cases kept are rdp_dev.h's, shared with k_rdp_long.hip, which
// takes the strides above this kernel's 1024.  What is this kernel's own:
//   - the work arrays are static LDS for 1024 readings;
//   - the clusters: a serial walk over the gaps, as in the reference, by one lane (a few hundred steps);
//   - the chords of every cluster in order: a second walk by that lane, into pairs of readings.
// launch_rdp, the one launcher of FeatureScan, is at the end of this file; a long stride it hands to k_rdp_long.hip's own launch.
#include "rdp_dev.h"
#include "k_rdp_lds.h"

namespace lsdhip {

// One scan (blockIdx.x) with the map's resolution and origin given: the body of both kernels below.
__device__ __forceinline__ void rdp_scan(const double* __restrict__ scans /* n x stride x {range, angle} */, const int* __restrict__ lens,
                                         int stride, double mapResol, double mapOriX, double mapOriY, int region_point_limit,
                                         double thre_line, double line_dist_thre_m, const RdpOut& o) {
    __shared__ double px[kRdpShortMaxLen], py[kRdpShortMaxLen];
    __shared__ unsigned char brk[kRdpShortMaxLen], split[kRdpShortMaxLen];
    __shared__ short cs[kRdpShortMaxLen], ce[kRdpShortMaxLen];
    __shared__ short stk[2 * kRdpShortMaxLen];                 // spans still to look at (RDP), later: the chords (a, b) in order
    __shared__ int s_cells, s_nch;
    const RdpLds<short, false> w{px, py, cs, ce, stk, brk, split, 2 * kRdpShortMaxLen};
    const size_t scan = blockIdx.x;
    const int lane = threadIdx.x;
    const int len_lp = min(lens[scan], min(stride, kRdpShortMaxLen));
    const double* sc = scans + scan * (size_t)stride * 2;
    if (rdp_empty_scan(len_lp, scan, o)) return;
    rdp_metric_gaps(sc, len_lp, w);
    if (lane == 0) {                                                               // RegionSegmentation's walk :297-330
        int cellNumber = 0, startNum = 0;
        for (int i = 0; i < len_lp; i++) {
            if (brk[i]) {
                cs[cellNumber] = (short)startNum; ce[cellNumber] = (short)i;
                if (abs(i - startNum) >= region_point_limit) cellNumber++;
                startNum = i + 1;
            }
            if (!brk[i] && i == len_lp - 1) cs[0] = (short)startNum;      // the last cluster joins the first
        }
        s_cells = cellNumber;
    }
    __syncthreads();
    const int cells = s_cells;
    rdp_split_merge(sc, len_lp, cells, thre_line, w);
    const RdpFrame f = rdp_pixel_frame(len_lp, mapResol, mapOriX, mapOriY, scan, o, w);
    // the chords of every cluster, in order (:45-71): its first reading, its split points, its last reading
    if (lane == 0) {
        int nch = 0;
        for (int cidx = 0; cidx < cells; cidx++) {
            const int sp = cs[cidx], ep = ce[cidx];
            const int len_axis = ep > sp ? ep - sp + 1 : len_lp + ep - sp + 1;
            int prev = sp;
            for (int j = 0; j < len_axis; j++) {
                int v = sp + j;
                if (v >= len_lp) v -= len_lp;
                if (split[v] && nch < kRdpShortMaxLen - 1) { stk[2 * nch] = (short)prev; stk[2 * nch + 1] = (short)v; nch++; prev = v; }
            }
            if (nch < kRdpShortMaxLen) { stk[2 * nch] = (short)prev; stk[2 * nch + 1] = (short)ep; nch++; }
        }
        s_nch = nch;
    }
    __syncthreads();
    rdp_chords(0, s_nch, [&](int ci, int& a, int& b) { a = stk[2 * ci]; b = stk[2 * ci + 1]; return true; }, f, line_dist_thre_m / mapResol,
               scan, o, w);
}

__global__ __launch_bounds__(64) void k_rdp(const double* __restrict__ scans, const int* __restrict__ lens,
                                            int stride, int oriMapCol, int oriMapRow, double mapResol, double mapOriX, double mapOriY,
                                            int region_point_limit, double thre_line, double line_dist_thre_m,
                                            lsd_line* __restrict__ lines_out, int* __restrict__ n_lines, double* __restrict__ pts_out, int pts_cap,
                                            int* __restrict__ n_pts, double* __restrict__ lidar_pos, int* __restrict__ im_size) {
    (void)oriMapCol; (void)oriMapRow;                          // (carried by structMapParam, unused by FeatureScan)
    rdp_scan(scans, lens, stride, mapResol, mapOriX, mapOriY, region_point_limit, thre_line, line_dist_thre_m,
             RdpOut{lines_out, n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size});
}

// The fleet's FeatureScan: the three values come from the record of the scan's map (rdp_map_of_scan).
__global__ __launch_bounds__(64) void k_rdp_maps(const double* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                 const lsd_map_ref* __restrict__ maps, int n_maps, const int32_t* __restrict__ map_of,
                                                 int scans_per_seq, int region_point_limit, double thre_line, double line_dist_thre_m,
                                                 lsd_line* __restrict__ lines_out, int* __restrict__ n_lines, double* __restrict__ pts_out,
                                                 int pts_cap, int* __restrict__ n_pts, double* __restrict__ lidar_pos,
                                                 int* __restrict__ im_size) {
    const RdpOut o{lines_out, n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size};
    const lsd_map_ref* __restrict__ m = rdp_map_of_scan(maps, n_maps, map_of, scans_per_seq, o);
    if (!m) return;
    rdp_scan(scans, lens, stride, m->mapResol, m->mapOriX, m->mapOriY, region_point_limit, thre_line, line_dist_thre_m, o);
}

void launch_rdp(const RdpScans& a, const RdpOut& o, hipStream_t s) {
    if (a.stride > kRdpShortMaxLen) {                  // a long scan (lsd_set_scan_capacity): the kernels of k_rdp_long.hip
        rdp_long_launch(a, o, s);
        return;
    }
    if (a.maps)
        hipLaunchKernelGGL(k_rdp_maps, dim3(a.n), dim3(64), 0, s, a.scans, a.lens, a.stride, a.maps, a.n_maps, a.map_of, a.scans_per_seq,
                           a.region_point_limit, a.thre_line, a.line_dist_thre_m, o.lines, o.n_lines, o.pts, o.pts_cap, o.n_pts, o.lidar_pos,
                           o.im_size);
    else
        hipLaunchKernelGGL(k_rdp, dim3(a.n), dim3(64), 0, s, a.scans, a.lens, a.stride, 0, 0, a.mapResol, a.mapOriX, a.mapOriY,
                           a.region_point_limit, a.thre_line, a.line_dist_thre_m, o.lines, o.n_lines, o.pts, o.pts_cap, o.n_pts, o.lidar_pos,
                           o.im_size);
}

}  // namespace lsdhip
