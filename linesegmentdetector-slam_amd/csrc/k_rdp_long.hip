// k_rdp_long.hip -- myrdp::FeatureScan for scans of 1025 .. 4096 readings (gfx950): one wavefront per scan, dynamic LDS.
//
// The same function as k_rdp.hip (LSD/myRDP.cpp:9-185 with RegionSegmentation, SplitMerge, SplitMergeAssistant and
// getThresholdDeltaDist), the same outputs at the same strides, the same bits; launch_rdp sends a launch here when its stride is above
// k_rdp's 1024.  The phases of a scan are rdp_dev.h's, shared with k_rdp.hip.  What differs:
//   - the work arrays are dynamic LDS sized from the launch's stride (k_rdp_lds.h: 26 bytes per reading);
//   - no lane walks over all readings.  k_rdp's two walks by lane 0 -- RegionSegmentation's cluster walk and the listing of the chords
//     -- are ordered compactions here (ballot + the kept lanes below, over chunks of 64, the idiom of k_ingest):
//       clusters  the readings behind which the gap is over the threshold are listed in order (B); run j is [B[j-1] + 1, B[j]] (the first
//                 from 0); the reference writes a run at cs[cellNumber] and moves on only if abs(i - startNum) >= region_point_limit,
//                 so the clusters are the runs that pass that test, in order -- a second compaction over B; where the last reading
//                 has no gap behind it, cs[0] = B[last] + 1 (0 without a gap anywhere): the last run joins cluster 0, whichever
//                 run that is;
//       chords    the clusters are disjoint and ascending, except that a joined cluster 0 starts behind every other one and runs
//                 through the end of the scan: in the order (reading - cs[0]) mod len, clusters and the readings inside them both
//                 ascend.  Each reading lists itself once as its cluster's first reading, once as a split point, once as its
//                 cluster's last reading (P, a compaction in that order); the chords are the neighbours (P[t-1], P[t]) where P[t]
//                 does not begin a cluster.
// One wavefront, not four: the batch is the parallelism (one scan per workgroup, hundreds of scans per launch), the farthest-point
// search keeps its shuffle reduction with its first-maximum rule, and the barriers stay wave-local.
// Kept as they are: everything rdp_dev.h's head lists (vertical chords with NaN distances, cvt_x86, 0 doubling as "invalid" in the
// raster, len_lp < 1 writing the six zeros, the first maximum under the strict '>').  Line records stay at 360 per scan: a scan with
// more reports the full count and stores the first 360.
// Domain: region_point_limit >= 1, the reference's.  Below 1 a cluster of ONE reading can exist, whose span the reference takes for
// the whole scan plus one (its wrap-around formula at ep == sp); that is not restated here -- such a cluster gives one chord of
// length 0 -- and every index stays inside its array.
#include "rdp_dev.h"
#include "k_rdp_lds.h"

namespace lsdhip {

constexpr unsigned kFirstOfCluster = 0x8000u;       // flag on an entry of P (the readings' indices take 15 bits at most)

extern __shared__ double rdp_long_lds_base[];

// One scan (blockIdx.x) with the map's resolution and origin given: the body of both kernels below.
__device__ __forceinline__ void rdp_long_scan(const double* __restrict__ scans /* n x stride x {range, angle} */, const int* __restrict__ lens,
                                              int stride, double mapResol, double mapOriX, double mapOriY, int region_point_limit,
                                              double thre_line, double line_dist_thre_m, const RdpOut& o) {
    // the launch's dynamic LDS, rdp_long_lds(stride) bytes: every array holds `stride` elements (stk: 2 x stride)
    double* px = rdp_long_lds_base;
    double* py = px + stride;
    unsigned short* cs = reinterpret_cast<unsigned short*>(py + stride);
    unsigned short* ce = cs + stride;
    unsigned short* stk = ce + stride;                 // in turn: the breaks B, the spans still to look at (RDP), the chord points P
    unsigned char* brk = reinterpret_cast<unsigned char*>(stk + 2 * stride);       // a gap behind the reading; later: first / last of a cluster
    unsigned char* split = brk + stride;
    const int stk_cap = 2 * stride;
    const RdpLds<unsigned short, true> w{px, py, cs, ce, stk, brk, split, stk_cap};
    const size_t scan = blockIdx.x;
    const int lane = threadIdx.x;
    const int len_lp = min(lens[scan], stride);
    const double* sc = scans + scan * (size_t)stride * 2;
    if (rdp_empty_scan(len_lp, scan, o)) return;
    rdp_metric_gaps(sc, len_lp, w);
    // RegionSegmentation's walk :297-330 as two compactions.  B: the readings with a gap behind them, in order
    int nb = 0;
    for (int c0 = 0; c0 < len_lp; c0 += 64) {
        const int i = c0 + lane;
        const bool b = i < len_lp && brk[i];
        const unsigned long long m = __ballot(b);
        if (b) stk[nb + lanes_below(m)] = (unsigned short)i;                       // nb + below <= i < stride
        nb += __builtin_popcountll(m);
    }
    const bool joins = !brk[len_lp - 1];                                           // the last run joins cluster 0 (:361-365)
    __syncthreads();
    // the runs [B[j-1] + 1, B[j]] that are long enough, in order: the clusters
    int cells = 0;
    for (int c0 = 0; c0 < nb; c0 += 64) {
        const int j = c0 + lane;
        int startNum = 0, i = 0;
        bool keep = false;
        if (j < nb) {
            i = stk[j];
            startNum = j ? stk[j - 1] + 1 : 0;
            keep = abs(i - startNum) >= region_point_limit;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) { const int at = cells + lanes_below(m); cs[at] = (unsigned short)startNum; ce[at] = (unsigned short)i; }   // at <= j < stride
        cells += __builtin_popcountll(m);
    }
    const int lastStart = nb ? stk[nb - 1] + 1 : 0;                                // startNum when the walk ends
    __syncthreads();
    if (joins && cells > 0 && lane == 0) cs[0] = (unsigned short)lastStart;        // (lastStart <= len_lp - 1: the last reading is no break)
    __syncthreads();
    rdp_split_merge(sc, len_lp, cells, thre_line, w);
    for (int i = lane; i < len_lp; i += 64) brk[i] = 0;                            // from here: 1 = first reading of a cluster, 2 = last
    const RdpFrame f = rdp_pixel_frame(len_lp, mapResol, mapOriX, mapOriY, scan, o, w);
    for (int c = lane; c < cells; c += 64) brk[cs[c]] = 1;                         // (the clusters are disjoint: one writer per reading)
    __syncthreads();
    for (int c = lane; c < cells; c += 64) brk[ce[c]] |= 2;
    __syncthreads();
    // the chord points of every cluster, in order (:45-71): its first reading, its split points, its last reading -> P
    const int rot = joins && cells > 0 ? cs[0] : 0;
    int n_p = 0;
    for (int c0 = 0; c0 < len_lp; c0 += 64) {
        const int r = c0 + lane;
        int v = 0;
        bool first = false, mid = false, last = false;
        if (r < len_lp) {
            v = r + rot;
            if (v >= len_lp) v -= len_lp;
            first = brk[v] & 1; mid = split[v]; last = brk[v] & 2;
        }
        const unsigned long long mf = __ballot(first), mm = __ballot(mid), ml = __ballot(last);
        int at = n_p + lanes_below(mf) + lanes_below(mm) + lanes_below(ml);
        if (first) { if (at < stk_cap) stk[at] = (unsigned short)(v | kFirstOfCluster); at++; }
        if (mid) { if (at < stk_cap) stk[at] = (unsigned short)v; at++; }
        if (last) { if (at < stk_cap) stk[at] = (unsigned short)v; }
        n_p += __builtin_popcountll(mf) + __builtin_popcountll(mm) + __builtin_popcountll(ml);
    }
    n_p = min(n_p, stk_cap);                                                       // (in the domain n_p <= len_lp: a reading is one of the three)
    __syncthreads();
    rdp_chords(1, n_p, [&](int ci, int& a, int& b) {                               // the chord (P[ci - 1], P[ci])
                   if (stk[ci] & kFirstOfCluster) return false;
                   a = stk[ci - 1] & (kFirstOfCluster - 1u); b = stk[ci];
                   return true;
               }, f, line_dist_thre_m / mapResol, scan, o, w);
}

__global__ __launch_bounds__(64) void k_rdp_long(const double* __restrict__ scans, const int* __restrict__ lens, int stride, double mapResol,
                                                 double mapOriX, double mapOriY, int region_point_limit, double thre_line,
                                                 double line_dist_thre_m, lsd_line* __restrict__ lines_out, int* __restrict__ n_lines,
                                                 double* __restrict__ pts_out, int pts_cap, int* __restrict__ n_pts,
                                                 double* __restrict__ lidar_pos, int* __restrict__ im_size) {
    rdp_long_scan(scans, lens, stride, mapResol, mapOriX, mapOriY, region_point_limit, thre_line, line_dist_thre_m,
                  RdpOut{lines_out, n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size});
}

// The fleet's form (k_rdp_maps)
__global__ __launch_bounds__(64) void k_rdp_maps_long(const double* __restrict__ scans, const int* __restrict__ lens, int stride,
                                                      const lsd_map_ref* __restrict__ maps, int n_maps, const int32_t* __restrict__ map_of,
                                                      int scans_per_seq, int region_point_limit, double thre_line, double line_dist_thre_m,
                                                      lsd_line* __restrict__ lines_out, int* __restrict__ n_lines,
                                                      double* __restrict__ pts_out, int pts_cap, int* __restrict__ n_pts,
                                                      double* __restrict__ lidar_pos, int* __restrict__ im_size) {
    const RdpOut o{lines_out, n_lines, pts_out, pts_cap, n_pts, lidar_pos, im_size};
    const lsd_map_ref* __restrict__ m = rdp_map_of_scan(maps, n_maps, map_of, scans_per_seq, o);
    if (!m) return;
    rdp_long_scan(scans, lens, stride, m->mapResol, m->mapOriX, m->mapOriY, region_point_limit, thre_line, line_dist_thre_m, o);
}

// Once per context, before its first long launch: LDS above 64 KiB needs the kernels' dynamic-LDS limit raised (lsd_set_scan_capacity
// has checked the size against the device's limit).  An error here leaves nothing queued.
hipError_t prepare_rdp_long(size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rdp_long), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_rdp_maps_long), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// launch_rdp's other half (rdp_dev.h): this file's two kernels with the stride's dynamic LDS
void rdp_long_launch(const RdpScans& a, const RdpOut& o, hipStream_t s) {
    const size_t lds = rdp_long_lds(a.stride);
    if (a.maps)
        hipLaunchKernelGGL(k_rdp_maps_long, dim3(a.n), dim3(64), lds, s, a.scans, a.lens, a.stride, a.maps, a.n_maps, a.map_of, a.scans_per_seq,
                           a.region_point_limit, a.thre_line, a.line_dist_thre_m, o.lines, o.n_lines, o.pts, o.pts_cap, o.n_pts, o.lidar_pos,
                           o.im_size);
    else
        hipLaunchKernelGGL(k_rdp_long, dim3(a.n), dim3(64), lds, s, a.scans, a.lens, a.stride, a.mapResol, a.mapOriX, a.mapOriY,
                           a.region_point_limit, a.thre_line, a.line_dist_thre_m, o.lines, o.n_lines, o.pts, o.pts_cap, o.n_pts, o.lidar_pos,
                           o.im_size);
}

}  // namespace lsdhip
