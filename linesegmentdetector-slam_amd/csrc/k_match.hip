// k_match.hip -- the scan-to-map matching batch of FeatureAssociation on the device (SURVEY 8f "next" #2), gfx950.
//
// Replaces the body of myfa::thread_ScanToMapMatch (LSD/myFA.cpp:197-270) and its callees NormalizedLineDirection
// (:272-305), rotateScanIm (:307-357) and CalcScore (:359-396), which the reference runs on a 30-thread pool: for every
// (map line, scan line) pair, the four start/end matchings each give a candidate pose; the scan's image points are
// rotated to it and scored against mapCache.
// One lane per candidate: the sums of CalcScore are accumulated in point order (as the reference does), the scan
// points are read by all lanes at the same address (broadcast), mapCache is gathered.  sin/cos/atan are the correctly
// rounded ones of crmath.h.  Bound: L2/HBM gather latency; ~30 flops per point.
#include "match_dev.h"

namespace lsdhip {

__global__ __launch_bounds__(64) void k_match(const double* __restrict__ map_cache, int cols, int rows,
                                              const lsd_line* __restrict__ map_lines, const lsd_line* __restrict__ scan_lines,
                                              const double* __restrict__ pts /* n x {x, y, ang} */, int n_points,
                                              double lidx, double lidy, double lastx, double lasty,
                                              const int* __restrict__ pairs, int n_cand, double zmax, double max_esti_dist,
                                              double* __restrict__ out /* n_cand x {x, y, ang, score} */) {
    const int cidx = blockIdx.x * 64 + threadIdx.x;
    match_candidate(cidx < n_cand, cidx, map_cache, cols, rows, map_lines, scan_lines, pts, n_points, lidx, lidy, lastx, lasty, pairs, zmax,
                    max_esti_dist, out);
}

void launch_match(const double* map_cache, int cols, int rows, const lsd_line* map_lines, const lsd_line* scan_lines,
                  const double* pts, int n_points, double lidx, double lidy, double lastx, double lasty, const int* pairs,
                  int n_pairs, double zmax, double max_esti_dist, double* out, hipStream_t s) {
    const int n_cand = 4 * n_pairs;
    hipLaunchKernelGGL(k_match, dim3((n_cand + 63) / 64), dim3(64), 0, s, map_cache, cols, rows, map_lines, scan_lines, pts,
                       n_points, lidx, lidy, lastx, lasty, pairs, n_cand, zmax, max_esti_dist, out);
}

}  // namespace lsdhip
