// k_ingest.hip -- the drivers' scan read loop for a BATCH of raw lidar scans (gfx950): one wavefront per scan.
//
// Replaces the loop that drops the readings with an infinite range and packs the rest to the front of lidarPointPolar[]
// (the file driver, LSD/main_on_windows.cpp:104-123; the ROS node's laserCallback, LSD/main_on_linux.cpp:53-66) and writes exactly
// what k_rdp reads: scans[n][stride] with the kept readings first in beam order and every slot from lens[i] to stride +0.0 / +0.0,
// and lens[n].  Two input layouts:
//   pairs      n_beams (range, angle) doubles per scan, the file driver's Lidar.txt.  A reading is kept iff `range != INFINITY` as the
//              reference evaluates it (:115): -inf and NaN are KEPT, only +inf is dropped.
//   LaserScan  n_beams float ranges per scan and (angle_min, angle_increment) floats per scan, sensor_msgs/LaserScan.  Kept iff
//              `ranges[i] != INFINITY` in float (:57); range = (double)ranges[i]; angle = (double)(angle_min + i * angle_increment),
//              the callback's expression on float fields (:60): the product and the sum are each rounded to SINGLE precision
//              (__fmul_rn / __fadd_rn: never contracted into an FMA).
// take (optional, one int per scan): where it is 0 the scan has lens = 0 and an all-zero row.
// Per scan the wavefront walks the beams in chunks of 64: the keep mask by ballot, a lane's slot = the running base + the kept lanes
// below it (mbcnt), one 16-byte store of the pair; then the same wavefront zero-fills the tail.  No LDS, no atomics; the output
// order is the beam order by construction.
// NOT reproduced: laserCallback stores a finite reading at lidarPointPolar[i], not [len_lp], and then hands the first len_lp entries to
// FeatureScan, so with any infinite range it reads stale entries of earlier messages.  The file driver packs; so does this kernel.
#include "lsd_internal.h"
#include "devmath.h"

namespace lsdhip {

template <bool kLaserScan>
__global__ __launch_bounds__(64) void k_ingest(const double2* __restrict__ raw /* n x n_beams x {range, angle} */,
                                               const float* __restrict__ ranges /* n x n_beams */,
                                               const float* __restrict__ min_inc /* n x {angle_min, angle_increment} */, int n_beams,
                                               const int* __restrict__ take, double2* __restrict__ scans, int* __restrict__ lens, int stride) {
    const int scan = blockIdx.x, lane = threadIdx.x;
    double2* out = scans + (size_t)scan * stride;
    int base = 0;                                                                  // kept so far: the same in every lane
    if (!take || take[scan] != 0) {
        float a_min = 0.f, a_inc = 0.f;
        if (kLaserScan) { a_min = min_inc[2 * scan]; a_inc = min_inc[2 * scan + 1]; }
        for (int c = 0; c < n_beams; c += 64) {
            const int i = c + lane;
            double2 v = make_double2(0.0, 0.0);
            bool keep = false;
            if (i < n_beams) {
                if (kLaserScan) {
                    const float r = ranges[(size_t)scan * n_beams + i];
                    keep = r != INFINITY;
                    v = make_double2((double)r, (double)__fadd_rn(a_min, __fmul_rn((float)i, a_inc)));
                } else {
                    v = raw[(size_t)scan * n_beams + i];
                    keep = v.x != (double)INFINITY;
                }
            }
            const unsigned long long m = __ballot(keep);
            const int below = lanes_below(m);
            if (keep) out[base + below] = v;                                      // base + below <= i < n_beams <= stride
            base += __builtin_popcountll(m);
        }
    }
    for (int i = base + lane; i < stride; i += 64) out[i] = make_double2(0.0, 0.0);
    if (lane == 0) lens[scan] = base;
}

void launch_ingest(const lsd_polar* raw, const float* ranges, const float* min_inc, int n, int n_beams, const int* take, lsd_polar* scans,
                   int* lens, int stride, hipStream_t s) {
    double2* out = reinterpret_cast<double2*>(scans);
    if (raw)
        hipLaunchKernelGGL(k_ingest<false>, dim3(n), dim3(64), 0, s, reinterpret_cast<const double2*>(raw), nullptr, nullptr, n_beams, take, out,
                           lens, stride);
    else
        hipLaunchKernelGGL(k_ingest<true>, dim3(n), dim3(64), 0, s, nullptr, ranges, min_inc, n_beams, take, out, lens, stride);
}

}  // namespace lsdhip
