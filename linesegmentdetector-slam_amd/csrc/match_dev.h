// match_dev.h -- the candidate of the scan-to-map matching (one lane per candidate), shared by k_match (k_match.hip) and the
// device FeatureAssociation (k_fa.hip).  The body of myfa::thread_ScanToMapMatch (LSD/myFA.cpp:197-270) for matching
// i = (cidx & 3) + 1 of pair cidx >> 2; see the head of k_match.hip.
#pragma once
#include "lsd_internal.h"
#include "devmath.h"

namespace lsdhip {

__device__ __forceinline__ double deg2rad_ref(double x) { return x / 180.0 * kPi; }     // baseFunc.cpp:6-12 (pi = 4*atan(1))

__device__ __forceinline__ double line_direction(double staX, double staY, double endX, double endY) {   // myFA.cpp:272-305
    double angle;
    if (staX == endX && staY != endY) angle = staY < endY ? 90 : -90;
    else if (staX != endX && staY == endY) angle = staX < endX ? 0 : 180;
    else angle = atan_g((endY - staY) / (endX - staX)) * 180.0 / kPi;                    // atand, baseFunc.cpp:14-16
    if (angle < 0 && staX > endX) return angle + 180;
    if (angle > 0 && staX > endX) return angle - 180;
    return angle;
}

// Every lane of the wavefront calls it (the point loop is skipped by a ballot); lanes with act == false write nothing.
__device__ __forceinline__ void match_candidate(bool act, int cidx, const double* __restrict__ map_cache, int cols, int rows,
                                                const lsd_line* __restrict__ map_lines, const lsd_line* __restrict__ scan_lines,
                                                const double* __restrict__ pts, int n_points, double lidx, double lidy, double lastx,
                                                double lasty, const int* __restrict__ pairs, double zmax, double max_esti_dist,
                                                double* __restrict__ out) {
    const int p = act ? cidx >> 2 : 0, i = (cidx & 3) + 1;                   // :205-249
    const lsd_line ml = map_lines[pairs[2 * p]], sl = scan_lines[pairs[2 * p + 1]];
    const bool mrev = i >= 3, srev = (i == 2 || i == 4);
    const double msx = mrev ? ml.x2 : ml.x1, msy = mrev ? ml.y2 : ml.y1, mex = mrev ? ml.x1 : ml.x2, mey = mrev ? ml.y1 : ml.y2;
    const double ssx = srev ? sl.x2 : sl.x1, ssy = srev ? sl.y2 : sl.y1, sex = srev ? sl.x1 : sl.x2, sey = srev ? sl.y1 : sl.y2;
    double angDiff = line_direction(msx, msy, mex, mey) - line_direction(ssx, ssy, sex, sey);   // :252-258, :310
    double sd, cd;
    sincos_g(deg2rad_ref(angDiff), sd, cd);                                   // sind / cosd
    const double rlx = (lidx - ssx) * cd - (lidy - ssy) * sd + msx;           // :323-324
    const double rly = (lidx - ssx) * sd + (lidy - ssy) * cd + msy;
    const double ddx = rlx - lastx, ddy = rly - lasty;
    const bool near_ = sqrt(ddx * ddx + ddy * ddy) < max_esti_dist || lastx == -1;   // :330
    double sumValidDist = 0, sumMaxDist = 0, numValidPoint = 0;               // CalcScore
    if (__ballot(act && near_)) {
        // kPtBatch points at a time: their gathers are issued together, then accumulated in point order (the sums are the
        // reference's, term by term); one gather after the other would leave each lane waiting on the memory latency per point
        constexpr int kPtBatch = 8;
        for (int c0 = 0; c0 < n_points; c0 += kPtBatch) {
            double v[kPtBatch];
            bool ok[kPtBatch];
#pragma unroll
            for (int u = 0; u < kPtBatch; u++) {
                const int c = c0 + u;
                ok[u] = false;
                v[u] = 0;
                if (c < n_points) {
                    const double px = pts[3 * c], py = pts[3 * c + 1];        // same address in every lane
                    const double ox = px - ssx, oy = py - ssy;                // :317-320
                    const double rx = ox * cd - oy * sd + msx;                // :333-336
                    const double ry = ox * sd + oy * cd + msy;
                    const int x = cvt_x86(round(rx)), y = cvt_x86(round(ry)); // :368-369
                    ok[u] = act && near_ && y >= 0 && y < rows && x >= 0 && x < cols;
                    if (ok[u]) v[u] = map_cache[(size_t)y * cols + x];
                }
            }
#pragma unroll
            for (int u = 0; u < kPtBatch; u++) {
                if (ok[u]) {
                    numValidPoint += 1;
                    if (v[u] >= zmax) sumMaxDist += 10;                      // :374-378
                    else sumValidDist += v[u];
                }
            }
        }
    }
    if (!act) return;
    double ang = 0, score = HUGE_VAL;
    if (near_) {
        while (angDiff <= -180) angDiff += 360;                               // :339-342
        while (angDiff > 180) angDiff -= 360;
        ang = angDiff;
        const double numAllPoint = n_points;
        if (n_points != 0 && !(numValidPoint < 0.7 * numAllPoint))            // :248-263 (no scan points: the score stays infinite), :388-392
            score = (sumValidDist + sumMaxDist) / (numValidPoint) + 10 * (numAllPoint - numValidPoint) / numAllPoint;
    }
    double* o = out + (size_t)cidx * 4;
    o[0] = rlx; o[1] = rly; o[2] = ang; o[3] = score;
}

}  // namespace lsdhip
