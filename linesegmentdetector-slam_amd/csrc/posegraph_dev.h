// posegraph_dev.h -- what the pose graph's kernels share as ONE text (k_pgbuild.hip: append, near, closure; k_posegraph.hip: the
// relaxation): the wrap of an angle in degrees, a pose in the frame of another, a pose composed with a motion, and the 3 x 3 inverse in the
// cofactor form of lsd_enqueue_fa_carry_correct_device's step 5.  include/lsd_hip.h, "pose graph", is the rule; fp64 without FMA.
#pragma once
#include "lsd_internal.h"
#include "match_dev.h"

namespace lsdhip {

struct PgPose { double x, y, a; };

__device__ __forceinline__ double pg_wrap(double v) { return v - 360.0 * floor((v + 180.0) / 360.0); }

// rel(a, q): q in the frame of a
__device__ __forceinline__ PgPose pg_rel(const PgPose& a, const PgPose& q) {
    double s, c;
    sincos_g(deg2rad_ref(a.a), s, c);
    const double dx = q.x - a.x, dy = q.y - a.y;
    return PgPose{c * dx + s * dy, c * dy - s * dx, pg_wrap(q.a - a.a)};
}

// comp(p, z): the pose a motion z, given in the frame of p, leads to
__device__ __forceinline__ PgPose pg_comp(const PgPose& p, const PgPose& z) {
    double s, c;
    sincos_g(deg2rad_ref(p.a), s, c);
    return PgPose{p.x + (c * z.x - s * z.y), p.y + (s * z.x + c * z.y), pg_wrap(p.a + z.a)};
}

// S (row major) -> inv(j, i) = cof(i, j) * invdet; false, with det set, where !(det > 0) or 1 / det is not finite
__device__ __forceinline__ bool pg_inv3(const double* S, double* inv, double& det) {
    auto cof = [&](int a, int b) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        return S[a1 * 3 + b1] * S[a2 * 3 + b2] - S[a1 * 3 + b2] * S[a2 * 3 + b1];
    };
    det = (cof(0, 0) * S[0] + cof(1, 0) * S[3]) + cof(2, 0) * S[6];
    const double invdet = 1 / det;
    if (!(det > 0) || !isfinite(invdet)) return false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) inv[j * 3 + i] = cof(i, j) * invdet;
    return true;
}

// the integration's test for a scan skipped whole (k_gridmap.hip): not finite, the "no pose" sentinel, or far outside
__device__ __forceinline__ bool pg_pose_skipped(const PgPose& p) {
    return !(isfinite(p.x) && isfinite(p.y) && isfinite(p.a)) || fabs(p.x + 1) < 1e-4 || fabs(p.x) > 1048576.0 || fabs(p.y) > 1048576.0;
}

}  // namespace lsdhip
