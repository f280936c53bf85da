// posegraph_dev.h -- what the pose graph's kernels share as ONE text (k_pgbuild.hip: append, near, closure; k_posegraph.hip: the
// relaxation; k_pgplace.hip, k_pgloops.hip: place recognition): the wrap of an angle in degrees, a pose in the frame of another, a pose
// composed with a motion, the 3 x 3 inverse in the cofactor form of lsd_enqueue_fa_carry_correct_device's step 5, the counts of a head
// clamped to the arrays (pg_n_nodes, pg_n_edges) and what near, recognize and loop_select leave for a closure chain (pg_hand_over).
// include/lsd_hip.h, "pose graph", is the rule; fp64 without FMA.
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

// a head's counts as every kernel reads them: never below 0, never beyond the arrays
__device__ __forceinline__ int pg_n_nodes(const lsd_pg_head* head, int nodes_cap) { return min(max(head->n_nodes, 0), nodes_cap); }
__device__ __forceinline__ int pg_n_edges(const lsd_pg_head* head, int edges_cap) { return min(max(head->n_edges, 0), edges_cap); }

// where place recognition puts a query whose scan it found at node `anchor`, `shift` sectors of 5.625 degrees on: the search's first pose
__device__ __forceinline__ PgPose pg_turned(const lsd_pg_node* nodes, int anchor, int shift) {
    return PgPose{nodes[anchor].x, nodes[anchor].y, pg_wrap(nodes[anchor].ang - (double)shift * 5.625)};
}

// What k_pg_near, k_pg_place_pick and k_pg_loop_select leave for a closure chain, by every lane of ONE workgroup of `lanes`: the near
// record, the pose the search starts from (qp: read where anchor >= 0 only), the query's length, ALL nodes_cap rows of the selection -- the
// anchor's window among the nodes a query may close on, the sentinel elsewhere -- and the query's row.
__device__ __forceinline__ void pg_hand_over(const lsd_pg_node* nodes, int nodes_cap, int n_nodes, const lsd_polar* store, const int* store_lens,
                                             int store_stride, int gap, int window, int j, int anchor, int n_cand, double d2, const PgPose& qp,
                                             const PgHandOver& out, int tid, int lanes) {
    const bool has_q = j >= 0 && j < n_nodes;
    if (tid == 0) {
        out.rec->anchor = anchor; out.rec->query = j; out.rec->n_cand = n_cand; out.rec->reserved = 0;
        out.rec->d2 = anchor >= 0 ? d2 : 0.0;
        out.q_pose->x = anchor >= 0 ? qp.x : -1.0;
        out.q_pose->y = anchor >= 0 ? qp.y : 0.0;
        out.q_pose->ang = anchor >= 0 ? qp.a : 0.0;
        *out.q_len = has_q ? store_lens[j] : 0;
    }
    for (int k = tid; k < nodes_cap; k += lanes) {
        const bool in = anchor >= 0 && abs(k - anchor) <= window && k <= j - gap;
        out.sel[k].x = in ? nodes[k].x : -1.0;
        out.sel[k].y = in ? nodes[k].y : 0.0;
        out.sel[k].ang = in ? nodes[k].ang : 0.0;
    }
    if (has_q) {
        const lsd_polar* src = store + (size_t)j * (size_t)store_stride;
        for (int i = tid; i < store_stride; i += lanes) out.q_scan[i] = src[i];
    }
}

}  // namespace lsdhip
