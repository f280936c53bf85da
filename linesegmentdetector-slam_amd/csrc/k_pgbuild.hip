// k_pgbuild.hip -- what builds a pose graph on the device (include/lsd_hip.h, "pose graph", is the rule; restated in
// tests/pose_graph_cases.py): keyframes and odometry edges from a tick's frames (k_pg_append), the loop candidate of a track's last node
// with the poses of its neighbourhood and the query gathered into a batch of one row (k_pg_near; posegraph_dev.h: pg_hand_over), and the closure edge from the response
// record of that query (k_pg_closure).  One launch each, no workspace, no atomics; fp64 without FMA.
#include "lsd_internal.h"
#include "posegraph_dev.h"

namespace lsdhip {

constexpr int kPgBuildLanes = 256;
static_assert(sizeof(lsd_polar) == 16, "a reading is one 16-byte access");

// The candidates are decided in order by lane 0 -- the decision depends on the last one kept --, which hands the node a kept candidate
// became to the workgroup through LDS; all lanes copy its row.  Two barriers per candidate: a tick has a few frames.
__global__ __launch_bounds__(kPgBuildLanes) void k_pg_append(const lsd_polar* __restrict__ scans, const int* __restrict__ lens, int n_cand,
                                                             int stride, const uint8_t* __restrict__ poses, size_t pose_pitch, lsd_pg_head* head,
                                                             lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                                                             lsd_pg_track* track, int32_t track_id, lsd_polar* store, int* store_lens,
                                                             int store_stride, lsd_pg_append_par par, lsd_pg_append_rep* rep) {
    __shared__ int s_new;
    const int tid = (int)threadIdx.x;
    int n_nodes = 0, n_edges = 0, last = -1, added_n = 0, added_e = 0, dropped = 0;
    uint32_t flags = 0;
    PgPose raw{0.0, 0.0, 0.0};
    if (tid == 0) {
        n_nodes = pg_n_nodes(head, nodes_cap);
        n_edges = pg_n_edges(head, edges_cap);
        last = track->last;
        raw = PgPose{track->raw[0], track->raw[1], track->raw[2]};
    }
    const int copy = min(stride, store_stride);
    for (int t = 0; t < n_cand; t++) {
        if (tid == 0) {
            int made = -1;
            const double* qp = reinterpret_cast<const double*>(poses + (size_t)t * pose_pitch);
            const PgPose q{qp[0], qp[1], qp[2]};
            if (pg_pose_skipped(q) || lens[t] <= 0) dropped++;
            else if (last < 0 || last >= n_nodes) {                  // the first frame of a track
                if (n_nodes == nodes_cap) flags |= LSD_PG_APPEND_NODES_FULL;
                else {
                    made = n_nodes;
                    lsd_pg_node& nd = nodes[made];
                    nd.x = q.x; nd.y = q.y; nd.ang = q.a;
                    nd.raw[0] = q.x; nd.raw[1] = q.y; nd.raw[2] = q.a;
                    nd.flags = made == 0 ? LSD_PG_NODE_FIXED : 0u;
                    nd.track = track_id;
                    nd.reserved = 0;
                }
            } else {
                const PgPose z = pg_rel(raw, q);
                if (z.x * z.x + z.y * z.y >= par.min_dist * par.min_dist || fabs(z.a) >= par.min_ang) {
                    if (n_nodes == nodes_cap) flags |= LSD_PG_APPEND_NODES_FULL;
                    else if (n_edges == edges_cap) flags |= LSD_PG_APPEND_EDGES_FULL;
                    else {
                        made = n_nodes;
                        const PgPose at = pg_comp(PgPose{nodes[last].x, nodes[last].y, nodes[last].ang}, z);
                        lsd_pg_node& nd = nodes[made];
                        nd.x = at.x; nd.y = at.y; nd.ang = at.a;
                        nd.raw[0] = q.x; nd.raw[1] = q.y; nd.raw[2] = q.a;
                        nd.flags = 0u;
                        nd.track = track_id;
                        nd.reserved = 0;
                        lsd_pg_edge& ed = edges[n_edges];
                        ed.i = last; ed.j = made; ed.flags = 0u; ed.reserved = 0u;
                        ed.z[0] = z.x; ed.z[1] = z.y; ed.z[2] = z.a;
#pragma unroll
                        for (int k = 0; k < 6; k++) ed.info[k] = par.info[k];
                        ed.chi2 = 0.0;
                        n_edges++;
                        added_e++;
                    }
                }
            }
            if (made >= 0) {
                n_nodes++;
                added_n++;
                last = made;
                raw = q;
                store_lens[made] = min(min(lens[t], stride), store_stride);
            }
            s_new = made;
        }
        __syncthreads();
        const int made = s_new;
        if (made >= 0) {
            const lsd_polar* src = scans + (size_t)t * (size_t)stride;
            lsd_polar* dst = store + (size_t)made * (size_t)store_stride;
            for (int i = tid; i < copy; i += kPgBuildLanes) dst[i] = src[i];
        }
        __syncthreads();
    }
    if (tid == 0) {
        head->n_nodes = n_nodes;
        head->n_edges = n_edges;
        track->last = last;
        track->raw[0] = raw.x; track->raw[1] = raw.y; track->raw[2] = raw.a;
        if (rep) { rep->nodes = added_n; rep->edges = added_e; rep->dropped = dropped; rep->flags = flags; }
    }
}

// A lane keeps the nearest candidate of its nodes (ascending i, strictly nearer replaces: the smallest i among equals), a tree over the
// lanes keeps (d2, i) in that order; then pg_hand_over with the query's own pose.
__global__ __launch_bounds__(kPgBuildLanes) void k_pg_near(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_track* track,
                                                           const lsd_polar* store, const int* store_lens, int store_stride, int gap, double radius,
                                                           int window, PgHandOver out) {
    __shared__ double s_d2[kPgBuildLanes];
    __shared__ int s_i[kPgBuildLanes], s_n[kPgBuildLanes];
    const int tid = (int)threadIdx.x;
    const int n_nodes = pg_n_nodes(head, nodes_cap), j = track->last;
    const bool has_q = j >= 0 && j < n_nodes;
    double best = 0.0;
    int best_i = -1, count = 0;
    if (has_q) {
        const double xj = nodes[j].x, yj = nodes[j].y, r2 = radius * radius;
        for (int i = tid; i <= j - gap; i += kPgBuildLanes) {
            const double dx = nodes[i].x - xj, dy = nodes[i].y - yj, d2 = dx * dx + dy * dy;
            if (d2 <= r2) {
                count++;
                if (best_i < 0 || d2 < best) { best = d2; best_i = i; }
            }
        }
    }
    s_d2[tid] = best; s_i[tid] = best_i; s_n[tid] = count;
    __syncthreads();
    for (int h = kPgBuildLanes / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const int oi = s_i[tid + h];
            const double od = s_d2[tid + h];
            if (oi >= 0 && (s_i[tid] < 0 || od < s_d2[tid] || (od == s_d2[tid] && oi < s_i[tid]))) { s_d2[tid] = od; s_i[tid] = oi; }
            s_n[tid] += s_n[tid + h];
        }
        __syncthreads();
    }
    const int anchor = s_i[0];
    const PgPose qp = tid == 0 && anchor >= 0 ? PgPose{nodes[j].x, nodes[j].y, nodes[j].ang} : PgPose{0.0, 0.0, 0.0};
    pg_hand_over(nodes, nodes_cap, n_nodes, store, store_lens, store_stride, gap, window, j, anchor, s_n[0], s_d2[0], qp, out, tid, kPgBuildLanes);
}

__global__ void k_pg_closure(lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, const lsd_pg_near_rec* near_rec,
                             const lsd_grid_response_rec* resp, lsd_pg_closure_par par, lsd_pg_closure_rep* rep) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n_nodes = pg_n_nodes(head, nodes_cap), n_edges = pg_n_edges(head, edges_cap);
    const int anchor = near_rec->anchor, query = near_rec->query;
    const uint32_t rf = resp->flags;
    const double z[3] = {resp->x, resp->y, resp->ang};
    const double c6[6] = {resp->cov[0], resp->cov[1], resp->cov[2], resp->cov[3], resp->cov[4], resp->cov[5]};
    bool fin = isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]);
#pragma unroll
    for (int i = 0; i < 6; i++) fin = fin && isfinite(c6[i]);
    uint32_t flags;
    int made = -1;
    double det = 0.0;
    if (anchor < 0 || anchor >= n_nodes || query < 0 || query >= n_nodes || anchor == query) flags = LSD_PG_CLOSURE_NO_ANCHOR;
    else if (!(rf & LSD_GRID_RESPONSE_VALID) || (rf & (LSD_GRID_RESPONSE_NONE | LSD_GRID_RESPONSE_EMPTY | LSD_GRID_RESPONSE_MISMATCH)))
        flags = LSD_PG_CLOSURE_NO_RESPONSE;
    else if (!fin) flags = LSD_PG_CLOSURE_NOT_FINITE;
    else {
        const double R[9] = {c6[0] * par.cov_scale + par.floor_xy, c6[1] * par.cov_scale, c6[3] * par.cov_scale,
                             c6[1] * par.cov_scale, c6[2] * par.cov_scale + par.floor_xy, c6[4] * par.cov_scale,
                             c6[3] * par.cov_scale, c6[4] * par.cov_scale, c6[5] * par.cov_scale + par.floor_ang};
        double I[9];
        if (!pg_inv3(R, I, det)) flags = LSD_PG_CLOSURE_SINGULAR;
        else if (n_edges == edges_cap) flags = LSD_PG_CLOSURE_FULL;
        else {
            flags = LSD_PG_CLOSURE_APPENDED;
            made = n_edges;
            const PgPose pa{nodes[anchor].x, nodes[anchor].y, nodes[anchor].ang};
            const PgPose rel = pg_rel(pa, PgPose{z[0], z[1], z[2]});
            double s, c, T[9], J[9];
            sincos_g(deg2rad_ref(pa.a), s, c);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                T[3 * r] = I[3 * r] * c + I[3 * r + 1] * s;
                T[3 * r + 1] = I[3 * r + 1] * c - I[3 * r] * s;
                T[3 * r + 2] = I[3 * r + 2];
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
                J[q] = c * T[q] + s * T[3 + q];
                J[3 + q] = c * T[3 + q] - s * T[q];
                J[6 + q] = T[6 + q];
            }
            lsd_pg_edge& ed = edges[made];
            ed.i = anchor; ed.j = query; ed.flags = LSD_PG_EDGE_CLOSURE; ed.reserved = 0u;
            ed.z[0] = rel.x; ed.z[1] = rel.y; ed.z[2] = rel.a;
            ed.info[0] = J[0]; ed.info[1] = J[1]; ed.info[2] = J[4]; ed.info[3] = J[2]; ed.info[4] = J[5]; ed.info[5] = J[8];
            ed.chi2 = 0.0;
            head->n_edges = n_edges + 1;
        }
    }
    if (rep) { rep->edge = made; rep->flags = flags; rep->det = det; }
}

void launch_pg_append(const lsd_polar* scans, const int* lens, int n_cand, int stride, const void* poses, size_t pose_pitch, lsd_pg_head* head,
                      lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, lsd_pg_track* track, int32_t track_id, lsd_polar* store,
                      int* store_lens, int store_stride, lsd_pg_append_par par, lsd_pg_append_rep* rep, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_append, dim3(1), dim3(kPgBuildLanes), 0, st, scans, lens, n_cand, stride, static_cast<const uint8_t*>(poses), pose_pitch,
                       head, nodes, nodes_cap, edges, edges_cap, track, track_id, store, store_lens, store_stride, par, rep);
}

void launch_pg_near(const lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, const lsd_pg_track* track, const lsd_polar* store,
                    const int* store_lens, int store_stride, int gap, double radius, int window, PgHandOver out, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_near, dim3(1), dim3(kPgBuildLanes), 0, st, head, nodes, nodes_cap, track, store, store_lens, store_stride, gap, radius,
                       window, out);
}

void launch_pg_closure(lsd_pg_head* head, const lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, const lsd_pg_near_rec* near_rec,
                       const lsd_grid_response_rec* resp, lsd_pg_closure_par par, lsd_pg_closure_rep* rep, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_closure, dim3(1), dim3(64), 0, st, head, nodes, nodes_cap, edges, edges_cap, near_rec, resp, par, rep);
}

}  // namespace lsdhip
