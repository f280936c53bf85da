// lsd_pg.hip -- the pose graph's part of the C ABI (include/lsd_hip.h, "pose graph"): the argument checks of the six device entries
// (k_pgbuild.hip: append, near, closure; k_posegraph.hip: the relaxation, plain and robust; k_pgprune.hip: the rejection of closures), of
// place recognition's two (k_pgplace.hip), the three that find every loop of a track (k_pgloops.hip), the marginals and the vet (k_pgmarg.hip) and the host conveniences, each one round trip through the context's staging (lsd_ctx.h: stage_round_trip).
#include <math.h>
#include <stddef.h>

#include "lsd_ctx.h"

static_assert(sizeof(lsd_pg_head) == 8 && sizeof(lsd_pg_node) == 64 && offsetof(lsd_pg_node, x) == 0 && offsetof(lsd_pg_node, y) == 8 &&
              offsetof(lsd_pg_node, ang) == 16 && offsetof(lsd_pg_node, raw) == 24 && offsetof(lsd_pg_node, flags) == 48 &&
              offsetof(lsd_pg_node, track) == 52 && offsetof(lsd_pg_node, reserved) == 56,
              "lsd_pg_node is 64 bytes and starts with a pose: an array of them is a d_poses argument of pitch 64");
static_assert(sizeof(lsd_pg_edge) == 96 && offsetof(lsd_pg_edge, flags) == 8 && offsetof(lsd_pg_edge, z) == 16 && offsetof(lsd_pg_edge, info) == 40 &&
              offsetof(lsd_pg_edge, chi2) == 88, "lsd_pg_edge is 96 bytes");
static_assert(sizeof(lsd_pg_track) == 32 && offsetof(lsd_pg_track, raw) == 8 && sizeof(lsd_pg_append_par) == 64 && sizeof(lsd_pg_append_rep) == 16 &&
              sizeof(lsd_pg_near_rec) == 24 && offsetof(lsd_pg_near_rec, d2) == 16 && sizeof(lsd_pg_closure_par) == 24 && sizeof(lsd_pg_closure_rep) == 16 &&
              offsetof(lsd_pg_closure_rep, det) == 8, "the records of building a pose graph");
static_assert(sizeof(lsd_pg_relax_par) == 56 && offsetof(lsd_pg_relax_par, iters) == 48 && sizeof(lsd_pg_relax_rep) == 56 &&
              offsetof(lsd_pg_relax_rep, iters) == 24 && offsetof(lsd_pg_relax_rep, flags) == 48, "the relaxation's parameters and report");
static_assert(sizeof(lsd_pg_robust_par) == 16 && offsetof(lsd_pg_robust_par, delta) == 8 && sizeof(lsd_pg_robust_rep) == 24 &&
              offsetof(lsd_pg_robust_rep, downweighted) == 16 && sizeof(lsd_pg_prune_par) == 16 && offsetof(lsd_pg_prune_par, max_reject) == 8 &&
              sizeof(lsd_pg_prune_rep) == 24 && offsetof(lsd_pg_prune_rep, worst_chi2) == 16, "the robust relaxation's and the prune's records");
static_assert(sizeof(lsd_pg_precond_par) == 8 && sizeof(lsd_pg_precond_rep) == 16 && offsetof(lsd_pg_precond_rep, fallbacks) == 12,
              "the preconditioner's records");
static_assert(sizeof(lsd_pg_marg_query) == 16 && sizeof(lsd_pg_marg_par) == 24 && offsetof(lsd_pg_marg_par, cg_iters) == 8 &&
              sizeof(lsd_pg_marg_rec) == 104 && offsetof(lsd_pg_marg_rec, steps) == 72 && offsetof(lsd_pg_marg_rec, flags) == 84 &&
              offsetof(lsd_pg_marg_rec, kind) == 88 && sizeof(lsd_pg_marg_rep) == 32 && sizeof(lsd_pg_vet_rep) == 24 &&
              offsetof(lsd_pg_vet_rep, edge) == 16, "the marginals' and the vet's records");
static_assert(sizeof(lsd_pg_desc) == 72 && sizeof(lsd_pg_place_par) == 32 && offsetof(lsd_pg_place_par, max_dist) == 20 && sizeof(lsd_pg_place_rec) == 16 &&
              offsetof(lsd_pg_place_rec, dist) == 8 && sizeof(lsd_pg_place_rep) == 16, "place recognition's records");
static_assert(sizeof(lsd_pg_loops_par) == 8 && sizeof(lsd_pg_loop_rec) == 16 && offsetof(lsd_pg_loop_rec, dist) == 12 && sizeof(lsd_pg_loops_rep) == 16,
              "the loops' records");
static_assert(sizeof(lsd_pg_reduce_par) == 24 && offsetof(lsd_pg_reduce_par, keep) == 16 && sizeof(lsd_pg_reduce_rep) == 48 &&
              offsetof(lsd_pg_reduce_rep, flags) == 44, "the reduce's records");

constexpr int kPgMaxNodes = 16384, kPgMaxEdges = 65536;

static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
static bool pg_nodes_cap_bad(int nodes_cap) { return nodes_cap < 1 || nodes_cap > kPgMaxNodes; }
static bool pg_caps_bad(int nodes_cap, int edges_cap) { return pg_nodes_cap_bad(nodes_cap) || edges_cap < 1 || edges_cap > kPgMaxEdges; }
static bool pg_stride_bad(const lsd_ctx* c, int stride) { return stride <= 0 || stride > c->scan_cap; }
// the hand-over's five pointers (lsd_internal.h: PgHandOver): 0 where they are all there and aligned, 1 where one is null, 2 where one is
// not aligned -- q_scan 16-byte, the records 8-byte, q_len 4-byte
static int pg_hand_over_bad(const PgHandOver& o) {
    if (!o.rec || !o.sel || !o.q_scan || !o.q_len || !o.q_pose) return 1;
    return (addr(o.q_scan) & 15) || ((addr(o.rec) | addr(o.sel) | addr(o.q_pose)) & 7) || (addr(o.q_len) & 3) ? 2 : 0;
}
static bool pg_real_bad(double v) { return !std::isfinite(v) || v < 0; }

static bool pg_append_par_bad(const lsd_pg_append_par& p) {
    for (int k = 0; k < 6; k++) if (!std::isfinite(p.info[k])) return true;
    return pg_real_bad(p.min_dist) || pg_real_bad(p.min_ang);
}

static bool pg_relax_par_bad(const lsd_pg_relax_par& p) {
    if (pg_real_bad(p.lambda0) || pg_real_bad(p.lambda_min) || pg_real_bad(p.up) || pg_real_bad(p.down) || pg_real_bad(p.cg_tol) || pg_real_bad(p.eps))
        return true;
    return p.up <= 1 || p.down < 1 || p.iters < 0 || p.iters > 65535 || p.cg_iters < 0 || p.cg_iters > 65535;
}

static bool pg_robust_par_bad(const lsd_pg_robust_par& r) {
    if (r.kernel < LSD_PG_KERNEL_NONE || r.kernel > LSD_PG_KERNEL_GM || r.scope > LSD_PG_ROBUST_ALL) return true;
    return r.kernel != LSD_PG_KERNEL_NONE && !(std::isfinite(r.delta) && r.delta > 0);
}

static bool pg_place_par_bad(const lsd_pg_place_par& p) {
    return p.gap < 1 || p.window < 0 || p.spread < 0 || p.k < 1 || p.k > LSD_PG_PLACE_MAX || p.pick < 0 || p.pick >= p.k || p.max_dist > 16320u ||
           p.min_sectors < 1 || p.min_sectors > (uint32_t)LSD_PG_DESC_SECTORS;
}

static bool pg_queries_bad(int q_lo, int n_q, int nodes_cap) { return q_lo < 0 || n_q < 0 || q_lo > nodes_cap - n_q; }
static bool pg_loops_par_bad(const lsd_pg_loops_par& p, int k) {
    return p.max_loops < 1 || p.max_loops > LSD_PG_LOOPS_MAX || p.spread < 0 || k < 1 || k > LSD_PG_PLACE_MAX;
}

static bool pg_precond_par_bad(const lsd_pg_precond_par& p) { return p.kind < LSD_PG_PRECOND_BLOCK || p.kind > LSD_PG_PRECOND_CHAIN || p.reserved != 0; }

static bool pg_reduce_par_bad(const lsd_pg_reduce_par& p) {
    return !(std::isfinite(p.cell) && p.cell > 0) || !(std::isfinite(p.ang_bin) && p.ang_bin > 0 && p.ang_bin <= 360) || p.keep < 1 || p.max_run < 1;
}

constexpr int kPgMaxSlots = 1024, kPgMaxQueries = 65536;
static bool pg_queries_n_bad(int n_q) { return n_q < 0 || n_q > kPgMaxQueries; }
static bool pg_marg_par_bad(const lsd_pg_marg_par& p) {
    return pg_real_bad(p.cg_tol) || p.cg_iters < 0 || p.cg_iters > 65535 || pg_precond_par_bad(lsd_pg_precond_par{p.precond, 0}) || p.slots < 1 ||
           p.slots > kPgMaxSlots || p.reserved != 0;
}

// the three host relaxations: one graph around the device entry, rob == nullptr for the plain one, pc != nullptr for the choice of
// preconditioner
static int pg_relax_host(lsd_ctx* c, lsd_pg_node* nodes, int n_nodes, lsd_pg_edge* edges, int n_edges, lsd_pg_relax_par par,
                         const lsd_pg_robust_par* rob, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep, const lsd_pg_precond_par* pc = nullptr,
                         lsd_pg_precond_rep* pc_rep = nullptr);

extern "C" {

int lsd_enqueue_pg_append_device(lsd_ctx* c, const lsd_polar* d_scans, const int* d_lens, int n_cand, int stride, const void* d_poses,
                                 size_t pose_pitch, lsd_pg_head* d_head, lsd_pg_node* d_nodes, int nodes_cap, lsd_pg_edge* d_edges, int edges_cap,
                                 lsd_pg_track* d_track, int32_t track, lsd_polar* d_store, int* d_store_lens, int store_stride,
                                 lsd_pg_append_par par, lsd_pg_append_rep* d_rep, void* stream) {
    if (!c || !d_scans || !d_lens || !d_poses || !d_head || !d_nodes || !d_edges || !d_track || !d_store || !d_store_lens) return LSD_ERR_INVALID;
    if (n_cand < 0 || pg_stride_bad(c, stride) || pg_stride_bad(c, store_stride)) return LSD_ERR_INVALID;
    if (pose_pitch < sizeof(lsd_position) || pose_pitch % 8 || pg_caps_bad(nodes_cap, edges_cap) || pg_append_par_bad(par)) return LSD_ERR_INVALID;
    if (((addr(d_scans) | addr(d_store)) & 15) || ((addr(d_poses) | addr(d_head) | addr(d_nodes) | addr(d_edges) | addr(d_track) | addr(d_rep)) & 7) ||
        ((addr(d_lens) | addr(d_store_lens)) & 3)) {
        c->err = "pg append: scans and store 16-byte, the records 8-byte, the lengths 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_cand == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_append(d_scans, d_lens, n_cand, stride, d_poses, pose_pitch, d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_track, track, d_store,
                         d_store_lens, store_stride, par, d_rep, s);
        return LSD_OK;
    });
}

int lsd_enqueue_pg_near_device(lsd_ctx* c, const lsd_pg_head* d_head, const lsd_pg_node* d_nodes, int nodes_cap, const lsd_pg_track* d_track,
                               const lsd_polar* d_store, const int* d_store_lens, int store_stride, int gap, double radius, int window,
                               lsd_pg_near_rec* d_rec, lsd_position* d_sel, lsd_polar* d_q_scan, int* d_q_len, lsd_position* d_q_pose, void* stream) {
    const PgHandOver out{d_rec, d_sel, d_q_scan, d_q_len, d_q_pose};
    const int out_bad = pg_hand_over_bad(out);
    if (!c || !d_head || !d_nodes || !d_track || !d_store || !d_store_lens || out_bad == 1) return LSD_ERR_INVALID;
    if (pg_nodes_cap_bad(nodes_cap) || pg_stride_bad(c, store_stride) || gap < 1 || window < 0 || pg_real_bad(radius)) return LSD_ERR_INVALID;
    if ((addr(d_store) & 15) || ((addr(d_head) | addr(d_nodes) | addr(d_track)) & 7) || (addr(d_store_lens) & 3) || out_bad) {
        c->err = "pg near: store and d_q_scan 16-byte, the records 8-byte, the lengths 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_near(d_head, d_nodes, nodes_cap, d_track, d_store, d_store_lens, store_stride, gap, radius, window, out, s);
        return LSD_OK;
    });
}

int lsd_enqueue_pg_closure_device(lsd_ctx* c, lsd_pg_head* d_head, const lsd_pg_node* d_nodes, int nodes_cap, lsd_pg_edge* d_edges, int edges_cap,
                                  const lsd_pg_near_rec* d_near, const lsd_grid_response_rec* d_resp, lsd_pg_closure_par par,
                                  lsd_pg_closure_rep* d_rep, void* stream) {
    if (!c || !d_head || !d_nodes || !d_edges || !d_near || !d_resp || pg_caps_bad(nodes_cap, edges_cap)) return LSD_ERR_INVALID;
    if (pg_real_bad(par.cov_scale) || pg_real_bad(par.floor_xy) || pg_real_bad(par.floor_ang)) return LSD_ERR_INVALID;
    if ((addr(d_head) | addr(d_nodes) | addr(d_edges) | addr(d_near) | addr(d_resp) | addr(d_rep)) & 7) {
        c->err = "pg closure: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_closure(d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_near, d_resp, par, d_rep, s);
        return LSD_OK;
    });
}

size_t lsd_pg_workspace_bytes(int nodes_cap, int edges_cap) { return pg_caps_bad(nodes_cap, edges_cap) ? 0 : pg_ws_bytes(nodes_cap, edges_cap); }

int lsd_enqueue_pg_relax_device(lsd_ctx* c, int n_graphs, const lsd_pg_head* d_heads, lsd_pg_node* d_nodes, int nodes_cap, lsd_pg_edge* d_edges,
                                int edges_cap, lsd_pg_relax_par par, void* d_workspace, lsd_pg_relax_rep* d_rep, void* stream) {
    if (!c || !d_heads || !d_nodes || !d_edges || !d_workspace || !d_rep || n_graphs < 0) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_relax_par_bad(par)) return LSD_ERR_INVALID;
    if ((addr(d_heads) | addr(d_nodes) | addr(d_edges) | addr(d_workspace) | addr(d_rep)) & 7) {
        c->err = "pg relax: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_graphs == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_relax(n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, par, d_workspace, d_rep, s);
        return LSD_OK;
    });
}

int lsd_enqueue_pg_relax_robust_device(lsd_ctx* c, int n_graphs, const lsd_pg_head* d_heads, lsd_pg_node* d_nodes, int nodes_cap,
                                       lsd_pg_edge* d_edges, int edges_cap, lsd_pg_relax_par par, lsd_pg_robust_par rob, void* d_workspace,
                                       lsd_pg_relax_rep* d_rep, lsd_pg_robust_rep* d_rob_rep, void* stream) {
    if (!c || !d_heads || !d_nodes || !d_edges || !d_workspace || !d_rep || n_graphs < 0) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_relax_par_bad(par) || pg_robust_par_bad(rob)) return LSD_ERR_INVALID;
    if ((addr(d_heads) | addr(d_nodes) | addr(d_edges) | addr(d_workspace) | addr(d_rep) | addr(d_rob_rep)) & 7) {
        c->err = "pg relax robust: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_graphs == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_relax_robust(n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, par, rob, d_workspace, d_rep, d_rob_rep, s);
        return LSD_OK;
    });
}

size_t lsd_pg_workspace_pc_bytes(int nodes_cap, int edges_cap, int kind) {
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_precond_par_bad(lsd_pg_precond_par{kind, 0})) return 0;
    return pg_ws_pc_bytes(nodes_cap, edges_cap, kind);
}

int lsd_enqueue_pg_relax_pc_device(lsd_ctx* c, int n_graphs, const lsd_pg_head* d_heads, lsd_pg_node* d_nodes, int nodes_cap, lsd_pg_edge* d_edges,
                                   int edges_cap, lsd_pg_relax_par par, lsd_pg_robust_par rob, lsd_pg_precond_par pc, void* d_workspace,
                                   lsd_pg_relax_rep* d_rep, lsd_pg_robust_rep* d_rob_rep, lsd_pg_precond_rep* d_pc_rep, void* stream) {
    if (!c || !d_heads || !d_nodes || !d_edges || !d_workspace || !d_rep || n_graphs < 0) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_relax_par_bad(par) || pg_robust_par_bad(rob) || pg_precond_par_bad(pc)) return LSD_ERR_INVALID;
    if ((addr(d_heads) | addr(d_nodes) | addr(d_edges) | addr(d_workspace) | addr(d_rep) | addr(d_rob_rep) | addr(d_pc_rep)) & 7) {
        c->err = "pg relax pc: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_graphs == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        if (pc.kind == LSD_PG_PRECOND_CHAIN) {
            launch_pg_relax_chain(n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, par, rob, d_workspace, d_rep, d_rob_rep, d_pc_rep, s);
            return LSD_OK;
        }
        launch_pg_relax_robust(n_graphs, d_heads, d_nodes, nodes_cap, d_edges, edges_cap, par, rob, d_workspace, d_rep, d_rob_rep, s);
        if (d_pc_rep) HIPCHK(c, hipMemsetAsync(d_pc_rep, 0, (size_t)n_graphs * sizeof(lsd_pg_precond_rep), s));
        return LSD_OK;
    });
}

int lsd_enqueue_pg_prune_device(lsd_ctx* c, int n_graphs, const lsd_pg_head* d_heads, lsd_pg_edge* d_edges, int edges_cap, lsd_pg_prune_par par,
                                lsd_pg_prune_rep* d_rep, void* stream) {
    if (!c || !d_heads || !d_edges || !d_rep || n_graphs < 0 || edges_cap < 1 || edges_cap > kPgMaxEdges) return LSD_ERR_INVALID;
    if (pg_real_bad(par.gate) || par.max_reject < 0 || par.max_reject > 64) return LSD_ERR_INVALID;
    if ((addr(d_heads) | addr(d_edges) | addr(d_rep)) & 7) {
        c->err = "pg prune: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_graphs == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_prune(n_graphs, d_heads, d_edges, edges_cap, par, d_rep, s);
        return LSD_OK;
    });
}

size_t lsd_pg_marginals_workspace_bytes(int nodes_cap, int edges_cap, int precond, int slots) {
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_precond_par_bad(lsd_pg_precond_par{precond, 0}) || slots < 1 || slots > kPgMaxSlots) return 0;
    return pg_marg_ws_bytes(nodes_cap, edges_cap, precond, slots);
}

int lsd_enqueue_pg_marginals_device(lsd_ctx* c, const lsd_pg_head* d_head, const lsd_pg_node* d_nodes, int nodes_cap, const lsd_pg_edge* d_edges,
                                    int edges_cap, const lsd_pg_head* d_prior, const lsd_pg_marg_query* d_queries, int n_q, lsd_pg_marg_par par,
                                    void* d_workspace, lsd_pg_marg_rec* d_recs, lsd_pg_marg_rep* d_rep, void* stream) {
    if (!c || !d_head || !d_nodes || !d_edges || !d_workspace || !d_rep || pg_queries_n_bad(n_q) || (n_q && (!d_queries || !d_recs)))
        return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_marg_par_bad(par)) return LSD_ERR_INVALID;
    if ((addr(d_head) | addr(d_nodes) | addr(d_edges) | addr(d_prior) | addr(d_queries) | addr(d_workspace) | addr(d_recs) | addr(d_rep)) & 7) {
        c->err = "pg marginals: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_q == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_marginals(d_head, d_prior, d_nodes, nodes_cap, d_edges, edges_cap, d_queries, n_q, par, d_workspace, d_recs, d_rep, s);
        return LSD_OK;
    });
}

int lsd_enqueue_pg_vet_device(lsd_ctx* c, const lsd_pg_head* d_head, const lsd_pg_node* d_nodes, int nodes_cap, lsd_pg_edge* d_edges, int edges_cap,
                              const lsd_pg_marg_query* d_queries, const lsd_pg_marg_rec* d_recs, int n_q, double gate, lsd_pg_vet_rep* d_rep,
                              void* stream) {
    if (!c || !d_head || !d_nodes || !d_edges || pg_queries_n_bad(n_q) || (n_q && (!d_queries || !d_recs))) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_real_bad(gate)) return LSD_ERR_INVALID;
    if ((addr(d_head) | addr(d_nodes) | addr(d_edges) | addr(d_queries) | addr(d_recs) | addr(d_rep)) & 7) {
        c->err = "pg vet: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_q == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_vet(d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_queries, d_recs, n_q, gate, d_rep, s);
        return LSD_OK;
    });
}

int lsd_pg_marginals(lsd_ctx* c, const lsd_pg_node* nodes, int n_nodes, const lsd_pg_edge* edges, int n_edges, int prior_edges,
                     const lsd_pg_marg_query* queries, int n_q, lsd_pg_marg_par par, lsd_pg_marg_rec* recs, lsd_pg_marg_rep* rep) {
    if (!c || !rep || n_nodes < 0 || n_nodes > kPgMaxNodes || n_edges < 0 || n_edges > kPgMaxEdges || (n_nodes && !nodes) || (n_edges && !edges))
        return LSD_ERR_INVALID;
    if (pg_queries_n_bad(n_q) || (n_q && (!queries || !recs)) || pg_marg_par_bad(par)) return LSD_ERR_INVALID;
    if (n_q == 0) return LSD_OK;
    const int nc = n_nodes ? n_nodes : 1, ec = n_edges ? n_edges : 1;      // (a cap is at least 1)
    const lsd_pg_head head{n_nodes, n_edges}, prior{n_nodes, prior_edges};
    lsd_pg_head *d_head, *d_prior; lsd_pg_node* d_no; lsd_pg_edge* d_ed; lsd_pg_marg_query* d_qu; lsd_pg_marg_rec* d_recs; lsd_pg_marg_rep* d_rep;
    uint8_t* d_ws;
    auto plan = [&](StagePass& k) {
        k.in(d_head, &head, 1); k.in(d_prior, &prior, 1); k.in(d_no, nodes, n_nodes); k.in(d_ed, edges, n_edges); k.in(d_qu, queries, n_q);
        k.out(d_recs, recs, n_q); k.out(d_rep, rep, 1); k.scratch(d_ws, pg_marg_ws_bytes(nc, ec, par.precond, par.slots));
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_pg_marginals_device(c, d_head, d_no, nc, d_ed, ec, prior_edges < 0 ? nullptr : d_prior, d_qu, n_q, par, d_ws, d_recs, d_rep,
                                               c->stream);
    });
}

int lsd_pg_vet(lsd_ctx* c, const lsd_pg_node* nodes, int n_nodes, lsd_pg_edge* edges, int n_edges, const lsd_pg_marg_query* queries,
               const lsd_pg_marg_rec* recs, int n_q, double gate, lsd_pg_vet_rep* reps) {
    if (!c || n_nodes < 0 || n_nodes > kPgMaxNodes || n_edges < 0 || n_edges > kPgMaxEdges || (n_nodes && !nodes) || (n_edges && !edges))
        return LSD_ERR_INVALID;
    if (pg_queries_n_bad(n_q) || (n_q && (!queries || !recs)) || pg_real_bad(gate)) return LSD_ERR_INVALID;
    if (n_q == 0) return LSD_OK;
    const int nc = n_nodes ? n_nodes : 1, ec = n_edges ? n_edges : 1;
    const lsd_pg_head head{n_nodes, n_edges};
    lsd_pg_head* d_head; lsd_pg_node* d_no; lsd_pg_edge* d_ed; lsd_pg_marg_query* d_qu; lsd_pg_marg_rec* d_recs; lsd_pg_vet_rep* d_reps;
    auto plan = [&](StagePass& k) {
        k.in(d_head, &head, 1); k.in(d_no, nodes, n_nodes); k.both(d_ed, edges, n_edges); k.in(d_qu, queries, n_q); k.in(d_recs, recs, n_q);
        k.out(d_reps, reps, n_q);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_pg_vet_device(c, d_head, d_no, nc, d_ed, ec, d_qu, d_recs, n_q, gate, reps ? d_reps : nullptr, c->stream);
    });
}

int lsd_enqueue_pg_describe_device(lsd_ctx* c, const lsd_pg_head* d_head, int nodes_cap, const lsd_polar* d_store, const int* d_store_lens,
                                   int store_stride, double range_max, lsd_pg_desc* d_desc, void* stream) {
    if (!c || !d_head || !d_store || !d_store_lens || !d_desc) return LSD_ERR_INVALID;
    if (pg_nodes_cap_bad(nodes_cap) || pg_stride_bad(c, store_stride) || !(std::isfinite(range_max) && range_max > 0)) return LSD_ERR_INVALID;
    if ((addr(d_store) & 15) || ((addr(d_head) | addr(d_desc)) & 7) || (addr(d_store_lens) & 3)) {
        c->err = "pg describe: store 16-byte, head and descriptors 8-byte, the lengths 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_describe(d_head, nodes_cap, d_store, d_store_lens, store_stride, range_max, d_desc, s);
        return LSD_OK;
    });
}

int lsd_enqueue_pg_recognize_device(lsd_ctx* c, const lsd_pg_head* d_head, const lsd_pg_node* d_nodes, int nodes_cap, const lsd_pg_track* d_track,
                                    const lsd_polar* d_store, const int* d_store_lens, int store_stride, const lsd_pg_desc* d_desc,
                                    lsd_pg_place_par par, uint32_t* d_work, lsd_pg_place_rec* d_recs, lsd_pg_place_rep* d_rep, lsd_pg_near_rec* d_near,
                                    lsd_position* d_sel, lsd_polar* d_q_scan, int* d_q_len, lsd_position* d_q_pose, void* stream) {
    const PgHandOver out{d_near, d_sel, d_q_scan, d_q_len, d_q_pose};
    const int out_bad = pg_hand_over_bad(out);
    if (!c || !d_head || !d_nodes || !d_track || !d_store || !d_store_lens || !d_desc || !d_work || !d_recs || !d_rep || out_bad == 1)
        return LSD_ERR_INVALID;
    if (pg_nodes_cap_bad(nodes_cap) || pg_stride_bad(c, store_stride) || pg_place_par_bad(par)) return LSD_ERR_INVALID;
    if ((addr(d_store) & 15) || ((addr(d_head) | addr(d_nodes) | addr(d_track) | addr(d_desc) | addr(d_recs) | addr(d_rep)) & 7) ||
        ((addr(d_store_lens) | addr(d_work)) & 3) || out_bad) {
        c->err = "pg recognize: store and d_q_scan 16-byte, the records and descriptors 8-byte, the lengths and d_work 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_recognize(d_head, d_nodes, nodes_cap, d_track, d_store, d_store_lens, store_stride, d_desc, par, d_work, d_recs, d_rep, out, s);
        return LSD_OK;
    });
}

int lsd_pg_describe(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n, int stride, double range_max, lsd_pg_desc* desc_out) {
    if (!c || n < 0 || n > kPgMaxNodes || pg_stride_bad(c, stride) || !(std::isfinite(range_max) && range_max > 0)) return LSD_ERR_INVALID;
    if (n == 0) return LSD_OK;
    if (!scans || !lens || !desc_out) return LSD_ERR_INVALID;
    const size_t nn = (size_t)n;
    const lsd_pg_head head{n, 0};
    lsd_pg_head* d_head; lsd_polar* d_sc; int* d_len; lsd_pg_desc* d_desc;
    auto plan = [&](StagePass& k) { k.in(d_sc, scans, nn * stride); k.in(d_head, &head, 1); k.out(d_desc, desc_out, nn); k.in(d_len, lens, nn); };
    return stage_round_trip(c, plan, [&]() -> int {
        HIPCHK(c, hipMemsetAsync(d_desc, 0, nn * sizeof(lsd_pg_desc), c->stream));      // (valid == 0: every row is described)
        return lsd_enqueue_pg_describe_device(c, d_head, n, d_sc, d_len, stride, range_max, d_desc, c->stream);
    });
}

int lsd_pg_recognize(lsd_ctx* c, const lsd_pg_desc* desc, int n_nodes, int query, lsd_pg_place_par par, lsd_pg_place_rec* recs, lsd_pg_place_rep* rep) {
    if (!c || !desc || !recs || !rep || pg_nodes_cap_bad(n_nodes) || pg_place_par_bad(par)) return LSD_ERR_INVALID;
    const size_t nn = (size_t)n_nodes;
    const lsd_pg_head head{n_nodes, 0};
    const lsd_pg_track track{query, 0, {0.0, 0.0, 0.0}};
    lsd_pg_head* d_head; lsd_pg_track* d_tr; lsd_pg_desc* d_desc; uint32_t* d_work; lsd_pg_place_rec* d_recs; lsd_pg_place_rep* d_rep;
    auto plan = [&](StagePass& k) {
        k.in(d_head, &head, 1); k.in(d_tr, &track, 1); k.in(d_desc, desc, nn); k.out(d_recs, recs, par.k); k.out(d_rep, rep, 1); k.scratch(d_work, nn);
    };
    return stage_round_trip(c, plan, [&] {
        return enqueue_on(c, c->stream, [&](hipStream_t s) {
            launch_pg_recognize(d_head, nullptr, n_nodes, d_tr, nullptr, nullptr, 1, d_desc, par, d_work, d_recs, d_rep, PgHandOver{}, s);   // no hand-over
            return LSD_OK;
        });
    });
}

int lsd_enqueue_pg_recognize_all_device(lsd_ctx* c, const lsd_pg_head* d_head, int nodes_cap, const lsd_pg_desc* d_desc, lsd_pg_place_par par,
                                        int q_lo, int n_q, lsd_pg_place_rec* d_recs, lsd_pg_place_rep* d_reps, void* stream) {
    if (!c || !d_head || !d_desc || !d_recs || !d_reps) return LSD_ERR_INVALID;
    if (pg_nodes_cap_bad(nodes_cap) || pg_place_par_bad(par) || pg_queries_bad(q_lo, n_q, nodes_cap)) return LSD_ERR_INVALID;
    if ((addr(d_head) | addr(d_desc) | addr(d_recs) | addr(d_reps)) & 7) {
        c->err = "pg recognize all: head, descriptors, records and reports 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    if (n_q == 0) return LSD_OK;
    return enqueue_on(c, stream, [&](hipStream_t s) {
        HIPCHK(c, launch_pg_recognize_all(d_head, nodes_cap, d_desc, par, q_lo, n_q, d_recs, d_reps, s));
        return LSD_OK;
    });
}

size_t lsd_pg_loops_workspace_bytes(int n_q, int k, int edges_cap) {
    if (n_q < 0 || n_q > kPgMaxNodes || k < 1 || k > LSD_PG_PLACE_MAX || edges_cap < 1 || edges_cap > kPgMaxEdges) return 0;
    return pg_loops_ws_bytes(n_q, k, edges_cap);
}

int lsd_enqueue_pg_loops_device(lsd_ctx* c, const lsd_pg_place_rec* d_recs, const lsd_pg_place_rep* d_reps, int q_lo, int n_q, int k,
                                const lsd_pg_head* d_head, int nodes_cap, const lsd_pg_edge* d_edges, int edges_cap, lsd_pg_loops_par par,
                                void* d_workspace, lsd_pg_loop_rec* d_loops, lsd_pg_loops_rep* d_rep, void* stream) {
    if (!c || !d_recs || !d_reps || !d_head || !d_edges || !d_workspace || !d_loops || !d_rep) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_loops_par_bad(par, k) || pg_queries_bad(q_lo, n_q, nodes_cap)) return LSD_ERR_INVALID;
    if ((addr(d_recs) | addr(d_reps) | addr(d_head) | addr(d_edges) | addr(d_workspace) | addr(d_loops) | addr(d_rep)) & 7) {
        c->err = "pg loops: every pointer 8-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_loops(d_recs, d_reps, n_q, k, d_head, d_edges, edges_cap, par, d_workspace, d_loops, d_rep, s);
        return LSD_OK;
    });
}

int lsd_enqueue_pg_loop_select_device(lsd_ctx* c, const lsd_pg_head* d_head, const lsd_pg_node* d_nodes, int nodes_cap, const lsd_polar* d_store,
                                      const int* d_store_lens, int store_stride, int gap, int window, const lsd_pg_loop_rec* d_loops,
                                      const lsd_pg_loops_rep* d_loops_rep, int m, lsd_pg_near_rec* d_near, lsd_position* d_sel, lsd_polar* d_q_scan,
                                      int* d_q_len, lsd_position* d_q_pose, void* stream) {
    const PgHandOver out{d_near, d_sel, d_q_scan, d_q_len, d_q_pose};
    const int out_bad = pg_hand_over_bad(out);
    if (!c || !d_head || !d_nodes || !d_store || !d_store_lens || !d_loops || !d_loops_rep || out_bad == 1) return LSD_ERR_INVALID;
    if (pg_nodes_cap_bad(nodes_cap) || pg_stride_bad(c, store_stride) || gap < 1 || window < 0 || m < 0 || m >= LSD_PG_LOOPS_MAX) return LSD_ERR_INVALID;
    if ((addr(d_store) & 15) || ((addr(d_head) | addr(d_nodes) | addr(d_loops) | addr(d_loops_rep)) & 7) || (addr(d_store_lens) & 3) || out_bad) {
        c->err = "pg loop select: store and d_q_scan 16-byte, the records 8-byte, the lengths 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_loop_select(d_head, d_nodes, nodes_cap, d_store, d_store_lens, store_stride, gap, window, d_loops, d_loops_rep, m, out, s);
        return LSD_OK;
    });
}

size_t lsd_pg_reduce_workspace_bytes(int nodes_cap, int edges_cap, int store_stride) {
    return pg_caps_bad(nodes_cap, edges_cap) || store_stride < 1 ? 0 : pg_reduce_ws_bytes(nodes_cap, edges_cap, store_stride);
}

int lsd_enqueue_pg_reduce_device(lsd_ctx* c, lsd_pg_head* d_head, lsd_pg_node* d_nodes, int nodes_cap, lsd_pg_edge* d_edges, int edges_cap,
                                 lsd_pg_track* d_tracks, int n_tracks, lsd_polar* d_store, int* d_store_lens, int store_stride, lsd_pg_desc* d_desc,
                                 lsd_pg_reduce_par par, int32_t* d_map, lsd_pg_reduce_rep* d_rep, void* d_workspace, void* stream) {
    if (!c || !d_head || !d_nodes || !d_edges || !d_tracks || !d_store || !d_store_lens || !d_map || !d_workspace) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_stride_bad(c, store_stride) || n_tracks < 1 || pg_reduce_par_bad(par)) return LSD_ERR_INVALID;
    if (((addr(d_store) | addr(d_workspace)) & 15) || ((addr(d_head) | addr(d_nodes) | addr(d_edges) | addr(d_tracks) | addr(d_desc) | addr(d_rep)) & 7) ||
        ((addr(d_store_lens) | addr(d_map)) & 3)) {
        c->err = "pg reduce: store and workspace 16-byte, the records and descriptors 8-byte, the lengths and d_map 4-byte aligned";
        return LSD_ERR_INVALID;
    }
    return enqueue_on(c, stream, [&](hipStream_t s) {
        launch_pg_reduce(d_head, d_nodes, nodes_cap, d_edges, edges_cap, d_tracks, n_tracks, d_store, d_store_lens, store_stride, d_desc, par, d_map,
                         d_rep, d_workspace, s);
        return LSD_OK;
    });
}

int lsd_pg_reduce(lsd_ctx* c, lsd_pg_head* head, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, lsd_pg_track* tracks,
                  int n_tracks, lsd_polar* store, int* store_lens, int store_stride, lsd_pg_desc* desc, lsd_pg_reduce_par par, int32_t* map,
                  lsd_pg_reduce_rep* rep) {
    if (!c || !head || !nodes || !edges || !tracks || !store || !store_lens || !map || !rep) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_stride_bad(c, store_stride) || n_tracks < 1 || pg_reduce_par_bad(par)) return LSD_ERR_INVALID;
    const size_t rows = (size_t)nodes_cap * store_stride;
    lsd_pg_head* d_head; lsd_pg_node* d_no; lsd_pg_edge* d_ed; lsd_pg_track* d_tr; lsd_polar* d_store; int* d_sl; lsd_pg_desc* d_desc = nullptr;
    int32_t* d_map; lsd_pg_reduce_rep* d_rep; uint8_t* d_ws;
    auto plan = [&](StagePass& k) {
        k.both(d_store, store, rows); k.scratch(d_ws, pg_reduce_ws_bytes(nodes_cap, edges_cap, store_stride)); k.both(d_head, head, 1);
        k.both(d_no, nodes, nodes_cap); k.both(d_ed, edges, edges_cap); k.both(d_tr, tracks, n_tracks);
        if (desc) k.both(d_desc, desc, nodes_cap);
        k.out(d_rep, rep, 1); k.both(d_sl, store_lens, nodes_cap); k.out(d_map, map, nodes_cap);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_pg_reduce_device(c, d_head, d_no, nodes_cap, d_ed, edges_cap, d_tr, n_tracks, d_store, d_sl, store_stride, desc ? d_desc : nullptr,
                                            par, d_map, d_rep, d_ws, c->stream);
    });
}

int lsd_pg_recognize_all(lsd_ctx* c, const lsd_pg_desc* desc, int n_nodes, int q_lo, int n_q, lsd_pg_place_par par, lsd_pg_place_rec* recs,
                         lsd_pg_place_rep* reps) {
    if (!c || !desc || pg_nodes_cap_bad(n_nodes) || pg_place_par_bad(par) || pg_queries_bad(q_lo, n_q, n_nodes)) return LSD_ERR_INVALID;
    if (n_q == 0) return LSD_OK;
    if (!recs || !reps) return LSD_ERR_INVALID;
    const size_t nn = (size_t)n_nodes, nq = (size_t)n_q;
    const lsd_pg_head head{n_nodes, 0};
    lsd_pg_head* d_head; lsd_pg_desc* d_desc; lsd_pg_place_rec* d_recs; lsd_pg_place_rep* d_reps;
    auto plan = [&](StagePass& k) { k.in(d_head, &head, 1); k.in(d_desc, desc, nn); k.out(d_recs, recs, nq * par.k); k.out(d_reps, reps, nq); };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_pg_recognize_all_device(c, d_head, n_nodes, d_desc, par, q_lo, n_q, d_recs, d_reps, c->stream);
    });
}

int lsd_pg_loops(lsd_ctx* c, const lsd_pg_place_rec* recs, const lsd_pg_place_rep* reps, int n_q, int k, const lsd_pg_edge* edges, int n_edges,
                 lsd_pg_loops_par par, lsd_pg_loop_rec* loops, lsd_pg_loops_rep* rep) {
    if (!c || !loops || !rep || n_q < 0 || n_q > kPgMaxNodes || n_edges < 0 || n_edges > kPgMaxEdges || pg_loops_par_bad(par, k)) return LSD_ERR_INVALID;
    if ((n_q && (!recs || !reps)) || (n_edges && !edges)) return LSD_ERR_INVALID;
    const int nc = n_q ? n_q : 1, ec = n_edges ? n_edges : 1;              // (a cap is at least 1)
    const size_t nq = (size_t)n_q;
    const lsd_pg_head head{nc, n_edges};
    lsd_pg_head* d_head; lsd_pg_place_rec* d_recs; lsd_pg_place_rep* d_reps; lsd_pg_edge* d_ed; uint8_t* d_ws; lsd_pg_loop_rec* d_loops;
    lsd_pg_loops_rep* d_rep;
    auto plan = [&](StagePass& p) {
        p.in(d_head, &head, 1); p.in(d_recs, recs, nq * k); p.in(d_reps, reps, nq); p.in(d_ed, edges, n_edges); p.scratch(d_ws, pg_loops_ws_bytes(n_q, k, ec));
        p.out(d_loops, loops, par.max_loops); p.out(d_rep, rep, 1);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_pg_loops_device(c, d_recs, d_reps, 0, n_q, k, d_head, nc, d_ed, ec, par, d_ws, d_loops, d_rep, c->stream);
    });
}

int lsd_pg_relax(lsd_ctx* c, lsd_pg_node* nodes, int n_nodes, lsd_pg_edge* edges, int n_edges, lsd_pg_relax_par par, lsd_pg_relax_rep* rep) {
    return pg_relax_host(c, nodes, n_nodes, edges, n_edges, par, nullptr, rep, nullptr);
}

int lsd_pg_relax_robust(lsd_ctx* c, lsd_pg_node* nodes, int n_nodes, lsd_pg_edge* edges, int n_edges, lsd_pg_relax_par par, lsd_pg_robust_par rob,
                        lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep) {
    if (!rob_rep || pg_robust_par_bad(rob)) return LSD_ERR_INVALID;
    return pg_relax_host(c, nodes, n_nodes, edges, n_edges, par, &rob, rep, rob_rep);
}

int lsd_pg_relax_pc(lsd_ctx* c, lsd_pg_node* nodes, int n_nodes, lsd_pg_edge* edges, int n_edges, lsd_pg_relax_par par, lsd_pg_robust_par rob,
                    lsd_pg_precond_par pc, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep, lsd_pg_precond_rep* pc_rep) {
    if (!rob_rep || !pc_rep || pg_robust_par_bad(rob) || pg_precond_par_bad(pc)) return LSD_ERR_INVALID;
    return pg_relax_host(c, nodes, n_nodes, edges, n_edges, par, &rob, rep, rob_rep, &pc, pc_rep);
}

int lsd_pg_append(lsd_ctx* c, const lsd_polar* scans, const int* lens, int n_cand, int stride, const lsd_position* poses, lsd_pg_head* head,
                  lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap, lsd_pg_track* track_rec, int32_t track, lsd_polar* store,
                  int* store_lens, int store_stride, lsd_pg_append_par par, lsd_pg_append_rep* rep) {
    if (!c || !scans || !lens || !poses || !head || !nodes || !edges || !track_rec || !store || !store_lens || !rep) return LSD_ERR_INVALID;
    if (n_cand < 0 || pg_stride_bad(c, stride) || pg_stride_bad(c, store_stride)) return LSD_ERR_INVALID;
    if (pg_caps_bad(nodes_cap, edges_cap) || pg_append_par_bad(par)) return LSD_ERR_INVALID;
    for (int i = 0; i < n_cand; i++) if (lens[i] < 0 || lens[i] > stride) return LSD_ERR_INVALID;
    if (n_cand == 0) return LSD_OK;
    const size_t nc = (size_t)n_cand, rows = (size_t)nodes_cap * store_stride;
    lsd_polar *d_sc, *d_store; int *d_len, *d_sl; lsd_position* d_po; lsd_pg_head* d_head; lsd_pg_node* d_no; lsd_pg_edge* d_ed; lsd_pg_track* d_tr;
    lsd_pg_append_rep* d_rep;
    auto plan = [&](StagePass& k) {
        k.in(d_sc, scans, nc * stride); k.in(d_len, lens, nc); k.in(d_po, poses, nc); k.both(d_head, head, 1); k.both(d_no, nodes, nodes_cap);
        k.both(d_ed, edges, edges_cap); k.both(d_tr, track_rec, 1); k.both(d_store, store, rows); k.both(d_sl, store_lens, nodes_cap); k.out(d_rep, rep, 1);
    };
    return stage_round_trip(c, plan, [&] {
        return lsd_enqueue_pg_append_device(c, d_sc, d_len, n_cand, stride, d_po, sizeof(lsd_position), d_head, d_no, nodes_cap, d_ed, edges_cap, d_tr,
                                            track, d_store, d_sl, store_stride, par, d_rep, c->stream);
    });
}

}  // extern "C"

static int pg_relax_host(lsd_ctx* c, lsd_pg_node* nodes, int n_nodes, lsd_pg_edge* edges, int n_edges, lsd_pg_relax_par par,
                         const lsd_pg_robust_par* rob, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep, const lsd_pg_precond_par* pc,
                         lsd_pg_precond_rep* pc_rep) {
    if (!c || !rep || n_nodes < 0 || n_nodes > kPgMaxNodes || n_edges < 0 || n_edges > kPgMaxEdges || (n_nodes && !nodes) || (n_edges && !edges))
        return LSD_ERR_INVALID;
    if (pg_relax_par_bad(par)) return LSD_ERR_INVALID;
    const int nc = n_nodes ? n_nodes : 1, ec = n_edges ? n_edges : 1;      // (a cap is at least 1)
    const lsd_pg_head head{n_nodes, n_edges};
    lsd_pg_head* d_head; lsd_pg_node* d_no; lsd_pg_edge* d_ed; lsd_pg_relax_rep* d_rep; lsd_pg_robust_rep* d_rob; uint8_t* d_ws;
    lsd_pg_precond_rep* d_pc;
    const size_t ws_bytes = pc ? pg_ws_pc_bytes(nc, ec, pc->kind) : pg_ws_bytes(nc, ec);
    auto plan = [&](StagePass& k) {                                        // (no nodes, no edges: the region of one still has its address)
        k.in(d_head, &head, 1); k.both(d_no, nodes, n_nodes); k.both(d_ed, edges, n_edges); k.out(d_rep, rep, 1); k.scratch(d_ws, ws_bytes);
        k.out(d_rob, rob_rep, 1);
        if (pc) k.out(d_pc, pc_rep, 1);
    };
    return stage_round_trip(c, plan, [&] {
        if (pc) return lsd_enqueue_pg_relax_pc_device(c, 1, d_head, d_no, nc, d_ed, ec, par, *rob, *pc, d_ws, d_rep, d_rob, d_pc, c->stream);
        return rob ? lsd_enqueue_pg_relax_robust_device(c, 1, d_head, d_no, nc, d_ed, ec, par, *rob, d_ws, d_rep, d_rob, c->stream)
                   : lsd_enqueue_pg_relax_device(c, 1, d_head, d_no, nc, d_ed, ec, par, d_ws, d_rep, c->stream);
    });
}
