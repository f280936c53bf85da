// k_pgchain.hip -- the relaxation of pose graphs with the block-tridiagonal preconditioner (lsd_enqueue_pg_relax_pc_device with
// LSD_PG_PRECOND_CHAIN; include/lsd_hip.h, "pose graph", is the rule; restated in tests/pose_graph_chain_cases.py).
// The body is pgrelax_dev.h's, the text k_posegraph.hip compiles, with kRobust and kChain set: M is the part of the damped normal matrix
// along the odometry chains, factored by block cyclic reduction once per outer iteration and applied wherever the rule says z = M^-1 r.
// ONE WORKGROUP PER GRAPH, the factor and the apply out of the workspace: one barrier per level and direction of an apply, two per level
// of the factor (the eliminated positions, then the positions that stay).
#include "pgrelax_dev.h"

namespace lsdhip {

size_t pg_ws_pc_bytes(int nodes_cap, int edges_cap, int kind) {
    return pg_ws_bytes(nodes_cap, edges_cap) + (kind == LSD_PG_PRECOND_CHAIN ? pg_chain_ws_bytes(nodes_cap) : 0);
}

__global__ __launch_bounds__(kPgLanes) void k_pg_relax_chain(const lsd_pg_head* heads, lsd_pg_node* all_nodes, int nc, lsd_pg_edge* all_edges,
                                                             int ec, lsd_pg_relax_par par, uint8_t* ws_all, size_t ws_bytes,
                                                             lsd_pg_relax_rep* reps, lsd_pg_robust_par rp, lsd_pg_robust_rep* rob_reps,
                                                             lsd_pg_precond_rep* pc_reps) {
    pg_relax_body<true, true>(heads, all_nodes, nc, all_edges, ec, par, ws_all, ws_bytes, reps, rp, rob_reps, pc_reps);
}

void launch_pg_relax_chain(int n_graphs, const lsd_pg_head* heads, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                           lsd_pg_relax_par par, lsd_pg_robust_par rob, void* ws, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep,
                           lsd_pg_precond_rep* pc_rep, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_relax_chain, dim3(n_graphs), dim3(kPgLanes), 0, st, heads, nodes, nodes_cap, edges, edges_cap, par,
                       static_cast<uint8_t*>(ws), pg_ws_pc_bytes(nodes_cap, edges_cap, LSD_PG_PRECOND_CHAIN), rep, rob, rob_rep, pc_rep);
}

}  // namespace lsdhip
