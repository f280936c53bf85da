// k_posegraph.hip -- the relaxation of pose graphs (lsd_enqueue_pg_relax_device; include/lsd_hip.h, "pose graph", is the rule; DESIGN.md
// 8.1.15; restated in tests/pose_graph_cases.py): Levenberg-Marquardt over SE(2), the linear step by conjugate gradients preconditioned
// with the inverse 3 x 3 diagonal blocks.  ONE WORKGROUP PER GRAPH: every loop is bounded by a parameter, no workgroup waits for another.
// The body is pgrelax_dev.h's, ONE text that is compiled three times: here without and with the robust kernels (kRobust = false is
// lsd_enqueue_pg_relax_device, kRobust = true is lsd_enqueue_pg_relax_robust_device), and in k_pgchain.hip with the
// block-tridiagonal preconditioner beside them (kChain).
#include "pgrelax_dev.h"

namespace lsdhip {

size_t pg_ws_bytes(int nodes_cap, int edges_cap) {
    const size_t b = pg_ws_doubles(nodes_cap, edges_cap) * 8 + pg_ws_words(nodes_cap, edges_cap) * 4;
    return (b + 255) & ~(size_t)255;
}

__global__ __launch_bounds__(kPgLanes) void k_pg_relax(const lsd_pg_head* heads, lsd_pg_node* all_nodes, int nc, lsd_pg_edge* all_edges, int ec,
                                                       lsd_pg_relax_par par, uint8_t* ws_all, size_t ws_bytes, lsd_pg_relax_rep* reps) {
    pg_relax_body<false, false>(heads, all_nodes, nc, all_edges, ec, par, ws_all, ws_bytes, reps, lsd_pg_robust_par{}, nullptr, nullptr);
}

__global__ __launch_bounds__(kPgLanes) void k_pg_relax_robust(const lsd_pg_head* heads, lsd_pg_node* all_nodes, int nc, lsd_pg_edge* all_edges,
                                                              int ec, lsd_pg_relax_par par, uint8_t* ws_all, size_t ws_bytes,
                                                              lsd_pg_relax_rep* reps, lsd_pg_robust_par rp, lsd_pg_robust_rep* rob_reps) {
    pg_relax_body<true, false>(heads, all_nodes, nc, all_edges, ec, par, ws_all, ws_bytes, reps, rp, rob_reps, nullptr);
}

void launch_pg_relax(int n_graphs, const lsd_pg_head* heads, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                     lsd_pg_relax_par par, void* ws, lsd_pg_relax_rep* rep, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_relax, dim3(n_graphs), dim3(kPgLanes), 0, st, heads, nodes, nodes_cap, edges, edges_cap, par,
                       static_cast<uint8_t*>(ws), pg_ws_bytes(nodes_cap, edges_cap), rep);
}

void launch_pg_relax_robust(int n_graphs, const lsd_pg_head* heads, lsd_pg_node* nodes, int nodes_cap, lsd_pg_edge* edges, int edges_cap,
                            lsd_pg_relax_par par, lsd_pg_robust_par rob, void* ws, lsd_pg_relax_rep* rep, lsd_pg_robust_rep* rob_rep, hipStream_t st) {
    hipLaunchKernelGGL(k_pg_relax_robust, dim3(n_graphs), dim3(kPgLanes), 0, st, heads, nodes, nodes_cap, edges, edges_cap, par,
                       static_cast<uint8_t*>(ws), pg_ws_bytes(nodes_cap, edges_cap), rep, rob, rob_rep);
}

}  // namespace lsdhip
