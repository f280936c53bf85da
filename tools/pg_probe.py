#!/usr/bin/env python3
"""Developer probe: the pose graph (csrc/k_posegraph.hip, csrc/k_pgbuild.hip, csrc/k_pgprune.hip), measured, with no
threshold.  One JSON line each:

  relax     lsd_enqueue_pg_relax_device on closed loops of 64 / 512 / 4096 nodes with one closure per 64 nodes, 1 and 64 graphs per launch:
            events around the launch from a warm context, the median, minimum and maximum of REPS launches.  The nodes are put back from a
            pristine copy in front of the first event, since the update is in place.  The report of graph 0 says what the time bought: outer
            iterations, CG steps, chi2 before and after.
  robust    lsd_enqueue_pg_relax_robust_device on the same graphs and settings, Huber (delta 1) and Geman-McClure (delta 3) on the closures:
            the same figures and the robust report of graph 0.
  close     one PoseGraph.close_device chain (near, clear, the store integrated at the selection, likelihood, match + response of one row,
            closure) on a 2048 x 2048 scratch grid, a loop of 64 keyframes of 360 beams in a square room of 160 cells: events around the call.
  optimize  one PoseGraph.optimize_device chain (robust relaxation, prune, refit) on that graph of 65 keyframes after its closure, with a
            false closure 10 -> 40 written into the edge tensor: events around the call, and what the three reports say.
Usage: tools/pg_probe.py [--reps 20] > profiles/pg_probe.log"""
import argparse, importlib, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import pose_graph_cases as pg
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    ctx = lsd.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn, before=lambda: None):
        before(); fn(); torch.cuda.synchronize()                                # warm
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before(); a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    # 1. the relaxation
    par = dict(pg.RELAX_DEFAULTS, iters=10, cg_iters=300, cg_tol=1e-6, eps=1e-6)
    for n in (64, 512, 4096):
        nodes, edges, _ = pg.loop_graph(n, np.random.default_rng(n), radius=n / 4.0, bias=0.3 * 64 / n, closures=n // 64)
        for graphs in (1, 64):
            heads = np.zeros(graphs, lsd.PG_HEAD_DTYPE)
            heads["n_nodes"], heads["n_edges"] = len(nodes), len(edges)
            pristine = dev(np.tile(nodes.view(np.uint8), graphs))
            d_no, d_ed, d_hd = pristine.clone(), dev(np.tile(edges.view(np.uint8), graphs)), dev(heads.view(np.uint8))
            d_ws = torch.zeros(graphs * lsd.pg_workspace_bytes(len(nodes), len(edges)), dtype=torch.uint8, device="cuda")
            d_rp = torch.zeros(graphs * 56, dtype=torch.uint8, device="cuda")
            fn = lambda: ctx.enqueue_pg_relax_device(graphs, d_hd.data_ptr(), d_no.data_ptr(), len(nodes), d_ed.data_ptr(), len(edges), d_ws.data_ptr(),
                                                     d_rp.data_ptr(), par, s)
            med, lo, hi = timed(fn, lambda: d_no.copy_(pristine))
            rep = d_rp.cpu().numpy().view(lsd.PG_RELAX_REP_DTYPE)
            assert all(r.tobytes() == rep[0].tobytes() for r in rep)            # equal graphs, equal bytes
            r = rep[0]
            print(json.dumps(dict(what="relax", nodes=len(nodes), edges=len(edges), graphs=graphs, ms_median=med, ms_min=lo, ms_max=hi,
                                  outer=int(r["iters"]), cg_steps=int(r["cg_iters"]), accepted=int(r["accepted"]), flags=int(r["flags"]),
                                  chi2_before=float(r["chi2_before"]), chi2_after=float(r["chi2_after"]),
                                  us_per_cg_step=1e3 * med / max(int(r["cg_iters"]), 1))), flush=True)
            d_rr = torch.zeros(graphs * 24, dtype=torch.uint8, device="cuda")
            for kernel, delta in (("huber", 1.0), ("gm", 3.0)):
                rob = lsd.pg_robust(kernel=kernel, delta=delta)
                fn = lambda: ctx.enqueue_pg_relax_robust_device(graphs, d_hd.data_ptr(), d_no.data_ptr(), len(nodes), d_ed.data_ptr(), len(edges),
                                                                d_ws.data_ptr(), d_rp.data_ptr(), rob, d_rr.data_ptr(), par, s)
                med, lo, hi = timed(fn, lambda: d_no.copy_(pristine))
                r, rr = d_rp.cpu().numpy().view(lsd.PG_RELAX_REP_DTYPE)[0], d_rr.cpu().numpy().view(lsd.PG_ROBUST_REP_DTYPE)[0]
                print(json.dumps(dict(what="robust", kernel=kernel, delta=delta, nodes=len(nodes), edges=len(edges), graphs=graphs, ms_median=med,
                                      ms_min=lo, ms_max=hi, outer=int(r["iters"]), cg_steps=int(r["cg_iters"]), accepted=int(r["accepted"]),
                                      flags=int(r["flags"]), cost_before=float(r["chi2_before"]), cost_after=float(r["chi2_after"]),
                                      chi2_plain=float(rr["chi2_plain"]), downweighted=int(rr["downweighted"]), w_min=float(rr["w_min"]),
                                      us_per_cg_step=1e3 * med / max(int(r["cg_iters"]), 1))), flush=True)

    # 2. one close_device chain on a 2048 x 2048 scratch grid
    cols = rows = 2048
    resol, range_max, n_key, n_beams = 0.05, 60.0, 64, 360
    lo_w, hi_w = 944.0, 1104.0                                                  # the room's walls, in cells

    def room_scan(p):
        out = []
        for k in range(n_beams):
            a = -math.pi + 2 * math.pi * (k + 0.5) / n_beams
            th = a + math.radians(p[2])
            c, sn = math.cos(th), math.sin(th)
            ts = [(hi_w - p[0]) / c if c > 0 else (lo_w - p[0]) / c if c < 0 else math.inf, (hi_w - p[1]) / sn if sn > 0 else (lo_w - p[1]) / sn if sn < 0 else math.inf]
            out.append((min(t for t in ts if t > 0) * resol, a))
        return np.array(out)
    truth = [(1024.0 + 40.0 * math.cos(2 * math.pi * k / n_key), 1024.0 + 40.0 * math.sin(2 * math.pi * k / n_key), pg.wrap(360.0 * k / n_key + 90.0))
             for k in range(n_key + 1)]
    rng, odom = np.random.default_rng(3), [truth[0]]
    for k in range(1, n_key + 1):
        z = pg.rel(truth[k - 1], truth[k])
        odom.append(pg.comp(odom[-1], (z[0] + 0.05 * rng.normal(), z[1] + 0.05 * rng.normal(), z[2] + 0.05)))
    scans = np.stack([room_scan(p) for p in truth])
    graph = lsd.PoseGraph(n_key + 8, n_key + 16, n_beams, ctx=ctx)
    scratch = lsd.GridMapper(cols, rows, resol, 0.0, 0.0, range_max, ctx=ctx)
    graph.append_device(dev(scans), dev(np.full(n_key + 1, n_beams, np.int32)), dev(np.array(odom)), append=dict(min_dist=2.0))
    search = dict(wx=12, wy=12, na=8, ang_step=0.5, min_beams=30, min_num=1, min_den=8)
    pristine = graph._edges.clone(), graph._head.clone()

    def restore():
        graph._edges.copy_(pristine[0]); graph._head.copy_(pristine[1])
    fn = lambda: graph.close_device(scratch, gap=n_key // 2, radius=10.0, window=2, search=search, response=dict(rx=2, ry=2, ra=1))
    med, lo, hi = timed(fn, restore)
    near, rep = graph.closure_report()
    print(json.dumps(dict(what="close", grid=[cols, rows], keyframes=int(graph.head()[0]), beams=n_beams, window=2, search=search, ms_median=med,
                          ms_min=lo, ms_max=hi, anchor=int(near["anchor"]), query=int(near["query"]), candidates=int(near["n_cand"]),
                          closure_flags=int(rep["flags"]))), flush=True)

    # 3. one optimize_device chain on that graph: its closure stays, a false one 10 -> 40 is written behind it
    n_nodes, n_edges = graph.head()
    false = pg.edge(10, 40, tuple(v + o for v, o in zip(pg.rel(truth[10], truth[40]), (6.0, -5.0, 25.0))), (25.0, 0.0, 25.0, 0.0, 0.0, 9.0), lsd.PG_EDGE_CLOSURE)
    graph._edges[n_edges:n_edges + 1].copy_(dev(np.array([false], lsd.PG_EDGE_DTYPE).view(np.uint8).reshape(1, -1)))
    graph._head.copy_(dev(np.array([(n_nodes, n_edges + 1)], lsd.PG_HEAD_DTYPE).view(np.uint8).reshape(-1)))
    pristine = graph._edges.clone(), graph._nodes.clone()

    def restore2():
        graph._edges.copy_(pristine[0]); graph._nodes.copy_(pristine[1])
    relax = dict(iters=20, cg_iters=3 * n_nodes)
    fn = lambda: graph.optimize_device(dict(kernel="huber", delta=1.0), 11.345, relax=relax)
    med, lo, hi = timed(fn, restore2)
    rr, pr, rf = graph.robust_report(), graph.prune_report(), graph.report()
    print(json.dumps(dict(what="optimize", keyframes=n_nodes, edges=n_edges + 1, kernel="huber", delta=1.0, gate=11.345, relax=relax, ms_median=med,
                          ms_min=lo, ms_max=hi, downweighted=int(rr["downweighted"]), w_min=float(rr["w_min"]), candidates=int(pr["candidates"]),
                          rejected=int(pr["rejected"]), worst_edge=int(pr["worst_edge"]), worst_chi2=float(pr["worst_chi2"]),
                          closures_left=int(pr["closures_left"]), refit_outer=int(rf["iters"]), refit_cg_steps=int(rf["cg_iters"]),
                          refit_chi2=float(rf["chi2_after"]))), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
