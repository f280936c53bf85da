#!/usr/bin/env python3
"""Developer probe: the pose graph (csrc/k_posegraph.hip, csrc/k_pgbuild.hip), measured, with no threshold.  One JSON line each:

  relax     lsd_enqueue_pg_relax_device on closed loops of 64 / 512 / 4096 nodes with one closure per 64 nodes, 1 and 64 graphs per launch:
            events around the launch from a warm context, the median, minimum and maximum of REPS launches.  The nodes are put back from a
            pristine copy in front of the first event, since the update is in place.  The report of graph 0 says what the time bought: outer
            iterations, CG steps, chi2 before and after.
  close     one PoseGraph.close_device chain (near, clear, the store integrated at the selection, likelihood, match + response of one row,
            closure) on a 2048 x 2048 scratch grid, a loop of 64 keyframes of 360 beams in a square room of 160 cells: events around the call.
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
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
