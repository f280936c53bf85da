#!/usr/bin/env python3
"""Developer probe: the reduce of the pose graph (csrc/k_pgreduce.hip), measured, with no threshold.  One JSON line each:

  reduce    lsd_enqueue_pg_reduce_device on a track of 512 / 4096 / 16384 keyframes of 360 beams in which every second keyframe lies where
            the one in front of it lies, so that one node in two is retired: events around the call from a warm context, the median,
            minimum and maximum of REPS calls; head, nodes, edges, track, lengths, descriptors and the store are put back from pristine
            copies in front of the first event, since the reduce works in place.  `rows_moved` and `row_bytes` say what the mover had to
            carry (each row is read and written twice: out to the scratch, in to its place).
  split     (--only split) per size a fresh child process of this probe (`--only reduce --sizes N`) under `rocprofv3 --kernel-trace
            --stats`, its kernel statistics read back: microseconds per call of the ranks (k_pgr_rank), the runs (k_pgr_runs), the rows
            (all launches of k_pgr_rows summed) and the other six launches, and the rows' GB/s -- the mover's traffic over the rows' time.
  before_after  two laps of 2048 keyframes round a circle with a closure every 64 keyframes, 4096 nodes in a PoseGraph: one
            recognize_all_device and one relax_device, then reduce_device (the second lap's keyframes that carry no closure go), then the
            same two calls again.

Usage: tools/pg_reduce_probe.py [--reps 10] [--only reduce,before_after] [--sizes 512,4096,16384] > profiles/pg_reduce_probe.log
       tools/pg_reduce_probe.py --only split >> profiles/pg_reduce_probe.log"""
import argparse, csv, glob, importlib, json, math, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def track_graph(lsd, np, places_xy, headings, closures=(), noise=0.0, seed=0):
    """nodes, edges of one track through the given poses: odometry edges between neighbours (z from the poses plus noise), closure edges."""
    rng = np.random.default_rng(seed)
    n = len(places_xy)
    nodes = np.zeros(n, lsd.PG_NODE_DTYPE)
    nodes["x"], nodes["y"], nodes["ang"] = places_xy[:, 0], places_xy[:, 1], headings
    nodes["raw"] = np.stack([nodes["x"], nodes["y"], nodes["ang"]], axis=1)
    nodes["flags"][0] = lsd.PG_NODE_FIXED
    pairs = [(k, k + 1, 0) for k in range(n - 1)] + [(i, j, lsd.PG_EDGE_CLOSURE) for i, j in closures]
    edges = np.zeros(len(pairs), lsd.PG_EDGE_DTYPE)
    for e, (i, j, fl) in enumerate(pairs):
        a = math.radians(headings[i])
        dx, dy = places_xy[j] - places_xy[i]
        z = (math.cos(a) * dx + math.sin(a) * dy, math.cos(a) * dy - math.sin(a) * dx, (headings[j] - headings[i] + 180.0) % 360.0 - 180.0)
        edges[e] = (i, j, fl, 0, tuple(v + noise * rng.normal() for v in z), (4.0, 0.0, 4.0, 0.0, 0.0, 1.0), 0.0)
    return nodes, edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="reduce,before_after")
    ap.add_argument("--sizes", default="512,4096,16384", help="the node counts of `reduce`, comma separated")
    args = ap.parse_args()
    only = set(args.only.split(","))
    for n in [int(v) for v in args.sizes.split(",")] if "split" in only else ():
        with tempfile.TemporaryDirectory() as out:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "reduce", "--", sys.executable,
                   os.path.abspath(__file__), "--only", "reduce", "--sizes", str(n), "--reps", str(args.reps)]
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = next((json.loads(l) for l in child.stdout.splitlines() if l.startswith("{")), None)
            stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
            if child.returncode != 0 or line is None or not stats:
                print(json.dumps(dict(what="split", nodes=n, error=(child.stderr or child.stdout)[-400:])), flush=True)
                continue
            calls = args.reps + 1                                                 # (the warm call is traced too)
            us = dict(ranks=0.0, runs=0.0, rows=0.0, others=0.0)
            for row in csv.DictReader(open(stats[0])):
                name = row.get("Name") or row.get("KernelName") or ""
                total = float(next(v for k_, v in row.items() if k_.startswith("TotalDuration"))) / 1e3 / calls
                if "k_pgr_" not in name:
                    continue
                us["ranks" if "k_pgr_rank" in name else "runs" if "k_pgr_runs" in name else "rows" if "k_pgr_rows" in name else "others"] += total
            print(json.dumps(dict(what="split", nodes=n, us_per_call=us, us_kernels=sum(us.values()), ms_events=line["ms_median"],
                                  mover_traffic_mb=line["mover_traffic_mb"], rows_gb_per_s=line["mover_traffic_mb"] / 1e3 / (us["rows"] / 1e6) if us["rows"] else None)),
                  flush=True)
    if only <= {"split"}:
        return                                                                # (no GPU work in this process: the children did it)
    import numpy as np
    import torch
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    ctx = lsd.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    beams = 360

    def timed(fn, before=lambda: None, reps=None):
        before(); fn(); torch.cuda.synchronize()                                # warm
        ms = []
        for _ in range(args.reps if reps is None else reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before(); a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    for n in [int(v) for v in args.sizes.split(",")] if "reduce" in only else ():
        rng = np.random.default_rng(n)
        k = np.arange(n)
        xy = np.stack([12.0 * (k // 2) + 2.0, np.full(n, 2.0)], axis=1)           # keyframe 2m + 1 lies where keyframe 2m lies
        xy[-1, 0] += 12.0                                                         # (the track's last keyframe stays: a place of its own)
        nodes, edges = track_graph(lsd, np, xy, np.full(n, 5.0))
        head = np.array([(n, len(edges))], lsd.PG_HEAD_DTYPE)
        track = np.array([(n - 1, 0, (0.0, 0.0, 0.0))], lsd.PG_TRACK_DTYPE)
        lens = np.full(n, beams, np.int32)
        pristine = [dev(head.view(np.uint8)), dev(nodes.view(np.uint8)), dev(edges.view(np.uint8)), dev(track.view(np.uint8)),
                    torch.rand((n, beams, 2), dtype=torch.float64, device="cuda"), dev(lens),
                    torch.randint(1, 255, (n * 72,), dtype=torch.uint8, device="cuda")]
        work = [t.clone() for t in pristine]
        d_map, d_rep = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(48, dtype=torch.uint8, device="cuda")
        d_ws = torch.zeros(lsd.pg_reduce_workspace_bytes(n, len(edges), beams), dtype=torch.uint8, device="cuda")
        par = lsd.pg_reduce(cell=4.0, ang_bin=10.0, keep=1, max_run=64)

        def restore():
            for w_, p_ in zip(work, pristine):
                w_.copy_(p_)
        fn = lambda: ctx.enqueue_pg_reduce_device(work[0].data_ptr(), work[1].data_ptr(), n, work[2].data_ptr(), len(edges), work[3].data_ptr(), 1,
                                                  work[4].data_ptr(), work[5].data_ptr(), beams, work[6].data_ptr(), par, d_map.data_ptr(),
                                                  d_rep.data_ptr(), d_ws.data_ptr(), s)
        med, lo, hi = timed(fn, restore)
        rep = d_rep.cpu().numpy().view(lsd.PG_REDUCE_REP_DTYPE)[0]
        m = d_map.cpu().numpy()
        moved = int(((m >= 0) & (m != np.arange(n))).sum())
        row_bytes = beams * 16
        print(json.dumps(dict(what="reduce", nodes=n, beams=beams, retired=int(rep["retired"]), runs=int(rep["runs"]), nodes_after=int(rep["nodes_after"]),
                              edges_after=int(rep["edges_after"]), ms_median=med, ms_min=lo, ms_max=hi, rows_moved=moved, row_bytes=row_bytes,
                              mover_traffic_mb=4 * moved * row_bytes / 1e6, launches=9 + (n + 1023) // 1024,
                              workspace_mb=d_ws.numel() / 1e6)), flush=True)

    if "before_after" in only:
        lap, n = 2048, 4096
        k = np.arange(n)
        th = 2.0 * math.pi * (k % lap) / lap
        radius = lap * 3.0 / (2.0 * math.pi)
        xy = np.stack([radius + 50.0 + radius * np.cos(th), radius + 50.0 + radius * np.sin(th)], axis=1)
        heading = (np.degrees(th) + 90.0 + 180.0) % 360.0 - 180.0
        closures = [(q, q + lap) for q in range(0, lap, 64)]
        nodes, edges = track_graph(lsd, np, xy, heading, closures, noise=0.02, seed=1)
        graph = lsd.PoseGraph(n, len(edges) + 64, beams, ctx=ctx)
        head = np.array([(n, len(edges))], lsd.PG_HEAD_DTYPE)
        track = np.array([(n - 1, 0, (0.0, 0.0, 0.0))], lsd.PG_TRACK_DTYPE)
        graph._head.copy_(dev(head.view(np.uint8)))
        graph._nodes.copy_(dev(nodes.view(np.uint8).reshape(n, 64)))
        graph._edges[:len(edges)].copy_(dev(edges.view(np.uint8).reshape(len(edges), 96)))
        graph._tracks.copy_(dev(track.view(np.uint8).reshape(1, 32)))
        scan = np.stack([1.0 + 2.0 * np.random.default_rng(2).random((lap, beams)), np.tile(np.linspace(0.0, 2.0 * math.pi, beams, endpoint=False), (lap, 1))],
                        axis=2)
        graph._store.copy_(dev(np.concatenate([scan, scan])))                     # the second lap sees what the first saw
        graph._store_lens.fill_(beams)
        relax = dict(iters=10, cg_iters=300, cg_tol=1e-6, eps=1e-6)
        keep_nodes = graph._nodes.clone()

        def measure(tag):
            rec = timed(lambda: graph.recognize_all_device(4.0))
            rel = timed(lambda: graph.relax_device(relax, precond="chain"), lambda: graph._nodes.copy_(keep_nodes))
            r = graph.report()
            hn, he = graph.head()
            print(json.dumps(dict(what="before_after", when=tag, nodes=hn, edges=he, recognize_all_ms=rec, relax_ms=rel, relax_outer=int(r["iters"]),
                                  relax_cg_steps=int(r["cg_iters"]), chi2_after=float(r["chi2_after"]))), flush=True)
        measure("before")
        graph._nodes.copy_(keep_nodes)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); graph.reduce_device(dict(cell=2.0, ang_bin=10.0, keep=1, max_run=64)); b.record(); torch.cuda.synchronize()
        rep = graph.reduce_report()
        print(json.dumps(dict(what="before_after", when="reduce", ms=a.elapsed_time(b), retired=int(rep["retired"]), runs=int(rep["runs"]),
                              longest_run=int(rep["longest_run"]), dropped_edges=int(rep["dropped_edges"]))), flush=True)
        keep_nodes = graph._nodes.clone()
        measure("after")
    ctx.close()


if __name__ == "__main__":
    main()
