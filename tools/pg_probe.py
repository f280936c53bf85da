#!/usr/bin/env python3
"""Developer probe: the pose graph (csrc/k_posegraph.hip, csrc/k_pgbuild.hip, csrc/k_pgprune.hip, csrc/k_pgplace.hip, csrc/k_pgloops.hip;
DESIGN.md 8.1.15 .. 8.1.18), measured, with no threshold.  One JSON line each:

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
  describe  lsd_enqueue_pg_describe_device on a store of 64 / 4096 / 16384 keyframes of 360 readings: the whole store (every record's valid
            word cleared in front of the first event) and one new row (the last record's alone).
  recognize lsd_enqueue_pg_recognize_device (score + pick) for the last node of the same stores, and lsd_enqueue_pg_near_device on the same
            graphs next to it: events around the launches.
  close_place  one PoseGraph.close_place_device chain (describe, recognize, then close_device's tail) on the graph and the scratch grid of
            `close`.
  loops     (--only loops) on stores of 64 / 4096 / 16384 keyframes with EVERY keyframe as a query: lsd_enqueue_pg_recognize_all_device (one
            launch) beside the same queries put through lsd_enqueue_pg_recognize_device one call each, in the same session; then
            lsd_enqueue_pg_loops_device on the batch's records at max_loops 8 and 64; and one PoseGraph.close_all_device chain (max_loops 8)
            on the graph and the scratch grid of `close`.
  chain     (--only chain) lsd_enqueue_pg_relax_device beside lsd_enqueue_pg_relax_pc_device with the block-tridiagonal preconditioner
             on `relax`'s closed loops of 64 / 512 / 4096 nodes, with one closure per 64 nodes and with 6 closures, 1 and
            64 graphs per launch: the two entries ALTERNATE launch by launch in one session, events around each launch, the median, minimum
            and maximum of REPS launches each.  Per entry: outer iterations, CG steps, microseconds per CG step, and the solves that ended at
            cg_iters -- counted from calls of 1, 2, .. outer iterations, whose reports are each other's beginnings.
  marginals (--only marginals,vet) lsd_enqueue_pg_marginals_device: every node's covariance on the closed loops of 64 / 512 / 4096 nodes by
            both preconditioners, the prepare launch apart, the solve over slots = 1, 16, 256, 1024 on 4096 nodes, one iteration of
            lsd_enqueue_pg_relax_pc_device beside it; vet: one close_all_device chain without and with vet=.

Usage: tools/pg_probe.py [--reps 20] [--only relax,close,optimize,place] > profiles/pg_probe.log
       tools/pg_probe.py --only loops >> profiles/pg_probe.log
       tools/pg_probe.py --only chain >> profiles/pg_probe.log
       tools/pg_probe.py --only marginals,vet >> profiles/pg_probe.log"""
import argparse, importlib, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="relax,close,optimize,place", help="the sections to run, comma separated")
    args = ap.parse_args()
    only = set(args.only.split(","))
    import numpy as np
    import torch
    import pose_graph_cases as pg
    lsd = importlib.import_module("linesegmentdetector-slam_amd")
    ctx = lsd.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn, before=lambda: None, reps=None):
        before(); fn(); torch.cuda.synchronize()                                # warm
        ms = []
        for _ in range(args.reps if reps is None else reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before(); a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    # 1. the relaxation
    par = dict(pg.RELAX_DEFAULTS, iters=10, cg_iters=300, cg_tol=1e-6, eps=1e-6)
    for n in (64, 512, 4096) if "relax" in only else ():
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

    # 1b. the plain entry beside the chain preconditioner, alternating
    for n, closures in [(n, c) for n in (64, 512, 4096) for c in sorted({n // 64, 6})] if "chain" in only else ():
        nodes, edges, _ = pg.loop_graph(n, np.random.default_rng(n), radius=n / 4.0, bias=0.3 * 64 / n, closures=closures)
        for graphs in (1, 64):
            heads = np.zeros(graphs, lsd.PG_HEAD_DTYPE)
            heads["n_nodes"], heads["n_edges"] = len(nodes), len(edges)
            pristine = dev(np.tile(nodes.view(np.uint8), graphs))
            d_no, d_ed, d_hd = pristine.clone(), dev(np.tile(edges.view(np.uint8), graphs)), dev(heads.view(np.uint8))
            d_ws = torch.zeros(graphs * lsd.pg_workspace_pc_bytes(len(nodes), len(edges), "chain"), dtype=torch.uint8, device="cuda")
            d_rp, d_pc = torch.zeros(graphs * 56, dtype=torch.uint8, device="cuda"), torch.zeros(graphs * 16, dtype=torch.uint8, device="cuda")

            def entry(kind, p):
                if kind == "plain":
                    return ctx.enqueue_pg_relax_device(graphs, d_hd.data_ptr(), d_no.data_ptr(), len(nodes), d_ed.data_ptr(), len(edges), d_ws.data_ptr(),
                                                       d_rp.data_ptr(), p, s)
                return ctx.enqueue_pg_relax_pc_device(graphs, d_hd.data_ptr(), d_no.data_ptr(), len(nodes), d_ed.data_ptr(), len(edges), d_ws.data_ptr(),
                                                      d_rp.data_ptr(), "chain", None, None, d_pc.data_ptr(), p, s)
            ms, reps = {"plain": [], "chain": []}, {}
            for k in range(args.reps + 1):                                       # (the first round warms both)
                for kind in ("plain", "chain"):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    d_no.copy_(pristine); a.record(); entry(kind, par); b.record(); torch.cuda.synchronize()
                    if k:
                        ms[kind].append(a.elapsed_time(b))
                    reps[kind] = d_rp.cpu().numpy().view(lsd.PG_RELAX_REP_DTYPE).copy()
            pc = d_pc.cpu().numpy().view(lsd.PG_PRECOND_REP_DTYPE)[0]
            for kind in ("plain", "chain"):
                assert all(r.tobytes() == reps[kind][0].tobytes() for r in reps[kind])
                r, at_cap, before = reps[kind][0], 0, 0
                for it in range(1, int(r["iters"]) + 1):                         # the CG steps of each solve, from calls that stop after `it`
                    d_no.copy_(pristine); entry(kind, dict(par, iters=it)); torch.cuda.synchronize()
                    total = int(d_rp.cpu().numpy().view(lsd.PG_RELAX_REP_DTYPE)[0]["cg_iters"])
                    at_cap += total - before == par["cg_iters"]
                    before = total
                med = float(np.median(ms[kind]))
                print(json.dumps(dict(what="chain", entry=kind, nodes=len(nodes), edges=len(edges), closures=closures, graphs=graphs, ms_median=med,
                                      ms_min=float(min(ms[kind])), ms_max=float(max(ms[kind])), outer=int(r["iters"]), cg_steps=int(r["cg_iters"]),
                                      solves_at_cg_iters=int(at_cap), accepted=int(r["accepted"]), flags=int(r["flags"]),
                                      chi2_before=float(r["chi2_before"]), chi2_after=float(r["chi2_after"]),
                                      us_per_cg_step=1e3 * med / max(int(r["cg_iters"]), 1),
                                      **(dict(chain_edges=int(pc["chain_edges"]), paths=int(pc["paths"]), fallbacks=int(pc["fallbacks"])) if kind == "chain" else {}))),
                      flush=True)

    # 1c. marginal covariances: every node's, by both preconditioners; the prepare launch apart (a call whose one query, the fixed node's,
    # is not solved); the solve over `slots`; one CG step of lsd_enqueue_pg_relax_pc_device on the same graph beside it
    for n in (64, 512, 4096) if "marginals" in only else ():
        nodes, edges, _ = pg.loop_graph(n, np.random.default_rng(n), radius=n / 4.0, bias=0.3 * 64 / n, closures=n // 64)
        head = np.array([(len(nodes), len(edges))], lsd.PG_HEAD_DTYPE)
        d_no, d_ed, d_hd = dev(nodes.view(np.uint8)), dev(edges.view(np.uint8)), dev(head.view(np.uint8))
        every = lsd.pg_queries([(lsd.PG_MARG_NODE, k, 0) for k in range(n)])
        d_rep = torch.zeros(32, dtype=torch.uint8, device="cuda")

        def measure(what, qu, kind, slots, cg_iters=300, **more):
            d_q, d_recs = dev(qu.view(np.uint8)), torch.zeros(len(qu) * 104, dtype=torch.uint8, device="cuda")
            d_ws = torch.zeros(lsd.pg_marginals_workspace_bytes(n, len(edges), kind, slots), dtype=torch.uint8, device="cuda")
            marg = lsd.pg_marg(cg_tol=1e-6, cg_iters=cg_iters, precond=kind, slots=slots)
            fn = lambda: ctx.enqueue_pg_marginals_device(d_hd.data_ptr(), d_no.data_ptr(), n, d_ed.data_ptr(), len(edges), d_q.data_ptr(), len(qu),
                                                         d_ws.data_ptr(), d_recs.data_ptr(), d_rep.data_ptr(), marg, None, s)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()                # (a first call sizes the repetitions: 5 where one takes 0.3 s)
            med, lo, hi = timed(fn, reps=5 if a.elapsed_time(b) > 300.0 else None)
            recs = d_recs.cpu().numpy().view(lsd.PG_MARG_REC_DTYPE)
            solved = recs[(recs["flags"] & 0x777) != 0]
            steps = solved["steps"].reshape(-1) if len(solved) else np.zeros(1)
            rp = d_rep.cpu().numpy().view(lsd.PG_MARG_REP_DTYPE)[0]
            print(json.dumps(dict(what=what, nodes=n, edges=len(edges), precond=kind, queries=len(qu), slots=slots, workgroups=min(slots, len(qu)),
                                  ms_median=med, ms_min=lo, ms_max=hi, steps_per_column_mean=float(steps.mean()), steps_per_column_max=int(steps.max()),
                                  converged=int(((recs["flags"] & 7) == 7).sum()), fallbacks=int(rp["fallbacks"]),
                                  us_per_cg_step_and_workgroup=1e3 * med * min(slots, len(qu)) / max(float(steps.sum()), 1.0), **more)), flush=True)
        for kind in ("block", "chain"):
            measure("marginals_prepare", every[:1], kind, 1)
            measure("marginals_all_nodes", every, kind, 256)
        if n == 4096:
            for slots in (1, 16, 256, 1024):                                     # equal work at every setting: 1024 queries of 3 x 10 steps
                measure("marginals_slots", every[::4].copy(), "chain", slots, cg_iters=10, cg_iters_cap=10)
        d_ws = torch.zeros(lsd.pg_workspace_pc_bytes(n, len(edges), "chain"), dtype=torch.uint8, device="cuda")
        d_rp, pristine = torch.zeros(56, dtype=torch.uint8, device="cuda"), d_no.clone()
        one = dict(pg.RELAX_DEFAULTS, iters=1, cg_iters=300, cg_tol=1e-6, lambda0=0.0, lambda_min=0.0)
        fn = lambda: ctx.enqueue_pg_relax_pc_device(1, d_hd.data_ptr(), d_no.data_ptr(), n, d_ed.data_ptr(), len(edges), d_ws.data_ptr(), d_rp.data_ptr(),
                                                    "chain", None, None, None, one, s)
        med, lo, hi = timed(fn, lambda: d_no.copy_(pristine))
        r = d_rp.cpu().numpy().view(lsd.PG_RELAX_REP_DTYPE)[0]
        print(json.dumps(dict(what="marginals_baseline_relax_pc_one_iteration", nodes=n, edges=len(edges), ms_median=med, ms_min=lo, ms_max=hi,
                              cg_steps=int(r["cg_iters"]), us_per_cg_step=1e3 * med / max(int(r["cg_iters"]), 1))), flush=True)
    if only == {"marginals"}:
        ctx.close()
        return 0

    # 2. place recognition: describe, recognize and near on stores of 360 readings
    for n in (64, 4096, 16384) if "place" in only else ():
        rng = np.random.default_rng(n)
        nodes = np.zeros(n, lsd.PG_NODE_DTYPE)
        nodes["x"], nodes["y"], nodes["ang"] = rng.uniform(0, 2000, n), rng.uniform(0, 2000, n), rng.uniform(-180, 180, n)
        nodes["x"][n - 1], nodes["y"][n - 1] = nodes["x"][n // 4] + 1.0, nodes["y"][n // 4]      # near has a candidate as well
        store = np.stack([rng.uniform(0.5, 30.0, (n, 360)), np.tile(-math.pi + 2 * math.pi * (np.arange(360) + 0.5) / 360, (n, 1))], axis=2)
        store[n // 4, :, 0] = np.roll(store[n - 1, :, 0], 45)                      # the query's scan an eighth of a turn earlier
        head, track = np.array([(n, 0)], lsd.PG_HEAD_DTYPE), np.array([(n - 1, 0, (0.0, 0.0, 0.0))], lsd.PG_TRACK_DTYPE)
        d_hd, d_no, d_tr, d_st, d_ln = dev(head.view(np.uint8)), dev(nodes.view(np.uint8)), dev(track.view(np.uint8)), dev(store), dev(np.full(n, 360, np.int32))
        z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
        d_desc, d_work, d_recs, d_rep, d_near, d_sel = z(n, 72), z(n, dtype=torch.int32), z(8, 16), z(16), z(24), z(n, 3, dtype=torch.float64)
        d_row, d_len, d_pose = z(360, 2, dtype=torch.float64), z(1, dtype=torch.int32), z(3, dtype=torch.float64)
        valid = d_desc.view(torch.int16)[:, 35]                                  # (valid: bytes 70..71 of a record)
        fn = lambda: ctx.enqueue_pg_describe_device(d_hd.data_ptr(), n, d_st.data_ptr(), d_ln.data_ptr(), 360, 30.0, d_desc.data_ptr(), s)
        for what, before in (("describe_all", lambda: valid.zero_()), ("describe_one", lambda: valid[n - 1:].zero_())):
            med, lo, hi = timed(fn, before)
            print(json.dumps(dict(what=what, nodes=n, readings=360, ms_median=med, ms_min=lo, ms_max=hi)), flush=True)
        place = lsd.pg_place(gap=min(10, n // 2), window=2, spread=2, k=4, pick=0, max_dist=2000, min_sectors=32)
        fn = lambda: ctx.enqueue_pg_recognize_device(d_hd.data_ptr(), d_no.data_ptr(), n, d_tr.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), 360,
                                                     d_desc.data_ptr(), place, d_work.data_ptr(), d_recs.data_ptr(), d_rep.data_ptr(), d_near.data_ptr(),
                                                     d_sel.data_ptr(), d_row.data_ptr(), d_len.data_ptr(), d_pose.data_ptr(), s)
        med, lo, hi = timed(fn)
        rec, rep = d_recs.cpu().numpy().reshape(-1).view(lsd.PG_PLACE_REC_DTYPE)[0], d_rep.cpu().numpy().view(lsd.PG_PLACE_REP_DTYPE)[0]
        print(json.dumps(dict(what="recognize", nodes=n, ms_median=med, ms_min=lo, ms_max=hi, anchor=int(rec["anchor"]), shift=int(rec["shift"]),
                              dist=int(rec["dist"]), candidates=int(rep["n_cand"]), planted=n // 4)), flush=True)
        fn = lambda: ctx.enqueue_pg_near_device(d_hd.data_ptr(), d_no.data_ptr(), n, d_tr.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), 360, min(10, n // 2),
                                                10.0, 2, d_near.data_ptr(), d_sel.data_ptr(), d_row.data_ptr(), d_len.data_ptr(), d_pose.data_ptr(), s)
        med, lo, hi = timed(fn)
        nr = d_near.cpu().numpy().view(lsd.PG_NEAR_DTYPE)[0]
        print(json.dumps(dict(what="near", nodes=n, ms_median=med, ms_min=lo, ms_max=hi, anchor=int(nr["anchor"]), candidates=int(nr["n_cand"]))), flush=True)
    # 2b. every keyframe as a query: the batch beside the looped single entry, then the choice of the loops
    for n in (64, 4096, 16384) if "loops" in only else ():
        rng = np.random.default_rng(n)
        desc = np.zeros(n, lsd.PG_DESC_DTYPE)
        desc["v"], desc["n_hits"], desc["n_sectors"], desc["valid"] = rng.integers(0, 256, (n, 64)), 360, 64, 1
        gap = min(10, n // 2)
        for j in range(2 * gap, n, 7):                                            # every seventh keyframe has been seen before, turned
            desc["v"][j] = np.roll(desc["v"][(j * 5) % (j - gap)], j % 64)
        tracks = np.zeros(n, lsd.PG_TRACK_DTYPE)
        tracks["last"] = np.arange(n)
        z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
        d_hd, d_desc, d_tr = dev(np.array([(n, 0)], lsd.PG_HEAD_DTYPE).view(np.uint8)), dev(desc.view(np.uint8)), dev(tracks.view(np.uint8))
        d_no, d_st, d_ln = z(n, 64), z(n, 1, 2, dtype=torch.float64), z(n, dtype=torch.int32)
        k = 4
        place = lsd.pg_place(gap=gap, window=2, spread=2, k=k, pick=0, max_dist=2000, min_sectors=32)
        d_recs, d_reps, d_recs1, d_reps1 = z(n * k, 16), z(n, 16), z(n * k, 16), z(n, 16)
        d_work, d_near, d_sel, d_row, d_len, d_pose = z(n, dtype=torch.int32), z(24), z(n, 3, dtype=torch.float64), z(1, 2, dtype=torch.float64), z(1, dtype=torch.int32), z(3, dtype=torch.float64)
        batch = lambda: ctx.enqueue_pg_recognize_all_device(d_hd.data_ptr(), n, d_desc.data_ptr(), place, 0, n, d_recs.data_ptr(), d_reps.data_ptr(), s)

        def looped():
            for q in range(n):
                ctx.enqueue_pg_recognize_device(d_hd.data_ptr(), d_no.data_ptr(), n, d_tr.data_ptr() + 32 * q, d_st.data_ptr(), d_ln.data_ptr(), 1,
                                                d_desc.data_ptr(), place, d_work.data_ptr(), d_recs1.data_ptr() + 16 * k * q, d_reps1.data_ptr() + 16 * q,
                                                d_near.data_ptr(), d_sel.data_ptr(), d_row.data_ptr(), d_len.data_ptr(), d_pose.data_ptr(), s)
        med, lo, hi = timed(batch)
        med1, lo1, hi1 = timed(looped)
        equal = bool(torch.equal(d_recs, d_recs1) and torch.equal(d_reps, d_reps1))
        print(json.dumps(dict(what="recognize_all", nodes=n, queries=n, k=k, ms_median=med, ms_min=lo, ms_max=hi, looped_single_ms_median=med1,
                              looped_single_ms_min=lo1, looped_single_ms_max=hi1, speedup=med1 / med, same_bytes=equal,
                              pairs=int((d_recs.cpu().numpy().reshape(-1).view(lsd.PG_PLACE_REC_DTYPE)["anchor"] >= 0).sum()))), flush=True)
        ecap = 4 * n
        d_ed, d_ws, d_loops, d_lrep = z(ecap, 96), z(lsd.pg_loops_workspace_bytes(n, k, ecap)), z(64, 16), z(16)
        d_hd2 = dev(np.array([(n, n - 1 + n // 64)], lsd.PG_HEAD_DTYPE).view(np.uint8))
        ed = np.zeros(ecap, lsd.PG_EDGE_DTYPE)
        ed["i"][:n - 1], ed["j"][:n - 1] = np.arange(n - 1), np.arange(1, n)
        for c in range(n // 64):                                                  # one closure per 64 nodes that the graph already has
            ed[n - 1 + c] = (c * 64 // 2, c * 64 + 63, lsd.PG_EDGE_CLOSURE, 0, (0, 0, 0), (1, 0, 1, 0, 0, 1), 0)
        d_ed.copy_(dev(ed.view(np.uint8).reshape(ecap, 96)))
        for max_loops in (8, 64):
            lp = lsd.pg_loops(max_loops=max_loops, spread=2)
            fn = lambda: ctx.enqueue_pg_loops_device(d_recs.data_ptr(), d_reps.data_ptr(), 0, n, k, d_hd2.data_ptr(), n, d_ed.data_ptr(), ecap, lp,
                                                     d_ws.data_ptr(), d_loops.data_ptr(), d_lrep.data_ptr(), s)
            med, lo, hi = timed(fn)
            r = d_lrep.cpu().numpy().view(lsd.PG_LOOPS_REP_DTYPE)[0]
            print(json.dumps(dict(what="find_loops", nodes=n, records=n * k, edges=int(n - 1 + n // 64), max_loops=max_loops, ms_median=med, ms_min=lo,
                                  ms_max=hi, pairs=int(r["n_pairs"]), known=int(r["n_known"]), loops=int(r["n_loops"]))), flush=True)
    if not only & {"close", "optimize", "place", "loops", "vet"}:
        ctx.close()
        return 0

    # 3. one close_device chain on a 2048 x 2048 scratch grid
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
    if "place" in only:
        place = dict(gap=n_key // 2, window=2, spread=2, k=4, pick=0, max_dist=2000, min_sectors=32)
        fp = lambda: graph.close_place_device(scratch, place=place, search=search, response=dict(rx=2, ry=2, ra=1))
        med, lo, hi = timed(fp, restore)
        near, rep = graph.closure_report()
        rec = graph.place_records()[0]
        print(json.dumps(dict(what="close_place", grid=[cols, rows], keyframes=int(graph.head()[0]), beams=n_beams, place=place, search=search,
                              ms_median=med, ms_min=lo, ms_max=hi, anchor=int(near["anchor"]), shift=int(rec["shift"]), dist=int(rec["dist"]),
                              query=int(near["query"]), candidates=int(near["n_cand"]), closure_flags=int(rep["flags"]))), flush=True)
        restore()
    if "loops" in only:
        place = dict(gap=n_key // 2, window=2, spread=2, k=4, pick=0, max_dist=2000, min_sectors=32)
        fa = lambda: graph.close_all_device(scratch, place=place, loops=dict(max_loops=8, spread=2), search=search, response=dict(rx=2, ry=2, ra=1))
        med, lo, hi = timed(fa, restore)
        rep, (nears, creps) = graph.loops_report(), graph.closure_reports()
        print(json.dumps(dict(what="close_all", grid=[cols, rows], keyframes=int(graph.head()[0]), beams=n_beams, place=place, max_loops=8, search=search,
                              ms_median=med, ms_min=lo, ms_max=hi, pairs=int(rep["n_pairs"]), known=int(rep["n_known"]), loops=int(rep["n_loops"]),
                              anchors=[int(v) for v in nears["anchor"]], queries=[int(v) for v in nears["query"]],
                              closure_flags=[int(v) for v in creps["flags"]])), flush=True)
        restore()
    if "vet" in only:                                                           # one close_all_device chain without and with vet=
        place = dict(gap=n_key // 2, window=2, spread=2, k=4, pick=0, max_dist=2000, min_sectors=32)
        for vet in (None, dict(gate=16.27, marg=dict(cg_tol=1e-8, cg_iters=200, precond="chain", slots=256))):
            fa = lambda: graph.close_all_device(scratch, place=place, loops=dict(max_loops=8, spread=2), search=search, response=dict(rx=2, ry=2, ra=1),
                                                vet=vet)
            med, lo, hi = timed(fa, restore)
            more = {}
            if vet:
                vr, mr = graph.vet_reports(), graph.marginal_records()
                more = dict(vet_flags=[int(v) for v in vr["flags"]], d2=[float(v) for v in vr["d2"]], steps=[[int(x) for x in r["steps"]] for r in mr])
            print(json.dumps(dict(what="close_all_vet" if vet else "close_all_no_vet", keyframes=int(graph.head()[0]), max_loops=8, ms_median=med, ms_min=lo,
                                  ms_max=hi, closure_flags=[int(v) for v in graph.closure_reports()[1]["flags"]], **more)), flush=True)
            restore()
    if not only & {"close", "optimize"}:
        ctx.close()
        return 0
    med, lo, hi = timed(fn, restore)
    near, rep = graph.closure_report()
    print(json.dumps(dict(what="close", grid=[cols, rows], keyframes=int(graph.head()[0]), beams=n_beams, window=2, search=search, ms_median=med,
                          ms_min=lo, ms_max=hi, anchor=int(near["anchor"]), query=int(near["query"]), candidates=int(near["n_cand"]),
                          closure_flags=int(rep["flags"]))), flush=True)

    # 4. one optimize_device chain on that graph: its closure stays, a false one 10 -> 40 is written behind it
    if "optimize" not in only:
        ctx.close()
        return 0
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
