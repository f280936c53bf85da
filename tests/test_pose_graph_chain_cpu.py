"""The relaxation with the block-tridiagonal preconditioner, the restatement alone (tests/pose_graph_chain_cases.py; include/lsd_hip.h,
"pose graph"): the campaign reaches every class, kind BLOCK is the robust relaxation byte for byte, the factor and the
apply solve M z = r, the chain rule ends where the dense reference ends and needs a fraction of the plain rule's CG steps, the records have
the header's sizes and the kernel has no scratch frame.  No GPU."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import pose_graph_cases as pg
import pose_graph_chain_cases as cc
import pose_graph_robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest difference between the restated factor + apply and numpy.linalg.solve on the assembled M, relative to the largest entry of the
# solution, measured on the graphs of cc.well_posed() at their final poses, was 3.5e-14 (loop_256_4).
SOLVE_BOUND = 10 * 3.5e-14
# The largest pose difference (pixels / degrees) between the chain rule and the dense Gauss-Newton on the same graphs was 8.2e-10
# (well_posed_8_1); ten times that covers the libm of another host and CG stopping by cg_tol, as 8.1.15 does.
DENSE_BOUND = 10 * 8.2e-10


def same(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def poses(nodes):
    return np.stack([nodes["x"], nodes["y"], nodes["ang"]], axis=1)


def pose_diff(a, b):
    d = np.abs(a - b)
    d[:, 2] = np.abs([pg.wrap(v) for v in a[:, 2] - b[:, 2]])
    return float(d.max())


def test_campaign_reaches_every_class():
    count = collections.Counter()
    campaign = cc.campaign()
    assert len({c["name"] for c in campaign}) == len(campaign)
    for case in campaign:
        count.update(cc.classes_of(case, cc.run_case(case)[5]))
    short = {c: count[c] for c in cc.CLASSES if count[c] < (1 if c in cc.ONCE_CLASSES else 3)}
    assert not short, short
    assert count["n_1025"] == 1 and count["n_4097"] == 1
    # the fallback's bytes are the plain rule's: an iteration that fell back leaves what kind BLOCK leaves where every iteration did
    fell = [c for c in campaign if all(cc.run_case(c)[5]["fell_back"]) and cc.run_case(c)[5]["fell_back"]]
    assert fell
    for c in fell:
        n, e, rep, rr, _ = cc.relax_pc(c["nodes"], c["edges"], c["par"], c["rob"], cc.BLOCK)
        got = cc.run_case(c)
        assert same(got[0], n) and same(got[1], e) and same(got[2], rep) and same(got[3], rr), c["name"]
        assert int(got[4]["fallbacks"]) == int(rep["iters"])


def test_chain_edges_paths_and_positions_on_a_small_graph():
    """Two tracks interleaved, a chord that loses and a closure between neighbours, by hand."""
    E = lambda i, j, fl=0: pg.edge(i, j, (1.0, 0.0, 0.0), flags=fl)
    edges = np.array([E(0, 2), E(1, 3), E(2, 4), E(5, 3), E(0, 4), E(4, 5, pg.EDGE_CLOSURE), E(4, 6, pg.EDGE_DISABLED)], pg.EDGE_DTYPE)
    valid = [True] * 6 + [False]
    chain, up_edge, before, up, down, cand, lo, hi = cc.chain_of(7, edges, valid)
    assert chain == [True, True, True, True, False, False, False]
    node_at, paths = cc.positions(7, up_edge, before, hi)
    assert paths == [[0, 2, 4], [1, 3, 5], [6]] and node_at == [0, 2, 4, 1, 3, 5, 6]
    tr = {}
    nodes = np.array([pg.node(float(k), 0.0, 0.0, pg.NODE_FIXED if k == 0 else 0) for k in range(7)], pg.NODE_DTYPE)
    pc = cc.relax_pc(nodes, edges, dict(pg.RELAX_DEFAULTS, iters=1), rc.rob(rc.NONE, 0.0), cc.CHAIN, tr)[4]
    assert tuple(pc) == (4, 3, 3, 0)
    assert tuple(cc.relax_pc(nodes[:0], edges[:0], dict(pg.RELAX_DEFAULTS), rc.rob(rc.NONE, 0.0), cc.CHAIN)[4]) == (0, 0, 0, 0)


def test_block_is_the_robust_relaxation_byte_for_byte():
    """The outer loop restated here with kind BLOCK against pose_graph_robust_cases' own, on both of the older campaigns."""
    seen = 0
    for k, case in enumerate(pg.relax_campaign()):
        if len(case["nodes"]) > 257:
            continue
        r = rc.rob(rc.NONE, 0.0, k % 2)
        want = rc.relax_robust(case["nodes"], case["edges"], case["par"], r)
        got = cc.relax_pc(case["nodes"], case["edges"], case["par"], r, cc.BLOCK)
        assert all(same(g, w) for g, w in zip(got[:4], want)), case["name"]
        assert not got[4].tobytes().strip(b"\0"), case["name"]
        seen += 1
    for case in rc.relax_campaign():
        if len(case["nodes"]) > 257:
            continue
        want = rc.run_relax_case(case)[:4]
        got = cc.relax_pc(case["nodes"], case["edges"], case["par"], case["rob"], cc.BLOCK)
        assert all(same(g, w) for g, w in zip(got[:4], want)), case["name"]
        seen += 1
    assert seen >= 80


_well = {}


def well(case):
    if case["name"] not in _well:
        tr = {}
        _well[case["name"]] = cc.relax_pc(case["nodes"], case["edges"], case["par"], case["rob"], cc.CHAIN, tr) + (tr,)
    return _well[case["name"]]


@pytest.mark.parametrize("case", cc.well_posed(), ids=lambda c: c["name"])
def test_factor_and_apply_solve_m(case):
    Dg, Cs = well(case)[5]["last_blocks"]
    F = cc.factor(Dg, Cs)
    assert F is not None
    r = np.random.default_rng(len(Dg)).normal(size=(len(Dg), 3))
    x = np.array(cc.apply(F, [list(v) for v in r]))
    ref = np.linalg.solve(cc.dense_of(Dg, Cs), r.reshape(-1)).reshape(-1, 3)
    diff = float(np.abs(x - ref).max() / np.abs(ref).max())
    print("%s: N = %d, largest difference to numpy.linalg.solve %.3g of the largest entry" % (case["name"], len(Dg), diff))
    assert diff <= SOLVE_BOUND


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 1025))
def test_factor_and_apply_at_the_sizes_of_the_levels(n):
    """A random symmetric positive definite block-tridiagonal matrix at the sizes where a level has and has not an upper neighbour."""
    rng = np.random.default_rng(n)
    Cs = [rng.normal(size=(3, 3)).tolist() for _ in range(n - 1)]
    Dg = []
    for t in range(n):
        A = rng.normal(size=(3, 3))
        Dg.append((A @ A.T + 8.0 * np.eye(3)).tolist())
    F = cc.factor(Dg, Cs)
    r = rng.normal(size=(n, 3))
    x = np.array(cc.apply(F, r.tolist()))
    ref = np.linalg.solve(cc.dense_of(Dg, Cs), r.reshape(-1)).reshape(-1, 3)
    assert float(np.abs(x - ref).max() / np.abs(ref).max()) <= SOLVE_BOUND


@pytest.mark.parametrize("case", cc.well_posed(), ids=lambda c: c["name"])
def test_chain_rule_ends_at_the_dense_minimum(case):
    nodes, _, rep, _, pc, tr = well(case)
    ref = pg.dense_gauss_newton(case["nodes"], case["edges"])
    diff = pose_diff(poses(nodes), ref)
    print("%s: largest pose difference %.3g, %d outer iterations, %d CG steps, %d fallbacks" % (case["name"], diff, rep["iters"], rep["cg_iters"],
                                                                                                pc["fallbacks"]))
    assert rep["flags"] & pg.CONVERGED and int(pc["fallbacks"]) == 0
    assert diff <= DENSE_BOUND
    if case["name"].startswith("loop_"):
        assert max(tr["cg_steps"]) >= 5                                      # four closures: the chain PCG really iterates


def cg_graphs():
    nodes, edges, _ = pg.loop_graph(256, np.random.default_rng(7256), closures=4)
    n2, e2 = cc.interleaved(2, 40, np.random.default_rng(7300), closures=3)
    return (("loop_256_4", nodes, edges), ("interleaved_2x40", n2, e2))


@pytest.mark.parametrize("name,nodes,edges", cg_graphs(), ids=lambda v: v if isinstance(v, str) else "")
def test_chain_needs_at_most_half_the_cg_steps(name, nodes, edges):
    """Four outer iterations with cg_iters = 3 N, which neither rule reaches.  The restatement's own counts:
    loop_256_4: plain 254 + 342 + 328 + 338 = 1262, chain 13 + 13 + 13 + 13 = 52;  interleaved_2x40: plain 99 + 106 + 107 + 114 = 426,
    chain 13 + 13 + 13 + 13 = 52."""
    par = dict(pg.RELAX_DEFAULTS, iters=4, cg_iters=3 * len(nodes), cg_tol=1e-8)
    steps = {}
    for kind in (cc.BLOCK, cc.CHAIN):
        tr = {}
        rep = cc.relax_pc(nodes, edges, par, rc.rob(rc.NONE, 0.0), kind, tr)[2]
        assert "iters" not in tr["cg_ends"] and len(tr["cg_ends"]) == 4 and not any(tr["fell_back"]), (kind, tr["cg_ends"])
        steps[kind] = int(rep["cg_iters"])
        print("%s kind %d: CG steps %s = %d" % (name, kind, tr["cg_steps"], steps[kind]))
    assert steps[cc.CHAIN] > 0 and 2 * steps[cc.CHAIN] <= steps[cc.BLOCK]


def test_struct_sizes_and_names_match_the_header():
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name, size in cc.SIZES.items():
        m = re.search(r"typedef struct %s \{.*?\} %s;[^\n]*" % (name, name), src, re.S)
        assert m, name
        assert int(re.search(r"/\* (\d+) bytes", m.group(0)).group(1)) == size, name
    body = re.search(r"typedef struct lsd_pg_precond_rep \{(.*?)\} lsd_pg_precond_rep;", src, re.S).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == list(cc.PRECOND_REP_DTYPE.names) and cc.PRECOND_REP_DTYPE.itemsize == 16
    assert re.search(r"enum \{ LSD_PG_PRECOND_BLOCK = %d, LSD_PG_PRECOND_CHAIN = %d \}" % (cc.BLOCK, cc.CHAIN), src)
    assert re.search(r"#define LSD_ABI_VERSION 1\b", src)


def test_python_mirror_has_the_same_records(lsdmod):
    import ctypes as C
    assert cc.PRECOND_REP_DTYPE == lsdmod.PG_PRECOND_REP_DTYPE
    assert (lsdmod.PG_PRECOND_BLOCK, lsdmod.PG_PRECOND_CHAIN) == (cc.BLOCK, cc.CHAIN)
    assert (C.sizeof(lsdmod.lsd_pg_precond), lsdmod.lsd_pg_precond.reserved.offset) == (8, 4)
    for name in ("lsd_enqueue_pg_relax_pc_device", "lsd_pg_workspace_pc_bytes", "lsd_pg_relax_pc"):
        assert name in lsdmod.EXPORTED_SYMBOLS
    p = lsdmod.pg_precond("chain")
    assert (p.kind, p.reserved) == (cc.CHAIN, 0) and lsdmod.pg_precond(p) is p
    assert lsdmod.pg_precond().kind == cc.BLOCK and lsdmod.pg_precond(kind="chain").kind == cc.CHAIN and lsdmod.pg_precond(dict(kind=1)).kind == cc.CHAIN
    with pytest.raises(lsdmod.LsdError):
        lsdmod.pg_precond("ilu")
    with pytest.raises(lsdmod.LsdError):
        lsdmod.pg_precond(dict(sort="chain"))
    # sizes need no device: BLOCK is the plain workspace, CHAIN adds 51 doubles and 6 words per node, rounded up to 256 bytes
    plain = lsdmod.pg_workspace_bytes(4096, 4200)
    assert lsdmod.pg_workspace_pc_bytes(4096, 4200, "block") == plain > 0
    assert lsdmod.pg_workspace_pc_bytes(4096, 4200, "chain") == plain + ((4096 * (51 * 8 + 6 * 4) + 255) // 256) * 256
    assert lsdmod.pg_workspace_pc_bytes(4096, 4200, 2) == 0 and lsdmod.pg_workspace_pc_bytes(16385, 4200, "chain") == 0


def test_kernel_stays_out_of_scratch(tmp_path):
    """The compiler's own resource summary of k_pgchain.hip for gfx950: one kernel, no scratch frame."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc", "k_pgchain.hip")
    out = str(tmp_path / "k_pgchain.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True)
    text = open(out).read()
    m = re.search(r"\.set _ZN6lsdhip\d+k_pg_relax_chainE\w*\.private_seg_size, (\d+)", text)
    assert m and int(m.group(1)) == 0
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0", "0"]          # (sincos_g2, which the body calls as k_posegraph.hip's do, and the kernel)
    assert len(re.findall(r"^\s*\.amdhsa_kernel ", text, re.M)) == 1
