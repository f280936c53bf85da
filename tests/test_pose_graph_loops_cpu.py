"""Every loop of a track in one pass: the restatement alone (tests/pose_graph_loops_cases.py; include/lsd_hip.h, "pose graph"; DESIGN.md
8.1.18).  The campaigns reach every class, the batch is the single entry query by query, the choice of the loops agrees with a plain
sort-and-filter, the two-lap fixture holds its conditions, the records have the header's sizes and the new kernels need no scratch.  No GPU."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import pose_graph_cases as pg
import pose_graph_loops_cases as pl
import pose_graph_place_cases as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_campaign_reaches_every_class():
    count = collections.Counter()
    for case in pl.batch_campaign() + pl.batch_campaign(big=True):
        count.update(pl.batch_classes_of(case, pl.run_batch_case(case)[1]))
    short = {c: count[c] for c in pl.BATCH_CLASSES + pl.BATCH_ONCE if count[c] < (1 if c in pl.BATCH_ONCE else 3)}
    assert not short, short


def test_loops_and_select_campaigns_reach_every_class():
    count = collections.Counter()
    for case in pl.loops_campaign():
        count.update(pl.loops_classes_of(case, pl.run_loops_case(case)[1]))
    short = {c: count[c] for c in pl.LOOPS_CLASSES if count[c] < 3}
    assert not short, short
    count = collections.Counter()
    for case in pl.select_campaign():
        assert case["ms"]
        for m in case["ms"]:
            count.update(pl.select_classes_of(case, m))
    short = {c: count[c] for c in pl.SELECT_CLASSES if count[c] < 3}
    assert not short, short


def test_recognize_all_is_the_single_entry_query_by_query():
    """On the whole campaign: row q is what recognize writes with the track's last at q_lo + q, and the rows behind the range keep their
    bytes."""
    for case in pl.batch_campaign() + pl.batch_campaign(big=True):
        (recs, reps), _ = pl.run_batch_case(case)
        g = pg.copy_graph(case["graph"])
        nq = case["n_q"]
        assert recs[nq:].tobytes() == case["recs"][nq:].tobytes() and reps[nq:].tobytes() == case["reps"][nq:].tobytes(), case["name"]
        step = max(1, nq // 6)                                                # (the restatement is deterministic: a sample says it again)
        for q in list(range(0, nq, step)) + ([nq - 1] if nq else []):
            g["tracks"][0]["last"] = case["q_lo"] + q
            _, r, rep, *_ = pp.recognize(g, 0, case["desc"], case["par"], np.zeros(len(g["nodes"]), np.uint32), np.zeros((g["store"].shape[1], 2)))
            assert recs[q].tobytes() == r.tobytes() and reps[q].tobytes() == rep.tobytes(), (case["name"], q)
            assert int(reps[q]["query"]) == case["q_lo"] + q


def test_the_choice_of_loops_against_a_plain_sort_and_filter():
    for case in pl.loops_campaign():
        (loops, rep), _ = pl.run_loops_case(case)
        kept = pl.loops_by_sorting(case["recs"], case["reps"], case["n_q"], case["head_edges"], case["edges"], case["par"])
        n = int(rep["n_loops"])
        assert n == len(kept), case["name"]
        assert [tuple(int(v) for v in l) for l in loops[:n]] == kept, case["name"]
        assert all(tuple(int(v) for v in l) == (-1, -1, 0, 0) for l in loops[n:]), case["name"]
        assert 0 <= int(rep["n_known"]) <= int(rep["n_pairs"]) and int(rep["reserved"]) == 0


def test_select_is_recognizes_tail():
    """For a loop whose records came from a batch, the selection equals what recognize leaves for that query and that anchor."""
    seen = 0
    for case in pl.select_campaign():
        g = pg.copy_graph(case["graph"])
        for m in case["ms"]:
            near, sel, row, q_len, q_pose = pl.run_select_case(case, m)
            L = case["loops"][m]
            if int(L["query"]) < 0:
                assert int(near["anchor"]) == -1 and q_len == 0 and tuple(q_pose) == pg.SENTINEL and (sel == np.array(pg.SENTINEL)).all()
                assert (row == 0.125).all()
                continue
            n_nodes = pg.clamp(g["head"][0]["n_nodes"], len(g["nodes"]))
            j, a = int(L["query"]), int(L["anchor"])
            pa = pg.pose_of(g["nodes"][a])
            want = pp.leave_for_anchor(g, j, n_nodes, a, case["gap"], case["window"], np.full_like(row, 0.125),
                                       (pa[0], pa[1], pg.wrap(pa[2] - int(L["shift"]) * 5.625)))
            assert want[0].tobytes() == sel.tobytes() and want[1].tobytes() == row.tobytes() and want[2] == q_len
            assert want[3].tobytes() == q_pose.tobytes()
            assert (int(near["query"]), int(near["n_cand"]), float(near["d2"])) == (j, int(case["loops_rep"]["n_loops"]), float(int(L["dist"])))
            seen += 1
    assert seen >= 9


def test_end_to_end_closes_every_loop_of_two_laps():
    E = pl.end_to_end()
    n, gap = E["n_nodes"], pl.E2E["place"]["gap"]
    T = E["truth"]
    assert n == 48
    # 1. close_place_device at the end of the track appends exactly one closure
    assert int(E["single_closure_rep"]["flags"]) == pg.APPENDED
    assert int(E["single"]["head"][0]["n_edges"]) == int(E["g1"]["head"][0]["n_edges"]) + 1
    # 2. find_loops at max_loops = 8, spread = 2 fills at least four rounds
    assert (pl.E2E["loops"]["max_loops"], pl.E2E["loops"]["spread"]) == (8, 2)
    n_loops = int(E["loops_rep"]["n_loops"])
    assert n_loops >= 4
    # 3. every filled loop's anchor is within one index of the true nearest old node of its query
    for L in E["loops"][:n_loops]:
        j = int(L["query"])
        true_nearest = int(np.argmin(np.hypot(T[:j - gap + 1, 0] - T[j, 0], T[:j - gap + 1, 1] - T[j, 1])))
        assert abs(int(L["anchor"]) - true_nearest) <= 1, (j, int(L["anchor"]), true_nearest)
    # 4. every filled loop's closure is appended
    assert all(int(f) == pg.APPENDED for f in E["closure_reps"]["flags"][:n_loops])
    assert all(int(f) == pg.NO_ANCHOR for f in E["closure_reps"]["flags"][n_loops:])
    assert E["n_edges"] == int(E["g1"]["head"][0]["n_edges"]) + n_loops

    # 5. the relaxation with all loops beats the one with the single closure, which beats none
    def mean_error(nodes):
        return float(np.mean(np.hypot(nodes["x"][:n] - T[:n, 0], nodes["y"][:n] - T[:n, 1])))
    before, single, every = mean_error(E["g1"]["nodes"]), mean_error(E["single_relaxed"]["nodes"]), mean_error(E["g3"]["nodes"])
    print("loops: %d filled %s; mean keyframe error %.4f (odometry) -> %.4f (one closure) -> %.4f (all loops) pixels"
          % (n_loops, [(int(L["query"]), int(L["anchor"])) for L in E["loops"][:n_loops]], before, single, every))
    assert every < single < before
    pa, hi = E["planes"]
    assert pa.shape == (pp.PLACE_ROOM["rows"], pp.PLACE_ROOM["cols"]) and hi.sum() > 0


def test_struct_sizes_match_the_header_and_the_python_mirror(lsdmod):
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name, size in pl.SIZES.items():
        m = re.search(r"typedef struct %s\s+\{.*?\} %s;[^\n]*" % (name, name), src, re.S)
        assert m, name
        assert int(re.search(r"/\* (\d+) bytes", m.group(0)).group(1)) == size, name
    assert (pl.LOOP_REC_DTYPE.itemsize, pl.LOOPS_REP_DTYPE.itemsize) == (16, 16)
    assert re.search(r"#define LSD_PG_LOOPS_MAX 64\b", src) and lsdmod.PG_LOOPS_MAX == pl.LOOPS_MAX
    assert (pl.LOOP_REC_DTYPE, pl.LOOPS_REP_DTYPE) == (lsdmod.PG_LOOP_REC_DTYPE, lsdmod.PG_LOOPS_REP_DTYPE)
    import ctypes as C
    assert C.sizeof(lsdmod.lsd_pg_loops) == pl.SIZES["lsd_pg_loops_par"]
    assert [f for f, _ in lsdmod.lsd_pg_loops._fields_] == list(pl.LOOPS_KEYS)
    assert lsdmod.PG_LOOPS_DEFAULTS == pl.LOOPS_DEFAULTS
    for name in ("lsd_enqueue_pg_recognize_all_device", "lsd_enqueue_pg_loops_device", "lsd_enqueue_pg_loop_select_device",
                 "lsd_pg_loops_workspace_bytes", "lsd_pg_recognize_all", "lsd_pg_loops"):
        assert name in lsdmod.EXPORTED_SYMBOLS
    p = lsdmod.pg_loops(dict(max_loops=3), spread=5)
    assert (p.max_loops, p.spread) == (3, 5)
    p = lsdmod.pg_loops()
    assert (p.max_loops, p.spread) == (8, 2)
    assert re.search(r"#define LSD_ABI_VERSION 1\b", src)


def test_kernels_stay_out_of_scratch(tmp_path):
    """The compiler's own resource summary of k_pgloops.hip for gfx950: five kernels, none with a scratch frame, the batch kernel with the
    single entry's packed byte SAD (16 per shift, 64 shifts)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc", "k_pgloops.hip")
    out = str(tmp_path / "k_pgloops.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True)
    text = open(out).read()
    names = ("k_pg_recognize_all", "k_pg_loops_closures", "k_pg_loops_mark", "k_pg_loops_pick", "k_pg_loop_select")
    found = {}
    for name in names:
        m = re.search(r"\.set _ZN6lsdhip\d+%sE\w*\.private_seg_size, (\d+)" % name, text)
        assert m, name
        found[name] = int(m.group(1))
    assert found == dict.fromkeys(names, 0), found
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0"] * len(names)
    assert "flat_load" not in text                                          # every row and record is read in its own address space
    assert text.count("v_sad_u8") == 64 * 16
