"""Place recognition's restatement alone (tests/pose_graph_place_cases.py; include/lsd_hip.h, "pose graph"): the campaigns
reach every class, the distance agrees with a plain triple loop, a turned scan gives the shift and the heading the rule says, the end-to-end
fixture is a loop that pose proximity cannot see and appearance closes, and the records have the header's sizes.  No GPU."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import pose_graph_cases as pg
import pose_graph_place_cases as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_describe_campaign_reaches_every_class():
    count = collections.Counter()
    for case in pp.describe_campaign() + pp.describe_campaign(long_row=True):
        count.update(pp.describe_classes_of(case, pp.run_describe_case(case)[1]))
    short = {c: count[c] for c in pp.DESCRIBE_CLASSES if count[c] < 3}
    assert not short, short
    assert sorted({c["store"].shape[1] for c in pp.describe_campaign()}) == sorted(pp.DESCRIBE_STRIDES)


def test_recognize_campaign_reaches_every_class():
    count = collections.Counter()
    for case in pp.recognize_campaign() + pp.recognize_campaign(big=True):
        count.update(pp.recognize_classes_of(case, pp.run_recognize_case(case)[1]))
    short = {c: count[c] for c in pp.RECOGNIZE_CLASSES + pp.ONCE if count[c] < (1 if c in pp.ONCE else 3)}
    assert not short, short


def test_distance_against_a_plain_triple_loop():
    rng = np.random.default_rng(2)
    pairs = [(rng.integers(0, 256, 64), rng.integers(0, 256, 64)) for _ in range(4)]
    a = rng.integers(0, 256, 64)
    pairs += [(a, np.roll(a, -5)), (np.tile(a[:32], 2), np.roll(np.tile(a[:32], 2), -40)), (np.zeros(64, int), np.full(64, 255)), (a, a)]
    for a, c in pairs:
        best = None
        for s in range(64):
            d = 0
            for k in range(64):
                d += abs(int(a[(k + s) % 64]) - int(c[k]))
            if best is None or d < best[0]:
                best = (d, s)
        assert pp.distance(a, c) == best
    assert pp.distance(pairs[4][0], pairs[4][1]) == (0, 5) and pp.distance(pairs[5][0], pairs[5][1]) == (0, 8)
    assert pp.distance(pairs[6][0], pairs[6][1]) == (pp.MAX_DIST, 0)


def test_a_turned_scan_gives_its_shift_and_the_heading_minus_the_shift():
    seen = collections.Counter()
    for case in pp.recognize_campaign():
        if "turn" not in case:
            continue
        (_, recs, rep, near, _, _, _, q_pose), _ = pp.run_recognize_case(case)
        m, anchor = case["turn"], case["anchor"]
        assert (int(recs[0]["anchor"]), int(recs[0]["shift"]), int(recs[0]["dist"])) == (anchor, m, 0), case["name"]
        nd = case["graph"]["nodes"][anchor]
        assert (q_pose[0], q_pose[1]) == (nd["x"], nd["y"])
        want = float(nd["ang"]) - m * 5.625                                   # the query looks m sectors to the right of the anchor's heading
        assert q_pose[2] == want - 360.0 * np.floor((want + 180.0) / 360.0) and -180.0 <= q_pose[2] < 180.0
        assert float(near["d2"]) == 0.0 and int(near["anchor"]) == anchor
        seen[m] += 1
    assert all(seen[m] == 3 for m in pp.TURNS)


def test_selection_and_gather_are_nears():
    """What recognize leaves for an anchor is what near leaves for the same anchor, but for the pose."""
    for case in pg.near_campaign():
        (rec, sel, row, q_len, q_pose), tr = pg.run_near_case(case)
        g = case["graph"]
        q0 = np.full((g["store"].shape[1], 2), 0.125)
        mine = pp.leave_for_anchor(g, tr["j"], tr["n_nodes"], int(rec["anchor"]), case["gap"], case["window"], q0, tuple(q_pose))
        assert mine[0].tobytes() == sel.tobytes() and mine[1].tobytes() == row.tobytes() and mine[2] == q_len
        assert mine[3].tobytes() == q_pose.tobytes(), case["name"]


def test_end_to_end_closes_a_loop_that_pose_proximity_cannot_see():
    E = pp.end_to_end()
    n, j, gap = E["n_nodes"], E["n_nodes"] - 1, pp.E2E["gap"]
    assert n == 25 and pp.E2E["radius"] == 10.0
    # 1. near at radius 10 finds nothing
    assert int(E["near_by_pose"]["anchor"]) == -1 and int(E["near_by_pose"]["query"]) == j
    # 2. round 0 is at most one index from the true nearest old node
    T = E["truth"]
    true_nearest = int(np.argmin(np.hypot(T[:j - gap + 1, 0] - T[j, 0], T[:j - gap + 1, 1] - T[j, 1])))
    r0 = E["recs"][0]
    assert int(r0["anchor"]) >= 0 and abs(int(r0["anchor"]) - true_nearest) <= 1
    # 3. no other unsuppressed node has that distance (round 0: nothing is suppressed yet)
    best = E["trace"]["D"].min(axis=1)
    assert int((best == int(r0["dist"])).sum()) == 1
    # 4. the closure is appended
    assert int(E["closure_rep"]["flags"]) == pg.APPENDED and int(E["near"]["anchor"]) == int(r0["anchor"])
    # 5. the relaxation brings the keyframes nearer to the truth

    def mean_error(nodes):
        return float(np.mean(np.hypot(nodes["x"][:n] - T[:n, 0], nodes["y"][:n] - T[:n, 1])))
    before, after = mean_error(E["g2"]["nodes"]), mean_error(E["g3"]["nodes"])
    print("place: anchor %d (true nearest %d), dist %d, shift %d; mean keyframe error %.4f -> %.4f pixels (ratio %.3f)"
          % (int(r0["anchor"]), true_nearest, int(r0["dist"]), int(r0["shift"]), before, after, after / before))
    assert after < before
    # the heading handed to the match is the anchor's turned by the shift, not the drifted one
    assert abs(pg.wrap(E["q_pose"][2] - T[j, 2])) <= 5.625 < abs(pg.wrap(float(E["g1"]["nodes"][j]["ang"]) - T[j, 2]))
    pa, hi = E["planes"]
    assert pa.shape == (pp.PLACE_ROOM["rows"], pp.PLACE_ROOM["cols"]) and hi.sum() > 0


def test_struct_sizes_match_the_header_and_the_python_mirror(lsdmod):
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name, size in pp.SIZES.items():
        m = re.search(r"typedef struct %s \{.*?\} %s;[^\n]*" % (name, name), src, re.S)
        assert m, name
        assert int(re.search(r"/\* (\d+) bytes", m.group(0)).group(1)) == size, name
    assert (pp.DESC_DTYPE.itemsize, pp.PLACE_REC_DTYPE.itemsize, pp.PLACE_REP_DTYPE.itemsize) == (72, 16, 16)
    assert pp.DESC_DTYPE.fields["n_hits"][1] == 64 and pp.DESC_DTYPE.fields["n_sectors"][1] == 68 and pp.DESC_DTYPE.fields["valid"][1] == 70
    assert re.search(r"#define LSD_PG_DESC_SECTORS 64\b", src) and re.search(r"#define LSD_PG_PLACE_MAX 8\b", src)
    assert (pp.DESC_DTYPE, pp.PLACE_REC_DTYPE, pp.PLACE_REP_DTYPE) == (lsdmod.PG_DESC_DTYPE, lsdmod.PG_PLACE_REC_DTYPE, lsdmod.PG_PLACE_REP_DTYPE)
    import ctypes as C
    assert C.sizeof(lsdmod.lsd_pg_place) == pp.SIZES["lsd_pg_place_par"]
    assert [f for f, _ in lsdmod.lsd_pg_place._fields_] == list(pp.PLACE_KEYS) + ["reserved"]
    assert lsdmod.PG_PLACE_DEFAULTS == pp.PLACE_DEFAULTS and (lsdmod.PG_DESC_SECTORS, lsdmod.PG_PLACE_MAX) == (pp.SECTORS, pp.PLACE_MAX)
    for name in ("lsd_enqueue_pg_describe_device", "lsd_enqueue_pg_recognize_device", "lsd_pg_describe", "lsd_pg_recognize"):
        assert name in lsdmod.EXPORTED_SYMBOLS
    p = lsdmod.pg_place(dict(k=3), pick=2, max_dist=7)
    assert (p.gap, p.window, p.spread, p.k, p.pick, p.max_dist, p.min_sectors, p.reserved) == (10, 2, 2, 3, 2, 7, 16, 0)


def test_kernels_stay_out_of_scratch(tmp_path):
    """The compiler's own resource summary of k_pgplace.hip for gfx950: three kernels, none with a scratch frame, the score kernel with the
    packed byte SAD (16 per shift, 64 shifts)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "linesegmentdetector-slam_amd", "csrc", "k_pgplace.hip")
    out = str(tmp_path / "k_pgplace.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True)
    text = open(out).read()
    found = {}
    for name in ("k_pg_describe", "k_pg_place_score", "k_pg_place_pick"):
        m = re.search(r"\.set _ZN6lsdhip\d+%sE\w*\.private_seg_size, (\d+)" % name, text)
        assert m, name
        found[name] = int(m.group(1))
    assert found == {"k_pg_describe": 0, "k_pg_place_score": 0, "k_pg_place_pick": 0}, found
    assert re.findall(r"; ScratchSize: (\d+)", text) == ["0", "0", "0"]
    assert "flat_load" not in text                                          # every row and record is read in its own address space
    assert text.count("v_sad_u8") == 64 * 16
