"""Ray casting on the grid, without a GPU: the restatement of tests/grid_ray_cases.py alone.  What the campaign reaches, a second
formulation that walks every ray cell by cell, the half-way coordinates, the summary rule on hand-made counts, and the scenario the
feature exists for: an intruder in front of a mapped wall is screened out of the scan before it is integrated."""
import math

import numpy as np
import pytest

import grid_cases as gc
import grid_ray_cases as rc


@pytest.fixture(scope="module")
def runs(oracle):
    """(case, out, sums, scans_out, trace) of the campaign: the restatement, computed once."""
    return [(case,) + rc.run_case(case) for case in rc.campaign()]


def test_every_class_is_reached_three_times(runs):
    count = {c: 0 for c in rc.CLASSES}
    for case, out, sums, so, trace in runs:
        for c in rc.classes_of(case, trace, sums):
            count[c] += 1
    low = {c: n for c, n in count.items() if n < (1 if c == "scan_len_1025" else 3)}
    assert not low, low


def test_grids_are_small(runs):
    for case, *_ in runs:
        cols, rows = case["cols"], case["rows"]
        assert (cols <= 61 and rows <= 47) or (max(cols, rows) <= 300 and min(cols, rows) <= 5), case["name"]
        assert case["capacity"] == (2048 if case["scans"].shape[1] > 1024 else 1024), case["name"]
        assert case["range_max"] / case["resol"] < 32767


def test_cell_by_cell_walk_gives_the_same_records(runs):
    """The second formulation: a Python loop over the ray's cells, integers only, that stops at the first occupied cell.  It shows that
    the hit cell is occupied and that no cell before it is, and that the unknown cell reported lies before the hit."""
    beams = 0
    for case, out, sums, so, trace in runs:
        g = case["grid"].view(np.uint8)
        for t in trace:
            if t["skip"]:
                continue
            k_hit, k_unk, cell = rc.first_cells_brute(t["x0"], t["y0"], t["x1"], t["y1"], case["grid"])
            assert (k_hit, k_unk) == (t["k_hit"], t["k_unk"]), (case["name"], t["scan"], t["beam"])
            rec = out[t["scan"], t["beam"]]
            assert (int(rec["cx"]), int(rec["cy"]), int(rec["k_hit"])) == (cell[0], cell[1], k_hit)
            pose = case["poses"][t["scan"]]
            cells = gc.ray_cells(t["x0"], t["y0"], t["x1"], t["y1"])
            want = rc.record_of(pose, t["x1"], t["y1"], cells, k_hit, k_unk, t["m"], case["resol"], case["range_max"], case["par"]["tol"])
            assert np.array(want, rc.RAY_DTYPE).tobytes() == rec.tobytes(), (case["name"], t["scan"], t["beam"])
            if k_hit >= 0:
                assert g[cell[1], cell[0]] not in (0, 255)
                assert not (t["kinds"][:k_hit] == rc.OCC).any()
            beams += 1
    assert beams > 5000


def test_records_of_beams_that_are_not_cast_are_zero_and_slots_beyond_len_untouched(runs):
    fill = lambda nbytes, seed: ((np.arange(nbytes, dtype=np.uint64) * 2654435761 + seed) % 251 + 1).astype(np.uint8)
    for case, out, sums, so, trace in runs[::7]:
        fo, fs, fso, _ = rc.run_case(case, fill=fill)
        n, stride = case["scans"].shape[:2]
        beyond = np.arange(stride)[None, :] >= case["lens"][:, None]
        assert fo[~beyond].tobytes() == out[~beyond].tobytes() and fs.tobytes() == sums.tobytes()
        assert fo[beyond].tobytes() == fill(fo.nbytes, 1).view(rc.RAY_DTYPE).reshape(n, stride)[beyond].tobytes()
        assert fso[beyond].tobytes() == fill(fso.nbytes, 3).view(np.float64).reshape(n, stride, 2)[beyond].tobytes()
        zero = out[~beyond][out[~beyond]["cls"] == rc.NOT_CAST]
        assert zero.tobytes() == bytes(zero.nbytes)


def test_rint_in_place_of_round_changes_a_record(runs):
    changed = 0
    for case, out, sums, so, trace in runs:
        if not case["name"].startswith("half_way"):
            continue
        o2 = rc.run_case(case, rnd=gc.c_rint)[0]
        assert o2.tobytes() != out.tobytes(), case["name"]
        changed += 1
    assert changed == 3


def test_screened_scans(runs):
    """The angle's bits always, the range's bits unless the class is dropped; in place gives the same rows."""
    for case, out, sums, so, trace in runs:
        n, stride = case["scans"].shape[:2]
        live = np.arange(stride)[None, :] < case["lens"][:, None]
        src, got = case["scans"].view(np.uint64), so.view(np.uint64)
        assert (got[..., 1][live] == src[..., 1][live]).all()
        dropped = ((case["par"]["drop_mask"] >> out["cls"]) & 1).astype(bool) & live
        assert (got[..., 0][dropped] == rc.QUIET_NAN).all() and (got[..., 0][live & ~dropped] == src[..., 0][live & ~dropped]).all()
    for case, out, sums, so, trace in runs[::9]:
        o2, s2, so2, _ = rc.run_case(case, in_place=True)
        live = np.arange(case["scans"].shape[1])[None, :] < case["lens"][:, None]
        assert o2.tobytes() == out.tobytes() and s2.tobytes() == sums.tobytes() and so2[live].tobytes() == so[live].tobytes()


def test_summary_rule_on_hand_made_counts():
    par = rc.ray_par(min_beams=4, ok_num=1, ok_den=2)
    n = lambda agree, short: [0, 0, 0, agree, short, 0, 0]
    assert rc.summary_flags(n(2, 2), par) == (4, True) and rc.summary_flags(n(1, 3), par) == (4, False)
    assert rc.summary_flags(n(3, 1), par) == (4, True) and rc.summary_flags(n(3, 0), par) == (3, False)          # judged = min_beams - 1
    big = rc.ray_par(min_beams=1, ok_num=(1 << 32) - 2, ok_den=(1 << 32) - 1)
    assert rc.summary_flags([0, 0, 4095, 0, 1, 0, 0], big) == (4096, False)       # 4095 * (2^32 - 1) < 4096 * (2^32 - 2): beyond 2^32, and
    assert (4095 * ((1 << 32) - 1)) % (1 << 32) >= (4096 * ((1 << 32) - 2)) % (1 << 32)      # a 32-bit product would say otherwise
    assert rc.summary_flags([0, 0, 4096, 0, 0, 0, 0], big) == (4096, True)
    assert rc.summary_flags(n(0, 0), rc.ray_par(min_beams=0)) == (0, True)


def test_gate_and_flags(runs):
    gated = passed = 0
    for case, out, sums, so, trace in runs:
        for i in range(len(case["lens"])):
            skipped = gc.scan_skip(case["poses"][i]) is not None
            s = sums[i]
            assert bool(s["flags"] & rc.SKIPPED) == skipped and s["pad"] == 0
            assert s["judged"] == s["n"][2:6].sum()
            head = s.tobytes()[:24]
            if case["par"]["gate"] and not skipped and not s["flags"] & rc.CONSISTENT:
                assert s["x"] == -1.0 and head[8:] == case["poses"][i].tobytes()[8:]
                assert gc.scan_skip((s["x"], s["y"], s["ang"])) == "scan_sentinel"
                gated += 1
            else:
                assert head == case["poses"][i].tobytes()
                passed += 1
            if skipped:
                assert not s["n"].any() and not s["flags"] & rc.CONSISTENT
            else:
                assert s["n"].sum() == case["lens"][i]
    assert gated >= 3 and passed >= 3


# ---- the scenario: an intruder in front of a mapped wall -----------------------------------------------------------------------------------
COLS, ROWS, RESOL, RANGE_MAX = 61, 47, 0.1, 8.0
WALLS = (4.3, 56.3, 4.3, 42.3)                 # x_lo, x_hi, y_lo, y_hi of the room, in cells


def wall_range(px, py, th):
    """Metres from (px, py) (cells) to the room's walls along th."""
    c, s = math.cos(th), math.sin(th)
    t = [((WALLS[1] if c > 0 else WALLS[0]) - px) / c if c else math.inf, ((WALLS[3] if s > 0 else WALLS[2]) - py) / s if s else math.inf]
    return min(t) * RESOL


def room_scan(px, py, n):
    a = -math.pi + 2 * math.pi * np.arange(n) / n
    return np.stack([[wall_range(px, py, th) for th in a], a], 1)


@pytest.fixture(scope="module")
def mapped_room(oracle):
    pa, hi = np.zeros((ROWS, COLS), np.uint32), np.zeros((ROWS, COLS), np.uint32)
    poses = np.array([(20.0, 15.0, 0.0), (30.4, 23.7, 0.0), (41.2, 30.1, 0.0)])
    scans = np.stack([room_scan(p[0], p[1], 1440) for p in poses])
    gc.integrate(scans, np.full(3, 1440, np.int32), poses, COLS, ROWS, RESOL, RANGE_MAX, pa, hi)
    return pa, hi, gc.publish(pa, hi, min_pass=1, occ_num=1, occ_den=10)


def cast(scan, pose, grid, **kw):
    par = rc.ray_par(tol=2 * RESOL, drop_mask=1 << rc.SHORT, **kw)
    n = len(scan)
    out, sums, so = np.zeros((1, n), rc.RAY_DTYPE), np.zeros(1, rc.SUM_DTYPE), np.zeros((1, n, 2))
    rc.raycast(scan[None], np.array([n], np.int32), np.array([pose]), grid, RESOL, RANGE_MAX, par, out, sums, so)
    return out[0], sums[0], so


def test_an_intruder_is_screened_out_and_a_displaced_pose_is_gated(mapped_room):
    pa, hi, grid = mapped_room
    assert (grid == 100).sum() > 150 and (grid == 0).sum() > 1500
    pose = (26.3, 20.8, 0.0)
    scan = room_scan(pose[0], pose[1], 360)
    intruder = np.arange(170, 190)                                    # a blob 1.5 m in front of the wall it hides
    scan[intruder, 0] -= 1.5
    assert (scan[intruder, 0] > 0.5).all()
    wall = np.setdiff1d(np.arange(360), intruder)
    out, s, so = cast(scan, pose, grid)
    assert (out["cls"][intruder] == rc.SHORT).all()
    assert not (out["cls"][wall] == rc.SHORT).any()
    assert s["flags"] & rc.CONSISTENT
    blob = set()
    for j in intruder:
        x1, y1 = gc.beam_ends(pose, scan[j, 0], scan[j, 1], RESOL, RANGE_MAX)[2:4]
        blob.add((y1, x1))
        assert grid[y1, x1] == 0 and hi[y1, x1] == 0                  # in the room, not on a wall
    ys, xs = (np.array(v) for v in zip(*sorted(blob)))
    p2, h2 = pa.copy(), hi.copy()
    gc.integrate(so, np.array([360], np.int32), np.array([s.tolist()[:3]]), COLS, ROWS, RESOL, RANGE_MAX, p2, h2)
    assert not h2[ys, xs].any() and h2.sum() == hi.sum() + len(wall)
    p3, h3 = pa.copy(), hi.copy()
    gc.integrate(scan[None], np.array([360], np.int32), np.array([pose]), COLS, ROWS, RESOL, RANGE_MAX, p3, h3)
    assert h3[ys, xs].all()
    # a pose displaced by 10 cells into the room, along its diagonal (along a wall the ranges to that wall would still agree): not
    # consistent at 1 / 2, and with the gate the integration adds nothing
    moved = (pose[0] + 10.0 * math.sqrt(0.5), pose[1] + 10.0 * math.sqrt(0.5), 0.0)
    clean = room_scan(pose[0], pose[1], 360)
    out, s, so = cast(clean, moved, grid, gate=1)
    assert not s["flags"] & rc.CONSISTENT and s["x"] == -1.0 and s["judged"] >= 300
    p4, h4 = pa.copy(), hi.copy()
    gc.integrate(so, np.array([360], np.int32), np.array([s.tolist()[:3]]), COLS, ROWS, RESOL, RANGE_MAX, p4, h4)
    assert np.array_equal(p4, pa) and np.array_equal(h4, hi)
    out, s, so = cast(clean, moved, grid, gate=0)
    assert not s["flags"] & rc.CONSISTENT and s["x"] == moved[0]
