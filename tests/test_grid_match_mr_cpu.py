"""The coarse-to-fine campaign (tests/grid_match_mr_cases.py) under the restatement alone: every class is reached, the coarse plane against
a second, gathering formulation, the bound S <= U on every block, the records of the pruned search equal to the plain restatement's on the
new campaign and on the whole plain one at five block sizes, why the refinement test is >= and not >, and the recovery of large known
displacements in the room.  No GPU."""
import numpy as np
import pytest

import grid_match_cases as gm
import grid_match_mr_cases as mr


@pytest.fixture(scope="module")
def traced(oracle):
    """(case, what prepare() gives, records, stats, trace, classes) of the new campaign at each case's own block size."""
    out = []
    for case in mr.mr_campaign():
        prep = mr.prepare_case(case)
        rec, stats, trace = mr.run_mr_case(case, prepared=prep)
        out.append((case, prep, rec, stats, trace, mr.mr_classes_of(case, trace, stats)))
    return out


@pytest.fixture(scope="module")
def plain_cases(oracle):
    """(case, what prepare() gives, the plain restatement's records) of the new campaign and of the whole plain one."""
    out = []
    for case in mr.mr_campaign() + gm.match_campaign():
        out.append((case, mr.prepare_case(case), gm.run_match_case(case)[0]))
    return out


def test_every_class_is_reached(traced):
    count = {c: 0 for c in mr.MR_CLASSES}
    for case, _, _, _, _, classes in traced:
        assert classes <= set(mr.MR_CLASSES), classes - set(mr.MR_CLASSES)
        assert case["corr"].shape[1] <= 61 and case["corr"].shape[0] <= 47
        for c in classes:
            count[c] += 1
    for c, n in count.items():
        assert n >= (1 if c == "nb_1025" else 3), (c, n)
    assert sum(1 for case, *_ in traced if case["capacity"] > 1024) == 1               # the 1025 case runs once, at a raised capacity


def test_the_hand_made_cases_reach_what_they_were_made_for(traced):
    by = {case["name"]: classes for case, _, _, _, _, classes in traced}
    for v in range(3):
        assert "U_equals_L_wins" in by["equal_peaks_%d" % v]
        assert "zero_block_pruned" in by["prior_pruned_%d" % v]
        assert "low_rim" in by["low_rim_%d" % v]
        assert "angle_no_survivor" in by["lonely_%d" % v]
        assert {"L_from_other_angle", "winner_outside_seeds"} <= by["other_angle_%d" % v]
        assert "survivors_over_256" in by["peaks_many_%d" % v] and "fine_over_256" in by["peaks_fine_%d" % v]
        for k in (1, 63, 64, 65):
            assert "survivors_%d" % k in by["peaks%d_%d" % (k, v)]


def test_coarse_plane_is_the_gathered_maximum():
    """The definition read cell by cell, the rim on the low side included."""
    rng = np.random.default_rng(3)
    planes = [gm.random_plane(rng, 13, 9, 0.4), gm.random_plane(rng, 1, 1, 1.0), gm.random_plane(rng, 40, 1, 0.5), gm.random_plane(rng, 2, 33, 0.5),
              gm.recovery()[0]]
    for corr in planes:
        rows, cols = corr.shape
        for b in (2, 3, 5, 16) if corr.size < 1000 else (4,):
            got = mr.coarse_plane(corr, b)
            assert got.shape == (rows + b - 1, cols + b - 1) and got.dtype == np.uint8
            for y in range(-(b - 1), rows):
                for x in range(-(b - 1), cols):
                    cells = [int(corr[y + v, x + u]) for v in range(b) for u in range(b) if 0 <= y + v < rows and 0 <= x + u < cols]
                    assert got[y + b - 1, x + b - 1] == max(cells, default=0), (b, x, y)
            assert got[b - 1:, b - 1:].max() == corr.max() and (got[0, 0] == corr[0, 0])


def test_the_bound_holds_on_every_block(plain_cases):
    for case, prep, _ in plain_cases:
        se = case["search"]
        for b in mr.BLOCKS:
            trace = mr.run_mr_case(case, b, prepared=prep)[2]
            assert mr.bound_holds(trace, b, se["wx"], se["wy"]), (case["name"], b)


def test_records_equal_the_plain_search(plain_cases):
    """The new campaign and the whole plain one, at b = 2, 3, 4, 8, 16: all 56 bytes of every record."""
    assert len(plain_cases) == len(mr.mr_campaign()) + len(gm.match_campaign())
    for case, prep, want in plain_cases:
        for b in mr.BLOCKS:
            rec, stats, _ = mr.run_mr_case(case, b, prepared=prep)
            assert rec.tobytes() == want.tobytes(), (case["name"], b)
            skipped = (want["flags"] & gm.SKIPPED) != 0
            assert not stats[skipped].view(np.uint32).any()
            live = stats[~skipped]
            assert (live["refined"] >= 1).all() and (live["refined"] <= live["blocks"]).all() and (live["lower_bound"] <= want["score"][~skipped]).all()


def test_the_refinement_test_is_at_least_not_above(traced):
    """Equal peaks at i = -3 and i = +1: the block of i = +1 has U == L and holds the winner by i^2 + j^2.  With > it is pruned and the
    record becomes the seed's i = -3."""
    for case, prep, rec, _, _, _ in traced:
        if not case["name"].startswith("equal_peaks_"):
            continue
        wrong = mr.run_mr_case(case, strict=True, prepared=prep)[0]
        assert (rec[0]["di"], rec[0]["dj"], rec[0]["da"]) == (1, 0, 0) and rec.tobytes() == gm.run_match_case(case)[0].tobytes()
        assert (wrong[0]["di"], wrong[0]["dj"], wrong[0]["score"]) == (-3, 0, rec[0]["score"]) and wrong.tobytes() != rec.tobytes()


def test_score_prior_survives_the_pruning(traced):
    for case, _, rec, stats, trace, classes in traced:
        if "zero_block_pruned" in classes:
            assert any(not t["skip"] and rec[t["scan"]]["score_prior"] == t["prior"] > 0 for t in trace), case["name"]


def test_the_room_at_large_displacements(traced):
    """With the correctly rounded sin / cos: the five displacements come back as exactly the inverse offsets, and blocks are pruned."""
    corr, scans, lens, truth = gm.recovery()
    seen = 0
    for case, _, rec, stats, _, _ in traced:
        if "offset" not in case:
            continue
        seen += 1
        dx, dy, k = case["offset"]
        assert rec["di"].tolist() == [-dx] * 3 and rec["dj"].tolist() == [-dy] * 3 and rec["da"].tolist() == [-k] * 3
        assert (rec["flags"] == gm.ACCEPTED).all() and rec[["x", "y", "ang"]].tolist() == [tuple(t) for t in truth]
        assert (rec["score"] == 255 * rec["n_beams"]).all() and (stats["lower_bound"] == rec["score"]).all()
        assert (stats["refined"] < stats["blocks"]).all() and (stats["fine"] < 31 * 31 * 7).all(), stats      # something was pruned
    assert seen == len(mr.ROOM_OFFSETS) == 5
