"""Global scan-to-grid localisation: the restatement of tests/grid_locate_cases.py alone, no GPU.  The branch-and-bound
rule equals the exhaustive search (levels = 0) on every case, the campaign reaches every class, `>` in the frontier test is not the rule,
and the asymmetric room is recovered from poses nobody told the search."""
import numpy as np
import pytest

import grid_locate_cases as lc
import grid_match_mr_cases as mr


@pytest.fixture(scope="module")
def results(oracle):
    return list(zip(lc.campaign(), lc.expected()))


def test_pyramid_is_the_coarse_plane_and_builds_level_from_level():
    """plane_h is 8.1.8's coarse plane at b = 2^h, and four reads of plane_(h-1) at stride 2^(h-1) give plane_h."""
    rng = np.random.default_rng(3)
    for cols, rows in ((61, 47), (1, 1), (1, 257), (33, 9)):
        corr = lc.gm.random_plane(rng, cols, rows, 0.3)
        assert lc.plane(corr, 0).tobytes() == corr.tobytes()
        for h in range(1, 9):
            pl = lc.plane(corr, h)
            if h <= 4:
                assert pl.tobytes() == mr.coarse_plane(corr, 1 << h).tobytes(), (cols, rows, h)
            half, m = 1 << (h - 1), (1 << h) - 1
            prev = np.zeros((rows + m + half, cols + m + half), np.uint8)          # plane_(h-1) in plane_h's frame, 0 outside it
            prev[half:half + rows + half - 1, half:half + cols + half - 1] = lc.plane(corr, h - 1)
            built = np.maximum(np.maximum(prev[:rows + m, :cols + m], prev[:rows + m, half:half + cols + m]),
                               np.maximum(prev[half:half + rows + m, :cols + m], prev[half:half + rows + m, half:half + cols + m]))
            assert built.tobytes() == pl.tobytes(), (cols, rows, h)
        buf = lc.pyramid(corr, 8)
        assert len(buf) == lc.pyramid_offset(cols, rows, 9)
        assert buf[lc.pyramid_offset(cols, rows, 5):lc.pyramid_offset(cols, rows, 6)].tobytes() == lc.plane(corr, 5).tobytes()


def test_branch_and_bound_equals_the_exhaustive_search(results):
    """All 64 record bytes but lower_bound, on every scan of every case.  A scan that ends in OVERFLOW has no counterpart at levels = 0
    (no level above the candidates is formed there): it is held to the stated record instead, and its case to a twin that does not
    overflow."""
    compared = overflowed = 0
    for c, (rec, st, _) in results:
        flat, _, _ = lc.run_case(c, levels=0)
        a, b = rec.view(np.uint8).reshape(-1, 64).copy(), flat.view(np.uint8).reshape(-1, 64).copy()
        a[:, lc.LOWER_BOUND_BYTES] = b[:, lc.LOWER_BOUND_BYTES] = 0
        for i in range(len(rec)):
            if rec[i]["flags"] == lc.OVERFLOW:
                overflowed += 1
                r = rec[i]
                assert (r["x"], r["y"], r["ang"]) == (-1.0, -1.0, 0.0) and not np.signbit(r["ang"])
                assert [int(r[k]) for k in ("score", "n_beams", "cx", "cy", "a", "n_best")] == [0] * 6 and r["lower_bound"] > 0
                h = min(h for h in range(1, 9) if st[i]["frontier"][h])      # the levels below the overflowing one are not run
                assert st[i]["frontier"][h] == c["par"]["max_nodes"] + 1 and not st[i]["frontier"][:h].any()
                continue
            compared += 1
            assert a[i].tobytes() == b[i].tobytes(), (c["name"], i, rec[i], flat[i])
            assert flat[i]["lower_bound"] >= rec[i]["lower_bound"]
    assert compared == sum(len(r) for _, (r, _, _) in results) - 3 and overflowed == 3


def test_overflow_is_one_node_away(results):
    by_name = {c["name"]: (c, r) for c, r in results}
    for v in range(3):
        (ca, (ra, sa, _)), (cb, (rb, sb, _)) = by_name["max_nodes_at_%d" % v], by_name["max_nodes_below_%d" % v]
        assert ca["par"]["max_nodes"] == cb["par"]["max_nodes"] + 1 == int(sa[0]["frontier"][1:].max())
        assert ra[0]["flags"] in (lc.ACCEPTED, lc.REJECTED) and rb[0]["flags"] == lc.OVERFLOW and ra[0]["lower_bound"] == rb[0]["lower_bound"]


def test_every_class_is_reached(results):
    count = {k: 0 for k in lc.CLASSES}
    for c, (rec, st, trace) in results:
        for k in lc.classes_of(c, rec, st, trace):
            count[k] += 1
    short = {k: n for k, n in count.items() if n < (1 if k in lc.ONCE else 3)}
    assert not short, short
    flags = np.concatenate([r["flags"] for _, (r, _, _) in results])
    assert set(flags.tolist()) == {lc.ACCEPTED, lc.REJECTED, lc.NOT_FOUND, lc.OVERFLOW, lc.EMPTY}     # each outcome is exactly one flag


def test_statistics_add_up(results):
    for c, (rec, st, _) in results:
        p = c["par"]
        H = p["levels"]
        for r, s in zip(rec, st):
            if r["flags"] == lc.EMPTY:
                assert not s.tobytes().strip(b"\0") and r["lower_bound"] == 0
                continue
            nbx, nby = -(-p["nx"] >> H), -(-p["ny"] >> H)
            assert s["top_nodes"] == p["n_ang"] * nbx * nby and not s["frontier"][H + 1:].any() and s["scored"] >= s["top_nodes"]
            assert s["scored"] <= s["top_nodes"] + 4 * int(s["frontier"][1:].sum())
            if H == 0:
                assert s["scored"] == s["top_nodes"] == p["n_ang"] * p["nx"] * p["ny"]
            if r["flags"] in (lc.ACCEPTED, lc.REJECTED):
                assert 1 <= r["n_best"] <= s["frontier"][0] and r["lower_bound"] <= r["score"]


def test_greater_than_is_not_the_rule(results):
    """Where the greedy descent already reaches the winner's score, L == S_win: the winner's own ancestors have U == L at some level at
    the latest at level 0, and `>` throws the winner away.  On the uniform plane every candidate goes, and the record says NOT_FOUND."""
    changed = 0
    for c, (rec, _, _) in results:
        if not c["name"].startswith(("uniform_", "mirror2_", "accept+0_")):
            continue
        other, _, _ = lc.run_case(c, ge=False)
        assert rec[0]["flags"] in (lc.ACCEPTED, lc.REJECTED) and rec[0]["lower_bound"] == rec[0]["score"]
        assert other[0]["flags"] == lc.NOT_FOUND and other.tobytes() != rec.tobytes(), c["name"]
        changed += 1
    assert changed == 9


def test_recovery_of_the_asymmetric_room(oracle):
    """An L-shaped room with a pillar, integrated at five whole-cell poses; scans simulated from three OTHER whole-cell poses at headings
    that are multiples of the step come back as exactly their cell and heading index, over the whole grid and 360 degrees, unambiguously:
    under the exhaustive restatement, and under the branch-and-bound one with a small part of the work."""
    c, truth = lc.recovery()
    assert (c["par"]["nx"], c["par"]["ny"], c["par"]["n_ang"] * c["par"]["ang_step"]) == (c["cols"], c["rows"], 360.0)
    flat, flat_st, _ = lc.run_case(c, levels=0)
    rec, st, _ = lc.run_case(c)
    for r in (flat, rec):
        assert [(int(v["cx"]), int(v["cy"]), int(v["a"])) for v in r] == truth
        assert (r["n_best"] == 1).all() and (r["flags"] == lc.ACCEPTED).all()
        assert [(v["x"], v["y"], v["ang"]) for v in r] == [(float(x), float(y), a * lc.RECOVERY_STEP) for x, y, a in truth]
    a, b = rec.view(np.uint8).reshape(-1, 64).copy(), flat.view(np.uint8).reshape(-1, 64).copy()
    a[:, lc.LOWER_BOUND_BYTES] = b[:, lc.LOWER_BOUND_BYTES] = 0
    assert a.tobytes() == b.tobytes()
    assert (flat_st["scored"] == 120 * 61 * 47).all() and (st["scored"] * 100 < flat_st["scored"]).all()
