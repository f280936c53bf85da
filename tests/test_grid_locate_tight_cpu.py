"""The tight global localisation: the restatement of tests/grid_locate_tight_cases.py alone, no GPU.  Whatever the flag
word, every scan that does not overflow has the exhaustive search's record; the bound only rises, the frontiers only shrink, an overflow
under the tight rule is an overflow under the existing one and not the other way round; tight = 0 and levels <= 1 ARE the existing rule."""
import numpy as np
import pytest

import grid_locate_cases as lc
import grid_locate_tight_cases as tc


@pytest.fixture(scope="module")
def results(oracle):
    """(case, {tight: (records, statistics, traces)}, the existing rule's (records, statistics, trace)) over both campaigns."""
    old = [(c, res, lc.run_case(c)) for c, (res, _) in zip(tc.campaign(), tc.expected())]
    return [(c, res, want) for c, res, want in zip(lc.campaign(), tc.expected_existing(), lc.expected())] + old


def but_lower_bound(rec):
    a = np.array(rec).reshape(-1).view(np.uint8).reshape(-1, 64).copy()
    a[:, lc.LOWER_BOUND_BYTES] = 0
    return a


def test_both_campaigns_are_what_they_are_meant_to_be(results):
    assert len(lc.campaign()) == 106 and len(results) == 106 + len(tc.campaign())
    for c in tc.campaign():
        p = c["par"]
        assert c["corr"].shape[1] <= 61 and c["corr"].shape[0] <= 47 and p["levels"] <= 5 and p["n_ang"] <= 65, c["name"]


def test_every_tight_equals_the_exhaustive_search(results):
    """All 64 record bytes but lower_bound against levels = 0; lower_bound at least the existing rule's and at most S_win."""
    compared = 0
    for c, res, (old, _, _) in results:
        flat, _, _ = lc.run_case(c, levels=0)
        b = but_lower_bound(flat)
        for tight in tc.TIGHTS:
            rec = res[tight][0]
            a = but_lower_bound(rec)
            for i in range(len(rec)):
                if rec[i]["flags"] == lc.OVERFLOW:
                    r = rec[i]
                    assert (r["x"], r["y"], r["ang"]) == (-1.0, -1.0, 0.0) and not np.signbit(r["ang"])
                    assert [int(r[k]) for k in ("score", "n_beams", "cx", "cy", "a", "n_best")] == [0] * 6 and r["lower_bound"] > 0
                    continue
                compared += 1
                assert a[i].tobytes() == b[i].tobytes(), (c["name"], tight, i, rec[i], flat[i])
                assert rec[i]["lower_bound"] >= old[i]["lower_bound"], (c["name"], tight, i)
                if rec[i]["flags"] in (lc.ACCEPTED, lc.REJECTED):
                    assert rec[i]["lower_bound"] <= rec[i]["score"], (c["name"], tight, i)
    assert compared > 4 * 130


def test_bounds_rise_and_frontiers_shrink(results):
    """frontier[h] and first_count[h] against |F_h| of the existing rule with nothing cut off; bound[h] never falls on the way down."""
    for c, res, _ in results:
        _, whole, _ = lc.run_case(dict(c, par=dict(c["par"], max_nodes=tc.UNLIMITED)))
        H = c["par"]["levels"]
        for tight in tc.TIGHTS:
            for i, st in enumerate(res[tight][1]):
                assert (st["frontier"] <= whole[i]["frontier"]).all() and (st["first_count"] <= whole[i]["frontier"]).all(), (c["name"], tight, i)
                assert not st["frontier"][H + 1:].any() and not st["bound"][H + 1:].any() and not st["reserved"].any()
                b = [int(v) for v in st["bound"][:H + 1] if v]
                assert b == sorted(b, reverse=True), (c["name"], tight, i, st["bound"])
                if not tight & tc.RETRY:
                    assert not st["retried"] and not st["first_count"].any()
                if not tight & tc.PROBE:
                    assert len(set(b)) <= 1
                for h in range(9):
                    assert bool(st["retried"] >> h & 1) == bool(st["first_count"][h]) and (not st["first_count"][h] or st["first_count"][h] > c["par"]["max_nodes"])
                if res[tight][0][i]["flags"] == lc.EMPTY:
                    assert not st.tobytes().strip(b"\0") and res[tight][0][i]["lower_bound"] == 0


def test_an_overflow_under_tight_is_one_under_the_existing_rule(results):
    rescued = {t: [] for t in tc.TIGHTS}
    for c, res, (old, _, _) in results:
        for tight in tc.TIGHTS:
            for i, r in enumerate(res[tight][0]):
                if r["flags"] == lc.OVERFLOW:
                    assert old[i]["flags"] == lc.OVERFLOW, (c["name"], tight, i)
                elif old[i]["flags"] == lc.OVERFLOW:
                    rescued[tight].append(c["name"])
    assert not rescued[0] and not rescued[tc.RETRY]                  # a retry without a raised bound rebuilds the same set
    for v in range(3):                                               # the converse fails
        assert "probe_rescue_%d" % v in rescued[tc.PROBE] and "probe_rescue_%d" % v in rescued[3]
        assert "retry_rescue_%d" % v in rescued[3] and "retry_rescue_%d" % v not in rescued[tc.PROBE]


def test_no_flag_and_one_level_are_the_existing_rule(results):
    """All 64 + 48 bytes."""
    one_level = 0
    for c, res, (old, old_st, _) in results:
        for tight in tc.TIGHTS if c["par"]["levels"] <= 1 else (0,):
            rec, st, _ = res[tight]
            assert rec.tobytes() == old.tobytes(), (c["name"], tight)
            assert st.view(np.uint8).reshape(-1, 128)[:, :48].tobytes() == old_st.tobytes(), (c["name"], tight)
            assert not st["retried"].any() and not st["first_count"].any()
        one_level += c["par"]["levels"] <= 1
    assert one_level >= 6


def test_every_added_class_is_reached():
    count = {k: 0 for k in tc.CLASSES}
    for c, (res, wrong) in zip(tc.campaign(), tc.expected()):
        for k in tc.classes_of(c, res, wrong):
            count[k] += 1
    short = {k: n for k, n in count.items() if n < (1 if k in tc.ONCE else 3)}
    assert not short, short


def test_the_stated_cases(results):
    by_name = {c["name"]: (c, res) for c, res, _ in results}
    for v in range(3):
        c, res = by_name["probe_rescue_%d" % v]
        assert res[1][0][0]["flags"] == res[3][0][0]["flags"] == lc.ACCEPTED and not res[3][1][0]["retried"]
        c, res = by_name["retry_rescue_%d" % v]
        st, st1 = res[3][1][0], res[1][1][0]
        h = int(st["retried"]).bit_length() - 1
        assert st["retried"] == 1 << h and res[3][0][0]["flags"] == lc.ACCEPTED and res[1][0][0]["flags"] == lc.OVERFLOW
        assert st1["frontier"][h] == st["first_count"][h] > c["par"]["max_nodes"] >= st["frontier"][h] and st["scored"] > st1["scored"]
        c, res = by_name["retry_fails_%d" % v]
        st = res[3][1][0]
        h = int(np.flatnonzero(st["frontier"])[0])
        assert st["retried"] >> h & 1 and st["first_count"][h] >= st["frontier"][h] > c["par"]["max_nodes"] and st["bound"][h] and not st["bound"][:h].any()
        assert res[3][0][0]["lower_bound"] == st["bound"][h]
        c, res = by_name["top_overflow_%d" % v]
        H = c["par"]["levels"]
        for tight in tc.TIGHTS:
            st = res[tight][1][0]
            assert st["frontier"][H] > c["par"]["max_nodes"] and not st["frontier"][:H].any() and not st["retried"] and st["scored"] == st["top_nodes"]
        c, res = by_name["floor_over_win_%d" % v]
        assert all(res[t][0][0]["flags"] == lc.NOT_FOUND for t in tc.TIGHTS)
        c, res = by_name["empty_between_%d" % v]
        assert [int(f) for f in res[3][0]["flags"]] == [lc.ACCEPTED, lc.EMPTY, res[3][0][2]["flags"]] and res[0][0][0]["flags"] == lc.OVERFLOW


def test_the_larger_index_is_not_the_rule():
    """Where two nodes tie for a heading's best, starting the probe from the larger index states other bounds."""
    changed = 0
    for c, (res, wrong) in zip(tc.campaign(), tc.expected()):
        if c["name"].startswith("head_tie_"):
            assert wrong.tobytes() != res[3][1].tobytes() and (wrong["bound"] != res[3][1]["bound"]).any(), c["name"]
            changed += 1
    assert changed == 3


def test_recovery_is_unchanged(oracle):
    c, truth = lc.recovery()
    want, want_st, _ = lc.run_case(c)
    ds = tc.dense_case(c)
    for tight in tc.TIGHTS:
        rec, st, _ = tc.run_dense(ds, c["par"], tight)
        assert but_lower_bound(rec).tobytes() == but_lower_bound(want).tobytes(), tight
        assert [(int(v["cx"]), int(v["cy"]), int(v["a"])) for v in rec] == truth
        assert (rec["lower_bound"] >= want["lower_bound"]).all() and (st["frontier"] <= want_st["frontier"]).all()
        if tight == 0:
            assert rec.tobytes() == want.tobytes()


def test_python_mirrors(lsdmod):
    assert lsdmod.GRID_LOCATE_TIGHT_STATS_DTYPE == tc.TIGHT_STATS_DTYPE and lsdmod.GRID_LOCATE_TIGHT_STATS_DTYPE.itemsize == 128
    assert (lsdmod.GRID_LOCATE_TIGHT_PROBE, lsdmod.GRID_LOCATE_TIGHT_RETRY) == (tc.PROBE, tc.RETRY) == (1, 2)
    assert [lsdmod.grid_locate_tight(t) for t in (None, 0, False, True, "probe", "retry", 1, 2, 3)] == [0, 0, 0, 3, 1, 2, 1, 2, 3]
    for bad in (4, -1, "both", 1.5):
        with pytest.raises(lsdmod.LsdError):
            lsdmod.grid_locate_tight(bad)
