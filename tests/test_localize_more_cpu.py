"""Six more recorded logs (fa_restatement.MORE_LOGS) and the ground-truth anchor, without a GPU: the fixtures, the selection rule on
tests/golden/localize_survey.json, the glibc replay against the correctly rounded one, and the way-point figures of every committed
log recomputed from the correctly rounded replay (tests/fa_logs.py says how a way-point meets a frame)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import fa_logs
import fa_restatement as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SURVEY = json.load(open(os.path.join(GOLDEN, "localize_survey.json")))
ANCHORED = ("f3key", "f4key") + fr.MORE_LOGS               # the committed logs that carry way-points (data/ has none)


def packer():
    spec = importlib.util.spec_from_file_location("make_localize_logs", os.path.join(GOLDEN, "make_localize_logs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def survey_of(name):
    return SURVEY["logs"][name if "_" in name else name + "_1"]


def test_survey_lists_all_logs_and_the_selection_follows_from_it():
    mk = packer()
    assert list(SURVEY["logs"]) == mk.all_logs() and len(SURVEY["logs"]) == 19
    assert sum(r["frames"] for r in SURVEY["logs"].values()) == 4066 - 99
    assert tuple(mk.select(SURVEY["logs"])) == tuple(SURVEY["selected"]) == fr.MORE_LOGS
    assert len(set(fr.MORE_LOGS)) == 6 and not set(fr.MORE_LOGS) & set(fr.LOGS) and "f3key_1" not in fr.MORE_LOGS and "f4key_1" not in fr.MORE_LOGS
    for key in ("f3key", "f4key"):
        mine = [n for n in SURVEY["logs"] if n.startswith(key) and not n.endswith("_1")]
        assert max(mine, key=lambda n: SURVEY["logs"][n]["frames"]) in fr.MORE_LOGS


@pytest.mark.parametrize("name", fr.MORE_LOGS)
def test_more_log_fixtures(name):
    m, mp, lid, odom = fr.load_log(name)
    n = survey_of(name)["frames"]
    z = np.load(os.path.join(GOLDEN, "localize_%s.npz" % name))
    assert int(z["n_frames"]) == n and lid.shape == (n, 360, 2) and odom.shape == (n + 1, 3)
    assert odom[0, 0] == 0 and np.array_equal(odom[-1], odom[-2]) and np.array_equal(odom[1:n], z["odom_raw"][1:])
    assert m.shape == (int(mp[1]), int(mp[0])) and mp[2] == 0.025
    assert fr.log_lidar(z).shape[0] == n + 1                # one lidar frame more than the driver replays (:183)
    assert np.array_equal(mp, fr.load_log(fr.LOG_MAPS[name])[1])          # all logs of a key share one mapParam.txt


@pytest.mark.parametrize("name", ANCHORED)
def test_way_point_fixtures(name):
    real, rec = fr.load_way_points(name)
    n = survey_of(name)["frames"]
    assert real.shape == (20, 2) and rec.shape == (20,) and (np.diff(rec) > 0).all() and 1 <= rec[0] and rec[-1] <= n


@pytest.mark.parametrize("name", ANCHORED)
def test_fixtures_hold_the_reference_files(name):
    mk = packer()
    if not os.path.isdir(mk.REF):
        pytest.skip("the reference tree is not here")
    log = mk.read_log(name)
    z = np.load(os.path.join(GOLDEN, "localize_%s.npz" % name))
    assert np.array_equal(fr.log_lidar(z), log["lidar"])
    for k in ("odom", "odom_raw", "map_param", "n_frames", "real_pos", "recorded"):
        assert np.array_equal(z[k], log[k]), k


@functools.lru_cache(maxsize=None)
def replays(name):
    from oracle import oracle
    lsdmod = importlib.import_module("linesegmentdetector-slam_amd")
    oracle.build()
    return fa_logs.replay(oracle, lsdmod, name, None), fa_logs.replay(oracle, lsdmod, name, oracle.lib_cr())


@pytest.mark.parametrize("name", fr.MORE_LOGS)
def test_replay_glibc_scores_against_correctly_rounded_ones(name):
    a, b = replays(name)
    branches = [r["branch"] for _, r, _ in a]
    assert len(a) == survey_of(name)["frames"] and branches.count(fr.UKF) > len(a) // 2
    for t, ((xa, ra, ka), (xb, rb, kb)) in enumerate(zip(a, b)):
        assert ra["branch"] == rb["branch"] and ra["n_kept"] == rb["n_kept"], t
        ka, kb = np.array(ka).reshape(-1, 4), np.array(kb).reshape(-1, 4)
        assert np.allclose(ka, kb, rtol=0, atol=1e-9), t          # the same kept candidates, in the same sorted order
        assert np.allclose(xa, xb, rtol=0, atol=1e-6, equal_nan=True), (t, xa[:3], xb[:3])


@pytest.mark.parametrize("name", ANCHORED)
def test_ground_truth_figures(name):
    """The way-point errors of the correctly rounded replay equal the survey's (glibc's) within 1e-6 * mapResol metres -- the bound the
    test above puts on states, in pixels -- and a log the survey saw keep its fix keeps it."""
    glibc, cr = replays(name)
    want = survey_of(name)
    _, mp, _, _ = fr.load_log(name)
    real, rec = fr.load_way_points(name)
    tol = 1e-6 * mp[2]
    for run in (glibc, cr):
        got = fa_logs.summary(run, mp, real, rec)
        print(name, "median %.6f m (survey %.6f), max %.6f m (survey %.6f)" % (got["median_error_m"], want["median_error_m"],
                                                                             got["max_error_m"], want["max_error_m"]))
        assert abs(got["median_error_m"] - want["median_error_m"]) <= tol and abs(got["max_error_m"] - want["max_error_m"]) <= tol
        assert got["way_points_without_pose"] == want["way_points_without_pose"]
        if want["resets_after_first_fix"] == 0:
            assert got["resets_after_first_fix"] == 0
    got = fa_logs.summary(glibc, mp, real, rec)
    counts = [k for k in want if not k.endswith("_error_m")]
    assert {k: got[k] for k in counts} == {k: want[k] for k in counts}      # the survey's record, reproduced from the fixture
