"""The scan-side parity campaign on the CPU: what tests/scan_cases.py generates, through both builds of the oracle.

The GPU tests hold k_rdp and the matching kernel to the oracle's correctly rounded build bit for bit.  Here: that build and the glibc
build agree on everything but the 1-ulp sind / cosd of a line record; the campaign reaches every edge it claims to; every matching
case shows its condition in the oracle's own result; and the oracle itself runs a slice of it clean under AddressSanitizer."""
import collections
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def campaign_refs(oracle):
    camp = sc.campaign()
    cr = oracle.lib_cr()
    return camp, [sc.reference(oracle, g, None) for g in camp], [sc.reference(oracle, g, cr) for g in camp]


def test_generator_is_deterministic_and_inside_the_domain():
    a, b = sc.campaign(reps=15), sc.campaign(reps=15)
    assert [g["name"] for g in a] == [g[0] for g in sc.GROUPS]
    for g, h in zip(a, b):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g["scans"], h["scans"]))
        assert sorted({len(s) for s in g["scans"]}) == sorted(sc.LENGTHS)
        assert g["map_param"][2] >= 0.025 and g["limit"] >= 1
        for s in g["scans"]:
            assert np.isfinite(s).all() and s[:, 0].min() > 0 and s[:, 0].max() <= 60
    assert {g["limit"] for g in a} == {1, 2, 3, 8} and {g["thre_line"] for g in a} == {0.01, 0.08, 0.3}
    assert {g["line_dist"] for g in a} == {0, 0.5, 2} and {g["map_param"][2] for g in a} >= {0.025, 0.2}


def test_both_oracle_builds_agree_except_for_one_ulp_of_dx_dy(campaign_refs):
    camp, glibc, cr = campaign_refs
    differing = 0
    for g, ra, rb in zip(camp, glibc, cr):
        sc.check_bounds(rb)
        for i, (a, b) in enumerate(zip(ra, rb)):
            where = (g["name"], i, g["tags"][i])
            assert a["n_lines"] == b["n_lines"] and a["im_size"] == b["im_size"] and a["lidar_pos"] == b["lidar_pos"], where
            assert a["pts"].tobytes() == b["pts"].tobytes(), where
            bad = sc.line_diffs(a["lines"], b["lines"])
            assert set(bad) <= {"dx", "dy"}, (where, bad)
            if bad:
                differing += 1
                for f in ("dx", "dy"):
                    both_nan = np.isnan(a["lines"][f]) & np.isnan(b["lines"][f])      # (a zero-length line: atand(0 / 0))
                    assert (np.abs(a["lines"][f] - b["lines"][f])[~both_nan] <= 1e-15).all(), (where, f)
    print("scans whose dx / dy differ between glibc and the correctly rounded build: %d of %d" % (differing, sum(len(g["scans"]) for g in camp)))


def test_campaign_reaches_what_it_claims(campaign_refs):
    camp, _, cr = campaign_refs
    c = collections.Counter()
    for g, refs in zip(camp, cr):
        res, ox, oy = g["map_param"][2:]
        for i, (s, r) in enumerate(zip(g["scans"], refs)):
            _, wrapped, dropped_first = sc.clusters(s, g["limit"])
            c["wrapped cluster"] += wrapped
            c["dropped first cluster before a wrap"] += dropped_first
            L = r["lines"]
            c["infinite k"] += bool(np.isinf(L["k"]).any())
            c["NaN k"] += bool(np.isnan(L["k"]).any())
            c["more than 64 chords"] += r["n_lines"] > 64
            c["n_pts > small pts_cap"] += len(r["pts"]) > sc.PTS_CAP_SMALL
            c["range above 9"] += bool((s[:, 0] > 9).any())
            # an end point of a line on column 0 (or row 0) inside the image: its raster has that pixel, the list must not
            w, h = r["im_size"]
            on0 = ((L["x1"] == 0) & (L["y1"] > 0) & (L["y1"] < h)) | ((L["y1"] == 0) & (L["x1"] > 0) & (L["x1"] < w))
            if on0.any():
                assert len(r["pts"]) == 0 or (r["pts"][:, :2] != 0).all()
                c["pixel dropped by the 0-is-invalid rule"] += 1
            X = np.floor((s[:, 0] * np.cos(s[:, 1]) - ox) / res)
            if (X < 0).all():
                assert abs(w - np.ceil(0 - X.min())) <= 1        # maxX stayed at its initial 0 (+-1: numpy's cos is not the oracle's)
                c["all pixel columns negative"] += 1
            if g["tags"][i] == "nine_0" and len(s) >= 20:
                at, below, above = (refs[i + d]["n_lines"] for d in range(3))
                assert at == below and above < at, (g["name"], i, at, below, above)     # 9 and 9 - ulp split, 9 + ulp does not
                c["split decided by r > 9"] += 1
            if g["tags"][i] == "tie" and len(s) >= 20 and g["line_dist"] == 0:
                assert r["n_lines"] == 3, (g["name"], i)           # the first of the two equally far readings was taken
                c["exact tie, first wins"] += 1
    print(dict(c))
    for what in ("wrapped cluster", "dropped first cluster before a wrap", "infinite k", "NaN k", "more than 64 chords", "n_pts > small pts_cap",
                 "range above 9", "pixel dropped by the 0-is-invalid rule", "all pixel columns negative", "split decided by r > 9",
                 "exact tie, first wins"):
        assert c[what] >= 1, what


def test_delta_step_family_sits_on_every_step():
    seen = set()
    for g in sc.campaign(reps=15):
        for s, t in zip(g["scans"], g["tags"]):
            if t == "delta_steps":
                for step in sc.DELTA_STEPS:
                    for v in (np.nextafter(step, 0), step, np.nextafter(step, 9)):
                        if (s[:, 0] == v).any():
                            seen.add((float(step), float(v - step)))
    assert len(seen) == 3 * len(sc.DELTA_STEPS)


def _oracle_scores(oracle, c):
    return oracle.scan_to_map_match(*sc.case_args(c), _lib=oracle.lib_cr())


def test_matching_edge_cases_show_their_condition_in_the_oracle(oracle):
    cases = {c["name"]: c for c in sc.edge_cases()}
    # directions: count the branches from the restatement, then the oracle's wrapped angle for the +-180 / +-360 candidates
    c = cases["directions"]
    want = _oracle_scores(oracle, c)
    seen, pre = collections.Counter(), {}
    for p, (im, isc) in enumerate(c["pairs"]):
        for i in (1, 2, 3, 4):
            m, s = sc.candidate_ends(c["map_lines"][im], c["scan_lines"][isc], i)
            (am, bm, fm), (as_, bs, fs) = sc.line_direction(*m), sc.line_direction(*s)
            for b, f in ((bm, fm), (bs, fs)):
                seen[b] += 1; seen[f] += 1
            pre.setdefault(am - as_, []).append(want[p, i - 1, 2])
    assert all(seen[k] > 0 for k in ("vertical", "horizontal", "atan", "+180", "-180")), seen
    assert all(a == 180.0 for a in pre[180.0]) and all(a == 180.0 for a in pre[-180.0])      # (-180, 180]
    assert all(a == 0.0 for a in pre[360.0]) and all(a == 0.0 for a in pre[-360.0])
    assert np.isnan(want[:, :, 2]).any()                                                  # the zero-length line: atand(0 / 0)
    for name, c in cases.items():
        want = _oracle_scores(oracle, c)
        e = c["expect"]
        if "score0" in e:
            assert want[0, 0, 3] == e["score0"], (name, want[0, 0], e["score0"])
        if "n_points" in e:
            assert len(c["pts"]) == e["n_points"] and (np.isinf(want[:, :, 3]).all() if e["n_points"] == 0 else np.isfinite(want[:, :, 3]).any())
        if "n_pairs" in e:
            assert want.shape == (e["n_pairs"], 4, 4)
    assert {c["expect"]["n_points"] for c in cases.values() if "n_points" in c["expect"]} == {0, 1, 7, 8, 9, 17}
    assert {c["expect"]["n_pairs"] for c in cases.values() if "n_pairs" in c["expect"]} == {1, 15, 16, 17, 1000}
    assert cases["max_dist_at"]["last"][0] == 7.0 - 60.0 and (cases["z_occ"]["map_cache"] == 1.0).sum() == 3


def test_feature_scan_lines_take_the_axis_aligned_branches(maps, maps_meta, oracle):
    cases = sc.feature_scan_match_cases(oracle, maps, maps_meta, oracle.lib_cr())
    assert len(cases) >= 6
    kinds = collections.Counter()
    for c in cases:
        L = c["scan_lines"]
        assert np.array_equal(L["x1"], np.round(L["x1"])) and np.array_equal(L["y2"], np.round(L["y2"]))
        kinds["vertical"] += int(((L["x1"] == L["x2"]) & (L["y1"] != L["y2"])).sum())
        kinds["horizontal"] += int(((L["x1"] != L["x2"]) & (L["y1"] == L["y2"])).sum())
        want = _oracle_scores(oracle, c)
        kinds["finite"] += int(np.isfinite(want[:, :, 3]).sum())
        kinds["at_z_occ"] += int((c["map_cache"] == c["z_occ"]).sum() > 0)
    assert kinds["vertical"] > 0 and kinds["horizontal"] > 0 and kinds["finite"] > 0 and kinds["at_z_occ"] == len(cases), kinds


def test_oracle_runs_a_slice_of_the_campaign_asan_clean(oracle):
    """The oracle's AddressSanitizer pass (test_oracle.py) extended to FeatureScan and the matching: every 7th scan of every group
    (every length and family among them), every matching edge case."""
    so = oracle.build(asan=True)
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from oracle import oracle\n"
        "import scan_cases as sc\n"
        "L = oracle.lib(%r)\n"
        "n = 0\n"
        "for g in sc.campaign():\n"
        "    n += len(sc.reference(oracle, g, L, range(0, len(g['scans']), 7)))\n"
        "for c in sc.edge_cases():\n"
        "    oracle.scan_to_map_match(*sc.case_args(c), _lib=L)\n"
        "assert n > 700\n"
        "print('OK')\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), so)
    asan = sorted(glob.glob("/usr/lib/gcc/x86_64-linux-gnu/*/libasan.so"))
    if not asan:
        pytest.skip("libasan not installed")
    env = dict(os.environ, LD_PRELOAD=asan[-1], ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, p.stderr[-2000:]
