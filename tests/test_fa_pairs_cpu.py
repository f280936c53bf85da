"""The pair list on hand-made lines (tests/pair_cases.py) without a GPU: fa_restatement.pairs and the package's match_pairs against
the two-line loop of the reference written out here, the thresholds one by one, and the whole frame under the oracle's matching --
which shows that the frames the GPU test runs reach pairs, kept candidates and the filter."""
import math

import numpy as np
import pytest

import fa_restatement as fr
import pair_cases as pc


def loop_pairs(map_len, scan_len):
    """LSD/myFA.cpp:28-58: scan line outer, map line inner, the two conditions as written there."""
    out = []
    for cntScanLine in range(len(scan_len)):
        lenScanLine = float(scan_len[cntScanLine])
        if lenScanLine < 40:
            continue
        lenDiff = lenScanLine * 0.35
        for cntMapLine in range(len(map_len)):
            lenMapLine = float(map_len[cntMapLine])
            if lenMapLine < lenScanLine - lenDiff or lenMapLine > lenScanLine + lenDiff:
                continue
            out.append((cntMapLine, cntScanLine))
    return out


@pytest.mark.parametrize("name,mp,scan,last", pc.cases(), ids=[c[0] for c in pc.cases()])
def test_pairs_equal_the_reference_loop(name, mp, scan, last, lsdmod):
    want = loop_pairs(mp["len"], scan["len"])
    assert fr.pairs(mp["len"], scan["len"]) == want
    assert np.array_equal(lsdmod.match_pairs(mp, scan), np.array(want, np.int32).reshape(-1, 2))


def test_length_thresholds_one_by_one():
    assert 40.0 * 0.35 == 14.0 and pc.MAP_LENGTHS[:4] == (26.0, math.nextafter(26.0, 0.0), 54.0, math.nextafter(54.0, math.inf))
    every = set(range(len(pc.MAP_LENGTHS)))
    want = {"below40": set(), "40": {0, 2, 4, 6}, "nan": every, "inf": every}      # 26, 54, NaN and 40 against ls = 40
    for name, ls in pc.SCAN_LENGTHS:
        mp, scan = pc.length_case(ls)
        assert math.hypot(scan["dx"][1], scan["dy"][1]) == 40.0                   # real end points, the length overwritten
        pr = fr.pairs(mp["len"], scan["len"])
        assert {cm for cm, cs in pr if cs == 1} == want[name], name
        assert {cm for cm, cs in pr if cs == 0} == {2, 3, 4, 6} and not [p for p in pr if p[1] == 2]      # the ordinary 44 (28.6..59.4, NaN passes, inf does not), the short 30
        assert pr == sorted(pr, key=lambda p: (p[1], p[0]))                       # scan line outer, map line inner


def test_counts_reach_the_round_boundaries():
    assert set(pc.COUNTS) == {(0, 5), (5, 0), (1, 1), (16, 16), (15, 17), (17, 15), (1, 257), (257, 1), (360, 3)}
    assert {a * b for a, b in pc.COUNTS} >= {0, 1, 255, 256, 257}
    for n_scan, n_map in pc.COUNTS:
        mp, scan = pc.count_case(n_scan, n_map)
        assert (len(scan), len(mp)) == (n_scan, n_map)
        pr = fr.pairs(mp["len"], scan["len"])
        long_scan, long_map = (n_scan + 1) // 2, n_map - n_map // 4
        assert len(pr) == long_scan * long_map
        if n_scan * n_map >= 255:
            assert 0 < len(pr) < n_scan * n_map                                   # holes in the compaction
    for mp, scan in (pc.count_case(360, 3), pc.length_case(40.0)):               # every segment lies on a wall of the room
        for l in list(mp) + list(scan):
            assert pc.X0 <= min(l["x1"], l["x2"]) and max(l["x1"], l["x2"]) <= pc.X1 and pc.Y0 <= min(l["y1"], l["y2"]) and max(l["y1"], l["y2"]) <= pc.Y1


def test_frames_reach_kept_candidates_and_the_filter(oracle):
    m = pc.room()
    assert m.shape == (64, 96) and 24 <= len(pc.points()) <= 60
    mc = oracle.map_cache(m.copy(), pc.RES)
    x0, P0 = pc.state()
    seen = set()
    for name, mp, scan, last in pc.cases():
        pr = np.array(fr.pairs(mp["len"], scan["len"]), np.int32).reshape(-1, 2)
        cands = oracle.scan_to_map_match(mc, mp, scan, pc.points(), pc.LIDAR, last, pr).reshape(-1, 4) if len(pr) else np.zeros((0, 4))
        x, P, rep = fr.feature_association(cands, last, pc.SCAN_POSE, list(x0), P0.tolist(), len(pr))
        seen.add(rep["branch"])
        if len(pr) == 0:
            assert rep["branch"] == fr.RESET, name
        else:
            assert rep["n_kept"] > 0 and rep["branch"] == (fr.FIRST if last == pc.FIRST else fr.UKF), (name, rep["n_kept"])
            assert not any(math.isnan(v) for v in x), name
    assert seen == {fr.RESET, fr.FIRST, fr.UKF}
