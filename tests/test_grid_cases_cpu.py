"""The mapping campaign (tests/grid_cases.py) under the restatement alone: every class is reached, every ray is the 8-connected line the
closed form promises, round() is what the half-way class depends on, and the publish rule on hand-made counters.  No GPU."""
import numpy as np
import pytest

import grid_cases as gc


@pytest.fixture(scope="module")
def traced(oracle):
    """(case, pass, hit, trace, classes) of every case of the campaign, computed once."""
    out = []
    for case in gc.campaign():
        pa, hi, trace = gc.run_case(case)
        out.append((case, pa, hi, trace, gc.classes_of(case, trace)))
    return out


def test_every_class_is_reached(traced):
    count = {c: 0 for c in gc.CLASSES}
    for case, _, _, _, classes in traced:
        assert classes <= set(gc.CLASSES), classes - set(gc.CLASSES)
        assert case["cols"] <= gc.MAX_COLS and case["rows"] <= gc.MAX_ROWS
        for c in classes:
            count[c] += 1
    for c, n in count.items():
        assert n >= (1 if c == "scan_len_1025" else 3), (c, n)


def test_every_ray_is_a_connected_line(traced):
    rays = 0
    for case, _, _, trace, _ in traced:
        for t in trace:
            if t["skip"]:
                continue
            cells = t["cells"]
            n = max(abs(t["x1"] - t["x0"]), abs(t["y1"] - t["y0"]))
            assert len(cells) == n + 1 and len(set(map(tuple, cells.tolist()))) == n + 1
            assert tuple(cells[0]) == (t["x0"], t["y0"]) and tuple(cells[-1]) == (t["x1"], t["y1"])
            if n:
                step = np.abs(np.diff(cells, axis=0))
                assert step.max() == 1 and (step.max(axis=1) == 1).all()           # 8-connected, never standing still
            rays += 1
    assert rays > 3000


def test_counts_are_the_sum_of_the_rays(traced):
    """The planes against the trace: pass is the number of rays through a cell, hit the number of hitting rays that end in it."""
    for case, pa, hi, trace, _ in traced:
        want_p, want_h = np.zeros_like(pa), np.zeros_like(hi)
        for t in trace:
            if t["skip"]:
                continue
            for (x, y), ins in zip(t["cells"], t["inside"]):
                if ins:
                    want_p[y, x] += 1
            if t["hits"] and t["inside"][-1]:
                want_h[t["y1"], t["x1"]] += 1
        assert np.array_equal(pa, want_p) and np.array_equal(hi, want_h), case["name"]
        assert (hi <= pa).all()


def test_rint_would_change_the_half_way_class(traced):
    changed = 0
    for case, pa, hi, _, classes in traced:
        if "half_way" not in classes:
            continue
        pa2, hi2, _ = gc.run_case(case, rnd=gc.c_rint)
        changed += int(not (np.array_equal(pa, pa2) and np.array_equal(hi, hi2)))
    assert changed >= 1
    assert gc.c_round(2.5) == 3 and gc.c_rint(2.5) == 2 and gc.c_round(-2.5) == -3 and gc.c_round(0.49999999999999994) == 0
    assert gc.cvt_x86(float("nan")) == gc.INT_MIN and gc.cvt_x86(-7.9) == -7 and gc.cvt_x86(2147483648.0) == gc.INT_MIN


def test_accumulation_and_wrap(traced):
    """The planes are added to, modulo 2^32."""
    case, pa, hi, _, _ = traced[0]
    base_p = np.full_like(pa, 0xFFFFFFFF)
    base_h = np.arange(pa.size, dtype=np.uint32).reshape(pa.shape)
    pa2, hi2, _ = gc.run_case(case, pass_counts=base_p, hit_counts=base_h)
    assert np.array_equal(pa2, base_p + pa) and np.array_equal(hi2, base_h + hi)     # (uint32 sums wrap)
    assert (pa2[pa > 0] == pa[pa > 0] - 1).all()


def test_publish_rule_on_hand_made_counters():
    u = lambda *v: np.array(v, np.uint32)
    # below and at min_pass
    assert gc.publish(u(1, 2, 0), u(1, 2, 0)).tolist() == [-1, 100, -1]
    assert gc.publish(u(4, 5), u(0, 5), min_pass=5).tolist() == [-1, 100]
    assert gc.publish(u(0), u(0), min_pass=0).tolist() == [100]                        # 0 * den >= 0 * num
    # hit * den == pass * num exactly, and one either side
    assert gc.publish(u(20, 20, 20), u(1, 2, 3)).tolist() == [0, 100, 100]
    assert gc.publish(u(30, 30, 30), u(9, 10, 11), occ_num=1, occ_den=3).tolist() == [0, 100, 100]
    assert gc.publish(u(7, 7), u(6, 7), occ_num=1, occ_den=1).tolist() == [0, 100]
    # products beyond 2^32: 32-bit arithmetic would wrap them
    big = 0xFFFFFFFF
    assert gc.publish(u(big, big, big), u(429496729, 429496730, big)).tolist() == [0, 100, 100]   # 10 h against big: 4294967290 < big <= 4294967300
    assert gc.publish(u(4000000000), u(3000000000), occ_num=3, occ_den=4).tolist() == [100]       # 12e9 == 12e9
    assert gc.publish(u(4000000000), u(2999999999), occ_num=3, occ_den=4).tolist() == [0]
    assert gc.publish(u(1 << 31), u(1 << 30), occ_num=1, occ_den=2).tolist() == [100]              # 2^31 * 1 == 2^30 * 2: both wrap to 0 in 32 bits
    assert gc.publish(u(1 << 31), u((1 << 30) - 1), occ_num=1, occ_den=2).tolist() == [0]
