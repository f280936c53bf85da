"""The front-end campaign without a GPU (tests/front_cases.py): every class is reached, judged on the debug arrays of the correctly
rounded oracle; the glibc build and the correctly rounded build agree on everything but degMap (and on how many cases they differ
there is stated); the oracle's sorted list equals the numpy restatement of K3's rule; the packed pixel word is pinned as a numpy
function.  Every case takes part in every comparison."""
import numpy as np
import pytest

import front_cases as fc


@pytest.fixture(scope="module")
def refs(oracle):
    return {c.name: fc.reference(c, oracle) for c in fc.CASES}


def test_every_class_is_reached(refs):
    cases, counts = dict.fromkeys(fc.CLASSES, 0), dict.fromkeys(fc.CLASSES, 0)
    for c in fc.CASES:
        assert (refs[c.name][0]["w"], refs[c.name][0]["h"]) == c.wh, c                    # the size the case was built for
        for k, v in fc.classes_of(c, refs[c.name]).items():
            cases[k] += v > 0
            counts[k] += v
    print("front cases: %d cases, %d images; cases per class %s; counts per class %s" % (
        len(fc.CASES), sum(len(c.batch) for c in fc.CASES), cases, counts))
    for k in fc.CLASSES:
        assert cases[k] >= 1, k
    # what the classes do not say: the shapes, the parameters, the sequences
    shapes = {c.wh for c in fc.CASES if c.name.startswith("shape_")}
    assert len(shapes) >= 24 and {(2, 2), (2, 49), (97, 2), (32, 24), (33, 25), (64, 8), (65, 9)} <= shapes
    assert {w for w, _ in shapes} == {2, 3, 31, 32, 33, 63, 64, 65, 97} and {h for _, h in shapes} == {2, 3, 7, 8, 9, 23, 24, 25, 49}
    assert {c.wh[0] for c in fc.CASES if c.params["sca"] == 0.5} == {15, 16, 17}
    assert {c.params["angThre"] for c in fc.CASES} == {22.5, 45.0, 90.0, 1.0}
    assert {c.params["pseBin"] for c in fc.CASES} == set(fc.PSEBINS)
    for pb in fc.PSEBINS:                                                                  # every pseBin keeps pixels somewhere
        assert any(d["nb"] > 0 for c in fc.CASES if c.params["pseBin"] == pb for d in refs[c.name]), pb
    for pb in (65, 257):                                                                   # the top bit of the peer search on either side of 2^k + 1
        assert any(fc.classes_of(c, refs[c.name])["top_bit_peers"] for c in fc.CASES if c.params["pseBin"] == pb), pb
    for _, calls in fc.SEQUENCES:
        assert len({(fc.BY_NAME[n].batch.shape, tuple(sorted(fc.BY_NAME[n].params.items()))) for n in calls}) == 1


def test_sequences_put_a_blank_image_where_a_dense_one_was(refs):
    """Image 1 of the mixed call is blank where the dense call's image 1 keeps pixels in every wave that owns any; the other two
    images are the same in both, so only the blank image's state can be left over from the call before."""
    dense, mixed, blank = (refs[n] for n in ("seq_dense", "seq_blank_at_1", "seq_all_blank"))
    assert dense[1]["nb"] > 0 and dense[1]["maxGrad"] > 0 and (fc.kept_per_wave(dense[1])[:15] > 0).all()
    assert mixed[1]["nb"] == 0 and mixed[1]["maxGrad"] == 0
    assert mixed[0] is not mixed[1] and np.array_equal(mixed[0]["mag"], dense[0]["mag"]) and np.array_equal(mixed[2]["mag"], dense[2]["mag"])
    assert all(d["nb"] == 0 and d["maxGrad"] == 0 for d in blank)


def test_the_oracle_builds_agree_on_everything_but_the_angle(oracle, refs):
    differ, pixels = [], 0
    for c in fc.CASES:
        for i, (a, b) in enumerate(zip(fc.reference(c, oracle, cr=False), refs[c.name])):
            for k in ("gauss", "mag", "used0", "used", "ord_v", "ord_x", "ord_y"):
                assert a[k].tobytes() == b[k].tobytes(), (c, i, k)
            assert a["maxGrad"] == b["maxGrad"] and a["nb"] == b["nb"], (c, i)
            assert np.abs(a["deg"].view(np.int64) - b["deg"].view(np.int64)).max() <= 1, (c, i)
            k = int((a["deg"] != b["deg"]).sum())
            if k:
                pixels += k
                differ.append(c.name)
    differ = sorted(set(differ))
    print("front cases: degMap of the glibc build differs from the correctly rounded build's on %d of %d cases, %d pixels (1 ulp each): %s"
          % (len(differ), len(fc.CASES), pixels, differ))
    assert len(differ) > 0                                  # bit for bit against lib_cr asks more than DEG_ULP against glibc


def test_sorted_list_equals_the_restated_rule(refs):
    for c in fc.CASES:
        for i, d in enumerate(refs[c.name]):
            px, v = fc.sort_rule(d["mag"], d["maxGrad"], c.params["pseBin"])
            assert len(px) == d["nb"], (c, i)
            assert np.array_equal(px, d["ord_y"].astype(np.int64) * d["w"] + d["ord_x"]), (c, i)
            assert np.array_equal(v, d["ord_v"]), (c, i)


def test_gradient_restatement_and_threshold_codes(refs):
    """gradients() is what the class predicates stand on: its magnitude is the oracle's, and the code after the gradient pass is
    mag < gradThre off row 0 / column 0 (myLSD.cpp:165-166) with gradThre == 2 exactly at 90 degrees."""
    assert 2.0 / np.sin(90.0 / 180.0 * np.pi) == 2.0
    for c in fc.CASES:
        thre = 2.0 / np.sin(c.params["angThre"] / 180.0 * np.pi)
        for i, d in enumerate(refs[c.name]):
            gx, gy = fc.gradients(d["gauss"])
            assert np.array_equal(np.sqrt(gx * gx + gy * gy), d["mag"]), (c, i)
            code = (d["mag"] < thre).astype(np.uint8)
            code[0], code[:, 0] = 0, 0
            assert np.array_equal(code, d["used0"]), (c, i)


def test_near_tie_restatement(oracle, refs):
    """front_cases.grad_ties on hand-made angles (the rule's threshold is 1e-6 below pi, the window 1e-14 wide), and its count over
    the campaign, printed: the GPU test holds LSD_DBG_GRAD_TIES to it image by image."""
    import ctypes as C
    L = oracle.lib_cr()
    L.cr_atan2.restype, L.cr_atan2.argtypes = C.c_double, [C.c_double, C.c_double]
    pi = 3.14159265358979323846
    fake = lambda a: (lambda x, y: a)
    g = np.zeros((2, 2)); g[1, 1] = 1.0                                                    # one pixel with a gradient
    for a, deg, want in ((pi - 1e-6, pi - 1e-6, 1), (pi - 1e-6 + 4e-15, 0.0, 1), (pi - 1e-6 - 2e-14, pi - 1e-6 - 2e-14, 0), (pi, 0.0, 0),
                         (1.0, 1.0, 0)):
        d = {"gauss": g, "deg": np.array([[0.0, 0.0], [0.0, deg]])}
        assert fc.grad_ties(d, fake(a)) == want, a
    total = sum(fc.grad_ties(d, L.cr_atan2) for c in fc.CASES for d in refs[c.name])
    print("front cases: %d near ties of the gradient pass over the campaign" % total)


def test_packed_word_restatement():
    """float32 of the angle, round to nearest even, low two mantissa bits replaced by the code."""
    one = np.float32(1.0).view(np.uint32)
    u = 2.0 ** -23                                                                         # an ulp of 1.0f
    # 1 + 2.5 u ties to the even 1 + 2 u (word + 2, masked to + 0); 1 + 3.5 u ties to 1 + 4 u, where truncation would leave + 3 -> + 0
    deg = np.array([0.0, -0.0, 1.0, 1.0 + 2.5 * u, 1.0 + 3.5 * u, 1.0 + 3.5 * u * (1 - 2.0 ** -20), 1.0 + 7 * u, np.pi, -np.pi])
    got = fc.pw_of(deg, [0, 1, 0, 1, 0, 0, 1, 1, 0])
    want = [0, 0x80000001, one, one | 1, one + 4, one, (one + 4) | 1, 0x40490fd9, 0xc0490fd8]
    assert got.tolist() == [int(v) for v in want]
    assert fc.pw_of(np.zeros((2, 3)), np.ones((2, 3), np.uint8)).shape == (2, 3)

