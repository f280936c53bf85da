"""The line-record campaign without a GPU (tests/line_cases.py): every class is reached, judged on the correctly rounded oracle's
records; the numpy restatement of myLSD.cpp:280-368 from the four end points equals the oracle's k, b, len, orient and lineIm to the
bit on every case (dx / dy stay the oracle's: they need the correctly rounded sin / cos / atan); and how many cases' record bytes differ
between the glibc build and the correctly rounded build of the oracle is printed, with no threshold."""
import numpy as np
import pytest

import line_cases as lc


@pytest.fixture(scope="module")
def refs(oracle):
    return {repr(c): lc.reference(c, oracle) for c in lc.CASES + lc.batch_cases()}


def test_every_class_is_reached(refs):
    """The condition that keeps the campaign from quietly covering nothing: at least three cases per class (one for "over 128
    samples" and "over 8 lines"), by the records of oracle.lib_cr()."""
    cases, lines = dict.fromkeys(lc.CLASSES, 0), dict.fromkeys(lc.CLASSES, 0)
    for c in lc.CASES:
        for k, v in lc.classes_of(refs[repr(c)]["lines"], *c.map.shape).items():
            cases[k] += v > 0
            lines[k] += v
    print("line cases: %d cases, %d lines; cases per class %s; lines per class %s" % (
        len(lc.CASES), sum(len(refs[repr(c)]["lines"]) for c in lc.CASES), cases, lines))
    for k in lc.CLASSES:
        assert cases[k] >= lc.NEED[k], (k, cases[k])
    assert {c.sca for c in lc.CASES} == {0.3, 0.5, 1.0}
    for sca in (0.3, 0.5, 1.0):                             # lines at every scale (sca == 1 skips the rescale of :252-258)
        assert sum(len(refs[repr(c)]["lines"]) for c in lc.CASES if c.sca == sca) >= 50


def test_batch_maps_are_what_the_compaction_needs(refs):
    bc = lc.batch_cases()
    counts = [len(refs[repr(c)]["lines"]) for c in bc]
    assert len({c.map.tobytes() for c in bc}) == 16 and all(c.map.shape == (96, 128) for c in bc)
    assert [i for i, n in enumerate(counts) if n == 0] == list(lc.BATCH_NO_LINE)
    assert {1, 2, 3} <= set(counts) and max(counts) > 8     # below, at and above a capacity of 2; more than two wave strides
    for n in lc.BATCH_SIZES:
        idx = lc.batch_indices(n)
        assert len(idx) == n and counts[idx[0]] == 0 and counts[idx[-1]] == 0
        if n > 16:
            assert any(counts[i] == 0 for i in idx[1:-1]) and any(counts[i] > 2 for i in idx)


def test_restatement_equals_the_oracle_bit_for_bit(refs):
    bad = []
    for c in lc.CASES:
        r = refs[repr(c)]
        L = r["lines"]
        k, b, ln, orient = lc.fields_from_endpoints(L["x1"], L["y1"], L["x2"], L["y2"])
        for name, got in (("k", k), ("b", b), ("len", ln), ("orient", orient)):
            if got.tobytes() != np.ascontiguousarray(L[name]).tobytes():
                bad.append((repr(c), name))
        if not np.array_equal(lc.raster(L, *c.map.shape), r["lineIm"]):
            bad.append((repr(c), "lineIm"))
    assert not bad, bad


def test_restatement_on_hand_made_end_points():
    """What no map reaches (k NaN) and the corners of the conversion rules."""
    k, b, ln, orient = lc.fields_from_endpoints([3.0, 3.0, 5.0, 2.0, 2.0], [4.0, 4.0, 4.0, 7.0, 1.0], [3.0, 3.0, 9.0, 2.0, 6.0],
                                                [4.0, 1.0, 4.0, 9.0, 1.0 - 1e-300])
    assert np.isnan(k[0]) and np.isnan(b[0]) and ln[0] == 0 and orient[0] == 1
    assert k[1] == -np.inf and orient[1] == -1 and k[3] == np.inf and orient[3] == 1
    assert k[2] == 0 and not np.signbit(k[2]) and orient[2] == 1 and b[2] == 4.0
    s = lc.samples(3.0, 4.0, 3.0, 4.0, 10, 10)              # NaN: one sample, its conversion overflows, nothing is marked
    assert not s.along_x and len(s.xx) == 1 and s.xx[0] == lc.INT_MIN and not s.inside.any()
    s = lc.samples(0.5, 2.5, 6.5, 2.5, 10, 10)              # halves round away from zero; column 0 is inside and not marked
    assert s.along_x and list(s.xx) == list(range(0, 8)) and set(s.yy) == {3} and s.inside.all() and list(s.marked) == [False] + [True] * 7
    s = lc.samples(-2.5, -1.5, 3.0, -1.5, 10, 10)
    assert set(s.yy) == {-2} and not s.inside.any()
    assert lc._round(np.array([0.49999999999999994, -0.5, 2.5, -2.5000000000000004])).tolist() == [0.0, -1.0, 3.0, -3.0]
    assert lc._cvt(np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, -1.9, 1.9])).tolist() == [lc.INT_MIN] * 5 + [-1, 1]


def test_glibc_and_correctly_rounded_records(oracle, refs):
    """Recorded, not judged: on how many cases the glibc build's record bytes differ from the correctly rounded build's."""
    differ = []
    for c in lc.CASES:
        g = oracle.lsd(c.map.copy(), **c.params)
        if g["lines"].tobytes() != refs[repr(c)]["lines"].tobytes():
            differ.append(repr(c))
    print("line cases: the glibc build's record bytes differ from the correctly rounded build's on %d of %d cases %s" % (
        len(differ), len(lc.CASES), differ))


def test_hand_made_end_points_reach_what_no_map_does(monkeypatch, lsdmod):
    """HAND_RECS (test f of the GPU file): rint in place of round changes marked pixels of the x walk alone and of the y walk alone,
    row 1 / column 1 samples that rint would move onto the unmarked row 0 / column 0 among them; one record has k NaN; one walk is
    longer than two 64-lane strides; there are more records than two strides of the four wavefronts."""
    recs = lc.HAND_RECS
    rows, cols = lc.HAND_ROWS, lc.HAND_COLS
    k, b, ln, orient = lc.fields_from_endpoints(*recs.T)
    assert np.isnan(k).sum() == 1 and np.isinf(k).sum() >= 2 and (k == 0).sum() >= 2 and len(recs) > 8
    walks = [lc.samples(*r, rows, cols) for r in recs]
    assert max(len(s.xx) for s in walks) > 128
    assert any(s.inside.any() and not s.inside.all() for s in walks)                       # a walk that leaves the image
    L = np.zeros(len(recs), lsdmod.LINE_DTYPE)
    L["x1"], L["y1"], L["x2"], L["y2"] = recs.T
    along_x = np.array([s.along_x for s in walks])
    want = {g: lc.raster(L[along_x == g], rows, cols) for g in (True, False)}
    monkeypatch.setattr(lc, "_round", np.rint)
    for g in (True, False):
        mutant = lc.raster(L[along_x == g], rows, cols)
        lost = (want[g] == 255) & (mutant == 0)
        assert lost.sum() >= 20, (g, int(lost.sum()))
        assert lost[1, :].any() if g else lost[:, 1].any()                                   # pixels rint moves onto row 0 / column 0


def test_default_host_capacity_is_the_header_s(lsdmod):
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsd_hip.h")).read()
    m = re.search(r"Line capacity per image of the host entry points above \(default (\d+);", src)
    assert m and int(m.group(1)) == lsdmod.HOST_MAX_LINES_DEFAULT
    ctx_src = open(os.path.join(os.path.dirname(lsdmod.__file__), "csrc", "lsd_ctx.h")).read()
    assert re.search(r"int host_max_lines = %d;" % lsdmod.HOST_MAX_LINES_DEFAULT, ctx_src)
