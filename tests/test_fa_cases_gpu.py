"""The fusion campaign (tests/fa_cases.py) on the device: lsd_debug_fa_fuse (k_fa_fuse of csrc/k_fa.hip) against the restatement
(tests/fa_restatement.py), bit for bit -- state, P and report, one test per group.  tests/test_fa_cases_cpu.py shows that every
group reaches the boundary it was built for."""
import numpy as np
import pytest

import fa_cases as fc
import fa_restatement as fr
from test_localize_gpu import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def device(ctx, c):
    cands, last, sp, x, P = c
    st, rep = ctx.debug_fa_fuse(cands, last, sp, (x, P))
    return st.copy(), rep.copy()


def check(ctx, name, c):
    cands, last, sp, x, P = c
    st, rep = device(ctx, c)
    wx, wP, want = fr.feature_association(cands.tolist(), last, sp, list(x), P.tolist())
    try:
        same(st, wx, wP, rep, want)
    except AssertionError as e:
        raise AssertionError("case %s: %s" % (name, e)) from e
    return st, rep


def test_counts(ctx):
    """Candidate and kept counts on every wavefront, round and FA_LDS boundary at the default bound (1024 kept sort in LDS, 1025 in
    global memory); the cases with 257 and 1024 kept again with FA_LDS at and just below their count: byte-identical to the first run."""
    first = {}
    for name, c in fc.cases("counts"):
        first[name] = check(ctx, name, c)
    try:
        for name, c in fc.cases("counts"):
            k = int((c[0][:, 3] < 3).sum())
            for bound in fc.LDS_RERUNS.get(k, ()):
                ctx.debug_set_tuning("FA_LDS", bound)
                st, rep = device(ctx, c)
                assert st.tobytes() == first[name][0].tobytes() and rep.tobytes() == first[name][1].tobytes(), (name, bound)
    finally:
        ctx.debug_set_tuning("FA_LDS", 1024)


@pytest.mark.parametrize("group", [g for g in fc.GROUPS if g != "counts"])
def test_group(group, ctx):
    for name, c in fc.cases(group):
        check(ctx, name, c)
    if group == "ties":                                      # the global path keeps the same order of equal scores
        try:
            ctx.debug_set_tuning("FA_LDS", 0)
            for name, c in fc.cases(group):
                check(ctx, name + " (global)", c)
        finally:
            ctx.debug_set_tuning("FA_LDS", 1024)
