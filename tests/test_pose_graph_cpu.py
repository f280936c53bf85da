"""The pose graph's restatement alone (tests/pose_graph_cases.py; include/lsd_hip.h, "pose graph"): the campaign reaches
every class, the relaxation agrees with an independent dense Gauss-Newton, the chain append -> close -> relax -> rerender pulls a loop
straight, and the records have the header's sizes.  No GPU."""
import collections
import os
import re

import numpy as np
import pytest

import pose_graph_cases as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest pose difference (pixels / degrees) between the restatement and the dense reference measured on the well-posed class was
# 1.2e-8; ten times that covers the libm of another host and CG stopping by cg_tol.
WELL_POSED_BOUND = 10 * 1.2e-8


def test_relax_campaign_reaches_every_class():
    count = collections.Counter()
    for case in pg.relax_campaign():
        count.update(pg.relax_classes_of(case, pg.run_relax_case(case)[3]))
    short = {c: count[c] for c in pg.RELAX_CLASSES if count[c] < (1 if c in pg.ONCE else 3)}
    assert not short, short


def test_build_campaigns_reach_every_class():
    count = collections.Counter()
    for case in pg.append_campaign():
        count.update(pg.append_classes_of(case, pg.run_append_case(case)[2]))
    for case in pg.near_campaign():
        count.update(pg.near_classes_of(case, pg.run_near_case(case)[1]))
    for case in pg.closure_campaign():
        count[pg.CLOSURE_NAMES[int(pg.closure(case["graph"], case["near"], case["resp"], case["par"])[1]["flags"])]] += 1
    short = {c: count[c] for c in pg.APPEND_CLASSES + pg.NEAR_CLASSES + tuple(pg.CLOSURE_NAMES.values()) if count[c] < 3}
    assert not short, short


@pytest.mark.parametrize("case", pg.well_posed(), ids=lambda c: c["name"])
def test_relaxation_agrees_with_a_dense_gauss_newton(case):
    nodes, _, rep, _ = pg.run_relax_case(case)
    ref = pg.dense_gauss_newton(case["nodes"], case["edges"])
    got = np.stack([nodes["x"], nodes["y"], nodes["ang"]], axis=1)
    diff = np.abs(got - ref)
    diff[:, 2] = np.abs([pg.wrap(v) for v in got[:, 2] - ref[:, 2]])
    print("%s: largest pose difference %.3g, %d outer iterations, %d CG steps" % (case["name"], diff.max(), rep["iters"], rep["cg_iters"]))
    assert rep["flags"] & pg.CONVERGED
    assert diff.max() <= WELL_POSED_BOUND


def test_reduction_shape_is_the_headers():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 1023, 1024, 1025, 3000):
        v = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, size=n)
        s = [0.0] * 1024
        for t in range(min(n, 1024)):
            a = float(v[t])
            for k in range(t + 1024, n, 1024):
                a = a + float(v[k])
            s[t] = a
        h = 512
        while h >= 1:
            for t in range(h):
                s[t] = s[t] + s[t + h]
            h //= 2
        assert pg.reduce_shape(v) == s[0]


def test_end_to_end_pulls_the_loop_straight():
    E = pg.end_to_end()
    n = E["n_nodes"]
    assert n == 25 and int(E["closure_rep"]["flags"]) == pg.APPENDED and int(E["near"]["anchor"]) >= 0

    def mean_error(nodes):
        return float(np.mean(np.hypot(nodes["x"][:n] - E["truth"][:n, 0], nodes["y"][:n] - E["truth"][:n, 1])))
    before, after = mean_error(E["g2"]["nodes"]), mean_error(E["g3"]["nodes"])
    ce = int(E["closure_rep"]["edge"])
    chi_before, chi_after = float(E["e_before"][ce]["chi2"]), float(E["g3"]["edges"][ce]["chi2"])
    print("mean keyframe error %.4f -> %.4f pixels (ratio %.3f); closure chi2 %.4g -> %.4g" % (before, after, after / before, chi_before, chi_after))
    assert after < before
    assert chi_after < chi_before
    pa, hi = E["planes"]
    assert pa.shape == (pg.gm.ROOM["rows"], pg.gm.ROOM["cols"]) and max(pa.shape) <= 96 and hi.sum() > 0


def test_struct_sizes_and_offsets_match_the_header():
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name, size in pg.SIZES.items():
        m = re.search(r"typedef struct %s \{.*?\} %s;[^\n]*" % (name, name), src, re.S)
        assert m, name
        assert int(re.search(r"/\* (\d+) bytes", m.group(0)).group(1)) == size, name
    dtypes = {"lsd_pg_head": pg.HEAD_DTYPE, "lsd_pg_node": pg.NODE_DTYPE, "lsd_pg_edge": pg.EDGE_DTYPE, "lsd_pg_track": pg.TRACK_DTYPE,
              "lsd_pg_append_rep": pg.APPEND_REP_DTYPE, "lsd_pg_near_rec": pg.NEAR_DTYPE, "lsd_pg_closure_rep": pg.CLOSURE_REP_DTYPE,
              "lsd_pg_relax_rep": pg.RELAX_REP_DTYPE}
    for name, dt in dtypes.items():
        assert dt.itemsize == pg.SIZES[name], name
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == list(dt.names), (name, fields)
    assert pg.NODE_DTYPE.fields["flags"][1] == 48 and pg.EDGE_DTYPE.fields["z"][1] == 16 and pg.EDGE_DTYPE.fields["chi2"][1] == 88
    assert pg.RELAX_REP_DTYPE.fields["flags"][1] == 48 and pg.NEAR_DTYPE.fields["d2"][1] == 16
    for name, value in (("LSD_PG_NODE_FIXED", pg.NODE_FIXED), ("LSD_PG_EDGE_DISABLED", pg.EDGE_DISABLED), ("LSD_PG_EDGE_CLOSURE", pg.EDGE_CLOSURE),
                        ("LSD_PG_RELAX_CONVERGED", pg.CONVERGED), ("LSD_PG_RELAX_BREAKDOWN", pg.BREAKDOWN), ("LSD_PG_RELAX_NOT_FINITE", pg.RELAX_NOT_FINITE)):
        assert re.search(r"#define %s %du" % (name, value), src), name


def test_python_mirror_has_the_same_records(lsdmod):
    for mine, theirs in ((pg.HEAD_DTYPE, lsdmod.PG_HEAD_DTYPE), (pg.NODE_DTYPE, lsdmod.PG_NODE_DTYPE), (pg.EDGE_DTYPE, lsdmod.PG_EDGE_DTYPE),
                         (pg.TRACK_DTYPE, lsdmod.PG_TRACK_DTYPE), (pg.APPEND_REP_DTYPE, lsdmod.PG_APPEND_REP_DTYPE), (pg.NEAR_DTYPE, lsdmod.PG_NEAR_DTYPE),
                         (pg.CLOSURE_REP_DTYPE, lsdmod.PG_CLOSURE_REP_DTYPE), (pg.RELAX_REP_DTYPE, lsdmod.PG_RELAX_REP_DTYPE)):
        assert mine == theirs
    for name in ("lsd_enqueue_pg_append_device", "lsd_enqueue_pg_near_device", "lsd_enqueue_pg_closure_device", "lsd_enqueue_pg_relax_device",
                 "lsd_pg_workspace_bytes", "lsd_pg_relax", "lsd_pg_append"):
        assert name in lsdmod.EXPORTED_SYMBOLS
    assert pg.RELAX_DEFAULTS == lsdmod.PG_RELAX_DEFAULTS
