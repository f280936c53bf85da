"""The createMapCache campaign (tests/mapcache_cases.py) on the CPU: the restatement equals the oracle bit for bit on every case, and
every class reaches what it was built for -- otherwise tests/test_mapcache_cases_gpu.py would pass without exercising anything.
The last test measures how deep the floods of the map fixtures are against the levels the spread path plans."""
import numpy as np
import pytest

import mapcache_cases as mc
from conftest import tile2048

_floods = {}


def flood_of(c):
    if c.name not in _floods:
        _floods[c.name] = mc.flood(c.map, c.res, c.z)
    return _floods[c.name]


@pytest.mark.parametrize("cls", mc.CLASSES)
def test_restatement_equals_the_oracle(cls, oracle):
    assert mc.cases(cls)
    for c in mc.cases(cls):
        want = oracle.map_cache(c.map.copy(), c.res, c.z)
        assert flood_of(c).values.tobytes() == want.tobytes(), c


def test_detours_outlive_the_plan():
    """Depth at least planned + 1, so that k_mc_finish claims cells, at radius 10, radius 20 and z_occ_max_dis = 2.0; one case ends on
    the planned count exactly: its frontier is not empty when the plan ends, but nothing more is claimed."""
    seen = set()
    for c in mc.cases("detour"):
        f = flood_of(c)
        if c.name.endswith("exactly_planned"):
            assert f.depth == c.planned and f.frontiers[c.planned] > 0, (c, f.depth, c.planned)
        else:
            assert f.depth >= c.planned + 1, (c, f.depth, c.planned)
            seen.add((mc.cell_radius(c.res, c.z), c.z))
        assert c.planned == int(1.5 * mc.cell_radius(c.res, c.z)) + 3            # not the cap
        print("detour %-28s radius %2d depth %2d planned %2d cells past the plan %d" %
              (c.name, mc.cell_radius(c.res, c.z), f.depth, c.planned, int((f.level > c.planned).sum())))
    assert (10, 1.0) in seen and (20, 1.0) in seen and any(z == 2.0 for _, z in seen)
    assert any(c.name.endswith("exactly_planned") for c in mc.cases("detour"))
    assert flood_of(mc.BY_NAME["detour_r10_witness"]).depth == 25


def test_radius_cases_are_cut_off():
    radii = set()
    for c in mc.cases("radius"):
        f, r = flood_of(c), mc.cell_radius(c.res, c.z)
        radii.add(r)
        rows, cols = c.map.shape
        if c.name == "beyond_map":                           # nothing is cut off, and the plan is capped below 1.5 * radius + 3
            assert f.stopped == 0 and (f.level >= 0).all()
            assert c.planned == rows + cols < int(1.5 * r) + 3
        else:
            assert f.stopped > 0 and (f.level < 0).any(), c
        if r == 0:                                           # the neighbours of sources get 0 and nothing else is touched
            assert f.depth == 1 and not f.values[f.level >= 0].any() and (f.values[f.level < 0] == c.z).all()
    assert radii >= {0, 1, 2, 3, 5, 19, 20, 40, 100}
    q = {c.name: mc.cell_radius(c.res, c.z) for c in mc.cases("radius") if c.name.startswith("q_")}
    assert q == {"q_0.3_0.1": 2, "q_1.0_0.2": 5, "q_2.0_0.05": 40, "q_res_above_0.05": 19, "q_res_below_0.05": 20, "q_res_0.05": 20}
    assert 0.3 / 0.1 < 3.0 and 1.0 / 0.2 == 5.0 and 2.0 / 0.05 == 40.0
    print("radius: %d cases, radii %s, nodes stopped %d" % (len(mc.cases("radius")), sorted(radii),
                                                             sum(flood_of(c).stopped for c in mc.cases("radius"))))


def test_tie_cases_depend_on_the_queue_order():
    win, lose = np.zeros(4, int), np.zeros(4, int)
    for c in mc.cases("ties"):
        f = flood_of(c)
        assert f.sensitive > 0, c
        win += f.winners
        lose += f.losers
    assert (win > 0).all() and (lose > 0).all(), (win, lose)
    print("ties: %d cases, order-sensitive cells %d, winners %s losers %s (up, left, down, right)" %
          (len(mc.cases("ties")), sum(flood_of(c).sensitive for c in mc.cases("ties")), win.tolist(), lose.tolist()))


def test_shapes_cover_the_small_and_the_boundaries():
    shapes = {c.map.shape for c in mc.cases("shapes")}
    assert shapes >= {(1, 1), (1, 65), (65, 1), (2, 2), (3, 3)}
    assert {s[1] for s in shapes} >= {63, 64, 65}
    assert {s[0] * s[1] for s in shapes} >= {1023, 1024, 1025}
    assert any(s[0] * s[1] < 64 for s in shapes)                                  # fewer cells than the spread path has chunks
    corners = [c for c in mc.cases("shapes") if min(c.map.shape) > 1 and
               all(c.map[i, j] == 1 for i in (0, -1) for j in (0, -1))]
    assert corners
    b = mc.BY_NAME["borders_36x36"].map
    assert all((edge == 1).sum() > 3 for edge in (b[0], b[-1], b[:, 0], b[:, -1]))
    print("shapes: %d cases, %s" % (len(mc.cases("shapes")), sorted(shapes)))


def test_frontier_sizes_sit_on_the_round_boundaries():
    level0 = {flood_of(c).frontiers[0] for c in mc.cases("frontier")}
    assert level0 >= {1023, 1024, 1025, 2500}
    later = {c.name: max(flood_of(c).frontiers[1:]) for c in mc.cases("frontier")}
    assert later["checker_64x64"] == 2048 and later["lattice3_96x96"] > 2048
    assert flood_of(mc.BY_NAME["lattice3_96x96"]).frontiers[0] == 1024
    print("frontier: level 0 %s, largest later frontier %s" % (sorted(level0), later))


def test_values_only_one_is_occupied():
    m = mc.BY_NAME["mixed_40x52"].map
    assert set(np.unique(m)) == {0, 1, 2, 100, 254, 255}
    f = flood_of(mc.BY_NAME["mixed_40x52"])
    assert np.array_equal(f.level == 0, m == 1)
    for name in ("empty_36x36", "empty_of_255"):
        f = flood_of(mc.BY_NAME[name])
        assert (f.values == 1.0).all() and f.frontiers == []
    f = flood_of(mc.BY_NAME["full_36x36"])
    assert not f.values.any() and f.depth == 0
    print("values: %d cases, cell values %s" % (len(mc.cases("values")), sorted(set(np.unique(m)))))


@pytest.mark.parametrize("num_cus", [256, 128])
def test_batches_select_both_paths(num_cus):
    """G = min(64, 2 * num_cus // n): the one-workgroup kernel below 4, the smallest spread at 4, the cap of 64 at three maps."""
    G = lambda n: min(64, 2 * num_cus // n)
    assert G(mc.batch_size("one_workgroup", num_cus)) < 4 and G(mc.batch_size("smallest_spread", num_cus)) == 4
    assert G(mc.batch_size("three", num_cus)) == 64
    b = mc.batch("one_workgroup", num_cus)
    assert b.shape == (num_cus // 2 + 1, 64, 64) and b.dtype == np.uint8
    assert len({m.tobytes() for m in b}) == len(b)                                 # not one map repeated
    fl = [mc.flood(m, mc.BATCH_RES, mc.BATCH_Z) for m in b[:len(mc.BATCH_CORE)]]
    planned = mc.planned_levels(64, 64, mc.BATCH_RES, mc.BATCH_Z)
    assert any(f.depth > planned for f in fl) and any(f.frontiers and f.frontiers[0] > 1024 for f in fl)
    assert any(f.sensitive > 0 for f in fl) and any(not f.frontiers for f in fl) and any(f.depth == 0 and f.frontiers for f in fl)
    deep = sum(mc.flood(m, mc.BATCH_RES, mc.BATCH_Z).depth > planned for m in b)
    print("batch of %d maps: %d outlive the plan of %d levels" % (len(b), deep, planned))
    for name in mc.BATCHES:
        assert len(mc.batch(name, num_cus)) == mc.batch_size(name, num_cus)


# depth of the flood (the highest level at which a cell is claimed) of every map fixture, at its own res with z_occ_max_dis 1.0 and with
# the map callback's 2.0, against int(1.5 * cell_radius) + 3 planned levels: DESIGN.md, "createMapCache campaign"
FIXTURE_DEPTHS = {          # (depth, planned)
    ("map1", 1.0): (29, 33), ("map1", 2.0): (59, 63), ("mapValue", 1.0): (63, 63), ("mapValue", 2.0): (117, 123),
    ("aisle1", 1.0): (67, 63), ("aisle1", 2.0): (129, 123), ("aisle2", 1.0): (75, 63), ("aisle2", 2.0): (121, 123),
    ("aisle3", 1.0): (75, 63), ("aisle3", 2.0): (121, 123), ("f3key", 1.0): (67, 63), ("f3key", 2.0): (133, 123),
    ("f4key", 1.0): (66, 63), ("f4key", 2.0): (133, 123), ("tile2048", 1.0): (67, 63),
}


def test_fixture_floods_against_the_plan(maps, maps_meta, oracle):
    got = {}
    todo = [(name, maps[name], maps_meta[name]["res"], z) for name in sorted(maps_meta) for z in (1.0, 2.0)]
    todo.append(("tile2048", tile2048(maps["aisle1"]), 0.025, 1.0))
    for name, m, res, z in todo:
        f = mc.flood(m, res, z)
        assert f.values.tobytes() == oracle.map_cache(np.ascontiguousarray(m), res, z).tobytes(), (name, z)
        planned = mc.planned_levels(m.shape[0], m.shape[1], res, z)
        got[(name, z)] = (f.depth, planned)
        print("fixture %-9s z %.1f radius %2d depth %3d planned %3d stopped %7d order-sensitive %6d largest frontier %6d%s" %
              (name, z, mc.cell_radius(res, z), f.depth, planned, f.stopped, f.sensitive, f.max_frontier,
               "   <-- k_mc_finish claims cells" if f.depth > planned else ""))
    assert got == FIXTURE_DEPTHS
