"""The carry re-base without a GPU: the restatement's own properties (tests/fa_rebase.py), the claim the feature rests on -- a robot
tracked on map A keeps its track on map B, A grown by whole cells, once its carry is re-based, and loses it otherwise -- shown on the
restated loop with the oracle's FeatureScan and scores, and the ABI: the exported symbol, the lsd_map_frame layout, the Python layer's
refusals before the device is touched."""
import ctypes as C
import inspect
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import fa_rebase as rb
import fa_restatement as fr
from fa_resume import ResumableLoop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lsd_enqueue_fa_carry_rebase_device"
D_COLS, D_ROWS = 96, 80                                   # the growth of map B: a shift of 125 px, above maxEstiDist = 60
# the largest distance, in metres, between the pose of the log replayed on B from its first frame and the pose of the
# log switched from A to B mid-way with the re-base, as this file measures it (test_track_survives_a_grown_map prints the value), and
# the margin of 10 the assertion allows over it for the rounding of the shifted line records.
OBSERVED_M, MARGIN = 5.36e-5, 10.0


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return g


def bits(v):
    return np.array(v, np.float64).tobytes()


def tracked_state(seed=3):
    rng = np.random.default_rng(seed)
    x = [float(v) for v in rng.normal(300, 40, 9)]
    A = rng.normal(size=(9, 9))
    return x, (A @ A.T + 9 * np.eye(9)).tolist()


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------
def test_identity_for_equal_frames():
    x, P = tracked_state()
    f = (0.05, -12.3, 4.56)
    x1, P1 = rb.rebase_state(x, P, f, f)
    assert bits(x1) == bits(x) and bits(P1) == bits(P)


def test_equal_resolutions_shift_the_position_only():
    x, P = tracked_state()
    x1, P1 = rb.rebase_state(x, P, (0.025, -10.0, -7.5), (0.025, -12.4, -9.5))
    assert bits(P1) == bits(P) and bits(x1[2:]) == bits(x[2:])
    assert x1[0] == x[0] * 1.0 + (-10.0 - -12.4) / 0.025 and x1[1] == x[1] * 1.0 + (-7.5 - -9.5) / 0.025
    assert x1[0] != x[0] and x1[1] != x[1]


def test_resolution_scales_rates_and_covariance():
    x, P = tracked_state()
    x1, P1 = rb.rebase_state(x, P, (0.025, -10.0, -7.5), (0.05, -10.0, -7.5))        # s = 0.5: exact
    for k in range(9):
        assert x1[k] == (x[k] if k % 3 == 2 else x[k] * 0.5)
    d = [1.0 if k % 3 == 2 else 0.5 for k in range(9)]
    for i in range(9):
        for j in range(9):
            assert P1[i][j] == P[i][j] * d[i] * d[j]
    assert np.array_equal(np.array(P1), np.array(P1).T)                               # (a power of two: symmetry survives exactly)


def test_carries_without_a_pose_are_left_alone(built, lsdmod):
    frm, to = (0.025, -10.0, -7.5), (0.05, -12.4, -9.5)
    rx, rP = fr.reset_state()
    x1, P1 = rb.rebase_state(rx, rP, frm, to)
    assert bits(x1) == bits(rx) and bits(P1) == bits(rP)
    near = list(rx); near[0] = -1.00005; near[1] = 17.0                               # inside the reference's |x + 1| < 1e-4
    assert bits(rb.rebase_state(near, rP, frm, to)[0]) == bits(near)
    first = lsdmod.Context.fa_carry_init(odom0=(0.0, 1.5, -2.25))                     # frames == 0: the driver's first frame is still to come
    assert first["frames"] == 0 and rb.rebase_carry(first, frm, to).tobytes() == first.tobytes()
    c = ResumableLoop(0.025).carry(lsdmod.FA_CARRY_DTYPE)
    assert rb.rebase_carry(c, frm, to).tobytes() == c.tobytes()
    x, P = tracked_state()
    lp = ResumableLoop(0.025, x, P, odom0=(0.5, 0.25, 0.125))
    lp.ang_sum, lp.ang_count, lp.frames, lp.is_offset = 12.5, 3.0, 3, True
    rec = lp.carry(lsdmod.FA_CARRY_DTYPE)
    got = rb.rebase_carry(rec, frm, to)
    assert got["state"].tobytes() != rec["state"].tobytes()
    for f in ("odom", "ang_sum", "ang_count", "frames", "is_offset"):                 # metres, degrees, counts: not the map's
        assert got[f].tobytes() == rec[f].tobytes(), f
    nan = list(x); nan[0] = float("nan")
    assert math.isnan(rb.rebase_state(nan, P, frm, to)[0][0])


def test_metres_pose_is_kept_to_the_roundings_of_the_formula():
    rng = np.random.default_rng(11)
    frames = [(0.025, -10.0, -7.5), (0.05, -12.4, -9.5), (0.03, 1e3 / 3, -2e3 / 7), (0.1, 0.0, 0.0), (0.025, -12.4, -9.5)]
    for frm in frames:
        for to in frames:
            if frm == to:
                continue
            for _ in range(20):
                x = [float(v) for v in rng.normal(0, 2000, 9)]
                P = np.eye(9).tolist()
                x1, _ = rb.rebase_state(x, P, frm, to)
                m0, m1, bound = rb.metres(x, frm), rb.metres(x1, to), rb.metres_bound(x, x1, frm, to)
                for k in (0, 1):
                    # the exact value the formula approximates: x * (rf / rt) + (of - ot) / rt pixels of `to` is m0 itself in metres
                    err = abs(m1[k] - m0[k])
                    assert err <= bound[k], (frm, to, float(err), float(bound[k]))


# ---- 2. the claim, on the restatement ------------------------------------------------------------------------------------------------------
def test_track_survives_a_grown_map(oracle, lsdmod):
    m, mp, lid, odom = fr.load_log("data")
    mp = tuple(float(v) for v in mp)
    mc_a = oracle.map_cache(m.copy(), mp[2])
    ml_a = oracle.lsd(m.copy())["lines"]
    mc_b, ml_b, mp_b = rb.grow_map(mc_a, ml_a, mp, D_COLS, D_ROWS, lsdmod.z_occ_max_dis)
    assert math.hypot(D_COLS, D_ROWS) > lsdmod.maxEstiDist and mc_b.shape == (m.shape[0] + D_ROWS, m.shape[1] + D_COLS)
    scans, lens = lsdmod.lidar_frames(lid)
    n = len(scans)
    half = n // 2
    fa, fb = rb.frame_of(mp), rb.frame_of(mp_b)

    def scanner(map_param):
        cache = {}

        def fs(t):
            if t not in cache:
                r = oracle.feature_scan(scans[t, :lens[t]], map_param)
                cache[t] = (r["lines"], r["pts"], r["lidar_pos"])
            return cache[t]
        return fs
    fs_a, fs_b = scanner(mp), scanner(mp_b)
    match = lambda *a: oracle.scan_to_map_match(*a).reshape(-1, 4)

    whole = ResumableLoop(mp_b[2], odom0=odom[0])                                     # the whole log on B
    want = rb.replay(range(n), odom, whole, mc_b, ml_b, mp_b, fs_b, match)
    first = ResumableLoop(mp[2], odom0=odom[0])                                       # the first half on A
    on_a = rb.replay(range(half), odom, first, mc_a, ml_a, mp, fs_a, match)
    assert on_a[-1][2]["branch"] == fr.UKF and want[half - 1][2]["branch"] == fr.UKF  # a robot that is tracking when the map changes
    rec = first.carry(lsdmod.FA_CARRY_DTYPE)

    lost = ResumableLoop.from_carry(rec.copy(), mp_b[2])                              # the carry as it is, on B: off by the shift
    r = rb.replay([half], odom, lost, mc_b, ml_b, mp_b, fs_b, match)[0][2]
    assert r["branch"] == fr.RESET and r["n_kept"] == 0 and r["n_pairs"] > 0, r

    kept = rb.rebase_loop(ResumableLoop.from_carry(rec.copy(), mp[2]), fa, fb)       # the carry re-based: the track continues
    got = rb.replay(range(half, n), odom, kept, mc_b, ml_b, mp_b, fs_b, match)
    worst = 0.0
    for t, (x, P, rep) in zip(range(half, n), got):
        wx, wP, wrep = want[t]
        assert rep["branch"] == wrep["branch"], (t, rep["branch"], wrep["branch"])
        if rep["branch"] == fr.RESET:
            continue
        a, b = rb.metres(x, fb), rb.metres(wx, fb)
        worst = max(worst, math.hypot(float(a[0] - b[0]), float(a[1] - b[1])))
    print("re-based replay against the whole log on B: largest pose distance %.3e m over %d frames" % (worst, n - half))
    assert sum(rep["branch"] == fr.UKF for _, _, rep in got) > (n - half) // 2
    assert worst <= MARGIN * OBSERVED_M, worst


# ---- 3. the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_entry_is_exported(built, lsdmod):
    assert ENTRY in lsdmod.EXPORTED_SYMBOLS
    fn = getattr(lsdmod.load_library(), ENTRY)
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert fn.argtypes[5] is lsdmod.lsd_map_frame and fn.argtypes[6] is lsdmod.lsd_map_frame and fn.argtypes[4] is C.c_int32
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    decl = re.search(r"\bint %s\((.*?)\);" % ENTRY, src, re.S).group(1)
    assert [a.strip() for a in re.sub(r"\s+", " ", decl).split(",")] == [
        "lsd_ctx *ctx", "lsd_fa_carry *d_carry", "int n_seq", "const int32_t *d_key", "int32_t key", "lsd_map_frame from", "lsd_map_frame to",
        "void *stream"]
    assert callable(lsdmod.Context.enqueue_fa_carry_rebase_device)


def test_map_frame_layout_matches_the_header(lsdmod):
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    body = re.search(r"typedef struct lsd_map_frame \{(.*?)\} lsd_map_frame;", src, re.S).group(1)
    m = re.match(r"\s*double\s+([\w\s,]+);\s*$", body)
    names = [n.strip() for n in m.group(1).split(",")]
    assert names == ["mapResol", "mapOriX", "mapOriY"] == [n for n, _ in lsdmod.lsd_map_frame._fields_]
    assert C.sizeof(lsdmod.lsd_map_frame) == 24
    for k, n in enumerate(names):
        assert getattr(lsdmod.lsd_map_frame, n).offset == 8 * k and getattr(lsdmod.lsd_map_frame, n).size == 8


def test_python_layer_refuses_before_touching_the_device(lsdmod):
    """map_frame, and through it Context.enqueue_fa_carry_rebase_device and the rebase= keyword, refuse what the C entry refuses; a
    Context that was never created (no device here) shows that the checks come first."""
    E = lsdmod
    f = E.map_frame((0.05, -1.5, 2.25))
    assert (f.mapResol, f.mapOriX, f.mapOriY) == (0.05, -1.5, 2.25)
    g = E.map_frame((608, 480, 0.025, -10.0, -7.5))                                   # a map_param: its last three
    assert (g.mapResol, g.mapOriX, g.mapOriY) == (0.025, -10.0, -7.5) and E.map_frame(g) is not None
    inf, nan = float("inf"), float("nan")
    bad = [(0.0, 0.0, 0.0), (-0.05, 0.0, 0.0), (inf, 0.0, 0.0), (nan, 0.0, 0.0), (0.05, inf, 0.0), (0.05, 0.0, nan), (0.05, 0.0), (1, 2, 3, 4)]
    for v in bad:
        with pytest.raises(E.LsdError) as e:
            E.map_frame(v)
        assert e.value.status == E.LSD_ERR_INVALID, v
    cx = E.Context.__new__(E.Context)                                                 # no lsd_create: any use of the library would fail
    cx.h = cx.L = None
    ok = (0.05, 0.0, 0.0)
    for args in ((0x1000, 2, None, 0, bad[0], ok), (0x1000, 2, None, 0, ok, bad[5]), (0, 2, None, 0, ok, ok), (None, 2, None, 0, ok, ok),
                 (0x1000, 0, None, 0, ok, ok), (0x1000, -3, None, 0, ok, ok)):
        with pytest.raises(E.LsdError) as e:
            cx.enqueue_fa_carry_rebase_device(*args)
        assert e.value.status == E.LSD_ERR_INVALID, args
    for fn in (E.Localizer.set_map, E.FleetLocalizer.set_map, E.FleetLocalizer.set_map_device):
        assert inspect.signature(fn).parameters["rebase"].default is False, fn
    # Localizer.set_map_device keeps its parameter list (tests/test_map_update_cpu.py pins it): there the attribute is the switch
    assert "rebase" not in inspect.signature(E.Localizer.set_map_device).parameters
    assert "rebase_on_hand_over" in inspect.getsource(E._Ticks.__init__)
    assert list(inspect.signature(E.FleetLocalizer.set_map_device).parameters) == [
        "self", "i", "d_grid", "oriMapCol", "oriMapRow", "mapResol", "mapOriX", "mapOriY", "stream", "rebase"]
    assert list(inspect.signature(E.FleetLocalizer.reserve_map).parameters) == ["self", "i", "cols", "rows", "lines_cap"]
    assert list(inspect.signature(E.FleetLocalizer.rebase).parameters) == ["self", "robots", "from_map", "to_map"]
    assert isinstance(E.FleetLocalizer.map_counts, property)
