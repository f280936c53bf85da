"""The resumable replay loop without a GPU: the lsd_fa_carry record (its layout in include/lsd_hip.h, in ctypes and in FA_CARRY_DTYPE),
lsd_fa_carry_init, and the carried restatement (tests/fa_resume.py) against the whole-log one (tests/fa_restatement.py: Loop) with the
sequence cut at every frame boundary."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fa_restatement as fr
from fa_resume import ResumableLoop, same_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return g


class lsd_fa_state(C.Structure):
    _fields_ = [("x", C.c_double * 9), ("P", C.c_double * 81)]


class lsd_position(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("ang", C.c_double)]


CTYPES = {"lsd_fa_state": lsd_fa_state, "lsd_position": lsd_position, "double": C.c_double, "int32_t": C.c_int32}


def header_carry_fields():
    """(type, name) of the members of lsd_fa_carry, in the header's order."""
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    body = re.search(r"typedef struct lsd_fa_carry \{(.*?)\} lsd_fa_carry;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)


def test_carry_layout_matches_the_header(lsdmod):
    fields = header_carry_fields()
    assert [n for _, n in fields] == list(lsdmod.FA_CARRY_DTYPE.names)
    ct = type("lsd_fa_carry", (C.Structure,), {"_fields_": [(n, CTYPES[t]) for t, n in fields]})
    assert C.sizeof(ct) == lsdmod.FA_CARRY_DTYPE.itemsize == 768
    for t, n in fields:
        assert getattr(ct, n).offset == lsdmod.FA_CARRY_DTYPE.fields[n][1], n
        assert C.sizeof(CTYPES[t]) == lsdmod.FA_CARRY_DTYPE.fields[n][0].itemsize, n
    assert lsdmod.FA_CARRY_DTYPE["state"] == lsdmod.FA_STATE_DTYPE and lsdmod.FA_CARRY_DTYPE["odom"] == lsdmod.POS_DTYPE
    assert lsdmod.FA_CARRY_DTYPE["frames"] == np.int32 and lsdmod.FA_CARRY_DTYPE["is_offset"] == np.int32


def test_carry_init(built, lsdmod):
    c = lsdmod.Context.fa_carry_init(odom0=(0.0, 1.5, -2.25))
    assert c.dtype == lsdmod.FA_CARRY_DTYPE
    init = lsdmod.Context.fa_initial_state()
    assert c["state"].tobytes() == init.tobytes()
    assert (c["odom"]["x"], c["odom"]["y"], c["odom"]["ang"]) == (0.0, 1.5, -2.25)
    assert (c["ang_sum"], c["ang_count"], c["frames"], c["is_offset"]) == (0.0, 0.0, 0, 0)
    st = lsdmod.fa_state((np.arange(9.0), np.arange(81.0).reshape(9, 9)))
    c2 = lsdmod.Context.fa_carry_init(st[0])
    assert c2["state"].tobytes() == st[0].tobytes() and c2["odom"].tobytes() == bytes(24) and c2["frames"] == 0
    raw = (C.c_uint8 * 768)(*([0xAB] * 768))                 # every byte written, none left over from the caller's memory
    lsdmod.load_library().lsd_fa_carry_init(C.addressof(raw), None, lsdmod.lsd_position(0.0, 0.0, 0.0))
    assert bytes(raw) == lsdmod.Context.fa_carry_init().tobytes()
    rx, rP = fr.reset_state()
    assert ResumableLoop(0.025).carry(lsdmod.FA_CARRY_DTYPE).tobytes() == lsdmod.Context.fa_carry_init().tobytes()
    assert list(c["state"]["x"]) == rx and np.array_equal(c["state"]["P"].reshape(9, 9, order="F"), rP)


def synthetic_states(n, seed):
    """States the way FeatureAssociation hands them to the loop: resets, first frames, and poses whose angles sit at +-180 of the
    odometry (the offset bookkeeping's branches), one per frame."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        r = rng.random()
        if r < 0.1:
            x, P = fr.reset_state()
        else:
            x = [float(v) for v in rng.normal(300, 40, 9)]
            x[2] = float(rng.choice([rng.normal(0, 30), rng.normal(180, 10), rng.normal(-180, 10)]))
            A = rng.normal(size=(9, 9))
            P = (A @ A.T + 9 * np.eye(9)).tolist()
        out.append((x, P))
    return out


def check_against_loop(odom, resol, frames_states, split_after, dtype):
    """Loop over the whole sequence, and ResumableLoop rebuilt from its carry record after every frame in split_after: the scan pose,
    last pose and the loop's variables agree bit for bit at every frame."""
    loop = fr.Loop(odom, resol)
    res = ResumableLoop(resol, odom0=odom[0])
    for t, (x, P) in enumerate(frames_states):
        if t in split_after:
            res = ResumableLoop.from_carry(res.carry(dtype).copy(), resol)
        a, b = loop.scan_pose(t), res.scan_pose(odom[t + 1])
        assert all(same_float(u, v) for u, v in zip(a, b)), (t, a, b)
        assert loop.last_pose() == res.last_pose()
        loop.finish(t, x, P)
        res.finish(odom[t + 1], x, P)
        theta = 0.0
        for v in loop.ang_rotate:
            theta += v
        assert same_float(theta, res.ang_sum) and len(loop.ang_rotate) == res.ang_count == t + 1
        assert loop.is_offset == res.is_offset
    return loop, res


@pytest.mark.parametrize("name", fr.LOGS)
def test_resumable_loop_split_at_every_boundary(name, lsdmod):
    _, mp, _, odom = fr.load_log(name)
    n = len(odom) - 1
    states = synthetic_states(n, seed=len(name))
    check_against_loop(odom, mp[2], states, set(range(1, n)), lsdmod.FA_CARRY_DTYPE)


def test_first_frame_offset_survives_a_split(lsdmod):
    """cnt_frame == 1 is the sequence's first frame: a later call's first frame does not set isOffset, and a flag set by frame 0
    keeps adding 360 to negative offsets after the split."""
    _, mp, _, odom = fr.load_log("data")
    x0, P0 = fr.reset_state()
    a = list(x0); a[0] = 300.0; a[2] = fr.atand(odom[1][2]) + 170.0         # |angDiff| > 90 on the first frame: the flag is set
    b = list(x0); b[0] = 300.0; b[2] = fr.atand(odom[2][2]) - 10.0          # a negative angDiff later
    loop, res = check_against_loop(odom[:3], mp[2], [(a, P0), (b, P0)], {1}, lsdmod.FA_CARRY_DTYPE)
    assert res.is_offset and loop.ang_rotate[1] > 300
    c = list(x0); c[0] = 300.0; c[2] = fr.atand(odom[1][2]) + 170.0
    loop, res = check_against_loop(odom[:3], mp[2], [(b, P0), (c, P0)], {1}, lsdmod.FA_CARRY_DTYPE)
    assert not res.is_offset                                              # |angDiff| > 90 on the second frame only: no flag


def test_resumable_loop_replays_the_data_log(oracle, lsdmod):
    """The oracle's FeatureScan and scores drive the carried loop through the data/ log, cut after every frame, alongside Loop."""
    m, mp, lid, odom = fr.load_log("data")
    mc = oracle.map_cache(m.copy(), mp[2])
    ml = oracle.lsd(m.copy())["lines"]
    scans, lens = lsdmod.lidar_frames(lid)
    loop = fr.Loop(odom, mp[2])
    res = ResumableLoop(mp[2], odom0=odom[0])
    branches = []
    for t in range(len(scans)):
        res = ResumableLoop.from_carry(res.carry(lsdmod.FA_CARRY_DTYPE).copy(), mp[2])
        fs = oracle.feature_scan(scans[t, :lens[t]], mp)
        sp, last = res.scan_pose(odom[t + 1]), res.last_pose()
        assert all(same_float(u, v) for u, v in zip(sp, loop.scan_pose(t))) and last == loop.last_pose()
        lp = loop.lidar_pose(fs["lidar_pos"])
        pr = np.array(fr.pairs(ml["len"], fs["lines"]["len"]), np.int32).reshape(-1, 2)
        cands = oracle.scan_to_map_match(mc, ml, fs["lines"], fs["pts"], lp, last, pr).reshape(-1, 4) if len(pr) else np.zeros((0, 4))
        x, P, rep = fr.feature_association(cands, last, sp, res.x, res.P, len(pr))
        res.finish(odom[t + 1], x, P)
        loop.finish(t, x, P)
        branches.append(rep["branch"])
    assert branches.count(fr.UKF) > len(branches) // 2
    assert res.frames == len(scans) and res.x == loop.x and res.P == loop.P
