"""Relocalisation on the device (include/lsd_hip.h: lsd_enqueue_fa_lost_gather_device, lsd_enqueue_fa_carry_seed_device; csrc/k_falost.hip,
csrc/k_faseed.hip) restated on numpy records and Python floats, in the header's order, written from the header for the
tests (not from the HIP code), and the generated campaign both test files run.

Python floats are IEEE doubles without contraction, so every statement below rounds as the device build (-ffp-contract=off) rounds it.
The gather compares bytes and copies bytes; the seed's arithmetic is R of the correction's step 5 (tests/fa_correct_cases.py) and the
loop's angle offset (tests/fa_resume.py: ResumableLoop.finish) on fa_restatement.atand.
"""
import math

import numpy as np

import fa_correct_cases as fc
import fa_restatement as fr
import grid_locate_cases as lc
import grid_response_cases as gr

CARRY_DTYPE = fc.CARRY_DTYPE
SEED_REP_DTYPE = np.dtype([("pose", "f8", (3,)), ("ang_diff", "f8"), ("seq", "i4"), ("slot", "i4"), ("flags", "u4"), ("loc_flags", "u4")])
assert SEED_REP_DTYPE.itemsize == 48
SEEDED, UNUSED, BAD_PICK, HAS_POSE, NOT_LOCATED, AMBIGUOUS, NO_RESPONSE, NOT_FINITE = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_NAMES = {SEEDED: "seeded", UNUSED: "unused", BAD_PICK: "bad_pick", HAS_POSE: "has_pose", NOT_LOCATED: "not_located",
              AMBIGUOUS: "ambiguous", NO_RESPONSE: "no_response", NOT_FINITE: "not_finite"}
SEED_KEYS = ("var_xy", "var_ang", "cov_scale", "floor_xy", "floor_ang", "max_best")
SEED_DEFAULTS = (1.0, 1.0, 1.0, 1.0, 1.0, 1)                               # fa_seed()'s
INF, NAN = float("inf"), float("nan")


def no_pose(x0):
    """The project's one "no pose" test."""
    return abs(float(x0) + 1) < 0.0001


# ---- the gather ----------------------------------------------------------------------------------------------------------------------------
def lost_slot(carry, poses, lens):
    """The slot of one sequence, or -1: carry a CARRY_DTYPE record, poses float64 [frames_pitch, 3] (compared as bytes), lens [frames_pitch]."""
    if not no_pose(carry["state"]["x"][0]):
        return -1
    key = np.ascontiguousarray(carry["state"]["x"][:3]).view(np.uint64)
    words = np.ascontiguousarray(poses, np.float64).reshape(-1, 3).view(np.uint64)
    for t in range(len(words) - 1, -1, -1):
        if (words[t] == key).all() and lens[t] > 0:
            return t
    return -1


def gather(carries, poses, scans, lens, keys, key, max_lost, scans_out):
    """carries [n_seq], poses [n_seq, fp, 3], scans [n_seq, fp, stride, 2], lens [n_seq, fp], keys int32 [n_seq] or None, scans_out
    [max_lost, stride, 2] as it was before the call -> (scans_out, lens_out, pick, n_lost) after it."""
    n_seq, fp = lens.shape
    out, lens_out, pick = np.array(scans_out, np.float64), np.zeros(max_lost, np.int32), np.full(max_lost, -1, np.int32)
    j = 0
    for s in range(n_seq):
        if keys is not None and keys[s] != key:
            continue
        slot = lost_slot(carries[s], poses[s], lens[s])
        if slot < 0:
            continue
        if j < max_lost:
            pick[j], lens_out[j] = s * fp + slot, lens[s, slot]
            out[j] = scans[s, slot]
        j += 1
    return out, lens_out, pick, np.array([j, min(j, max_lost)], np.int32)


# ---- the seed ------------------------------------------------------------------------------------------------------------------------------
def seed_one(carry, n_seq_ok, pk, frames_pitch, loc, resp, par, trace=None):
    """One pick: carry (the record of sequence pk // frames_pitch, or None where that is outside the carries), loc one LOCATE_DTYPE record,
    resp one RESPONSE_DTYPE record or None, par a tuple of SEED_KEYS -> (the carry after or None, the report)."""
    var_xy, var_ang, cov_scale, floor_xy, floor_ang = (float(v) for v in par[:5])
    max_best = int(par[5])
    rep = np.zeros(1, SEED_REP_DTYPE)[0]
    rep["seq"], rep["slot"] = -1, -1
    tr = trace if trace is not None else {}
    if pk < 0:                                                               # 0
        rep["flags"] = UNUSED
        return carry, rep
    rep["seq"], rep["slot"] = pk // frames_pitch, pk % frames_pitch
    if not n_seq_ok:                                                         # 1
        rep["flags"] = BAD_PICK
        return carry, rep
    tr["sentinel"] = abs(float(carry["state"]["x"][0]) + 1)
    if not no_pose(carry["state"]["x"][0]):                                  # 2
        rep["flags"] = HAS_POSE
        return carry, rep
    rep["loc_flags"] = loc["flags"]
    if int(loc["flags"]) != lc.ACCEPTED:                                     # 3
        rep["flags"] = NOT_LOCATED
        return carry, rep
    tr["n_best"] = int(loc["n_best"])
    if int(loc["n_best"]) > max_best:                                        # 4
        rep["flags"] = AMBIGUOUS
        return carry, rep
    R = [[0.0] * 3 for _ in range(3)]
    if resp is not None:                                                     # 5
        rf = tr["resp_flags"] = int(resp["flags"])
        if not rf & gr.VALID or rf & (gr.NONE | gr.EMPTY | gr.MISMATCH):
            rep["flags"] = NO_RESPONSE
            return carry, rep
        z = [float(resp["x"]), float(resp["y"]), float(resp["ang"])]
        c = [float(v) for v in resp["cov"]]
        if not all(math.isfinite(v) for v in z + c):
            rep["flags"] = NOT_FINITE
            return carry, rep
        R = [[c[0] * cov_scale + floor_xy, c[1] * cov_scale, c[3] * cov_scale],
             [c[1] * cov_scale, c[2] * cov_scale + floor_xy, c[4] * cov_scale],
             [c[3] * cov_scale, c[4] * cov_scale, c[5] * cov_scale + floor_ang]]
    else:
        z = [float(loc["x"]), float(loc["y"]), float(loc["ang"])]
        if not all(math.isfinite(v) for v in z):
            rep["flags"] = NOT_FINITE
            return carry, rep
        R[0][0], R[1][1], R[2][2] = var_xy, var_xy, var_ang
    new = carry.copy()                                                       # 6
    new["state"]["x"] = z + [0.0] * 6
    P = [[0.0] * 9 for _ in range(9)]
    for i, v in enumerate((1.0, 1.0, 1.0, 0.1, 0.1, 0.1)):
        P[3 + i][3 + i] = v
    for i in range(3):
        for j in range(3):
            P[i][j] = R[i][j]
    new["state"]["P"] = np.array(P, np.float64).ravel(order="F")
    d = z[2] - fr.atand(float(carry["odom"]["ang"]))
    off = abs(d) > 90
    tr["d_raw"] = d
    if off and d < 0:
        d += 360
    new["ang_sum"], new["ang_count"], new["is_offset"] = 0.0 + d, 1.0, int(off)
    rep["pose"], rep["ang_diff"], rep["flags"] = z, d, SEEDED
    return new, rep


def seed(carries, frames_pitch, pick, loc, resp, par, traces=None):
    """carries CARRY_DTYPE [n_seq], pick int32 [n], loc LOCATE_DTYPE [n], resp RESPONSE_DTYPE [n] or None -> (carries after, reports [n])."""
    out = np.array(carries, CARRY_DTYPE)
    reps = np.zeros(len(pick), SEED_REP_DTYPE)
    for j, pk in enumerate(int(v) for v in pick):
        s = pk // frames_pitch if pk >= 0 else -1
        ok = 0 <= s < len(out)
        tr = {} if traces is None else traces[j]
        new, reps[j] = seed_one(out[s] if ok else None, ok, pk, frames_pitch, loc[j], None if resp is None else resp[j], par, tr)
        if ok:
            out[s] = new
    return out, reps


# ---- the gather's campaign -----------------------------------------------------------------------------------------------------------------
KINDS = ("lost", "pose", "lost_in_lo", "lost_in_hi", "out_lo", "out_hi", "nan", "zero_sign", "twice", "len0_larger", "no_slot", "all_empty",
         "key_out")
RESET_POSE = (-1.0, -1.0, 0.0)


def sequence(rng, kind, fp, stride):
    """(carry, poses [fp, 3], lens [fp], keyed out) of one sequence of `kind`."""
    x, P = fr.reset_state()
    poses = rng.normal(300, 40, (fp, 3))
    lens = rng.integers(1, stride + 1, fp).astype(np.int32)
    last = fp - 1
    if kind == "pose":
        x[:3] = [float(v) for v in rng.normal((300, 250, 20), (40, 40, 30))]
    elif kind in ("lost_in_lo", "lost_in_hi", "out_lo", "out_hi"):
        x[0] = -1.0 + {"lost_in_lo": -0.00009, "lost_in_hi": 0.00009, "out_lo": -0.00011, "out_hi": 0.00011}[kind]
    elif kind == "nan":
        x[0] = NAN
    if kind != "no_slot":
        poses[last] = x[:3]
    if kind == "zero_sign":                                                  # -0.0 against +0.0 in x[2]: no match by bytes
        poses[last, 2] = -0.0
        poses[0] = poses[0] if fp == 1 else x[:3]
    if kind in ("twice", "len0_larger") and fp > 1:
        poses[0] = x[:3]
    if kind == "len0_larger":
        lens[last] = 0
    if kind == "all_empty":
        lens[:] = 0
    return fc.carry_of(x, P, int(rng.integers(0, 4))), poses, lens, kind == "key_out"


def gather_case(name, n_seq, fp, stride, kinds, seed_no, max_lost):
    """kinds: one kind per sequence."""
    rng = np.random.default_rng(seed_no)
    parts = [sequence(rng, kinds[s], fp, stride) for s in range(n_seq)]
    keys = np.array([3 if out else 7 for _, _, _, out in parts], np.int32)
    scans = rng.uniform(0.1, 9.0, (n_seq, fp, stride, 2))
    return dict(name=name, n_seq=n_seq, frames_pitch=fp, stride=stride, kinds=list(kinds), carries=np.array([p[0] for p in parts], CARRY_DTYPE),
                poses=np.stack([p[1] for p in parts]), lens=np.stack([p[2] for p in parts]), scans=scans, key=7,
                keys=keys if (keys != 7).any() or seed_no % 2 else None, max_lost=max_lost, capacity=max(1024, stride))


def run_gather(c, scans_out=None):
    before = np.full((c["max_lost"], c["stride"], 2), 0.625) if scans_out is None else scans_out
    return gather(c["carries"], c["poses"], c["scans"], c["lens"], c["keys"], c["key"], c["max_lost"], before)


def with_max_lost(make):
    """The case at max_lost = 1, the number lost, one below it and one above it."""
    n = int(run_gather(make(1))[3][0])
    return [make(m) for m in sorted({1, n, n - 1, n + 1}) if 1 <= m <= 4096]


def gather_campaign():
    C = []
    shapes = [(1, 1, 1), (2, 2, 360), (3, 90, 1), (63, 91, 1), (64, 181, 1), (65, 2, 360), (1025, 1, 1), (3, 2, 1025), (65, 1, 7)]
    for n, (n_seq, fp, stride) in enumerate(shapes):                         # every kind in turn, at every shape
        kinds = [KINDS[s % len(KINDS)] for s in range(n_seq)]
        C += with_max_lost(lambda m: gather_case("mixed_%d_%d_%d_m%d" % (n_seq, fp, stride, m), n_seq, fp, stride, kinds, 100 + n, m))
    for n, (n_seq, fp, stride) in enumerate([(1, 2, 3), (3, 1, 1), (64, 2, 5), (65, 91, 1), (1025, 2, 1)]):
        C.append(gather_case("none_%d" % n_seq, n_seq, fp, stride, ["pose"] * n_seq, 200 + n, 3))
        C += with_max_lost(lambda m: gather_case("all_%d_m%d" % (n_seq, m), n_seq, fp, stride, ["lost"] * n_seq, 210 + n, m))
        only_last = ["pose"] * (n_seq - 1) + ["lost"]
        C += with_max_lost(lambda m: gather_case("only_last_%d_m%d" % (n_seq, m), n_seq, fp, stride, only_last, 220 + n, m))
    for n_seq, lo, hi in ((65, 40, 65), (1025, 50, 80), (1025, 246, 268), (1025, 1000, 1025)):   # across a wavefront, across a chunk of 256
        kinds = ["lost" if lo <= s < hi and (s - lo) % 2 == 0 else "pose" for s in range(n_seq)]
        C += with_max_lost(lambda m: gather_case("every_other_%d_%d_m%d" % (n_seq, lo, m), n_seq, 2, 3, kinds, 300 + lo, m))
    kinds = ["key_out" if s % 3 == 0 else "lost" for s in range(64)]
    C += with_max_lost(lambda m: gather_case("key_64_m%d" % m, 64, 2, 4, kinds, 401, m))
    return C


GATHER_CLASSES = (["n_seq_%d" % n for n in (1, 2, 3, 63, 64, 65, 1025)] + ["fp_%d" % n for n in (1, 2, 90, 91, 181)] +
                  ["stride_%d" % n for n in (1, 360, 1025)] + ["max_lost_1", "max_lost_eq", "max_lost_below", "max_lost_above"] +
                  ["none_lost", "all_lost", "only_last", "every_other_across_wave", "every_other_across_chunk", "key_leaves_out"] +
                  ["sentinel_in_lo", "sentinel_in_hi", "sentinel_out_lo", "sentinel_out_hi", "nan_not_lost", "zero_sign", "larger_slot_wins",
                   "len0_smaller_wins", "no_slot", "only_empty_scans", "rows_past_gathered"])


def gather_classes_of(c, got):
    """The classes a case reaches: predicates on the case and on the restatement's outputs (scans_out, lens_out, pick, n_lost)."""
    _, lens_out, pick, n_lost = got
    n, fp = int(n_lost[0]), c["frames_pitch"]
    slots = [lost_slot(c["carries"][s], c["poses"][s], c["lens"][s]) if c["keys"] is None or c["keys"][s] == c["key"] else -1
             for s in range(c["n_seq"])]
    lost = [s for s, t in enumerate(slots) if t >= 0]
    k = {"n_seq_%d" % c["n_seq"], "fp_%d" % fp, "stride_%d" % c["stride"]} & set(GATHER_CLASSES)
    m = c["max_lost"]
    k |= {name for name, hit in (("max_lost_1", m == 1 and n > 1), ("max_lost_eq", m == n), ("max_lost_below", m == n - 1),
                                 ("max_lost_above", m == n + 1), ("none_lost", n == 0), ("all_lost", n == c["n_seq"] > 1),
                                 ("only_last", lost == [c["n_seq"] - 1] and c["n_seq"] > 1), ("rows_past_gathered", (pick < 0).any())) if hit}
    if len(lost) > 2 and all(b - a == 2 for a, b in zip(lost, lost[1:])):
        k |= {"every_other_across_wave"} if lost[0] // 64 != lost[-1] // 64 else set()
        k |= {"every_other_across_chunk"} if lost[0] // 256 != lost[-1] // 256 else set()
    for s in range(c["n_seq"]):
        x = c["carries"][s]["state"]["x"]
        sent, words = abs(float(x[0]) + 1), np.ascontiguousarray(c["poses"][s]).view(np.uint64)
        key = np.ascontiguousarray(x[:3]).view(np.uint64)
        hits = [t for t in range(fp) if (words[t] == key).all()]
        by_value = [t for t in range(fp) if t not in hits and all(float(a) == float(b) for a, b in zip(c["poses"][s, t], x[:3]))]
        if c["keys"] is not None and c["keys"][s] != c["key"]:
            k |= {"key_leaves_out"} if lost_slot(c["carries"][s], c["poses"][s], c["lens"][s]) >= 0 else set()
            continue
        if slots[s] >= 0 and 0.00008 < sent < 0.0001:
            k.add("sentinel_in_%s" % ("lo" if x[0] < -1 else "hi"))
        if slots[s] < 0 and 0.0001 <= sent < 0.00012 and hits:
            k.add("sentinel_out_%s" % ("lo" if x[0] < -1 else "hi"))
        k |= {"nan_not_lost"} if math.isnan(x[0]) and slots[s] < 0 and hits else set()
        if no_pose(x[0]):
            k |= {"zero_sign"} if by_value and (not hits or slots[s] == hits[-1]) else set()
            k |= {"larger_slot_wins"} if len(hits) > 1 and slots[s] == hits[-1] else set()
            k |= {"len0_smaller_wins"} if len(hits) > 1 and c["lens"][s, hits[-1]] == 0 and slots[s] == hits[0] else set()
            k |= {"no_slot"} if not hits and slots[s] < 0 else set()
            k |= {"only_empty_scans"} if hits and slots[s] < 0 and not c["lens"][s][hits].any() else set()
    return k


# ---- the seed's campaign -------------------------------------------------------------------------------------------------------------------
def loc_rec(rng, flags=lc.ACCEPTED, n_best=1, pose=None):
    r = np.zeros(1, lc.LOCATE_DTYPE)[0]
    cx, cy, a = (int(v) for v in rng.integers(5, 400, 3))
    r["x"], r["y"], r["ang"] = (float(cx), float(cy), a * 0.5 - 90.0) if pose is None else pose
    r["cx"], r["cy"], r["a"], r["score"], r["n_beams"], r["flags"], r["n_best"], r["lower_bound"] = cx, cy, a, 9000, 60, flags, n_best, 8000
    if flags != lc.ACCEPTED and pose is None:
        r["x"], r["y"], r["ang"] = RESET_POSE
    return r


def seed_unit(name, seed_no, **kw):
    """One pick: dict(name, kind of pick, carry, loc, resp); kw adjusts it (see seed_campaign)."""
    rng = np.random.default_rng(seed_no)
    x, P = fr.reset_state()
    x[0] = kw.get("x0", -1.0)
    carry = fc.carry_of(x, P, seed_no & 3)                                   # ang_sum, ang_count, frames, is_offset: a reset robot's past
    carry["odom"]["ang"] = kw.get("odom_ang", float(rng.normal(0, 2)))
    best = kw.get("n_best", 1)                                               # "max" / "max+1": set per batch, against its max_best
    loc = loc_rec(rng, kw.get("loc_flags", lc.ACCEPTED), 1 if isinstance(best, str) else best, kw.get("loc_pose"))
    resp = fc.valid_resp(rng, (float(loc["x"]), float(loc["y"]), float(loc["ang"])), kw.get("resp_flags", gr.VALID))
    for field, v in kw.get("resp_set", ()):
        if isinstance(field, tuple):
            resp[field[0]][field[1]] = v
        else:
            resp[field] = v
    return dict(name=name, pick=kw.get("pick", "own"), carry=carry, loc=loc, resp=resp, best=best)


def seed_campaign():
    """Batches: dict(name, frames_pitch, par, with_resp, units).  Every unit has a sequence of its own."""
    na = lambda v, to: float(np.nextafter(np.float64(v), np.float64(to)))
    U = []
    for k in range(3):
        U.append(seed_unit("plain_%d" % k, 10 + k))
        U.append(seed_unit("unused_%d" % k, 20 + k, pick="unused"))
        U.append(seed_unit("bad_pick_%d" % k, 30 + k, pick=("bad", (0, 1, 1 << 20)[k])))
        U.append(seed_unit("has_pose_%d" % k, 40 + k, x0=(312.5, -1.00011, -0.99989)[k]))   # a carry that gained a pose since the gather
        U.append(seed_unit("sentinel_in_%d" % k, 45 + k, x0=(-1.00009, -0.99991, -1.0)[k]))
        for tag, fl in (("rejected", lc.REJECTED), ("not_found", lc.NOT_FOUND), ("overflow", lc.OVERFLOW), ("empty", lc.EMPTY),
                        ("two_bits", lc.ACCEPTED | lc.REJECTED), ("zero", 0)):
            U.append(seed_unit("loc_%s_%d" % (tag, k), 50 + k, loc_flags=fl))
        U.append(seed_unit("best_at_%d" % k, 60 + k, n_best="max"))
        U.append(seed_unit("best_above_%d" % k, 65 + k, n_best="max+1"))
        U.append(seed_unit("best_many_%d" % k, 67 + k, n_best=1 << 31))
        for tag, fl in (("none", gr.NONE), ("empty", gr.VALID | gr.EMPTY), ("mismatch", gr.VALID | gr.MISMATCH), ("unset", 0)):
            U.append(seed_unit("resp_%s_%d" % (tag, k), 70 + k, resp_flags=fl))
        U.append(seed_unit("resp_not_peak_%d" % k, 75 + k, resp_flags=gr.VALID | (gr.X_NOT_PEAK, gr.Y_NOT_PEAK, gr.A_NOT_PEAK)[k]))
        bad = (NAN, INF, -INF)[k]
        U.append(seed_unit("nf_resp_%d" % k, 80 + k, resp_set=[(("x", "y", "ang")[k], bad)], loc_pose=((bad, 5.0, 1.0), (5.0, bad, 1.0), (5.0, 6.0, bad))[k]))
        U.append(seed_unit("nf_cov_%d" % k, 85 + k, resp_set=[("ang", 3.0), (("cov", (0, 4, 5)[k]), bad)], loc_pose=(7.0, 8.0, bad)))
        for tag, ang in (("at_90", 90.0), ("above_90", na(90.0, INF)), ("below_-90", na(-90.0, -INF)), ("at_-90", -90.0), ("at_-270", -270.0),
                         ("at_270", 270.0)):
            U.append(seed_unit("d_%s_%d" % (tag, k), 90 + k, odom_ang=(0.0, -0.0, 0.0)[k], loc_pose=(40.0 + k, 25.0, ang),
                               resp_set=[("ang", ang)]))
        for tag, oa in (("zero", 0.0), ("inf", INF), ("-inf", -INF), ("nan", NAN)):
            U.append(seed_unit("odom_%s_%d" % (tag, k), 100 + k, odom_ang=oa, loc_pose=(50.0, 60.0, (10.0, 170.0, -170.0)[k]),
                               resp_set=[("ang", (10.0, 170.0, -170.0)[k])]))
    pars = [SEED_DEFAULTS, (0.25, 4.0, 2.0, 0.0, 0.5, 3), (9.0, 0.0625, 0.0, 1.5, 0.0, 1)]
    B = []
    for n, (par, fp) in enumerate(zip(pars, (1, 2, 91))):
        for with_resp in (False, True):
            if not with_resp and not (par[0] > 0 and par[1] > 0):
                continue
            us = [dict(u) for u in U if int(u["name"].rsplit("_", 1)[1]) == n]
            B.append(dict(name="par%d_%s" % (n, "resp" if with_resp else "loc"), frames_pitch=fp, par=par, with_resp=with_resp, units=us))
    for count in (1, 2, 3):                                                  # around the kernel's picks-per-workgroup boundary
        B.append(dict(name="count_%d" % count, frames_pitch=3, par=SEED_DEFAULTS, with_resp=count != 2, units=[dict(u) for u in U[7 * count:8 * count]]))
    return [arrays_of(b) for b in B]


def arrays_of(b):
    """The launch's arrays of a batch: carries (two more than the units: sequences no pick names), pick, loc, resp."""
    us, fp, max_best = b["units"], b["frames_pitch"], b["par"][5]
    n_seq = len(us) + 2
    rng = np.random.default_rng(len(us) * 7 + fp)
    order = rng.permutation(n_seq)[:len(us)]                                 # the picks are not in the carries' order
    spare = fc.carry_of(*fr.reset_state(), 1)
    carries = np.array([spare] * n_seq, CARRY_DTYPE)
    pick, loc, resp = np.zeros(len(us), np.int32), np.zeros(len(us), lc.LOCATE_DTYPE), np.zeros(len(us), gr.RESPONSE_DTYPE)
    for j, u in enumerate(us):
        s = int(order[j])
        carries[s], loc[j], resp[j] = u["carry"], u["loc"], u["resp"]
        pick[j] = -1 - j if u["pick"] == "unused" else n_seq * fp + u["pick"][1] if isinstance(u["pick"], tuple) else s * fp + int(rng.integers(0, fp))
    for j, u in enumerate(us):                                               # n_best relative to this batch's max_best
        if u["best"] == "max":
            loc[j]["n_best"] = max_best
        elif u["best"] == "max+1":
            loc[j]["n_best"] = max_best + 1
    return dict(b, n_seq=n_seq, carries=carries, pick=pick, loc=loc, resp=resp)


def run_seed(b, traces=None):
    return seed(b["carries"], b["frames_pitch"], b["pick"], b["loc"], b["resp"] if b["with_resp"] else None, b["par"], traces)


SEED_CLASSES = (sorted(FLAG_NAMES.values()) + ["with_resp", "without_resp", "best_at_max", "best_above_max", "d_at_90", "d_above_90",
                "d_below_minus_90", "d_minus_270", "odom_zero", "odom_inf", "odom_minus_inf", "odom_nan", "resp_none", "resp_empty",
                "resp_mismatch", "resp_unset", "not_peak_seeded", "nf_cov", "nf_pose", "gained_a_pose", "replaced_bookkeeping"])


def seed_classes_of(b, j, rep, tr, before, after):
    """The classes pick j of batch b reaches, from the restatement's report and trace and the carry before and after."""
    fl = int(rep["flags"])
    k = {FLAG_NAMES[fl]}
    if fl in (UNUSED, BAD_PICK):
        return k
    k.add("with_resp" if b["with_resp"] else "without_resp")
    if fl == HAS_POSE:
        k |= {"gained_a_pose"} if tr["sentinel"] > 1 else set()
        return k
    mb = b["par"][5]
    k |= {"best_at_max"} if fl == SEEDED and tr.get("n_best") == mb else set()
    k |= {"best_above_max"} if fl == AMBIGUOUS and tr.get("n_best") == mb + 1 else set()
    rf = tr.get("resp_flags")
    if fl == NO_RESPONSE:
        k |= {name for name, hit in (("resp_none", rf & gr.NONE), ("resp_empty", rf & gr.EMPTY), ("resp_mismatch", rf & gr.MISMATCH),
                                     ("resp_unset", rf == 0)) if hit}
    if fl == NOT_FINITE:
        r = b["resp"][j]
        k |= {"nf_cov"} if b["with_resp"] and not np.isfinite(r["cov"]).all() and np.isfinite([r["x"], r["y"], r["ang"]]).all() else set()
        k |= {"nf_pose"} if not b["with_resp"] or not np.isfinite([r["x"], r["y"], r["ang"]]).all() else set()
    if fl == SEEDED:
        d, oa = tr["d_raw"], float(before["odom"]["ang"])
        k |= {"not_peak_seeded"} if rf is not None and rf & (gr.X_NOT_PEAK | gr.Y_NOT_PEAK | gr.A_NOT_PEAK) else set()
        k |= {"d_at_90"} if d == 90.0 and not after["is_offset"] else set()
        k |= {"d_above_90"} if d == float(np.nextafter(90.0, INF)) and after["is_offset"] else set()
        k |= {"d_below_minus_90"} if d == float(np.nextafter(-90.0, -INF)) and after["is_offset"] and rep["ang_diff"] > 269 else set()
        k |= {"d_minus_270"} if d == -270.0 and rep["ang_diff"] == 90.0 and after["is_offset"] else set()
        k |= {"odom_zero"} if oa == 0 else set()
        k |= {"odom_inf"} if oa == INF else set()
        k |= {"odom_minus_inf"} if oa == -INF else set()
        k |= {"odom_nan"} if math.isnan(oa) and math.isnan(after["ang_sum"]) else set()
        if (after["ang_count"] == 1.0 and before["ang_count"] == 3.0 and after["frames"] == before["frames"] and
                after["odom"].tobytes() == before["odom"].tobytes()):
            k.add("replaced_bookkeeping")
    return k
