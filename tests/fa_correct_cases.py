"""The grid match response fused into a carry (include/lsd_hip.h: lsd_enqueue_fa_carry_correct_device; csrc/k_facorrect.hip; DESIGN.md
8.1.10) restated on Python floats, in the header's order, written from the header for the tests (not from the HIP code), and the generated
campaign both test files run.

Python floats are IEEE doubles without contraction, so every statement below rounds as the device build (-ffp-contract=off) rounds it;
every sum runs ascending from 0.0.  P is a list of rows (P[i][j] = P(i, j)); a carry record stores it column-major.  A unit of the
campaign is ONE sequence: its carry, the original poses of its frames_pitch slots, its response records, the four parameters and
whether the key lets it take part; batches() groups units that can share a launch.
"""
import math

import numpy as np

import fa_restatement as fr
import grid_response_cases as gr

STATE_DTYPE = np.dtype([("x", "f8", (9,)), ("P", "f8", (81,))])
POS_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8")])
CARRY_DTYPE = np.dtype([("state", STATE_DTYPE), ("odom", POS_DTYPE), ("ang_sum", "f8"), ("ang_count", "f8"), ("frames", "i4"), ("is_offset", "i4")])
REP_DTYPE = np.dtype([("innov", "f8", (3,)), ("d2", "f8"), ("det", "f8"), ("slot", "i4"), ("flags", "u4")])
assert CARRY_DTYPE.itemsize == 768 and REP_DTYPE.itemsize == 48
APPLIED, NO_POSE, NOT_FINITE, STALE, NO_RESPONSE, SINGULAR, GATED = 1, 2, 4, 8, 16, 32, 64
FLAG_NAMES = {APPLIED: "applied", NO_POSE: "no_pose", NOT_FINITE: "not_finite", STALE: "stale", NO_RESPONSE: "no_response",
              SINGULAR: "singular", GATED: "gated"}
DEFAULTS = (1.0, 1.0, 1.0, 0.0)                                            # cov_scale, floor_xy, floor_ang, gate: fa_correct()'s
INF, NAN = float("inf"), float("nan")


def words(values):
    """The bytes of doubles as uint64 words: what the slot search compares."""
    return np.array([float(v) for v in values], np.float64).view(np.uint64)


def dot(a, b):
    s = 0.0
    for u, v in zip(a, b):
        s += u * v
    return s


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def correct_state(x, P, poses, resp, par, trace=None):
    """x [9], P rows, poses float64 [frames_pitch, 3] (compared as bytes), resp RESPONSE_DTYPE [frames_pitch], par (cov_scale, floor_xy,
    floor_ang, gate) -> dict(flags, slot, innov, d2, det, x, P): x and P are the inputs unless flags == APPLIED.  trace: a dict that
    receives what classes_of reads."""
    x = [float(v) for v in x]
    P = [[float(v) for v in row] for row in P]
    cov_scale, floor_xy, floor_ang, gate = (float(v) for v in par)
    out = dict(flags=0, slot=-1, innov=[0.0, 0.0, 0.0], d2=0.0, det=0.0, x=x, P=P)
    tr = trace if trace is not None else {}
    pose_words = np.ascontiguousarray(poses, np.float64).reshape(-1, 3).view(np.uint64)
    tr.update(frames_pitch=len(pose_words), sentinel=abs(x[0] + 1), hits=[], resp_flags=None, gate=gate,
              not_finite=[("x", i) for i in range(9) if not math.isfinite(x[i])] +
                         [("P", i, j) for i in range(9) for j in range(9) if not math.isfinite(P[i][j])])
    if abs(x[0] + 1) < 0.0001:                                               # 1
        out["flags"] = NO_POSE
        return out
    if tr["not_finite"]:                                                     # 2
        out["flags"] = NOT_FINITE
        return out
    key = words(x[:3])                                                       # 3
    hits = [t for t in range(len(pose_words)) if (pose_words[t] == key).all()]
    tr["hits"] = hits
    tr["equal_by_value_only"] = [t for t in range(len(pose_words)) if t not in hits and
                                 all(float(a) == b for a, b in zip(pose_words[t].view(np.float64), x[:3]))]
    if not hits:
        out["flags"] = STALE
        return out
    slot = out["slot"] = hits[-1]
    r = resp[slot]                                                           # 4
    rf = tr["resp_flags"] = int(r["flags"])
    if not rf & gr.VALID or rf & (gr.NONE | gr.EMPTY | gr.MISMATCH):
        out["flags"] = NO_RESPONSE
        return out
    z = [float(r["x"]), float(r["y"]), float(r["ang"])]
    c = [float(v) for v in r["cov"]]
    bad = [("z", i) for i in range(3) if not math.isfinite(z[i])] + [("cov", i) for i in range(6) if not math.isfinite(c[i])]
    if bad:
        tr["not_finite"] = bad
        out["flags"] = NOT_FINITE
        return out
    R = [[c[0] * cov_scale + floor_xy, c[1] * cov_scale, c[3] * cov_scale],  # 5
         [c[1] * cov_scale, c[2] * cov_scale + floor_xy, c[4] * cov_scale],
         [c[3] * cov_scale, c[4] * cov_scale, c[5] * cov_scale + floor_ang]]
    S = [[P[a][b] + R[a][b] for b in range(3)] for a in range(3)]

    def cof(a, b):
        a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
        return S[a1][b1] * S[a2][b2] - S[a1][b2] * S[a2][b1]
    det = out["det"] = (cof(0, 0) * S[0][0] + cof(1, 0) * S[1][0]) + cof(2, 0) * S[2][0]
    invdet = fr.fdiv(1.0, det)
    if not det > 0 or not math.isfinite(invdet):
        out["flags"] = SINGULAR
        return out
    Sinv = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            Sinv[j][i] = cof(i, j) * invdet
    innov = out["innov"] = [z[q] - x[q] for q in range(3)]                   # 6
    t = [dot(Sinv[i], innov) for i in range(3)]
    d2 = out["d2"] = dot(innov, t)
    tr.update(Sinv=Sinv, R=R)
    if gate > 0 and not d2 <= gate:
        out["flags"] = GATED
        return out
    K = [[dot([P[i][r] for r in range(3)], [Sinv[r][q] for r in range(3)]) for q in range(3)] for i in range(9)]      # 7
    out["x"] = [x[i] + dot(K[i], innov) for i in range(9)]
    out["P"] = [[P[i][j] - dot(K[i], [P[j][r] for r in range(3)]) for j in range(9)] for i in range(9)]
    out["flags"] = APPLIED
    tr["K"] = K
    return out


def rows_of(rec):
    """(x [9], P rows) of a carry or state record."""
    st = rec["state"] if "state" in rec.dtype.names else rec
    return [float(v) for v in st["x"]], np.asarray(st["P"], np.float64).reshape(9, 9, order="F").tolist()


def correct_carry(rec, poses, resp, par, trace=None):
    """One carry record (CARRY_DTYPE, or the package's FA_CARRY_DTYPE) -> (the carry after, its report REP_DTYPE)."""
    x, P = rows_of(rec)
    o = correct_state(x, P, poses, resp, par, trace)
    new = rec.copy()
    if o["flags"] == APPLIED:
        new["state"]["x"] = o["x"]
        new["state"]["P"] = np.array(o["P"], np.float64).ravel(order="F")
    rep = np.zeros(1, REP_DTYPE)[0]
    rep["innov"], rep["d2"], rep["det"], rep["slot"], rep["flags"] = o["innov"], o["d2"], o["det"], o["slot"], o["flags"]
    return new, rep


# ---- units ---------------------------------------------------------------------------------------------------------------------------------
def spd(rng, n=9, ridge=9.0):
    A = rng.normal(size=(n, n))
    return A @ A.T + ridge * np.eye(n)


def carry_of(x, P, k=0):
    """A carry record around (x, P rows); the loop's other variables hold values a correction must leave alone."""
    c = np.zeros(1, CARRY_DTYPE)
    c["state"]["x"][0] = x
    c["state"]["P"][0] = np.array(P, np.float64).ravel(order="F")
    c["odom"][0] = (0.5 + k, -0.25, 0.125)
    c["ang_sum"], c["ang_count"], c["frames"], c["is_offset"] = 12.5 + k, 3.0, 3 + k, k & 1
    return c[0]


def valid_resp(rng, pose, flags=gr.VALID):
    """A response record as the response stage writes one around `pose`: a refined pose within half a cell / half a step, a covariance."""
    r = np.zeros(1, gr.RESPONSE_DTYPE)[0]
    sub = rng.uniform(-0.5, 0.5, 3)
    r["x"], r["y"], r["ang"] = pose[0] + round(rng.uniform(-2, 2)) + sub[0], pose[1] + round(rng.uniform(-2, 2)) + sub[1], pose[2] + sub[2] * 0.5
    C3 = spd(rng, 3, 0.05) * 0.4
    r["cov"] = (C3[0, 0], C3[0, 1], C3[1, 1], C3[0, 2], C3[1, 2], C3[2, 2])
    r["sub"], r["m"], r["score_centre"], r["n_used"], r["flags"] = sub, rng.integers(1, 1 << 20, 10), 7000, 40, flags
    return r


def unit(name, seed, frames_pitch=1, slot=None, par=DEFAULTS, origin="made", state=None):
    """A sequence whose carry matches slot `slot` (default: the last) of poses of noise, with a valid response in every slot."""
    rng = np.random.default_rng(seed)
    if state is None:
        x = [float(v) for v in np.concatenate([rng.normal((300, 250, 20), (40, 40, 30)), rng.normal(0, 2, 3), rng.normal(0, 0.3, 3)])]
        P = spd(rng).tolist()
    else:
        x, P = [float(v) for v in state[0]], [[float(v) for v in row] for row in state[1]]
    poses = rng.normal(300, 40, (frames_pitch, 3))
    slot = frames_pitch - 1 if slot is None else slot
    poses[slot] = x[:3]
    resp = np.array([valid_resp(rng, poses[t]) for t in range(frames_pitch)], gr.RESPONSE_DTYPE)
    return dict(name=name, carry=carry_of(x, P, seed & 3), poses=poses, resp=resp, par=tuple(float(v) for v in par), skip=False, origin=origin)


def set_x(u, i, v):
    """x[i] = v; the slot that matched follows a change of the pose."""
    old = words(u["carry"]["state"]["x"][:3])
    u["carry"]["state"]["x"][i] = v
    if i < 3:
        for t in range(len(u["poses"])):
            if (u["poses"][t].view(np.uint64) == old).all():
                u["poses"][t, i] = v
    return u


def set_P(u, i, j, v):
    u["carry"]["state"]["P"][j * 9 + i] = v
    return u


def run_unit(u, trace=None):
    """(carry after, report) of a unit; (the carry as it is, None) for a unit the key leaves out."""
    if u["skip"]:
        return u["carry"].copy(), None
    return correct_carry(u["carry"], u["poses"], u["resp"], u["par"], trace)


def nextafter(v, to):
    return float(np.nextafter(np.float64(v), np.float64(to)))


# (p, r) of the closed form, P = p I and R = r I, both powers of two.  The identities are exact only where 1 / (p + r)^3 is, so p + r is a
# power of two as well, which two powers of two reach only as p == r; the pose and the measurement are dyadic, so no product rounds.
POW2 = ((4.0, 4.0), (0.5, 0.5), (1024.0, 1024.0))


def campaign(log_states=()):
    """The units.  log_states: (x, P rows) of frames of the `data` log's replay (the CPU suite replays it with the oracle, the GPU suite on
    the device)."""
    U = []
    for k in range(3):                                                       # the plain case at every frames_pitch, the slot search
        for fp in (1, 3, 64, 65):
            U.append(unit("plain_%d_%d" % (fp, k), 100 + 10 * fp + k, fp))
            if fp > 1:
                U.append(unit("first_%d_%d" % (fp, k), 200 + 10 * fp + k, fp, slot=0))
                u = unit("twice_%d_%d" % (fp, k), 300 + 10 * fp + k, fp, slot=fp // 2)
                u["poses"][0] = u["poses"][fp // 2]                          # two slots match: the later one wins
                if k == 2:
                    u["poses"][fp - 1] = u["poses"][0]
                U.append(u)
                u = unit("stale_%d_%d" % (fp, k), 400 + 10 * fp + k, fp)
                u["poses"][fp - 1, k] += 0.125                               # the carry has moved on
                U.append(u)
        u = unit("skip_%d" % k, 500 + k, (1, 3, 65)[k])
        u["skip"] = True
        U.append(u)
        u = set_x(unit("zero_sign_%d" % k, 510 + k, 3), k, 0.0)               # a pose that differs from the carry in the sign of a zero
        u["poses"][2, k] = -0.0
        U.append(u)
        u = set_x(unit("zero_sign_match_%d" % k, 515 + k, 3), k, -0.0)        # ... and -0.0 on both sides matches
        U.append(u)
        U.append(set_x(unit("no_pose_%d" % k, 520 + k, (1, 3, 64)[k]), 0, -1.0))
        for tag, d in (("in_lo", -0.9999e-4), ("in_hi", 0.9999e-4), ("out_lo", -1.0001e-4), ("out_hi", 1.0001e-4)):
            U.append(set_x(unit("sentinel_%s_%d" % (tag, k), 530 + k, (1, 3, 65)[k]), 0, -1.0 + d))
        bad = (NAN, INF, -INF)[k]
        U.append(set_x(unit("nf_x0_%d" % k, 540 + k, 3), 0, bad))
        U.append(set_x(unit("nf_x8_%d" % k, 550 + k, 3), 8, bad))
        U.append(set_P(unit("nf_P88_%d" % k, 560 + k, 3), 8, 8, bad))
        u = unit("nf_cov4_%d" % k, 570 + k, 3)
        u["resp"]["cov"][2, 4] = bad
        U.append(u)
        u = unit("nf_cov4_other_slot_%d" % k, 575 + k, 3)                    # a slot that is not the carry's: never read
        u["resp"]["cov"][0, 4] = bad
        U.append(u)
        for tag, fl in (("none", gr.NONE), ("empty", gr.VALID | gr.EMPTY), ("mismatch", gr.VALID | gr.MISMATCH), ("unset", 0)):
            u = unit("resp_%s_%d" % (tag, k), 580 + k, (1, 3, 64)[k])
            u["resp"]["flags"][-1] = fl
            U.append(u)
        u = unit("resp_rejected_%d" % k, 590 + k, 3)                         # what the response stage writes behind a rejected match
        head = u["resp"][2][["x", "y", "ang"]].copy()
        u["resp"][2] = np.zeros(1, gr.RESPONSE_DTYPE)[0]
        u["resp"][2]["x"], u["resp"][2]["y"], u["resp"][2]["ang"], u["resp"][2]["flags"] = head["x"], head["y"], head["ang"], gr.NONE
        U.append(u)
        for tag, fl in (("x", gr.X_NOT_PEAK), ("all", gr.X_NOT_PEAK | gr.Y_NOT_PEAK | gr.A_NOT_PEAK)):
            u = unit("not_peak_%s_%d" % (tag, k), 600 + k, 3)
            u["resp"]["flags"][2] = gr.VALID | fl
            U.append(u)
        u = unit("cov_zero_%d" % k, 610 + k, 3, par=(1.0, 0.5 + k, 2.0, 0.0))
        u["resp"]["cov"][:] = 0.0
        U.append(u)
        u = unit("singular_zero_%d" % k, 620 + k, (1, 3, 65)[k], par=(1.0 + k, 0.0, 0.0, 0.0))
        u["resp"]["cov"][:] = 0.0
        for i in range(3):
            for j in range(3):
                set_P(u, i, j, 0.0)
        U.append(u)
        u = unit("det_negative_%d" % k, 630 + k, 3)
        u["resp"]["cov"][2, (0, 2, 5)[k]] = -1.0e4                           # (caller memory: no authentic covariance is negative)
        U.append(u)
        U.append(unit("cov_scale_zero_%d" % k, 640 + k, 3, par=(0.0, 1.0, 0.25 * (k + 1), 0.0)))
        U.append(unit("cov_scale_big_%d" % k, 645 + k, 3, par=(1000.0, 0.0, 0.0, 0.0)))
        u = unit("huge_ungated_%d" % k, 650 + k, 3)
        u["resp"]["x"][2] += 1.0e6 * (k + 1)                                 # gate = 0: a huge d2 is applied
        U.append(u)
        base = unit("gate_%d" % k, 660 + k, (1, 3, 3)[k])
        d2 = float(run_unit(base)[1]["d2"])
        for tag, g in (("eq", d2), ("below", nextafter(d2, 0.0)), ("above", nextafter(d2, INF)), ("wide", 2 * d2), ("tight", d2 / 2)):
            u = unit("gate_%s_%d" % (tag, k), 660 + k, (1, 3, 3)[k], par=DEFAULTS[:3] + (g,))
            U.append(u)
        u = unit("asymmetric_%d" % k, 670 + k, 3)
        set_P(u, 0, 1, u["carry"]["state"]["P"][1] + 0.75)                   # P(0,1) != P(1,0)
        set_P(u, 5, 2, u["carry"]["state"]["P"][2 * 9 + 5] - 1.5)
        U.append(u)
        p, r = POW2[k]
        x = [float(v) for v in (40.0 + k, 25.0, -3.0, 1.5, -0.5, 0.25, 0.125, 0.0, -0.0625)]
        u = unit("closed_form_%d" % k, 680 + k, 3, par=(1.0, r, r, 0.0), state=(x, (p * np.eye(9)).tolist()), origin="closed_form")
        u["resp"]["cov"][:] = 0.0
        u["resp"]["x"][2], u["resp"]["y"][2], u["resp"]["ang"][2] = x[0] + 1.5, x[1] - 0.75, x[2] + 0.25   # dyadic: nothing rounds
        U.append(u)
        x0, P0 = fr.reset_state()
        x0[:3] = (300.0 + k, 251.5, 17.25)
        U.append(unit("reset_cov_%d" % k, 690 + k, 3, state=(x0, P0)))
    for k, st in enumerate(log_states):
        U.append(unit("log_%d" % k, 700 + k, (1, 3, 64, 65)[k % 4], state=st, origin="log"))
    return U


CLASSES = (sorted(FLAG_NAMES.values()) + ["key_skip", "sentinel_in_lo", "sentinel_in_hi", "sentinel_out_lo", "sentinel_out_hi",
           "nf_x0", "nf_x8", "nf_P88", "nf_cov4"] + ["fp_%d" % n for n in (1, 3, 64, 65)] +
           ["slot_first", "slot_last", "slot_twice", "stale_zero_sign", "resp_none", "resp_empty", "resp_mismatch", "resp_rejected",
            "x_not_peak_applied", "cov_zero_floors", "singular_zero", "det_negative", "gate_eq", "gate_ulp_below", "gate_ulp_above",
            "gate_off_huge", "cov_scale_zero", "asymmetric", "log_state", "closed_form"])


def classes_of(u, tr, rep):
    """The classes a unit reaches: predicates on the restatement's trace `tr` and report `rep` (None, None for a unit the key leaves out)."""
    if u["skip"]:
        return {"key_skip"}
    c = {FLAG_NAMES[int(rep["flags"])], "fp_%d" % tr["frames_pitch"]} & set(CLASSES)
    s, fl, x0 = tr["sentinel"], int(rep["flags"]), float(u["carry"]["state"]["x"][0])
    for tag, inside in (("in", True), ("out", False)):                       # within 2e-8 of the threshold, on either side of it
        if (fl == NO_POSE) == inside and (0.9998e-4 < s < 1.0e-4 if inside else 1.0e-4 <= s < 1.0002e-4):
            c.add("sentinel_%s_%s" % (tag, "lo" if x0 < -1 else "hi"))
    if fl == NOT_FINITE:
        nf = tr["not_finite"]
        c |= {name for name, where in (("nf_x0", ("x", 0)), ("nf_x8", ("x", 8)), ("nf_P88", ("P", 8, 8)), ("nf_cov4", ("cov", 4))) if nf == [where]}
    hits, fp = tr["hits"], tr["frames_pitch"]
    if fp > 1 and hits:
        c |= {"slot_first"} if hits == [0] else set()
        c |= {"slot_last"} if hits == [fp - 1] else set()
        c |= {"slot_twice"} if len(hits) >= 2 and int(rep["slot"]) == hits[-1] else set()
    if fl == STALE and tr["equal_by_value_only"]:
        c.add("stale_zero_sign")
    rf = tr["resp_flags"]
    if fl == NO_RESPONSE:
        r = u["resp"][int(rep["slot"])]
        rest = r.tobytes()[24:184] + r.tobytes()[188:]                       # every byte but the pose and the flags
        c |= {"resp_none"} if rf & gr.NONE else set()
        c |= {"resp_rejected"} if rf == gr.NONE and not any(rest) else set()
        c |= {"resp_empty"} if rf & gr.EMPTY else set()
        c |= {"resp_mismatch"} if rf & gr.MISMATCH else set()
    if rf is not None and fl in (APPLIED, GATED, SINGULAR):
        cov, par, d2, det = [float(v) for v in u["resp"][int(rep["slot"])]["cov"]], u["par"], float(rep["d2"]), float(rep["det"])
        P3 = [u["carry"]["state"]["P"][j * 9 + i] for i in range(3) for j in range(3)]
        if fl == APPLIED:
            c |= {"x_not_peak_applied"} if rf == gr.VALID | gr.X_NOT_PEAK else set()
            c |= {"cov_zero_floors"} if not any(cov) and par[1] > 0 and par[2] > 0 else set()
            c |= {"gate_eq"} if par[3] > 0 and d2 == par[3] else set()
            c |= {"gate_ulp_above"} if par[3] > 0 and nextafter(d2, INF) == par[3] else set()
            c |= {"gate_off_huge"} if par[3] == 0 and d2 > 1e6 else set()
            c |= {"cov_scale_zero"} if par[0] == 0 and any(cov) else set()
            P = rows_of(u["carry"])[1]
            c |= {"asymmetric"} if any(P[i][j] != P[j][i] for i in range(9) for j in range(i)) else set()
            c |= {"log_state"} if u["origin"] == "log" else set()
            c |= {"closed_form"} if u["origin"] == "closed_form" else set()
        if fl == GATED and nextafter(d2, 0.0) == par[3]:
            c.add("gate_ulp_below")
        if fl == SINGULAR:
            c |= {"singular_zero"} if det == 0 and not any(cov) and not any(P3) and par[1] == 0 and par[2] == 0 else set()
            c |= {"det_negative"} if det < 0 else set()
    return c


def batches(units):
    """Launches over the units: one per (frames_pitch, parameters) -- the units that can share a launch, in campaign order --, then the
    counts around the kernel's sequences-per-workgroup boundary (1, 2, 3 and 65 sequences, the last by repeating units) from the largest
    group.  A batch: dict(name, frames_pitch, par, units, keys (int32 per unit, or None), key)."""
    groups = {}
    for u in units:
        groups.setdefault((len(u["poses"]), u["par"]), []).append(u)
    out = []
    for n, ((fp, par), us) in enumerate(groups.items()):
        out.append(dict(name="group_%d_fp%d" % (n, fp), frames_pitch=fp, par=par, units=us))
    fp, par = max((k for k in groups if k[0] == 3), key=lambda k: len(groups[k]))
    big = groups[(fp, par)]
    for count in (1, 2, 3, 65):
        out.append(dict(name="count_%d" % count, frames_pitch=fp, par=par, units=[big[(5 * count + i) % len(big)] for i in range(count)]))
    for n, b in enumerate(out):
        skips = [u["skip"] for u in b["units"]]
        b["key"] = 7
        b["keys"] = np.array([3 if s else 7 for s in skips], np.int32) if any(skips) or n % 2 else None
    return out


def run_batch(b):
    """(carries after CARRY_DTYPE [n], reports: a list of REP_DTYPE records, None where the key leaves the sequence out)."""
    got = [run_unit(u) for u in b["units"]]
    return np.array([c for c, _ in got], CARRY_DTYPE), [r for _, r in got]


# ---- a second formulation, in exact arithmetic ---------------------------------------------------------------------------------------------
def exact_update(x, P, Sinv, innov):
    """K, x' and P' of step 7 in fractions.Fraction from the same (rounded) Sinv and innovation, with the magnitudes the bound needs:
    returns (x' [9], P' rows, bx [9], bP rows), |computed - exact| <= b for every entry (roundings only; no underflow, which none of the
    campaign's magnitudes reaches).  With u = 2^-53 and g = 3u / (1 - 3u), the bound of a sum of three rounded products:
      a computed K(i,q) is off by at most eK(i,q) = g * sum_r |P(i,r) Sinv(r,q)|;
      the computed dot d^ of K^ with v is off from the exact dot of the EXACT K with v by at most g * sum|K^ v| + sum eK |v| =: e, and
      |d^| <= (1 + g) * sum|K^ v|;
      the last rounding, base + d^ or base - d^, adds at most u * (|base| + |d^|)."""
    from fractions import Fraction as F
    u = F(1, 2 ** 53)
    g = 3 * u / (1 - 3 * u)
    Fx, FP, FS, Fv = [F(v) for v in x], [[F(v) for v in r] for r in P], [[F(v) for v in r] for r in Sinv], [F(v) for v in innov]
    K = [[sum(FP[i][r] * FS[r][q] for r in range(3)) for q in range(3)] for i in range(9)]
    eK = [[g * sum(abs(FP[i][r] * FS[r][q]) for r in range(3)) for q in range(3)] for i in range(9)]
    Kh = [[F(dot([P[i][r] for r in range(3)], [Sinv[r][q] for r in range(3)])) for q in range(3)] for i in range(9)]     # the computed K

    def bound(i, vec, base):
        mag = sum(abs(Kh[i][q] * vec[q]) for q in range(3))
        return g * mag + sum(eK[i][q] * abs(vec[q]) for q in range(3)) + u * (abs(base) + (1 + g) * mag)
    xe = [Fx[i] + sum(K[i][q] * Fv[q] for q in range(3)) for i in range(9)]
    bx = [bound(i, Fv, Fx[i]) for i in range(9)]
    Pe = [[FP[i][j] - sum(K[i][r] * FP[j][r] for r in range(3)) for j in range(9)] for i in range(9)]
    bP = [[bound(i, [FP[j][r] for r in range(3)], FP[i][j]) for j in range(9)] for i in range(9)]
    return xe, Pe, bx, bP


# ---- recovery on the room of tests/grid_match_cases.py -------------------------------------------------------------------------------------
RECOVERY_DRAWS = 40
RECOVERY_RESPONSE = gr.params(2, 2, 1)


def recovery_draws():
    """Per draw of default_rng(1): for each of the room's three true poses, every component displaced by a uniform magnitude in 1..3 with a
    random sign (cells, cells, degrees)."""
    rng = np.random.default_rng(1)
    return [rng.uniform(1.0, 3.0, (3, 3)) * rng.choice((-1.0, 1.0), (3, 3)) for _ in range(RECOVERY_DRAWS)]


def recover(corr, scans, lens, truth, offsets):
    """The restatements of match, response and correction in sequence from carries at the reset covariance around truth + offsets: the
    corrected poses float64 [3, 3] and the reports."""
    import grid_match_cases as gm
    start = truth + offsets
    rec = gm.match(scans, lens, start, gm.ROOM["resol"], gm.ROOM["range_max"], corr, gm.RECOVERY_SEARCH)
    resp, _ = gr.response(scans, lens, start, rec, gm.ROOM["resol"], gm.ROOM["range_max"], corr, gm.RECOVERY_SEARCH["ang_step"], RECOVERY_RESPONSE)
    out, reps = [], []
    for s in range(len(truth)):
        x, P = fr.reset_state()
        x[:3] = [float(v) for v in start[s]]
        o = correct_state(x, P, start[s:s + 1], resp[s:s + 1], DEFAULTS)
        out.append(o["x"][:3])
        reps.append(o)
    return np.array(out), reps
