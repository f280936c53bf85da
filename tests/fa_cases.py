"""Seeded, deterministic candidate lists and filter states for the fusion campaign (shared by the CPU and GPU tests).

k_fa_fuse (csrc/k_fa.hip) compacts the candidates with score < 3 in rounds of 256 lanes (wavefronts of 64), ranks them by (score,
position) in LDS up to FA_LDS (1024) kept ones and in global memory above, fuses them on one lane and runs the UKF.  The groups below
are built to reach what the replay logs never do (24-87 kept candidates per frame, scores well inside (0, 3), a well conditioned P):
  counts       candidate and kept counts on and beside every wavefront, round and FA_LDS boundary
  ties         equal scores whose input positions lie in different wavefronts and rounds, on poses whose sum depends on the order
  keep_edges   scores on and beside 3, NaN, negative, infinite, subnormal, and those whose square under- or overflows
  first_edges  lastPose.x on and beside both ends of fabs(x + 1) < 0.0001, and NaN
  llt          a non-positive, a zero and a NaN pivot at every column, a garbage upper triangle, extreme scalings
  state_edges  large states, angles beyond +-360, NaN / inf in ScanPose and in a candidate's pose
Every case is (cands float64 [n, 4] = (x, y, ang, score), last_pose, scan_pose, x [9], P [9, 9]) for lsd_debug_fa_fuse / fa_restatement.
feature_association.  cases(group) returns a list of (name, case)."""
import math

import numpy as np

BOUNDARY = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1300)
COUNT_PAIRS = tuple((n, n) for n in BOUNDARY) + tuple((k + (k + 1) // 2, k) for k in BOUNDARY)      # (n, k): k kept of n
LDS_RERUNS = {257: (257, 256), 1024: (1024, 1023)}       # kept count -> the FA_LDS values its cases run at again
DROPPED = (3.0, 3.5, float("inf"), float("nan"))
GROUPS = ("counts", "ties", "keep_edges", "first_edges", "llt", "state_edges")
INF, NAN = float("inf"), float("nan")
LAST, SCAN_POSE = (300.0, 200.0, 10.0), (1.5, -2.25, 0.75)
SCORES = (0.5, 1.0, 1.5, 2.5)


def spd(seed=5):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(9, 9))
    return A @ A.T + 9 * np.eye(9)


def state(seed=5):
    return np.linspace(-3, 5, 9) + np.array([300.0, 200.0, 10.0, 0, 0, 0, 0, 0, 0]), spd(seed)


def poses(rng, n):
    """n poses around (300, 200, 10) whose magnitudes span ten decades, so that a sum in another order rounds differently."""
    mag = 10.0 ** rng.integers(-2, 9, size=(n, 3))
    return np.array([300.0, 200.0, 10.0]) + rng.normal(size=(n, 3)) * mag


def kept_scores(rng, k):
    """Half of the scores from a few repeated values (ties), half distinct."""
    s = np.where(rng.random(k) < 0.5, rng.choice(SCORES, k), rng.uniform(0.05, 2.99, k))
    return s


def case(cands, last=LAST, sp=SCAN_POSE, x=None, P=None, seed=5):
    sx, sP = state(seed)
    return (np.asarray(cands, np.float64).reshape(-1, 4), tuple(last), tuple(sp), sx if x is None else np.asarray(x, np.float64),
            sP if P is None else np.asarray(P, np.float64))


def count_case(n, k):
    """k kept candidates among n, the dropped ones (3.0, 3.5, inf, NaN in turn) at seeded positions between them."""
    rng = np.random.default_rng(1000 * n + k)
    sc = np.empty(n)
    drop = np.zeros(n, bool)
    drop[rng.permutation(n)[:n - k]] = True
    sc[~drop] = kept_scores(rng, k)
    sc[drop] = [DROPPED[i % 4] for i in range(n - k)]
    return case(np.concatenate([poses(rng, n), sc[:, None]], 1))


def big_poses(n):
    """The 1e16 / -1e16 device of tests/test_localize_gpu.py's `ties` case, n times: x = 1e16, small, small, -1e16, small, ..."""
    p = np.zeros((n, 3))
    i = np.arange(n)
    p[:, 0] = np.where(i % 5 == 0, 1e16, np.where(i % 5 == 3, -1e16, 1.1 + 0.7318 * i))
    p[:, 1] = np.where(i % 3 == 0, 1e16, np.where(i % 3 == 1, 3.3 + 1.37 * i, -1e16))
    p[:, 2] = (i * 37) % 360 - 180.0
    return p


def tie_cases():
    n = 700
    i = np.arange(n)
    rng = np.random.default_rng(7)
    far = np.empty(n)                                    # ties only between positions i and i + 256 (and i + 512): score by i % 256
    far[:] = 0.25 + (rng.permutation(256)[i % 256]) / 128.0
    out = [("one_score", case(np.c_[big_poses(n), np.full(n, 1.25)])),
           ("two_scores", case(np.c_[big_poses(n), np.where(i % 2 == 0, 2.0, 0.75)])),
           ("round_apart", case(np.c_[big_poses(n), far]))]
    return out


def order_matters(c):
    """True if fusing the kept candidates of case c in REVERSED tie order gives another weighted sum than the stable order."""
    cd = c[0]
    kept = [tuple(r) for r in cd if r[3] < 3]
    a = sorted(kept, key=lambda r: r[3])
    b = sorted(reversed(kept), key=lambda r: r[3])

    def sums(seq):
        sx = sy = 0.0
        for r in seq:
            w = 1 / (r[3] * r[3])
            sx += r[0] * w
            sy += r[1] * w
        return sx, sy
    return sums(a) != sums(b)


KEEP_EDGES = (("below3", math.nextafter(3.0, 0.0)), ("3", 3.0), ("above3", math.nextafter(3.0, INF)), ("nan", NAN), ("neg0", -0.0),
              ("neg1", -1.0), ("neginf", -INF), ("denorm", 5e-324), ("1e-200", 1e-200), ("1e200", 1e200), ("neg1e200", -1e200))


def keep_edge_cases():
    rng = np.random.default_rng(11)
    out = []
    for name, s in KEEP_EDGES:
        out.append((name + "_alone", case([(301.0, 199.0, 12.0, s)])))
        mixed = np.c_[poses(rng, 9), kept_scores(rng, 9)]
        mixed[4, 3] = s
        out.append((name + "_mixed", case(mixed)))
    return out


def first_thresholds():
    """The doubles around both ends of fabs(x + 1) < 0.0001, found with nextafter: for each end (inner, outer) with inner the last
    double for which the test holds and outer its neighbour on the far side."""
    def holds(x):
        return abs(x + 1) < 0.0001
    ends = []
    for guess, away in ((-1.0 + 0.0001, INF), (-1.0 - 0.0001, -INF)):
        x = guess
        while not holds(x):
            x = math.nextafter(x, -1.0)
        while holds(math.nextafter(x, away)):
            x = math.nextafter(x, away)
        ends.append((x, math.nextafter(x, away)))
    return ends


def first_edge_cases():
    cands = [(10.0, 20.0, 30.0, 2.0), (11.0, 19.0, 29.0, 1.25)]                # two kept, the better one second
    (hi_in, hi_out), (lo_in, lo_out) = first_thresholds()
    xs = (("minus1", -1.0), ("hi_inner", hi_in), ("hi_outer", hi_out), ("lo_inner", lo_in), ("lo_outer", lo_out), ("nan", NAN))
    return [(n, case(cands, last=(x, -1.0, 0.0))) for n, x in xs]


def int_llt(seed=3):
    """An integer lower-triangular L with a positive diagonal and P = L L^T, exact in fp64."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-3, 4, size=(9, 9))).astype(np.float64)
    L[np.arange(9), np.arange(9)] = rng.integers(1, 5, size=9)
    return L, L @ L.T


def llt_cases():
    cands = [(10.0, 20.0, 30.0, 1.25), (11.0, 19.0, 29.0, 2.0)]
    x = np.arange(9.0)
    L, P0 = int_llt()
    out = []
    for k in range(9):
        P = spd(3)
        P[k, :] *= 1e-9; P[:, k] *= 1e-9; P[k, k] = -1.0
        out.append(("negative_%d" % k, case(cands, x=x, P=P)))
        P = P0.copy()
        P[k, k] -= L[k, k] ** 2                                                # the pivot of column k is exactly 0
        out.append(("zero_%d" % k, case(cands, x=x, P=P)))
    for k in (0, 4, 8):
        P = spd(3)
        P[k, k] = NAN
        out.append(("nan_%d" % k, case(cands, x=x, P=P)))
    d = np.diag([100.0, 100.0, 100.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0.1])
    out.append(("reset_P", case(cands, x=x, P=d)))
    out.append(("exact_P", case(cands, x=x, P=P0)))
    P = spd(3)
    P[np.triu_indices(9, 1)] = np.random.default_rng(4).normal(size=36) * 1e6    # only the lower triangle may be read
    P[0, 8], P[1, 7] = NAN, INF
    out.append(("garbage_upper", case(cands, x=x, P=P)))
    out.append(("scaled_1e-300", case(cands, x=x, P=spd(3) * 1e-300)))
    out.append(("scaled_1e300", case(cands, x=x, P=spd(3) * 1e300)))
    return out


def state_edge_cases():
    cands = [(10.0, 20.0, 30.0, 1.25), (11.0, 19.0, 29.0, 2.0), (12.0, 21.0, 31.0, 0.5)]
    big = np.array([1e6, -1e6, 1e6, -1e6, 1e6, -1e6, 1e6, -1e6, 1e6])
    out = [("x_1e6", case(cands, x=big)),
           ("angles", case([(10.0, 20.0, 725.0, 1.25), (11.0, 19.0, 1090.0, 2.0), (12.0, 18.0, -400.0, 2.5)], x=[1.0, 2.0, -800.0, 0, 0, 400.0, 0, 0, 0], sp=(1.0, 2.0, 1000.0))),
           ("nan_scan_pose", case(cands, sp=(1.0, NAN, 0.5))),
           ("inf_pose", case(cands + [(INF, 5.0, 6.0, 1.0)])),
           ("inf_both_signs", case(cands + [(INF, 5.0, 6.0, 1.0), (-INF, 5.0, -INF, 1.5)]))]
    return out


def cases(group):
    if group == "counts":
        return [("n%d_k%d" % p, count_case(*p)) for p in COUNT_PAIRS]
    return dict(ties=tie_cases, keep_edges=keep_edge_cases, first_edges=first_edge_cases, llt=llt_cases, state_edges=state_edge_cases)[group]()
