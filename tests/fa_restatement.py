"""A restatement of the reference's FeatureAssociation (LSD/myFA.cpp:13-184), its ukf (:404-536) and the replay driver's frame loop
(LSD/main_on_windows.cpp:80-186) in plain Python floats, written from the reference for the tests (not from the HIP code).

Python floats are IEEE doubles without contraction, so the arithmetic below rounds exactly like the device build (-ffp-contract=off),
statement by statement, in this order:
  1. pairs: scan lines outer (len >= 40), map lines inner (within 35 % of the scan line's length), 4 candidates per pair;
  2. keep score < 3 in single-thread order (pair, then matching), then a stable ascending sort by score (glibc's qsort merge sort);
  3. branches: reset / first frame / fusion (w = 1/(s*s), sums from 0 in sorted order) + ukf;
  4. ukf: Eigen's unblocked LLT, sigma points from ROWS of L, constant-acceleration prediction, Xdiv*diag(Wc) rounded per entry,
     plain ascending sums from 0, the 3x3 inverse as Eigen's cofactor formula;
  5. the frame loop: ScanPose from the odometry and the mean of the past angle offsets, the offset bookkeeping.
sind / cosd / atand are the correctly rounded ones of crmath.h (its host build), as on the device.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = 3.14159265358979323846            # == 4.0 * atan(1.0) (baseFunc.cpp:4)
RESET, FIRST, UKF = 0, 1, 2
INF = float("inf")

_crm = None
LOGS = ("data", "f3key", "f4key")                      # the replay logs under tests/golden/ (make_localize_logs.py)
# Three more recorded logs per key (data<N> of data_f3key / data_f4key), chosen from tests/golden/localize_survey.json: the longest,
# the one with the most resets after its first fix, the one with the largest n_kept.  A list of its own: the resume, fleet and
# re-base suites run over LOGS only.
MORE_LOGS = ("f3key_9", "f3key_2", "f3key_3", "f4key_3", "f4key_2", "f4key_4")
LOG_MAPS = {"data": "mapValue", "f3key": "f3key", "f4key": "f4key"}
LOG_MAPS.update({n: n.split("_")[0] for n in MORE_LOGS})
LOG_FRAMES = {"data": 99, "f3key": 279, "f4key": 273}


def log_lidar(z):
    """The lidar frames float64 [frames in the file, 360, 2] of a packed log: stored whole ("lidar"), or as the ranges and the one
    angle column that every frame of the log shares ("lidar_range" [n, 360], "lidar_angle" [360])."""
    import numpy as np
    if "lidar" in z.files:
        return z["lidar"]
    r = z["lidar_range"]
    return np.stack([r, np.broadcast_to(z["lidar_angle"], r.shape)], 2).astype(np.float64)


def load_log(name):
    """(map u8, map_param [5], lidar float64 [frames, 360, 2] of the replayed frames, Odom vector [frames + 1, 3]) of a replay log."""
    import numpy as np
    g = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(g, "localize_%s.npz" % name))
    lid = np.load(os.path.join(g, "lidar.npz"))["lidar"] if name == "data" else log_lidar(z)
    n = int(z["n_frames"])
    return np.load(os.path.join(g, "maps.npz"))[LOG_MAPS[name]], z["map_param"], lid[:n], z["odom"]


def load_way_points(name):
    """(realPos.txt float64 [k, 2] in metres, recored_Odom.txt int [k]: the 1-based frame count at which the robot stood on each)."""
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "localize_%s.npz" % name))
    return z["real_pos"], z["recorded"]


def crm():
    """The host build of crmath.h (tests/crmath_host.cpp), compiled once per process."""
    global _crm
    if _crm is None:
        so = os.path.join(tempfile.mkdtemp(prefix="fa_crm"), "libcrm_host.so")
        flags = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"] + flags +
                       ["-o", so, os.path.join(ROOT, "tests", "crmath_host.cpp"), "-lm"], check=True)
        _crm = C.CDLL(so)
    return _crm


def _sincos(x):
    a, s, c = (C.c_double * 1)(x), (C.c_double * 1)(), (C.c_double * 1)()
    crm().crm_sincos_n(a, s, c, 1)
    return s[0], c[0]


def sind(x):
    return _sincos(x / 180.0 * PI)[0]


def cosd(x):
    return _sincos(x / 180.0 * PI)[1]


def atand(x):
    a, o = (C.c_double * 1)(x), (C.c_double * 1)()
    crm().crm_atan_n(a, o, 1)
    return o[0] * 180.0 / PI


def fdiv(a, b):
    """a / b with IEEE semantics (Python raises on a zero divisor)."""
    if b != 0 or math.isnan(b):
        return a / b
    if a == 0 or math.isnan(a):
        return float("nan")
    return math.copysign(INF, a) * math.copysign(1.0, b)


def c_round(v):
    """(int)round(v): C round, half away from zero."""
    a = abs(v)
    f = math.floor(a)
    r = f + 1 if a - f >= 0.5 else f                    # a - f is exact
    return float(int(math.copysign(r, v)))


# ---- 1. pairs ---------------------------------------------------------------------------------------------
def pairs(map_len, scan_len):
    out = []
    for cs, ls in enumerate(scan_len):
        ls = float(ls)
        if ls < 40:
            continue
        ld = ls * 0.35
        for cm, lm in enumerate(map_len):
            lm = float(lm)
            if lm < ls - ld or lm > ls + ld:
                continue
            out.append((cm, cs))
    return out


# ---- 2. keep + sort ---------------------------------------------------------------------------------------
def keep_sorted(cands):
    """cands: sequence of (x, y, ang, score) in single-thread order -> the kept ones, stably sorted by score."""
    kept = [tuple(float(v) for v in c) for c in cands if float(c[3]) < 3]
    return sorted(kept, key=lambda c: c[3])            # Python's sort is stable


# ---- 4. ukf ------------------------------------------------------------------------------------------------
def llt(P):
    """Eigen's llt_inplace::unblocked on a copy of P (list of rows): returns (m, k), k = -1 on success or the first column whose
    pivot was not positive (columns >= k keep P's values).  matrixL() is the lower triangle of m."""
    m = [list(map(float, r)) for r in P]
    for k in range(9):
        x = m[k][k]
        if k > 0:
            sq = 0.0
            for j in range(k):
                sq += m[k][j] * m[k][j]
            x -= sq
        if x <= 0:
            return m, k
        x = math.sqrt(x)
        m[k][k] = x
        for i in range(k + 1, 9):
            v = m[i][k]
            if k > 0:
                t = 0.0
                for j in range(k):
                    t += m[i][j] * m[k][j]
                v -= t
            m[i][k] = v / x
    return m, -1


def weights():
    L, alpha, ki, beta = 9, 1e-2, 0.0, 2.0
    lam = alpha * alpha * (L + ki) - L
    c = L + lam
    wm = [lam / c] + [0.5 / c] * 18
    wc = [lam / c] + [0.5 / c] * 18
    wc[0] += 1 - alpha * alpha + beta
    return wm, wc, math.sqrt(c)


def sigma_points(x, P):
    """Xset (9 x 19, rows of lists): column 0 = x, column j + 1 = x + c * L[j, :], column j + 10 = x - c * L[j, :] (row j of L:
    A = c * L^T, myFA.cpp:446-450).  Returns (Xset, llt return)."""
    m, k = llt(P)
    _, _, c = weights()
    Lm = [[m[i][j] if i >= j else 0.0 for j in range(9)] for i in range(9)]
    X = [[0.0] * 19 for _ in range(9)]
    for i in range(9):
        X[i][0] = x[i]
        for j in range(9):
            A = c * Lm[j][i]
            X[i][j + 1] = x[i] + A
            X[i][j + 10] = x[i] - A
    return X, k


def ukf(x_in, P_in, scan_pose, est):
    """myfa::ukf: x_in [9], P_in rows, scan_pose (x, y, ang), est (x, y, ang) -> (x [9], P rows, llt)."""
    x = [float(v) for v in x_in]
    x[0] += scan_pose[0]; x[1] += scan_pose[1]; x[2] += scan_pose[2]
    wm, wc, _ = weights()
    X, k = sigma_points(x, P_in)
    t = 1.0
    Xs = [[0.0] * 19 for _ in range(9)]
    for col in range(19):
        Xs[0][col] = X[0][col] + t * X[3][col] + 0.5 * t * t * X[6][col]
        Xs[1][col] = X[1][col] + t * X[4][col] + 0.5 * t * t * X[7][col]
        Xs[2][col] = X[2][col] + t * X[5][col] + 0.5 * t * t * X[8][col]
        Xs[3][col] = X[3][col] + t * X[6][col]
        Xs[4][col] = X[4][col] + t * X[7][col]
        Xs[5][col] = X[5][col] + t * X[8][col]
        Xs[6][col] = X[6][col]
        Xs[7][col] = X[7][col]
        Xs[8][col] = X[8][col]
    Xm = [0.0] * 9
    for col in range(19):
        for i in range(9):
            Xm[i] += wm[col] * Xs[i][col]
    Xd = [[Xs[i][col] - Xm[i] for col in range(19)] for i in range(9)]
    T = [[Xd[i][col] * wc[col] for col in range(19)] for i in range(9)]

    def dot(a, b):
        s = 0.0
        for u, v in zip(a, b):
            s += u * v
        return s
    G = [[dot(T[i], Xd[j]) for j in range(9)] for i in range(9)]
    Q = [1.0, 1.0, 1.0, 0.01, 0.01, 0.01, 0.0001, 0.0001, 0.0001]
    P1 = [[G[i][j] + (Q[i] if i == j else 0.0) for j in range(9)] for i in range(9)]
    Zm = Xm[:3]                                          # the same sums over the same rows (:480-487)
    Pzz = [[G[r][q] + (1.0 if r == q else 0.0) for q in range(3)] for r in range(3)]
    Pxz = [[G[i][q] for q in range(3)] for i in range(9)]

    def cof(r, q):
        r1, r2, q1, q2 = (r + 1) % 3, (r + 2) % 3, (q + 1) % 3, (q + 2) % 3
        return Pzz[r1][q1] * Pzz[r2][q2] - Pzz[r1][q2] * Pzz[r2][q1]
    det = (cof(0, 0) * Pzz[0][0] + cof(1, 0) * Pzz[1][0]) + cof(2, 0) * Pzz[2][0]
    invdet = fdiv(1.0, det)
    inv = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            inv[j][i] = cof(i, j) * invdet
    K = [[dot(Pxz[i], [inv[r][q] for r in range(3)]) for q in range(3)] for i in range(9)]
    Zd = [est[r] - Zm[r] for r in range(3)]
    xo = [Xm[i] + dot(K[i], Zd) for i in range(9)]
    Po = [[P1[i][j] - dot(K[i], Pxz[j]) for j in range(9)] for i in range(9)]
    return xo, Po, k


def reset_state():
    x = [-1.0, -1.0] + [0.0] * 7
    d = [100.0, 100.0, 100.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0.1]
    return x, [[d[i] if i == j else 0.0 for j in range(9)] for i in range(9)]


# ---- 3. one frame --------------------------------------------------------------------------------------------
def feature_association(cands, last_pose, scan_pose, x_in, P_in, n_pairs=0):
    """cands in single-thread order -> (x [9], P rows, report dict)."""
    kept = keep_sorted(cands)
    rep = dict(n_pairs=n_pairs, n_kept=len(kept), llt=-2, scan_pose=tuple(scan_pose))
    if not kept:
        x, P = reset_state()
        rep.update(branch=RESET, estimate=(-1.0, -1.0, 0.0), score=INF)
        return x, P, rep
    if abs(last_pose[0] + 1) < 0.0001:
        b = kept[0]
        x = [float(v) for v in x_in]
        x[0], x[1], x[2] = b[0], b[1], b[2]
        rep.update(branch=FIRST, estimate=b[:3], score=b[3])
        return x, [list(map(float, r)) for r in P_in], rep
    sx = sy = sa = sw = 0.0
    for c in kept:
        w = fdiv(1.0, c[3] * c[3])
        sx += c[0] * w
        sy += c[1] * w
        sa += c[2] * w
        sw += w
    est = (fdiv(sx, sw), fdiv(sy, sw), fdiv(sa, sw))
    score = fdiv(1.0, math.sqrt(sw / len(kept)))
    x, P, k = ukf(x_in, P_in, scan_pose, est)
    rep.update(branch=UKF, estimate=est, score=score, llt=k)
    return x, P, rep


# ---- 5. the frame loop ---------------------------------------------------------------------------------------
class Loop:
    """The replay driver's bookkeeping around FeatureAssociation.  frame(t, ...) for t = 0, 1, ... (cnt_frame = t + 1)."""

    def __init__(self, odom, map_resol, x0=None, P0=None):
        self.odom = [tuple(map(float, r)) for r in odom]
        self.resol = float(map_resol)
        rx, rP = reset_state()
        self.x = list(x0) if x0 is not None else rx
        self.P = [list(r) for r in P0] if P0 is not None else rP
        self.ang_rotate = []
        self.is_offset = False

    def scan_pose(self, t):
        if abs(self.x[0] + 1) < 0.0001:
            return (0.0, 0.0, 0.0)
        theta = 0.0
        for a in self.ang_rotate:
            theta += a
        theta = theta / len(self.ang_rotate) if self.ang_rotate else float("nan")
        o1, o0 = self.odom[t + 1], self.odom[t]
        tx, ty, ta = (o1[0] - o0[0]) / self.resol, (o1[1] - o0[1]) / self.resol, atand(o1[2] - o0[2])
        s, c = sind(theta), cosd(theta)
        return (tx * c - ty * s, ty * s + ty * c, ta)

    def lidar_pose(self, lidar_pos):
        return (c_round(lidar_pos[0]), c_round(lidar_pos[1]), 0.0)

    def last_pose(self):
        return (self.x[0], self.x[1], self.x[2])

    def finish(self, t, x, P):
        self.x, self.P = x, P
        ang = x[2] - atand(self.odom[t + 1][2])
        if abs(ang) > 90 and t == 0:
            self.is_offset = True
        if self.is_offset and ang < 0:
            ang += 360
        self.ang_rotate.append(ang)
