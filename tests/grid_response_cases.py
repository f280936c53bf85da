"""The response around a correlative match (csrc/k_gridresponse.hip): the rule restated in plain Python / numpy on the
helpers of tests/grid_match_cases.py and tests/grid_cases.py, and a generated campaign on small grids (at most 61 x 47 cells).

The restatement is the definition.  The end cells are the match's own (scored_ends, from the ORIGINAL pose); from there on the rule sums
bytes, compares integers and takes integer moments, and ends in one fp64 division per output (Python floats are IEEE doubles and never
fuse a multiply with an add).  Nothing has an iteration order, so the device must give the same bytes.

A case class is a predicate on the restatement's own TRACE, never on what the device gives.
"""
import math

import numpy as np

import grid_cases as gc
import grid_match_cases as gm

RESPONSE_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("ang", "f8"), ("cov", "f8", (6,)), ("sub", "f8", (3,)), ("m", "i8", (10,)),
                           ("score_centre", "u4"), ("n_used", "u4"), ("flags", "u4"), ("reserved", "u4")])
assert RESPONSE_DTYPE.itemsize == 192
VALID, NONE, X_NOT_PEAK, Y_NOT_PEAK, A_NOT_PEAK, EMPTY, MISMATCH = 1, 2, 4, 8, 16, 32, 64
MAX_OFFSET = 63


def params(rx=3, ry=3, ra=1, keep=(1, 2)):
    return dict(rx=rx, ry=ry, ra=ra, keep_num=keep[0], keep_den=keep[1])


def why_none(rec):
    """None, or why the scan of this match record gets no response."""
    fl = int(rec["flags"])
    if fl & gm.SKIPPED:
        return "none_skipped"
    if not fl & gm.ACCEPTED:
        return "none_rejected"
    if max(abs(int(rec["di"])), abs(int(rec["dj"])), abs(int(rec["da"]))) > MAX_OFFSET:
        return "none_range"
    return None


def parabola(m, c, p):
    """(the offset of the peak of the parabola through (-1, m), (0, c), (1, p), True if the centre is no peak) -- Python integers."""
    num, den = m - p, 2 * (m - 2 * c + p)
    if m > c or p > c or den >= 0:
        return 0.0, True
    if num == 0:
        return 0.0, False                                                # (0 / den is -0.0)
    return float(num) / float(den), False


def moments(R, rx, ry, ra, thr, kd):
    """(the ten moments as Python integers, n_used, the mask of the used candidates) of the volume R int64 [2 ra + 1, 2 ry + 1, 2 rx + 1]."""
    used = np.array([int(v) * kd >= thr for v in R.reshape(-1)], bool).reshape(R.shape)      # (Python integers: no product overflows)
    a, j, i = np.meshgrid(np.arange(-ra, ra + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    w = np.where(used, R, 0).astype(np.int64)                             # (every sum stays below 2^38)
    m = [int((w * f).sum()) for f in (1 + 0 * i, i, j, a, i * i, i * j, j * j, i * a, j * a, a * a)]
    return m, int(used.sum()), used


def response(scans, lens, poses, records, resol, range_max, corr, ang_step, rp, trace=None):
    """(the records RESPONSE_DTYPE [n], the volume uint32 [n, 2 ra + 1, 2 ry + 1, 2 rx + 1]) of the scans whose match wrote `records`
    (MATCH_DTYPE [n]) from the ORIGINAL poses float64 [n, 3].  rp: a dict of params().  trace: a list that receives one dict per scan."""
    rx, ry, ra, kn, kd = int(rp["rx"]), int(rp["ry"]), int(rp["ra"]), int(rp["keep_num"]), int(rp["keep_den"])
    assert 1 <= rx <= 7 and 1 <= ry <= 7 and 0 <= ra <= 7 and kd > 0 and kn <= kd          # (what the entry refuses is no case)
    step = float(ang_step)
    n = len(lens)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    records = np.ascontiguousarray(records)
    assert records.dtype == gm.MATCH_DTYPE and records.shape == (n,)
    out = np.zeros(n, RESPONSE_DTYPE)
    words = out.view(np.uint64).reshape(n, 24)
    rec_words = records.view(np.uint64).reshape(n, 7)
    vol = np.zeros((n, 2 * ra + 1, 2 * ry + 1, 2 * rx + 1), np.uint32)
    for s in range(n):
        rec = records[s]
        words[s, :3] = rec_words[s, :3]                                  # the record's pose as bits
        why = why_none(rec)
        if why:
            out[s]["flags"] = NONE
            if trace is not None:
                trace.append(dict(scan=s, none=why))
            continue
        di, dj, da, score = int(rec["di"]), int(rec["dj"]), int(rec["da"]), int(rec["score"])
        ang = float(poses[s, 2])
        R = np.zeros(vol.shape[1:], np.int64)
        nbs, ends_all, inside = {}, {}, {}
        no_pose = gc.scan_skip(poses[s]) is not None                      # (noise: no authentic record has such a pose)
        for ap in range(-ra, ra + 1):
            theta = ang + float(da + ap) * step
            ends = np.zeros((0, 2), np.int64) if no_pose else gm.scored_ends(scans[s], int(lens[s]), poses[s], theta, resol, range_max)
            R[ap + ra], inside[ap] = gm.scores(ends + np.array([di, dj], np.int64), corr, rx, ry)
            nbs[ap], ends_all[ap] = len(ends), ends
        vol[s] = R
        c = int(R[ra, ry, rx])
        flags = VALID | (0 if c == score else MISMATCH)
        m, n_used, used = moments(R, rx, ry, ra, score * kn, kd)
        axes = dict(x=(int(R[ra, ry, rx - 1]), c, int(R[ra, ry, rx + 1])), y=(int(R[ra, ry - 1, rx]), c, int(R[ra, ry + 1, rx])),
                    a=(int(R[ra - 1, ry, rx]), c, int(R[ra + 1, ry, rx])) if ra else None)
        sub = [0.0, 0.0, 0.0]
        for k, (axis, bit) in enumerate((("x", X_NOT_PEAK), ("y", Y_NOT_PEAK), ("a", A_NOT_PEAK))):
            if axes[axis] is not None:
                sub[k], flat = parabola(*axes[axis])
                flags |= bit if flat else 0
        cov = [0.0] * 6
        if m[0] > 0:
            W = float(m[0])
            cov = [float(m[4]) / W, float(m[5]) / W, float(m[6]) / W, (float(m[7]) / W) * step, (float(m[8]) / W) * step,
                   (float(m[9]) / W) * (step * step)]
        else:
            flags |= EMPTY
        r = out[s]
        r["x"], r["y"], r["ang"] = float(rec["x"]) + sub[0], float(rec["y"]) + sub[1], float(rec["ang"]) + sub[2] * step
        r["cov"], r["sub"], r["m"], r["score_centre"], r["n_used"], r["flags"] = cov, sub, m, c, n_used, flags
        if trace is not None:
            trace.append(dict(scan=s, none=None, nb=nbs, ends=ends_all, inside=inside, R=R, used=used, score=score, centre=c, axes=axes,
                              winner=(da, dj, di), m=m, n_used=n_used, flags=flags, sub=sub))
    return out, vol


def forge(case, s, di, dj, da):
    """The record (an array of one) the match would write for scan s if (da, dj, di) were its winner and it were accepted."""
    se = case["search"]
    x, y, ang = (float(v) for v in case["poses"][s])
    theta = ang + float(da) * se["ang_step"]
    ends = gm.scored_ends(case["scans"][s], int(case["lens"][s]), case["poses"][s], theta, case["resol"], case["range_max"])
    S, _ = gm.scores(ends + np.array([di, dj], np.int64), case["corr"], 0, 0)
    rec = np.zeros(1, gm.MATCH_DTYPE)
    rec["x"], rec["y"], rec["ang"] = x + float(di), y + float(dj), theta
    rec["score"], rec["n_beams"], rec["di"], rec["dj"], rec["da"], rec["flags"] = int(S[0, 0]), len(ends), di, dj, da, gm.ACCEPTED
    return rec


# ---- the classes -----------------------------------------------------------------------------------------------------------------------
NB_COUNTS = (0, 1, 63, 64, 65, 257, 1025)
CLASSES = (["rx_1", "rx_7", "ry_1", "ry_7", "ra_0", "ra_1", "ra_7", "tr_9", "tr_49", "tr_225"] + ["nb_%d" % k for k in NB_COUNTS] +
           ["window_over_%s" % e for e in ("left", "right", "top", "bottom")] +
           ["all_outside", "beyond_wx", "beyond_na", "rim_x", "rim_y", "rim_a", "plateau", "half_minus", "half_plus", "symmetric_peak",
            "keep_at_equality", "keep_one_below", "keep_one_above", "keep_all", "uniform_plane", "offset_63", "none_skipped", "none_rejected",
            "none_range", "none_noise", "mismatch", "sub_nonzero"])
ONCE = ("nb_1025",)                                                       # the classes one case is enough for


def classes_of(case, trace):
    got = set()
    rp, se = case["response"], case["search"]
    rx, ry, ra, kn, kd = rp["rx"], rp["ry"], rp["ra"], rp["keep_num"], rp["keep_den"]
    rows, cols = case["corr"].shape
    for v in (1, 7):
        got |= {"rx_%d" % v} if rx == v else set()
        got |= {"ry_%d" % v} if ry == v else set()
    if ra in (0, 1, 7):
        got.add("ra_%d" % ra)
    n_tr = (2 * rx + 1) * (2 * ry + 1)
    if n_tr in (9, 49, 225):
        got.add("tr_%d" % n_tr)
    responded = False
    for t in trace:
        if t["none"]:
            got.add(t["none"])
            if case.get("noise"):
                got.add("none_noise")
            continue
        responded = True
        da, dj, di = t["winner"]
        if max(abs(da), abs(dj), abs(di)) == MAX_OFFSET:
            got.add("offset_63")
        for ap, nb in t["nb"].items():
            if nb in NB_COUNTS:
                got.add("nb_%d" % nb)
            e = t["ends"][ap]
            if len(e):
                x, y = e[:, 0] + di, e[:, 1] + dj
                y_in, x_in = (y + ry >= 0) & (y - ry < rows), (x + rx >= 0) & (x - rx < cols)
                for name, hit in (("left", (x - rx < 0) & (x + rx >= 0) & y_in), ("right", (x + rx >= cols) & (x - rx < cols) & y_in),
                                  ("top", (y - ry < 0) & (y + ry >= 0) & x_in), ("bottom", (y + ry >= rows) & (y - ry < rows) & x_in)):
                    if hit.any():
                        got.add("window_over_" + name)
        if t["nb"][0] > 0 and not any(ins.any() for ins in t["inside"].values()):
            got.add("all_outside")
            assert t["flags"] & EMPTY
        if abs(di) + rx > se["wx"] or abs(dj) + ry > se["wy"]:
            got.add("beyond_wx")
        if ra and abs(da) + ra > se["na"]:
            got.add("beyond_na")
        for axis, off, w, bit in (("x", di, se["wx"], X_NOT_PEAK), ("y", dj, se["wy"], Y_NOT_PEAK), ("a", da, se["na"], A_NOT_PEAK)):
            if t["axes"][axis] is None:
                continue
            m, c, p = t["axes"][axis]
            if (off == w and p > c) or (off == -w and m > c):
                got.add("rim_" + axis)
                assert t["flags"] & bit
            if m == c == p and c > 0:
                got.add("plateau")
                assert t["flags"] & bit
            if m == c > p:
                got.add("half_minus")
                assert t["sub"]["xya".index(axis)] == -0.5
            if p == c > m:
                got.add("half_plus")
                assert t["sub"]["xya".index(axis)] == 0.5
            if m == p < c:
                got.add("symmetric_peak")
                assert not t["flags"] & bit
        if any(v != 0.0 for v in t["sub"]):
            got.add("sub_nonzero")
        thr = t["score"] * kn
        Rv = [int(v) for v in t["R"].reshape(-1)]
        if kn == 0:
            got.add("keep_all")
            assert t["n_used"] == len(Rv)
        elif thr > 0:
            if any(v * kd == thr for v in Rv if v != t["centre"]):
                got.add("keep_at_equality")
            if any(v * kd < thr <= (v + 1) * kd for v in Rv):
                got.add("keep_one_below")
            if any((v - 1) * kd <= thr < v * kd for v in Rv):
                got.add("keep_one_above")
        if t["R"].min() == t["R"].max() > 0 and t["n_used"] == len(Rv):
            got.add("uniform_plane")
            assert t["m"][4] * 3 == t["m"][0] * rx * (rx + 1)
        if t["flags"] & MISMATCH:
            got.add("mismatch")
    return got


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
ANY = dict(min_beams=0, min_num=0, min_den=1)                             # a search that accepts whatever wins


def rcase(name, mcase, rp, records=None, **kw):
    """A response case: the match case, the response's parameters and the match records -- the restatement's own unless given."""
    c = dict(mcase, name=name, response=rp, **kw)
    c["records"] = gm.run_match_case(mcase)[0] if records is None else np.ascontiguousarray(records)
    return c


def one_beam(name, cells, se, rp, end=(24, 15), pose=(20.0, 15.0, 0.0)):
    """One beam from `pose` ending in the cell `end`; the plane is 0 but for cells {(x, y): value}."""
    corr = np.zeros((31, 41), np.uint8)
    for (x, y), v in cells.items():
        corr[y, x] = v
    return rcase(name, gm.match_case(name, corr, 0.05, 1.0, [gm.beams_at_cells(pose, [end], 0.05)], [pose], se), rp)


def campaign():
    cases = []
    rng = np.random.default_rng(20250901)
    # the neighbourhood's sizes: 9, 49 and 225 translations, rx / ry at 1 and 7, ra at 0, 1 and 7; the window beyond the search's
    for v in range(3):
        corr = gm.random_plane(rng, 61 - 3 * v, 47 - 2 * v)
        b = np.stack([rng.uniform(0.05, 1.2, 65), rng.uniform(-math.pi, math.pi, 65)], 1)
        m = gm.match_case("sizes_%d" % v, corr, 0.05, 1.5, [b, b[:40]], [(rng.uniform(22, 38), rng.uniform(18, 28), rng.uniform(-180, 180)), (30.0, 20.0, 0.0)],
                          gm.search(2, 2, 1, 1.5, **ANY))
        recs = gm.run_match_case(m)[0]
        for rx, ry, ra, keep in ((1, 1, 0, (1, 2)), (3, 3, 1, (1, 2)), (7, 7, 7, (3, 4)), (1, 7, 1, (0, 1)), (7, 1, 0, (1, 1)), (2, 3, 2, (0, 5))):
            cases.append(rcase("sizes_%d_%d%d%d" % (v, rx, ry, ra), m, params(rx, ry, ra, keep), recs))
    # scored-beam counts around the wavefront, the workgroup and beyond the short capacity
    for n in NB_COUNTS:
        for v in range(3 if n != 1025 else 1):
            cols, rows = 61 - 3 * v, 47 - 2 * v
            corr = gm.random_plane(rng, cols, rows)
            scored = np.stack([rng.uniform(0.05, 1.2, n), rng.uniform(-math.pi, math.pi, n)], 1)
            extra = np.array([(math.nan, 0.1), (-0.5, 0.2), (5.0, 0.3)])             # never scored: NaN, non-positive, beyond range_max
            b = np.concatenate([scored, extra])
            b = b[rng.permutation(len(b))]
            m = gm.match_case("nb%d_%d" % (n, v), corr, 0.05, 1.5, [b], [(rng.uniform(22, 38), rng.uniform(18, 28), rng.uniform(-180, 180))],
                              gm.search(2, 1, 1, 0.5, **ANY), stride=len(b) + 5 * v, capacity=1024 if len(b) <= 1024 else 2048)
            cases.append(rcase("nb%d_%d" % (n, v), m, params((3, 1, 2)[v], (3, 2, 1)[v], (1, 1, 0)[v])))
    # windows over every edge; every candidate outside the grid; offsets of 63
    for v in range(3):
        corr = gm.random_plane(rng, 33 + v, 29, 0.6)
        fan = [(0.45 + 0.02 * k, k * 2 * math.pi / 16) for k in range(16)]
        m = gm.match_case("edges_%d" % v, corr, 0.05, 1.5, [fan] * 6,
                          [(16.0, 14.0, 0.0), (6.0 + v, 14.0, 0.0), (27.0 + v, 14.0, 0.0), (16.0, 5.0 + v, 0.0), (16.0, 23.0 - v, 0.0), (200.0, -150.0, 5.0)],
                          gm.search(5, 6, 1, 2.0, **ANY))
        cases.append(rcase("edges_%d" % v, m, params(3, 3, 1)))
        far = gm.match_case("far_%d" % v, corr, 0.05, 1.5, [fan] * 3, [(16.0, 14.0, 0.0)] * 3, gm.search(63, 63, 63, 0.25, **ANY))
        cases.append(rcase("far_%d" % v, far, params(2 + v, 2, 1), np.concatenate([forge(far, 0, 63, 3, 0), forge(far, 1, -2, -63, 1), forge(far, 2, 1, 0, -63)])))
    # a winner on the rim of the search window with a higher neighbour outside, on each axis (the other axes: a symmetric peak)
    for v in range(3):
        cases.append(one_beam("rim_x_%d" % v, {(25, 15): 100 + v, (26, 15): 150, (27, 15): 200}, gm.search(1, 1, 0, **ANY), params(1 + v, 1, 0)))
        cases.append(one_beam("rim_x_low_%d" % v, {(23, 15): 100 + v, (22, 15): 150}, gm.search(1, 1, 0, **ANY), params(1, 2, 0)))
        cases.append(one_beam("rim_y_%d" % v, {(24, 16): 90 + v, (24, 17): 140, (24, 18): 220}, gm.search(0, 1, 0, **ANY), params(1, 1 + v, 0)))
        # a beam of 4 cells turned by 14.5 degrees ends one cell up: the search has one angle, the response looks one step either side
        cases.append(one_beam("rim_a_%d" % v, {(24, 15): 100 + v, (24, 16): 150}, gm.search(0, 0, 0, 14.5, **ANY), params(1, 1, 1)))
        # the plateau m == c == p and the uniform plane: cov_xx = rx (rx + 1) / 3
        fan = [(0.3 + 0.01 * k, k * 2 * math.pi / 12 + 0.05) for k in range(12)]
        m = gm.match_case("uniform_%d" % v, np.full((31, 41), 17 + 100 * v, np.uint8), 0.05, 1.0, [fan], [(20.0, 15.0, 10.0 * v)],
                          gm.search(3, 2 + v, v, 1.0, **ANY))
        cases.append(rcase("uniform_%d" % v, m, params((1, 3, 7)[v], (7, 3, 1)[v], (0, 1, 1)[v])))
        # m == c > p: the offset is exactly -0.5 (the tie went to the zero offset); its mirror; the symmetric peak
        cases.append(one_beam("half_minus_%d" % v, {(23, 15): 200 + v, (24, 15): 200 + v, (25, 15): 50}, gm.search(1, 1, 0, **ANY), params(1, 1, 0)))
        cases.append(one_beam("half_plus_%d" % v, {(24, 14): 60, (24, 15): 180 + v, (24, 16): 180 + v}, gm.search(1, 1, 0, **ANY), params(2, 2, 0)))
        cases.append(one_beam("symmetric_%d" % v, {(23, 15): 80 + v, (24, 15): 200, (25, 15): 80 + v, (24, 14): 30, (24, 16): 30 + 5 * v},
                              gm.search(1, 1, 0, **ANY), params(1, 1, 0)))
        # the keep test at equality and one either side: score = 200 + 2 v, keep = 1 / 2
        cases.append(one_beam("keep_%d" % v, {(24, 15): 200 + 2 * v, (23, 15): 99 + v, (25, 15): 100 + v, (24, 14): 101 + v, (24, 16): 7},
                              gm.search(1, 1, 0, **ANY), params(1, 1, 0, (1, 2))))
    # records without a response: skipped, not accepted, an offset of 64, noise; a record whose score was altered
    for v in range(3):
        corr = gm.random_plane(rng, 47, 41, 0.5)
        good = [(0.6 + 0.1 * v, 0.5), (0.9, 2.0 + v), (0.4, -1.0)]
        poses = [(math.nan, 10, 0), (10, 10, -math.inf), (-1.0, 12, 0), (1048577.0, 3, 0), (21.0 + v, 17.0, 0.0), (25.0, 19.0 + v, 45.0)]
        m = gm.match_case("no_response_%d" % v, corr, 0.05, 2.0, [good] * len(poses), poses, gm.search(1, 2, 1, 2.0, **ANY))
        cases.append(rcase("skipped_%d" % v, m, params(2, 2, 1)))
        strict = dict(m, search=gm.search(1, 2, 1, 2.0, min_beams=1, min_num=1, min_den=1))
        cases.append(rcase("rejected_%d" % v, strict, params(2, 2, 1)))
        recs = gm.run_match_case(m)[0]
        recs["di"][4], recs["dj"][5] = 64, -64
        if v == 2:
            recs["dj"][5], recs["da"][5] = 0, 64
        cases.append(rcase("offset_64_%d" % v, m, params(2, 2, 1), recs))
        noise = rng.integers(0, 256, len(poses) * 56, dtype=np.uint8).view(gm.MATCH_DTYPE)
        cases.append(rcase("noise_%d" % v, m, params(1, 1, 1), noise, noise=True))
        recs = gm.run_match_case(m)[0]
        recs["score"][4] = (int(recs["score"][4]) + 1 + v) & 0xFFFFFFFF
        recs["score"][5] = 0xFFFFFFFF if v else (int(recs["score"][5]) - 1) & 0xFFFFFFFF
        cases.append(rcase("altered_%d" % v, m, params(2, 2, 1, (1, 2)), recs))
    # the room: displaced scans come back to the truth; the response is taken around it
    corr, scans, lens, truth = gm.recovery()
    for v, (dx, dy, k) in enumerate(gm.RECOVERY_OFFSETS[:3]):
        se = dict(gm.RECOVERY_SEARCH, min_num=1, min_den=8)
        moved = truth + np.array([dx + 0.3, dy - 0.2, k * se["ang_step"] + 0.4])
        m = dict(name="room_%d" % v, scans=scans, lens=lens, poses=moved, resol=gm.ROOM["resol"], range_max=gm.ROOM["range_max"], corr=corr,
                 cols=gm.ROOM["cols"], rows=gm.ROOM["rows"], search=se, capacity=1024)
        cases.append(rcase("room_%d" % v, m, params(2, 2, 1)))
    return cases


def run_case(case, records=None):
    trace = []
    out, vol = response(case["scans"], case["lens"], case["poses"], case["records"] if records is None else records, case["resol"],
                        case["range_max"], case["corr"], case["search"]["ang_step"], case["response"], trace)
    return out, vol, trace
