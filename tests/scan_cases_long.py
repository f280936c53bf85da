"""The scan-side campaign for lidars beyond 1024 readings (k_rdp_long.hip), shared by the CPU and GPU tests: the families, groups and
helpers of tests/scan_cases.py at the lengths where the long kernel can go wrong.

  SHORT_LENGTHS  scans of 1 .. 360 readings packed at SHORT_STRIDE = 1025: the long kernel on short scans (one chunk of 64 and less,
                 the chunk boundary, a few chunks)
  LONG_LENGTHS   each at its own stride: the first stride the long kernel takes, a UTM-30LX's 1081, 17 * 64 +- 1 (the kernel is one
                 wavefront: its compactions and its farthest-point search walk chunks of 64), 2^11 and its neighbours, the capacity
                 and one below (64 * 64 - 1)
A few repetitions per length and group, the family rotating with group, length and repetition: a few hundred scans in all.
The families reach at these lengths what tests/test_long_scans_cpu.py asserts: joined and dropped clusters, more chords than the 360
line records, split points in the first and the last chunk, more pixels than PTS_CAP_SMALL."""
import numpy as np

import scan_cases as sc

SHORT_STRIDE = 1025
SHORT_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 360)
LONG_LENGTHS = (1025, 1081, 1087, 1089, 2047, 2048, 2049, 4095, 4096)
REPS = 3
PTS_CAP_LONG = 32768                                                 # what the GPU campaign stores per scan (check_bounds holds the generator to it)


def fam_zigzag_long(rng, n, g):
    """scan_cases.fam_zigzag with the alternation over the whole arc: every `per`-th reading a split point where thre_line allows it,
    far more chords than the 360 line records of a scan."""
    rm = sc._rmax(g[1][2])
    rho = rng.uniform(3.0, min(5.0, 0.45 * rm))
    ang = rng.uniform(-3, 0) + np.arange(n) * min(0.003, 3.0 / max(n, 1))
    per = int(rng.integers(2, 5))
    r = np.full(n, rho) + np.where(np.arange(n) % per == 0, 0.12, 0.0)
    return sc._finish(rng, r, ang, g[1][2], 0.0)


def _scan(gi, li, rep, n, g):
    k = (7 * gi + 3 * li + 5 * rep) % 16
    rng = np.random.default_rng((977, gi, li, rep))
    if k == 15:
        return "zigzag_long", fam_zigzag_long(rng, n, g)
    return sc._family(k, rng, n, g)


def campaign(lengths=None):
    """[dict(name, map_param, limit, thre_line, line_dist, scans, tags)], one per scan_cases.GROUPS entry, as scan_cases.campaign()."""
    lengths = SHORT_LENGTHS + LONG_LENGTHS if lengths is None else lengths
    out = []
    for gi, g in enumerate(sc.GROUPS):
        scans, tags = [], []
        for n in lengths:
            li = (SHORT_LENGTHS + LONG_LENGTHS).index(n)
            for rep in range(REPS):
                tag, s = _scan(gi, li, rep, n, g)
                assert s.shape == (n, 2) and np.isfinite(s).all() and (s[:, 0] > 0).all() and (s[:, 0] <= 60).all()
                scans.append(np.ascontiguousarray(s)); tags.append(tag)
        out.append(dict(name=g[0], map_param=g[1], limit=g[2], thre_line=g[3], line_dist=g[4], scans=scans, tags=tags))
    return out


def stride_of(n):
    return SHORT_STRIDE if n <= 360 else n


def by_stride(group):
    """{stride: indices of the group's scans that are packed at it}, in the order of the lengths."""
    out = {}
    for i, s in enumerate(group["scans"]):
        out.setdefault(stride_of(len(s)), []).append(i)
    return out


def check_bounds(refs):
    for r in refs:
        assert max(r["im_size"]) <= sc.IMAGE_LIMIT and len(r["pts"]) <= PTS_CAP_LONG, (r["im_size"], len(r["pts"]))


# ---- what a scan reaches: RegionSegmentation and SplitMerge restated for counting ---------------------------------------------------
def walk(scan, limit):
    """RegionSegmentation's walk (myRDP.cpp:297-330): (clusters [(first, last)] with the last run joined to cluster 0 where the reference
    joins it, runs dropped by region_point_limit, joined)."""
    r, a = scan[:, 0], scan[:, 1]
    n = len(scan)
    px, py = r * np.cos(a), r * np.sin(a)
    brk = np.hypot(px - np.roll(px, -1), py - np.roll(py, -1)) > sc.thre_delta(r)
    cl, start, dropped = [], 0, 0
    for i in np.nonzero(brk)[0]:
        if i - start >= limit:
            cl.append([start, int(i)])
        else:
            dropped += 1
        start = int(i) + 1
    joined = bool(cl) and not brk[n - 1]
    if joined:
        cl[0][0] = start
    return cl, dropped, joined


def split_points(scan, limit, thre_line):
    """The readings SplitMergeAssistant (myRDP.cpp:219-272) flags, by the same rule (first maximum, 9 m threshold) in numpy's arithmetic:
    for counting where split points fall, not for comparing results."""
    r, a = scan[:, 0], scan[:, 1]
    n = len(scan)
    px, py = r * np.cos(a), r * np.sin(a)
    flags = np.zeros(n, bool)
    todo = [tuple(c) for c in walk(scan, limit)[0]]
    while todo:
        sp, ep = todo.pop()
        ln = ep - sp + 1 if ep > sp else n + ep - sp + 1
        if ln <= 2:
            continue
        idx = (sp + np.arange(1, ln - 1)) % n
        with np.errstate(all="ignore"):
            k = (py[ep] - py[sp]) / (px[ep] - px[sp])
            d = py[ep] - k * px[ep]
            dist = np.abs(k * px[idx] - py[idx] + d) / np.sqrt(k * k + 1)
        dist = np.where(np.isnan(dist), -1.0, dist)
        j = int(np.argmax(dist))                                     # the first maximum
        if not dist[j] > 0:
            continue
        im = int(idx[j])
        if dist[j] > (r[im] * thre_line if r[im] > 9 else thre_line):
            flags[im] = True
            todo += [(sp, im), (im, ep)]
    return np.nonzero(flags)[0]
