"""The two scan ingestion rules of k_ingest.hip restated in plain Python (no vectorisation, no device): what the drivers' read loops leave
in lidarPointPolar[] in front of FeatureScan.

pairs      the file driver (LSD/main_on_windows.cpp:104-123): a reading is kept iff `range != INFINITY`, so -inf and NaN stay.
LaserScan  laserCallback (LSD/main_on_linux.cpp:53-66) on the float fields of sensor_msgs/LaserScan: kept iff `ranges[i] != INFINITY` in
           float, angle = angle_min + i * angle_increment with the product and the sum each rounded to single precision (numpy float32
           scalars), packed to the front as the file driver packs (the callback's stale-slot indexing is not reproduced).
Both return (scans float64 [n, stride, 2]: the kept readings first in beam order, +0.0 after them; lens int32 [n]); take[i] == 0 gives
an empty scan."""
import numpy as np

INF32 = np.float32(np.inf)


def laserscan_angle(angle_min, angle_increment, i):
    return float(np.float32(angle_min) + np.float32(np.float32(i) * np.float32(angle_increment)))


def _pack(n, stride, beams, take):
    scans, lens = np.zeros((n, stride, 2), np.float64), np.zeros(n, np.int32)
    for s in range(n):
        if take is not None and not take[s]:
            continue
        for rng, ang in beams(s):
            scans[s, lens[s]] = (rng, ang)
            lens[s] += 1
    return scans, lens


def ingest_pairs(raw, stride=None, take=None):
    raw = np.asarray(raw, np.float64)
    return _pack(len(raw), stride or raw.shape[1], lambda s: [(r, a) for r, a in raw[s] if r != np.inf], take)


def ingest_laserscan(ranges, angle_min_inc, stride=None, take=None):
    rg, ami = np.asarray(ranges, np.float32), np.asarray(angle_min_inc, np.float32)
    return _pack(len(rg), stride or rg.shape[1],
                 lambda s: [(float(r), laserscan_angle(ami[s, 0], ami[s, 1], i)) for i, r in enumerate(rg[s]) if r != INF32], take)
