"""Do maps reach what tests/line_cases.py hands K5 as hand-made end points?  Runs the correctly rounded oracle (no GPU) on N random
small maps -- noise with walls, random cells, bars 1 ... 5 cells thick, blocks of unknown cells, at sca 0.3 / 0.5 / 1.0 -- and counts
the records with k NaN (x1 == x2 and y1 == y2) and the marked samples that lie exactly half-way between two cells, where C's round
and rint part.  Usage: python tools/line_probe.py [N=2000] [first seed=0]; prints one line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import line_cases as lc                                    # noqa: E402
from oracle import oracle                                  # noqa: E402


def random_map(seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(64, 200)), int(rng.integers(64, 200))
    kind = seed % 4
    if kind == 0:
        return lc.noise_with_walls(seed, rows, cols, walls=int(rng.integers(2, 10)), unknown=float(rng.uniform(0.1, 0.6)))
    if kind == 1:
        return rng.choice(np.array([lc.UNKNOWN, lc.OCC, lc.FREE], np.uint8), size=(rows, cols), p=[0.2, 0.05, 0.75])
    m = np.full((rows, cols), lc.FREE, np.uint8)
    for _ in range(int(rng.integers(1, 6))):
        if kind == 2:                                      # a bar 1 ... 5 cells thick at any angle
            x0, y0, a, L, t = rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(0, np.pi), rng.integers(20, 150), rng.integers(1, 6)
            s = np.arange(0, L, 0.5)
            for d in range(int(t)):
                xs = np.clip((x0 + s * np.cos(a) - d * np.sin(a)).astype(int), 0, cols - 1)
                ys = np.clip((y0 + s * np.sin(a) + d * np.cos(a)).astype(int), 0, rows - 1)
                m[ys, xs] = lc.OCC
        else:                                              # a block of unknown cells
            y0, x0 = int(rng.integers(0, rows - 8)), int(rng.integers(0, cols - 8))
            m[y0:y0 + int(rng.integers(4, 80)), x0:x0 + int(rng.integers(4, 80))] = lc.UNKNOWN
    return m


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    oracle.build()
    lines = nan = halves = 0
    for seed in range(first, first + n):
        m = random_map(seed)
        rows, cols = m.shape
        r = oracle.lsd(m.copy(), _lib=oracle.lib_cr(), sca=(0.3, 0.5, 1.0)[seed % 3])["lines"]
        lines += len(r)
        nan += int(np.isnan(r["k"]).sum())
        for x1, y1, x2, y2 in zip(r["x1"], r["y1"], r["x2"], r["y2"]):
            s = lc.samples(x1, y1, x2, y2, rows, cols)
            with np.errstate(all="ignore"):
                k = (y2 - y1) / (x2 - x1)
                v = (s.xx - x1) * k + y1 if s.along_x else (s.yy - y1) / k + x1
            halves += int((s.marked & (np.abs(v - np.trunc(v)) == 0.5)).sum())
    print("line probe: %d maps (seeds %d ...), %d lines, %d with k NaN, %d marked samples exactly on a half" % (n, first, lines, nan, halves))


if __name__ == "__main__":
    main()
