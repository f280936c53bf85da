"""The hand-off campaign: a plain numpy restatement of the multi-GPU hand-off of the line lists as include/lsd_hip.h states it
(lsd_shard_range, lsd_gather_layout, the device pack of lsd_gather_lines, lsd_gather_unpack), and a generated, deterministic set of
cases aimed at where a pack kernel goes wrong: shards around the 256 lanes of k_pack_counts, empty shards, counts beyond max_lines and
below 0, slabs cut at and inside an image, and every value of the two-bit flag word.  tests/test_gather_cases_cpu.py holds the
library's host side and the torch packer against the restatement; tests/test_gather_cases_gpu.py holds the device pack against it.
No GPU and no library is needed to import this module.

A class is a predicate on the restatement's own trace of a case (rank_trace), never on what a generator meant to build and never on
what the device gives: classes_of() is the only judge."""
import numpy as np

WORDS = 10                                                  # sizeof(lsd_line) == 80 bytes, moved as 10 int64 words
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
OK, INVALID, HIP, CAPACITY, INTERNAL = 0, 1, 3, 5, 7        # include/lsd_hip.h
FLAG_DROPPED, FLAG_GAVE_UP = 1, 2                           # bit 0: rows were dropped; bit 1: an image the region stage gave up

N_LOCALS = (0, 1, 255, 256, 257, 513)
MAX_LINES = (1, 7, 512)
WORLDS = (1, 2, 3, 5, 8)
CLASSES = tuple("n_local_%d" % n for n in N_LOCALS) + (
    "pad_some", "pad_none",
    "count_0", "count_1", "count_max", "count_max_plus_1", "count_int32_max", "count_minus_1", "count_int32_min", "rank_all_zero",
    "cap_eq_T", "cap_eq_T_minus_1", "cut_at_boundary", "cut_inside", "image_beyond_cut", "cap_1", "cap_gt_T",
    "flag_0", "flag_1", "flag_2", "flag_3", "mixed_ranks") + tuple("max_lines_%d" % m for m in MAX_LINES) + tuple(
    "world_%d" % w for w in WORLDS) + ("n_total_lt_world",)
NEED = 3                                                    # cases that must reach each class


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def shard(n_total, world, rank):
    """The contiguous shard [lo, hi) of rank `rank`: lo = ceil(rank * n_total / world)."""
    return -(-rank * n_total // world), -(-(rank + 1) * n_total // world)


def layout(n_total, world):
    """per: the images of the largest shard."""
    return max(hi - lo for lo, hi in (shard(n_total, world, r) for r in range(world)))


def pack(lines, counts, per, max_lines, cap_rows):
    """What one rank sends: lines int64 [n_local, max_lines, 10], counts int32 [n_local] -> (cpad int32 [per + 2], slab int64
    [cap_rows, 10]).  cpad: the counts clamped to 0 .. max_lines and zero-padded to per, [per] the rows in the slab, [per + 1] the flag
    word.  The slab: every image's first count records, image after image, cut at cap_rows; zero behind them."""
    counts = np.asarray(counts, np.int64)
    n_local = len(counts)
    assert lines.shape == (n_local, max_lines, WORDS) and n_local <= per
    c = np.clip(counts, 0, max_lines)
    total = int(c.sum())
    cpad = np.zeros(per + 2, np.int32)
    cpad[:n_local] = c
    cpad[per] = min(total, cap_rows)
    cpad[per + 1] = (FLAG_DROPPED if total > cap_rows or (counts > max_lines).any() else 0) | (FLAG_GAVE_UP if (counts < 0).any() else 0)
    slab = np.zeros((cap_rows, WORDS), np.int64)
    row = 0
    for j in range(n_local):
        k = min(int(c[j]), cap_rows - row)
        slab[row:row + k] = lines[j, :k]
        row += k
    return cpad, slab


def gathered(case):
    """What every rank holds after the two all-gathers: (counts_all int32 [world, per + 2], slabs_all int64 [world, cap_rows, 10])."""
    per = layout(case.n_total, case.world)
    packs = [pack(case.lines[r], case.counts[r], per, case.max_lines, case.cap_rows) for r in range(case.world)]
    return np.stack([p[0] for p in packs]), np.stack([p[1] for p in packs])


def unpack(counts_all, slabs_all, n_total, world, cap_rows):
    """The host side: (offsets int32 [n_total + 1], lines int64 [total, 10] in global image order, status).  A rank's slab holds
    counts_all[r][per] rows: the images from the cut on are shorter by what it dropped.  INTERNAL outranks CAPACITY."""
    per = layout(n_total, world)
    counts_all = np.asarray(counts_all).reshape(world, per + 2)
    slabs_all = np.asarray(slabs_all).reshape(world, cap_rows, WORDS)
    offsets = np.zeros(n_total + 1, np.int32)
    parts, total, flags = [np.zeros((0, WORDS), np.int64)], 0, 0
    for r in range(world):
        lo, hi = shard(n_total, world, r)
        rows, row = int(counts_all[r, per]), 0
        flags |= int(counts_all[r, per + 1])
        for g in range(lo, hi):
            k = min(int(counts_all[r, g - lo]), max(rows - row, 0))
            offsets[g] = total
            parts.append(slabs_all[r, row:row + k])
            row += k
            total += k
    offsets[n_total] = total
    return offsets, np.concatenate(parts), INTERNAL if flags & FLAG_GAVE_UP else CAPACITY if flags & FLAG_DROPPED else OK


# ---- the trace and the classes --------------------------------------------------------------------------------------------------
def rank_trace(case, r):
    """What the restatement goes through on rank r: n_local, per, the raw and the clamped counts, each image's first row, the rank's
    total T, the rows kept and the flag word."""
    lo, hi = shard(case.n_total, case.world, r)
    per = layout(case.n_total, case.world)
    raw = np.asarray(case.counts[r], np.int64)
    assert len(raw) == hi - lo
    cpad, _ = pack(case.lines[r], case.counts[r], per, case.max_lines, case.cap_rows)
    c = cpad[:hi - lo].astype(np.int64)
    return dict(n_local=hi - lo, per=per, raw=raw, c=c, off=np.cumsum(c) - c, T=int(c.sum()), kept=int(cpad[per]), flags=int(cpad[per + 1]))


def trace(case):
    return [rank_trace(case, r) for r in range(case.world)]


def classes_of(case, tr):
    """The classes a case reaches, from its parameters and the restatement's trace alone."""
    cap, m, out = case.cap_rows, case.max_lines, set()
    for t in tr:
        if t["n_local"] in N_LOCALS:
            out.add("n_local_%d" % t["n_local"])
        for name, v in (("count_0", 0), ("count_1", 1), ("count_max", m), ("count_max_plus_1", m + 1), ("count_int32_max", INT32_MAX),
                        ("count_minus_1", -1), ("count_int32_min", INT32_MIN)):
            if (t["raw"] == v).any():
                out.add(name)
        if t["n_local"] > 0 and not t["raw"].any():
            out.add("rank_all_zero")
        c, off, T = t["c"], t["off"], t["T"]
        if cap == T and t["flags"] == 0:
            out.add("cap_eq_T")
        if cap == T - 1:
            out.add("cap_eq_T_minus_1")
        if cap < T and ((off == cap) & (c > 0)).any():
            out.add("cut_at_boundary")
        if ((off < cap) & (cap < off + c)).any():
            out.add("cut_inside")
        if ((off >= cap) & (c > 0)).any():
            out.add("image_beyond_cut")
        if cap == 1 and T > 1:
            out.add("cap_1")
        if cap > T:
            out.add("cap_gt_T")
        out.add("flag_%d" % t["flags"])
    out.add("pad_some" if any(t["per"] > t["n_local"] for t in tr) else "pad_none")
    if case.world > 1 and sum(t["flags"] != 0 for t in tr) == 1:
        out.add("mixed_ranks")
    if m in MAX_LINES and (m != 512 or case.n_total <= 8):
        out.add("max_lines_%d" % m)
    if case.world in WORLDS and (case.world == 1 or case.n_total % case.world):
        out.add("world_%d" % case.world)
    if case.n_total < case.world:
        out.add("n_total_lt_world")
    return out


# ---- the campaign ---------------------------------------------------------------------------------------------------------------
_SPECIAL_WORDS = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x8000000000000000, 0x7FF0000000000000,
                           0xFFFFFFFFFFFFFFFF], np.uint64).view(np.int64)     # quiet / signalling NaNs, -0.0, inf, all ones


def records(rng, n_local, max_lines, counts):
    """int64 [n_local, max_lines, 10]: 80 random bytes per record (every word, the tail padding of structLinesInfo included), a NaN or
    another special bit pattern in one word of every third record, and at and past an image's count a pattern that is never zero and
    never a record of the case -- it must not travel."""
    raw = rng.integers(0, 256, size=(n_local * max_lines, 80), dtype=np.uint8).view(np.int64)
    idx = np.arange(0, len(raw), 3)
    raw[idx, idx % WORDS] = _SPECIAL_WORDS[(idx // 3) % len(_SPECIAL_WORDS)]
    raw = raw.reshape(n_local, max_lines, WORDS)
    stale = np.arange(max_lines)[None, :] >= np.clip(np.asarray(counts, np.int64), 0, max_lines)[:, None]
    pattern = (0x5A5A5A5A00000001 + np.arange(raw.size, dtype=np.int64)).reshape(raw.shape)
    raw[stale] = pattern[stale]
    return raw


class Case:
    """One hand-off of a whole world: lines[r] int64 [n_local_r, max_lines, 10] and counts[r] int32 [n_local_r] per rank, one cap_rows."""

    def __init__(self, name, n_total, world, max_lines, cap_rows, lines, counts):
        self.name, self.n_total, self.world, self.max_lines, self.cap_rows = name, n_total, world, max_lines, int(cap_rows)
        self.lines, self.counts = lines, counts
        assert self.cap_rows >= 1 and max_lines >= 1 and n_total >= 1 and world >= 1      # (what lsd_gather_lines accepts)

    def __repr__(self):
        return "%s(n_total=%d world=%d max_lines=%d cap_rows=%d)" % (self.name, self.n_total, self.world, self.max_lines, self.cap_rows)


def _cap_rows(cap, counts, max_lines):
    """cap = ("abs", cap_rows) or (kind, rank[, k]): cap_rows placed against that rank's total T.  A kind the rank's counts cannot give
    falls back to T + 2."""
    kind = cap[0]
    if kind == "abs":
        return cap[1]
    c = np.clip(np.asarray(counts[cap[1]], np.int64), 0, max_lines)
    off, T = np.cumsum(c) - c, int(c.sum())
    if kind == "T" and T >= 1:
        return T
    if kind == "T-1" and T >= 2:
        return T - 1
    if kind == "boundary":
        at = off[(c > 0) & (off > 0)]
        if len(at):
            return int(at[len(at) // 2])
    if kind == "inside":
        at = off[c >= 2]
        if len(at):
            return int(at[len(at) // 2]) + 1
    if kind == "above":
        return T + cap[2]
    return T + 2


def make_case(name, n_total, world, max_lines, cap, seed, special=(), zero_ranks=(), full_ranks=()):
    """special: (rank, local index, count) overrides, the index taken modulo the shard; zero_ranks / full_ranks: every count 0 /
    max_lines."""
    rng = np.random.default_rng(seed)
    counts = []
    for r in range(world):
        lo, hi = shard(n_total, world, r)
        c = rng.integers(0, max_lines + 1, hi - lo)
        if r in zero_ranks:
            c[:] = 0
        if r in full_ranks:
            c[:] = max_lines
        counts.append(c.astype(np.int32))
    for r, j, v in special:
        if len(counts[r]):
            counts[r][j % len(counts[r])] = v
    lines = [records(rng, len(c), max_lines, c) for c in counts]
    return Case(name, n_total, world, max_lines, _cap_rows(cap, counts, max_lines), lines, counts)


def _aimed():
    mk, out = make_case, []
    # shards on and around the 256 lanes of k_pack_counts (chunk 1, 1, 2, 3 images per lane), flagged and clean, cut and whole
    out += [mk("lanes_255", 255, 1, 3, ("T", 0), 1), mk("lanes_256", 256, 1, 2, ("inside", 0), 2), mk("lanes_257", 257, 1, 3, ("boundary", 0), 3),
            mk("lanes_513", 513, 1, 4, ("T", 0), 4, full_ranks=(0,)), mk("lanes_513_cut", 513, 1, 4, ("T-1", 0), 5, special=((0, 512, -1), (0, 256, 5))),
            mk("lanes_511_w2", 511, 2, 2, ("above", 0, 3), 6), mk("lanes_513_w2", 513, 2, 1, ("T", 0), 7, special=((1, 255, INT32_MAX),)),
            mk("lanes_514_w2", 514, 2, 2, ("inside", 1), 8, special=((0, 256, INT32_MIN),)), mk("lanes_510_w2", 510, 2, 3, ("above", 1, 1), 9),
            mk("lanes_1025_w2", 1025, 2, 1, ("boundary", 0), 10, special=((1, 511, 2),)), mk("lanes_1026_w2", 1026, 2, 2, ("above", 0, 7), 11,
                                                                                                zero_ranks=(1,)),
            mk("lanes_765_w3", 765, 3, 1, ("T", 2), 12, special=((1, 254, -1),))]
    # fewer images than ranks: empty shards
    out += [mk("empty_1_w2", 1, 2, 7, ("T", 0), 20, full_ranks=(0,)), mk("empty_2_w3", 2, 3, 7, ("above", 0, 1), 21),
            mk("empty_3_w5", 3, 5, 3, ("abs", 1), 22, full_ranks=(0, 2, 4)), mk("empty_3_w8", 3, 8, 7, ("inside", 0), 23, full_ranks=(0,)),
            mk("empty_5_w8", 5, 8, 2, ("above", 7, 4), 24, special=((7, 0, -1),))]
    # max_lines 512 with few images; max_lines 1
    out += [mk("wide_3_w2", 3, 2, 512, ("inside", 0), 30, special=((0, 0, 512), (0, 1, 513))), mk("wide_5_w3", 5, 3, 512, ("above", 0, 9), 31,
                                                                                                 special=((1, 0, 1), (2, 0, 512))),
            mk("wide_2_w1", 2, 1, 512, ("boundary", 0), 32, full_ranks=(0,)), mk("wide_7_w5", 7, 5, 512, ("T", 0), 33, special=((0, 0, 511), (3, 0, 0))),
            mk("one_9_w2", 9, 2, 1, ("T-1", 0), 34, full_ranks=(0,)), mk("one_7_w3", 7, 3, 1, ("above", 0, 2), 35, special=((2, 0, 2),)),
            mk("one_11_w5", 11, 5, 1, ("abs", 1), 36, full_ranks=(1,), special=((4, 0, INT32_MIN),))]
    # every flag word with the other ranks clean, on the first and on a later rank
    for k, (v, r) in enumerate(((8, 0), (INT32_MAX, 2), (-1, 1), (INT32_MIN, 4), (-1, 7), (8, 7))):
        world = (3, 3, 5, 5, 8, 8)[k]
        out.append(mk("mixed_%d" % k, (7, 13, 11, 23, 21, 13)[k], world, 7, ("abs", 7 * 5 + 1), 40 + k, special=((r, 1, v),)))
    # both bits on one rank: a negative count and a count above max_lines; a negative count and a cut
    out += [mk("both_a", 7, 2, 7, ("abs", 64), 50, special=((0, 0, -1), (0, 2, 8))), mk("both_b", 13, 3, 7, ("T-1", 1), 51, special=((1, 1, INT32_MIN),)),
            mk("both_c", 5, 1, 7, ("inside", 0), 52, special=((0, 4, -1), (0, 0, 7))), mk("both_d", 21, 5, 3, ("abs", 64), 53,
                                                                                        special=((3, 0, INT32_MAX), (3, 1, INT32_MIN)))]
    # a rank with nothing but zeros next to ranks with lines; a world of zeros
    out += [mk("zeros_a", 7, 2, 7, ("T", 0), 60, zero_ranks=(1,)), mk("zeros_b", 13, 5, 3, ("above", 1, 0), 61, zero_ranks=(0, 3)),
            mk("zeros_c", 5, 3, 7, ("abs", 4), 62, zero_ranks=(0, 1, 2))]
    return out


def _random(n_cases, seed):
    rng = np.random.default_rng(seed)
    kinds = ("T", "T-1", "boundary", "inside", "one", "above", "above")
    values = (-1, INT32_MIN, INT32_MAX, 0, 1)
    out = []
    for i in range(n_cases):
        world = int(rng.choice(WORLDS))
        n_total = int(rng.integers(1, 25))
        if world > 1 and n_total % world == 0:
            n_total += 1
        max_lines = int(rng.choice((1, 2, 3, 7, 7)))
        r = int(rng.integers(0, world))
        kind = kinds[int(rng.integers(0, len(kinds)))]
        cap = ("abs", 1) if kind == "one" else (kind, r, int(rng.integers(1, 6)))
        special = []
        for _ in range(int(rng.integers(0, 3)) if i % 2 else 0):
            v = values[int(rng.integers(0, len(values)))] if rng.integers(0, 3) else max_lines + 1
            special.append((int(rng.integers(0, world)), int(rng.integers(0, 64)), v))
        out.append(make_case("random_%02d" % i, n_total, world, max_lines, cap, 1000 + i, special=tuple(special),
                             zero_ranks=(int(rng.integers(0, world)),) if i % 7 == 3 else ()))
    return out


_campaign = None


def campaign():
    """The cases, generated once per process and never changed by a test."""
    global _campaign
    if _campaign is None:
        _campaign = _aimed() + _random(40, 7)
    return _campaign
