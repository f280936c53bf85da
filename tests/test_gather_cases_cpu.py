"""The hand-off campaign without a GPU (tests/gather_cases.py): every class is reached under the restatement alone; the library's host
side (lsd_gather_unpack through ctypes) and the torch packer (dist.pack_lines / compact_lines on CPU tensors) equal the restatement on
every case; and a cost-aware deal (lsd_shard_balanced) followed by hand-off and unpack gives the batch in perm order."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import gather_cases as gc


@pytest.fixture(scope="module")
def ldist():
    return importlib.import_module("linesegmentdetector-slam_amd.dist")


def test_every_class_is_reached():
    """The condition that keeps the campaign from quietly covering nothing: at least three cases per class, judged by classes_of on the
    restatement's trace."""
    hits = dict.fromkeys(gc.CLASSES, 0)
    for case in gc.campaign():
        got = gc.classes_of(case, gc.trace(case))
        assert got <= set(gc.CLASSES), got - set(gc.CLASSES)
        for k in got:
            hits[k] += 1
    print("gather cases: %d cases, %d rank hand-offs; cases per class %s" % (len(gc.campaign()), sum(c.world for c in gc.campaign()), hits))
    for k in gc.CLASSES:
        assert hits[k] >= gc.NEED, (k, hits[k])


def test_the_campaign_is_deterministic_and_its_records_use_every_word():
    a, b = gc._aimed() + gc._random(40, 7), gc.campaign()
    assert len(a) == len(b)
    seen_nan = False
    for x, y in zip(a, b):
        assert repr(x) == repr(y)
        for r in range(x.world):
            assert x.lines[r].tobytes() == y.lines[r].tobytes() and x.counts[r].tobytes() == y.counts[r].tobytes()
            live = np.arange(x.max_lines)[None, :] < np.clip(x.counts[r].astype(np.int64), 0, x.max_lines)[:, None]
            assert x.lines[r][~live].all()                                      # what must never travel is never zero
            if live.sum() >= 64:
                assert (x.lines[r][live] != 0).any(axis=0).all()                # every word of the record, the padding word included
            seen_nan |= bool(np.isnan(x.lines[r][live].view(np.float64)).any())
    assert seen_nan


def test_restatement_on_hand_made_shards():
    """The rule itself on a case small enough to write down."""
    assert [gc.shard(7, 3, r) for r in range(3)] == [(0, 3), (3, 5), (5, 7)] and gc.layout(7, 3) == 3
    assert [gc.shard(1, 2, r) for r in range(2)] == [(0, 1), (1, 1)] and gc.layout(1, 2) == 1
    lines = np.arange(3 * 2 * 10, dtype=np.int64).reshape(3, 2, 10) + 100
    cpad, slab = gc.pack(lines, np.array([2, -1, 5], np.int32), 4, 2, 3)
    assert cpad.tolist() == [2, 0, 2, 0, 3, 3]                                  # clamped, padded; 3 of 4 rows kept; both bits
    assert np.array_equal(slab, np.stack([lines[0, 0], lines[0, 1], lines[2, 0]]))
    cpad, slab = gc.pack(lines, np.array([1, 0, 1], np.int32), 3, 2, 4)
    assert cpad.tolist() == [1, 0, 1, 2, 0] and np.array_equal(slab[:2], np.stack([lines[0, 0], lines[2, 0]])) and not slab[2:].any()
    ca = np.array([[2, 1, 2, 3, 1], [1, 0, 0, 1, 2]], np.int32)                 # world 2, n_total 5: rank 0 dropped 2 of its 5 rows
    sl = np.arange(2 * 3 * 10, dtype=np.int64).reshape(2, 3, 10)
    offs, out, st = gc.unpack(ca, sl, 5, 2, 3)
    assert offs.tolist() == [0, 2, 3, 3, 4, 4] and st == gc.INTERNAL
    assert np.array_equal(out, np.concatenate([sl[0], sl[1, :1]]))


def _lib_unpack(L, ca, sl, case, lines_cap=None, want_lines=True):
    offs = np.full(case.n_total + 1, -7, np.int32)
    total = int(ca[:, :-2].sum())
    lines = np.full((max(total, 1), gc.WORDS), 0x3C3C3C3C, np.int64)
    st = L.lsd_gather_unpack(ca.ctypes.data, sl.ctypes.data, case.n_total, case.world, case.cap_rows, offs.ctypes.data,
                             lines.ctypes.data if want_lines else None, len(lines) if lines_cap is None else lines_cap)
    return st, offs, lines


def test_host_unpack_equals_the_restatement(lsdmod):
    """lsd_gather_unpack on the restated gathered arrays: offsets, line bytes and status on every case; the same offsets and status
    without lines_out; LSD_ERR_INVALID with room for one record less than arrives."""
    L = lsdmod.load_library()
    assert (lsdmod.LSD_OK, lsdmod.LSD_ERR_INVALID, lsdmod.LSD_ERR_HIP, lsdmod.LSD_ERR_CAPACITY, lsdmod.LSD_ERR_INTERNAL) == (
        gc.OK, gc.INVALID, gc.HIP, gc.CAPACITY, gc.INTERNAL)
    statuses = set()
    for case in gc.campaign():
        ca, sl = gc.gathered(case)
        per = gc.layout(case.n_total, case.world)
        assert lsdmod.gather_layout(case.n_total, case.world) == (per, case.world * (per + 2)), case
        assert [lsdmod.shard_range(case.n_total, case.world, r) for r in range(case.world)] == [
            gc.shard(case.n_total, case.world, r) for r in range(case.world)], case
        want_offs, want_lines, want_st = gc.unpack(ca, sl, case.n_total, case.world, case.cap_rows)
        statuses.add(want_st)
        st, offs, lines = _lib_unpack(L, ca, sl, case)
        assert st == want_st and np.array_equal(offs, want_offs), case
        assert lines[:len(want_lines)].tobytes() == want_lines.tobytes(), case
        assert (lines[len(want_lines):] == 0x3C3C3C3C).all(), case               # nothing written behind the records that arrived
        st, offs, _ = _lib_unpack(L, ca, sl, case, want_lines=False)
        assert st == want_st and np.array_equal(offs, want_offs), case
        if len(want_lines):
            st, _, _ = _lib_unpack(L, ca, sl, case, lines_cap=len(want_lines) - 1)
            assert st == gc.INVALID, case
        # the wrapper: what arrived is its result, or the `partial` of the error it raises
        if want_st == gc.OK:
            offs, recs = lsdmod.gather_unpack(ca, sl, case.n_total, case.world, case.cap_rows)
        else:
            with pytest.raises(lsdmod.LsdError) as e:
                lsdmod.gather_unpack(ca, sl, case.n_total, case.world, case.cap_rows)
            assert e.value.status == want_st, case
            offs, recs = e.value.partial
        assert np.array_equal(offs, want_offs) and recs.tobytes() == want_lines.tobytes(), case
    assert statuses == {gc.OK, gc.CAPACITY, gc.INTERNAL}


def test_torch_packer_equals_the_restatement(ldist):
    """dist.pack_lines on CPU tensors: slab bytes, clamped counts and over == (flag word != 0) on every rank of every case, and
    dist.compact_lines is the dense prefix (every clamped record, no cut)."""
    for case in gc.campaign():
        per = gc.layout(case.n_total, case.world)
        for r in range(case.world):
            cpad, slab = gc.pack(case.lines[r], case.counts[r], per, case.max_lines, case.cap_rows)
            n = len(case.counts[r])
            lines, counts = torch.from_numpy(case.lines[r].copy()), torch.from_numpy(case.counts[r].copy())
            got, c, over = ldist.pack_lines(lines, counts, case.cap_rows)
            assert got.numpy().tobytes() == slab.tobytes(), (case, r)
            assert c.dtype == torch.int64 and c.tolist() == cpad[:n].tolist(), (case, r)
            assert over.shape == (1,) and bool(over[0]) == (cpad[per + 1] != 0), (case, r)
            assert torch.equal(lines, torch.from_numpy(case.lines[r])) and torch.equal(counts, torch.from_numpy(case.counts[r]))
            T = int(cpad[:n].sum())
            _, whole = gc.pack(case.lines[r], case.counts[r], per, case.max_lines, max(T, 1))
            dense, c2 = ldist.compact_lines(lines, counts)
            assert dense.shape == (T, gc.WORDS) and dense.numpy().tobytes() == whole[:T].tobytes(), (case, r)
            assert c2.tolist() == cpad[:n].tolist(), (case, r)


@pytest.mark.parametrize("n_total,world,max_lines,seed", [(13, 3, 7, 1), (21, 8, 3, 2), (9, 2, 512, 3)])
def test_balanced_deal_arrives_in_perm_order(n_total, world, max_lines, seed, lsdmod):
    """lsd_shard_balanced, then hand-off and unpack, host only: rank r packs images perm[lo_r .. hi_r), and the unpacked batch holds
    image perm[g] at position g, as the header says."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_lines + 1, n_total).astype(np.int32)
    lines = gc.records(rng, n_total, max_lines, counts)
    costs = (rng.pareto(1.5, n_total) * 1e6 + 1).astype(np.int64)
    perm = lsdmod.shard_balanced(costs, world)
    assert sorted(perm.tolist()) == list(range(n_total)) and perm.tolist() != list(range(n_total))
    shards = [perm[slice(*gc.shard(n_total, world, r))] for r in range(world)]
    case = gc.Case("dealt", n_total, world, max_lines, int(counts.sum()) + 1, [lines[s] for s in shards], [counts[s] for s in shards])
    ca, sl = gc.gathered(case)
    offs, recs = lsdmod.gather_unpack(ca, sl, n_total, world, case.cap_rows)
    recs = recs.view(np.int64).reshape(-1, gc.WORDS)
    assert np.array_equal(np.diff(offs), counts[perm])
    for g in range(n_total):
        assert recs[offs[g]:offs[g + 1]].tobytes() == lines[perm[g], :counts[perm[g]]].tobytes(), g
