"""Parity at the edges of the region stage's LDS layout (-m gpu): the maps of tests/region_layout_cases.py -- small regions that leave the
small-region grower's window at either end, a list longer than the list ring, a region across more tiles than the tile cache holds, a
regrown and rejected region of ~90 pixels -- on the 4-wave and the 8-wave build against the correctly rounded oracle: the line records
byte for byte, the counts and lineIm.  tests/test_region_layout_cpu.py proves that the maps are what they are taken for."""
import numpy as np
import pytest

import region_layout_cases as rl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches(oracle):
    """{name: (maps [n, 256, 256], [(lines, lineIm) of the oracle per map])}, computed once."""
    singles = rl.single_maps()
    out = {}
    for name, maps in (("strokes", rl.stroke_batch()), ("long_diagonal_regrown", np.stack([singles[k] for k in sorted(singles)]))):
        refs = []
        for m in maps:
            r = oracle.lsd(m.copy(), _lib=oracle.lib_cr())
            refs.append((r["lines"], r["lineIm"]))
        maps.setflags(write=False)
        out[name] = (maps, refs)
    return out


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("name", ["strokes", "long_diagonal_regrown"])
def test_layout_edges_match_the_oracle(name, waves, batches, lsdmod, ctx):
    maps, refs = batches[name]
    assert len(maps) <= 8 and maps.shape[1:] == (256, 256)
    ctx.set_region_waves(waves)
    try:
        lines, offsets, ims = ctx.run_batch(maps.copy())
    finally:
        ctx.set_region_waves(0)
    bad = []
    for i, (ref_lines, ref_im) in enumerate(refs):
        got = lines[offsets[i]:offsets[i + 1]]
        if len(got) != len(ref_lines):
            bad.append((i, "count %d != %d" % (len(got), len(ref_lines))))
        elif got.tobytes() != ref_lines.tobytes():
            bad.append((i, "records"))
        if not np.array_equal(ims[i], ref_im):
            bad.append((i, "lineIm"))
    assert not bad, bad
    assert sum(len(r[0]) for r in refs) > 0
