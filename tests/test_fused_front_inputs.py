"""The synthetic inputs of tests/test_fused_front_gpu.py are maps the oracle takes (no GPU needed): it returns without error on each,
every image stays under the line capacity the GPU tests give the device entry point, and the shapes are the ones the cases are
built around."""
import numpy as np

import test_fused_front_gpu as t


def test_oracle_accepts_the_synthetic_inputs(oracle, maps):
    for name, batch, wh in (("tile", t.one_tile_plus_one(), (33, 25)), ("dense", t.dense(), (60, 60)),
                            ("empty", t.empty_next_to_full(), (120, 120)), ("batch", t.batch_of_three(maps), (96, 72))):
        assert batch.dtype == np.uint8 and batch.ndim == 3
        for im in batch:
            r = oracle.lsd(im.copy(), debug=True)
            d = r["dbg"]
            assert (d["w"], d["h"]) == wh, name
            assert len(r["lines"]) < t.MAX_LINES, name
            print(name, "lines", len(r["lines"]), "nb", d["nb"], "maxGrad", d["maxGrad"])
    # the dense case: every interior pixel has a non-zero gradient
    d = oracle.lsd(t.dense()[0].copy(), debug=True)["dbg"]
    assert (d["mag"][1:, 1:] > 0).all()
    # empty next to full: the Gaussian is zero up to the tile border and non-zero from it on
    g0, g1 = (oracle.lsd(im.copy(), debug=True)["dbg"]["gauss"] for im in t.empty_next_to_full())
    assert not g0[:, :32].any() and g0[50:85, 32].all()
    assert not g1[:24].any() and g1[24, 45:95].all()
