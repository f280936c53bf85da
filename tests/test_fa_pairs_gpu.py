"""The pair list of k_fa_prepare and a whole frame behind it on hand-made lines (tests/pair_cases.py): lsd_feature_association against
the restatement fed with fa_restatement.pairs and the device's own matching on those pairs -- n_pairs, n_kept, branch, state, P and
report bit for bit.  tests/test_fa_pairs_cpu.py checks the expected pairs against the reference's loop and shows what the frames reach."""
import numpy as np
import pytest

import fa_restatement as fr
import pair_cases as pc
from test_localize_gpu import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def map_cache(oracle):
    return oracle.map_cache(pc.room().copy(), pc.RES)


@pytest.mark.parametrize("name,mp,scan,last", pc.cases(), ids=[c[0] for c in pc.cases()])
def test_frame_on_hand_made_lines(name, mp, scan, last, ctx, map_cache):
    pts = pc.points()
    x0, P0 = pc.state()
    st, rep = ctx.feature_association(map_cache, mp, scan, pts, pc.LIDAR, last, pc.SCAN_POSE, (x0, P0))
    pairs = np.array(fr.pairs(mp["len"], scan["len"]), np.int32).reshape(-1, 2)
    if len(pairs):
        dev = ctx.scan_to_map_match(map_cache, mp, scan, pts, pc.LIDAR, last, pairs).reshape(-1)
        dev = np.stack([dev["x"], dev["y"], dev["ang"], dev["score"]], 1)
    else:
        dev = np.zeros((0, 4))
    wx, wP, want = fr.feature_association(dev, last, pc.SCAN_POSE, list(x0), P0.tolist(), len(pairs))
    assert rep["n_pairs"] == len(pairs)
    same(st, wx, wP, rep, want)
    assert np.array_equal([rep["scan_pose"][k] for k in ("x", "y", "ang")], pc.SCAN_POSE)
