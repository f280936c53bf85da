"""Device FeatureAssociation (csrc/k_fa.hip) against the restatement (tests/fa_restatement.py): the fusion kernel on hand-made lists,
single frames of build_case, the replay of the data/ log through lsd_localize, and the batched loop of lsd_enqueue_localize_device."""
import os

import numpy as np
import pytest

import fa_restatement as fr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def spd(seed=5):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(9, 9))
    return A @ A.T + 9 * np.eye(9)


def same(st, x, P, rep=None, want=None):
    assert np.array_equal(st["x"], np.array(x), equal_nan=True), (st["x"][:3], x[:3])
    assert np.array_equal(st["P"].reshape(9, 9, order="F"), np.array(P), equal_nan=True)
    if rep is not None:
        assert (int(rep["branch"]), int(rep["n_kept"]), int(rep["llt"])) == (want["branch"], want["n_kept"], want["llt"])
        est = np.array([rep["estimate"]["x"], rep["estimate"]["y"], rep["estimate"]["ang"], rep["score"]])
        assert np.array_equal(est, np.array(list(want["estimate"]) + [want["score"]]), equal_nan=True)


def fuse_case(ctx, lsdmod, cands, last, sp, x, P):
    st, rep = ctx.debug_fa_fuse(np.array(cands, np.float64).reshape(-1, 4), last, sp, (x, P))
    wx, wP, want = fr.feature_association(cands, last, sp, list(x), np.array(P).tolist())
    same(st, wx, wP, rep, want)
    return rep


CASES = {
    "reset": ([(1.0, 2.0, 3.0, 3.0), (1.0, 2.0, 3.0, INF)], (10.0, 10.0, 0.0)),
    "empty": ([], (10.0, 10.0, 0.0)),
    "first": ([(1.0, 1.0, 1.0, 2.5), (7.0, 8.0, 9.0, 0.5), (3.0, 3.0, 3.0, 0.5)], (-1.0, -1.0, 0.0)),
    "ties": ([(5.0, 0.0, 10.0, 2.0), (1e16, 3.0, 1.0, 1.0), (7.0, 0.0, 2.0, 3.0), (1.0, 5.0, 3.0, 1.0), (-1e16, 1.0, 4.0, 1.0)], (5.0, 5.0, 0.0)),
    "score0": ([(2.0, 2.0, 1.0, 0.0), (3.0, 2.0, 1.0, 1.0)], (3.0, 3.0, 0.0)),
    "wrap": ([(100.0, 200.0, 179.0, 1.0), (101.0, 199.0, -179.0, 1.0)], (3.0, 3.0, 0.0)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fuse_branches(name, ctx, lsdmod):
    cands, last = CASES[name]
    rep = fuse_case(ctx, lsdmod, cands, last, (1.5, -2.25, 0.75), np.linspace(-3, 5, 9), spd())
    assert rep["branch"] == {"reset": 0, "empty": 0, "first": 1}.get(name, 2)


def test_fuse_not_positive_definite(ctx, lsdmod):
    P = spd(3)
    P[4, :] *= 1e-9; P[:, 4] *= 1e-9; P[4, 4] = -1.0
    rep = fuse_case(ctx, lsdmod, [(10.0, 20.0, 30.0, 1.25), (11.0, 19.0, 29.0, 2.0)], (3.0, 3.0, 0.0), (0.5, 0.5, 0.5), np.arange(9.0), P)
    assert rep["llt"] == 4


def test_fuse_global_sort_path(ctx, lsdmod):
    """About 750 kept candidates with many tied scores: the default bound sorts them in LDS, bounds 7 and 0 in global memory;
    the three results are identical and equal the restatement."""
    rng = np.random.default_rng(9)
    n = 1000
    c = np.stack([rng.normal(300, 5, n), rng.normal(200, 5, n), rng.normal(0, 20, n), rng.choice([0.5, 1.0, 1.5, 2.5, 3.5], n)], 1)
    assert 500 < (c[:, 3] < 3).sum() < 1024
    got = []
    try:
        for bound in (1024, 7, 0):
            ctx.debug_set_tuning("FA_LDS", bound)
            st, rep = ctx.debug_fa_fuse(c, (300.0, 200.0, 0.0), (1.0, 2.0, 3.0), (np.arange(9.0), spd()))
            got.append((st.copy(), rep.copy()))
    finally:
        ctx.debug_set_tuning("FA_LDS", 1024)
    wx, wP, want = fr.feature_association(c.tolist(), (300.0, 200.0, 0.0), (1.0, 2.0, 3.0), list(np.arange(9.0)), spd().tolist())
    for st, rep in got:
        same(st, wx, wP, rep, want)
        assert st.tobytes() == got[0][0].tobytes() and rep.tobytes() == got[0][1].tobytes()


def test_nan_state_resets_the_next_frame(maps, maps_meta, lsdmod, ctx, oracle):
    """A kept score of 0 makes the state NaN; the next frame's lastPose is NaN, no candidate passes the distance test, and the
    frame resets (the score-0 quirk end to end on the device)."""
    st0, rep0 = ctx.debug_fa_fuse([(2.0, 2.0, 1.0, 0.0), (3.0, 2.0, 1.0, 1.0)], (3.0, 3.0, 0.0), (0.0, 0.0, 0.0), (np.arange(9.0), spd()))
    assert rep0["branch"] == fr.UKF and np.isnan(st0["x"][:3]).all()
    from matching_case import build_case
    case = build_case(maps["aisle1"], maps_meta["aisle1"]["res"], oracle, theta_deg=17.0)
    last = tuple(float(v) for v in st0["x"][:3])
    st, rep = ctx.feature_association(case["map_cache"], case["map_lines"], case["scan_lines"], case["pts"], case["lidar"], last, (0.0, 0.0, 0.0), st0)
    rx, rP = fr.reset_state()
    assert rep["branch"] == fr.RESET and rep["n_pairs"] > 20 and rep["n_kept"] == 0
    same(st, rx, rP)


@pytest.mark.parametrize("theta,last", [(17.0, (-1.0, -1.0, 0.0)), (0.0, "near"), (-63.0, "near"), (90.0, (5000.0, 5000.0, 0.0)), (17.0, "near")])
def test_feature_association_frames(theta, last, maps, maps_meta, lsdmod, ctx, oracle):
    from matching_case import build_case
    case = build_case(maps["aisle1"], maps_meta["aisle1"]["res"], oracle, theta_deg=theta)
    if last == "near":
        last = (case["lidar_map"][0] + 3.0, case["lidar_map"][1] - 2.0, theta)
    pairs = np.array(fr.pairs(case["map_lines"]["len"], case["scan_lines"]["len"]), np.int32).reshape(-1, 2)
    assert np.array_equal(pairs, lsdmod.match_pairs(case["map_lines"], case["scan_lines"]))
    x0, P0 = np.linspace(-2, 2, 9) + np.array([300, 260, theta, 0, 0, 0, 0, 0, 0]), spd(4)
    sp = (1.25, -0.5, 0.75)
    st, rep = ctx.feature_association(case["map_cache"], case["map_lines"], case["scan_lines"], case["pts"], case["lidar"], last, sp, (x0, P0))
    args = (case["map_cache"], case["map_lines"], case["scan_lines"], case["pts"], case["lidar"], last, pairs)
    dev = ctx.scan_to_map_match(*args).reshape(-1)
    dev = np.stack([dev["x"], dev["y"], dev["ang"], dev["score"]], 1)
    wx, wP, want = fr.feature_association(dev, last, sp, list(x0), P0.tolist(), len(pairs))
    same(st, wx, wP, rep, want)
    assert rep["n_pairs"] == len(pairs)
    cr = oracle.scan_to_map_match(*args, _lib=oracle.lib_cr()).reshape(-1, 4)
    cx, cP, crep = fr.feature_association(cr, last, sp, list(x0), P0.tolist(), len(pairs))
    same(st, cx, cP)
    gl = oracle.scan_to_map_match(*args).reshape(-1, 4)
    gx, gP, grep_ = fr.feature_association(gl, last, sp, list(x0), P0.tolist(), len(pairs))
    assert grep_["n_kept"] == rep["n_kept"] and grep_["branch"] == rep["branch"]
    kd, kg = np.array(fr.keep_sorted(dev)).reshape(-1, 4), np.array(fr.keep_sorted(gl)).reshape(-1, 4)
    assert np.allclose(kd, kg, rtol=0, atol=1e-9)           # the same kept set: poses and scores, in the same sorted order
    assert np.allclose(st["x"], gx, rtol=1e-9, atol=0, equal_nan=True)
    if theta == 0.0:
        assert rep["branch"] == fr.UKF


def data_log(lsdmod, name="data"):
    m, mp, lid, odom = fr.load_log(name)
    scans, lens = lsdmod.lidar_frames(lid)
    return m, mp, scans, lens, odom


def device_inputs(lsdmod, ctx, m, mp):
    mc = ctx.map_cache(m.copy(), float(mp[2]), lsdmod.z_occ_max_dis)
    ml = lsdmod.myLineSegmentDetector(m.copy(), m.shape[1], m.shape[0], 0.3, 0.6, 22.5, 0.7, 1024, ctx=ctx).linesInfo
    return mc, ml


@pytest.mark.parametrize("name", fr.LOGS)
def test_replay_log(name, lsdmod, ctx):
    m, mp, scans, lens, odom = data_log(lsdmod, name)
    states, reps = lsdmod.replay_log(m, mp, fr.load_log(name)[2], odom, ctx=ctx)
    assert len(states) == fr.LOG_FRAMES[name]
    mc, ml = device_inputs(lsdmod, ctx, m, mp)
    fs = ctx.feature_scan_batch(scans, lens, mp, pts_cap=8192)
    loop = fr.Loop(odom, mp[2])
    for t in range(len(scans)):
        sp, lp, last = loop.scan_pose(t), loop.lidar_pose(fs[t]["lidarPos"]), loop.last_pose()
        sl = fs[t]["linesInfo"]
        pr = np.array(fr.pairs(ml["len"], sl["len"]), np.int32).reshape(-1, 2)
        if len(pr):
            d = ctx.scan_to_map_match(mc, ml, sl, fs[t]["scanImPoint"], lp, last, pr).reshape(-1)
            d = np.stack([d["x"], d["y"], d["ang"], d["score"]], 1)
        else:
            d = np.zeros((0, 4))
        x, P, want = fr.feature_association(d, last, sp, loop.x, loop.P, len(pr))
        loop.finish(t, x, P)
        same(states[t], x, P, reps[t], want)
        assert reps[t]["n_pairs"] == len(pr)
        assert np.array_equal([reps[t]["scan_pose"][k] for k in ("x", "y", "ang")], sp)
    assert (reps["branch"] == fr.UKF).sum() > len(reps) // 2


def test_enqueue_localize_batched_equals_alone(lsdmod, ctx):
    import torch
    m, mp, scans, lens, odom = data_log(lsdmod)
    mc, ml = device_inputs(lsdmod, ctx, m, mp)
    S, pitch, pts_cap = 16, 40, 8192
    starts = [(7 * s) % 55 for s in range(S)]
    nfr = [pitch - (s % 5) * 6 for s in range(S)]
    sc = np.zeros((S, pitch, 360, 2)); ln = np.zeros((S, pitch), np.int32); od = np.zeros((S, pitch + 1, 3))
    for s in range(S):
        a = starts[s]
        sc[s, :nfr[s]] = scans[a:a + nfr[s]]; ln[s, :nfr[s]] = lens[a:a + nfr[s]]
        od[s, :nfr[s] + 1] = odom[a:a + nfr[s] + 1]
        od[s, 0, 0] = 0.0                                  # the driver's Odom[0].x = 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_sc, d_ln, d_od, d_mc = dev(sc.reshape(S * pitch, 360, 2)), dev(ln.reshape(-1)), dev(od), dev(mc)
    d_ml = dev(np.ascontiguousarray(ml).view(np.uint8))
    n = S * pitch
    d_lines = torch.zeros(n * 360 * 80, dtype=torch.uint8, device="cuda")
    d_nl, d_np = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    d_pts = torch.zeros(n * pts_cap * 3, dtype=torch.float64, device="cuda")
    d_lp, d_sz = torch.zeros(n * 2, dtype=torch.float64, device="cuda"), torch.zeros(n * 2, dtype=torch.int32, device="cuda")
    init = np.zeros(S, lsdmod.FA_STATE_DTYPE)
    init[:] = lsdmod.Context.fa_initial_state()
    d_init = dev(init.view(np.uint8))
    d_states = torch.zeros(n * 720, dtype=torch.uint8, device="cuda"); d_reps = torch.zeros(n * 72, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    mpar = lsdmod.lsd_map_param(int(mp[0]), int(mp[1]), float(mp[2]), float(mp[3]), float(mp[4]))
    ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, d_sc.data_ptr(), d_ln.data_ptr(), n, 360, mpar, 3, 0.08, 0.5, d_lines.data_ptr(),
                                                         d_nl.data_ptr(), d_pts.data_ptr(), pts_cap, d_np.data_ptr(), d_lp.data_ptr(), d_sz.data_ptr(), stream))
    ctx.enqueue_localize_device(d_mc.data_ptr(), mc.shape[1], mc.shape[0], d_ml.data_ptr(), len(ml), S, pitch, nfr, d_lines.data_ptr(),
                                d_nl.data_ptr(), d_pts.data_ptr(), pts_cap, d_np.data_ptr(), d_lp.data_ptr(), d_od.data_ptr(), float(mp[2]),
                                d_init.data_ptr(), d_states.data_ptr(), d_reps.data_ptr(), stream)
    torch.cuda.synchronize()
    states = d_states.cpu().numpy().view(lsdmod.FA_STATE_DTYPE).reshape(S, pitch)
    reps = d_reps.cpu().numpy().view(lsdmod.FA_REPORT_DTYPE).reshape(S, pitch)
    for s in range(S):
        a = starts[s]
        alone, arep = ctx.localize(mc, ml, scans[a:a + nfr[s]], lens[a:a + nfr[s]], od[s, :nfr[s] + 1], mp)
        assert np.array_equal(states[s, :nfr[s]]["x"], alone["x"], equal_nan=True), s
        assert np.array_equal(states[s, :nfr[s]]["P"], alone["P"], equal_nan=True), s
        assert np.array_equal(reps[s, :nfr[s]]["branch"], arep["branch"]) and np.array_equal(reps[s, :nfr[s]]["n_kept"], arep["n_kept"])
        assert not states[s, nfr[s]:]["x"].any()          # slots past a sequence's end are not written
