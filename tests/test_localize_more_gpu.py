"""Six more recorded logs (fa_restatement.MORE_LOGS) on the device: every frame of lsdmod.replay_log against the restatement fed with the
device's own candidates, and all six as ragged sequences of one fleet call on a two-map table, each byte-identical to its own
lsd_localize.  The fixtures only: nothing here reads the reference tree."""
import numpy as np
import pytest

import fa_restatement as fr
from test_localize_gpu import data_log, device_inputs, same

pytestmark = pytest.mark.gpu
PTS_CAP = 8192


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", fr.MORE_LOGS)
def test_replay_more_logs(name, lsdmod, ctx):
    m, mp, scans, lens, odom = data_log(lsdmod, name)
    states, reps = lsdmod.replay_log(m, mp, fr.load_log(name)[2], odom, ctx=ctx)
    assert len(states) == len(scans) == len(odom) - 1
    mc, ml = device_inputs(lsdmod, ctx, m, mp)
    fs = ctx.feature_scan_batch(scans, lens, mp, pts_cap=PTS_CAP)
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


def test_six_ragged_sequences_on_two_maps_in_one_call(lsdmod, ctx):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    keys = sorted(set(fr.LOG_MAPS[n] for n in fr.MORE_LOGS))
    assert len(keys) == 2
    table, maps, keep = [], {}, []
    for key in keys:
        m, mp, _, _ = fr.load_log(key)
        mc, ml = device_inputs(lsdmod, ctx, m, mp)
        d_mc, d_ml = dev(mc), dev(np.ascontiguousarray(ml).view(np.uint8))
        keep += [d_mc, d_ml]
        maps[key] = (mc, ml, mp)
        table.append(lsdmod.map_ref(d_mc.data_ptr(), mc.shape[1], mc.shape[0], d_ml.data_ptr(), len(ml), mp))
    logs = [data_log(lsdmod, n) for n in fr.MORE_LOGS]
    nfr = [len(l[2]) for l in logs]
    S, pitch = len(logs), max(nfr)
    assert len(set(nfr)) > 3 and min(nfr) < pitch - 100      # ragged, and long
    map_of = [keys.index(fr.LOG_MAPS[n]) for n in fr.MORE_LOGS]
    sc = np.zeros((S, pitch, 360, 2)); ln = np.zeros((S, pitch), np.int32); od = np.zeros((S, pitch + 1, 3))
    for s, (_, _, scans, lens, odom) in enumerate(logs):
        sc[s, :nfr[s]], ln[s, :nfr[s]], od[s, :nfr[s] + 1] = scans, lens, odom
    n = S * pitch
    d_sc, d_ln, d_od, d_of = dev(sc.reshape(n, 360, 2)), dev(ln.reshape(-1)), dev(od), dev(np.array(map_of, np.int32))
    d_lines = torch.zeros(n * 360 * 80, dtype=torch.uint8, device="cuda")
    d_nl, d_np = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    d_pts = torch.zeros(n * PTS_CAP * 3, dtype=torch.float64, device="cuda")
    d_lp, d_sz = torch.zeros(n * 2, dtype=torch.float64, device="cuda"), torch.zeros(n * 2, dtype=torch.int32, device="cuda")
    init = np.zeros(S, lsdmod.FA_STATE_DTYPE)
    init[:] = lsdmod.Context.fa_initial_state()
    d_init = dev(init.view(np.uint8))
    d_states = torch.zeros(n * 720, dtype=torch.uint8, device="cuda"); d_reps = torch.zeros(n * 72, dtype=torch.uint8, device="cuda")
    ctx.enqueue_feature_scan_maps_device(d_sc.data_ptr(), d_ln.data_ptr(), n, 360, table, d_of.data_ptr(), pitch, d_lines.data_ptr(),
                                         d_nl.data_ptr(), d_pts.data_ptr(), PTS_CAP, d_np.data_ptr(), d_lp.data_ptr(), d_sz.data_ptr(), stream=stream)
    ctx.enqueue_localize_maps_device(table, d_of.data_ptr(), S, pitch, nfr, d_lines.data_ptr(), d_nl.data_ptr(), d_pts.data_ptr(), PTS_CAP,
                                     d_np.data_ptr(), d_lp.data_ptr(), d_od.data_ptr(), d_init.data_ptr(), d_states.data_ptr(), d_reps.data_ptr(),
                                     stream)
    torch.cuda.synchronize()
    states = d_states.cpu().numpy().view(lsdmod.FA_STATE_DTYPE).reshape(S, pitch)
    reps = d_reps.cpu().numpy().view(lsdmod.FA_REPORT_DTYPE).reshape(S, pitch)
    for s, name in enumerate(fr.MORE_LOGS):
        mc, ml, mp = maps[fr.LOG_MAPS[name]]
        _, _, scans, lens, odom = logs[s]
        alone, arep = ctx.localize(mc, ml, scans, lens, odom, mp)
        assert states[s, :nfr[s]].tobytes() == alone.tobytes(), name
        assert reps[s, :nfr[s]].tobytes() == arep.tobytes(), name
        assert not states[s, nfr[s]:].view(np.uint8).any() and not reps[s, nfr[s]:].view(np.uint8).any()      # slots past a sequence's end are not written
        assert (arep["branch"] == fr.UKF).sum() > nfr[s] // 2
