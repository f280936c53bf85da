"""k_rdp (myrdp::FeatureScan) and the scan-to-map matching kernel against the oracle's correctly rounded build, bit for bit, over
the campaign of tests/scan_cases.py (tests/test_feature_scan_cpu.py shows on the CPU what that campaign reaches).

Bit for bit means: n_lines, n_pts, every stored line record with dx, dy and the zeroed padding, the pixel list, lidar_pos and
im_size have the oracle's bit patterns, -0.0 and +0.0 told apart.  The one thing not compared is WHICH NaN a NaN is: IEEE 754
leaves the sign and payload of a generated NaN to the implementation, x86 SSE produces 0xFFF8000000000000 for 0 / 0 and inf - inf
and gfx950 0x7FF8000000000000, so a NaN must be a NaN in the same place (scan_cases.bits); the campaign test prints how many
records that concerns."""
import numpy as np
import pytest

import scan_cases as sc

pytestmark = pytest.mark.gpu
GUARD = 256                                  # bytes of 0xA5 behind every output array


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def campaign():
    return {g["name"]: g for g in sc.campaign()}


def _guarded(n, dtype):
    raw = np.full(n * np.dtype(dtype).itemsize + GUARD, 0xA5, np.uint8)
    return raw, raw[:n * np.dtype(dtype).itemsize].view(dtype)


def _mp(lsdmod, g):
    p = g["map_param"]
    return lsdmod.lsd_map_param(int(p[0]), int(p[1]), float(p[2]), float(p[3]), float(p[4]))


def run_fs(ctx, lsdmod, packed, lens, g, pts_cap=sc.PTS_CAP):
    """lsd_feature_scan_batch through the C ABI into arrays prefilled with 0xA5 and followed by a guard.
    Returns (status, dict of arrays); asserts that every guard is intact."""
    n, stride = packed.shape[:2]
    lens = np.ascontiguousarray(lens, np.int32)
    bufs = dict(lines=_guarded(n * 360, lsdmod.LINE_DTYPE), n_lines=_guarded(n, np.int32), pts=_guarded(n * pts_cap * 3, np.float64),
                n_pts=_guarded(n, np.int32), lidar_pos=_guarded(n * 2, np.float64), im_size=_guarded(n * 2, np.int32))
    a = {k: v[1] for k, v in bufs.items()}
    st = ctx.L.lsd_feature_scan_batch(ctx.h, packed.ctypes.data, lens.ctypes.data, n, stride, _mp(lsdmod, g), g["limit"], g["thre_line"],
                                      g["line_dist"], a["lines"].ctypes.data, a["n_lines"].ctypes.data, a["pts"].ctypes.data, pts_cap,
                                      a["n_pts"].ctypes.data, a["lidar_pos"].ctypes.data, a["im_size"].ctypes.data)
    for k, (raw, _) in bufs.items():
        assert (raw[-GUARD:] == 0xA5).all(), "guard behind %s overwritten" % k
    out = dict(lines=a["lines"].reshape(n, 360), n_lines=a["n_lines"], pts=a["pts"].reshape(n, pts_cap, 3), n_pts=a["n_pts"],
               lidar_pos=a["lidar_pos"].reshape(n, 2), im_size=a["im_size"].reshape(n, 2))
    return st, out


def diffs(out, i, ref, pts_cap=sc.PTS_CAP):
    """What of scan i differs from the oracle's result, as a list of names (empty: bit-equal)."""
    bad = []
    if out["n_lines"][i] != ref["n_lines"]: bad.append("n_lines %d != %d" % (out["n_lines"][i], ref["n_lines"]))
    if out["n_pts"][i] != len(ref["pts"]): bad.append("n_pts %d != %d" % (out["n_pts"][i], len(ref["pts"])))
    bad += sc.line_diffs(out["lines"][i, :len(ref["lines"])], ref["lines"])
    m = min(len(ref["pts"]), pts_cap)
    if not np.array_equal(sc.bits(out["pts"][i, :m]), sc.bits(ref["pts"][:m])): bad.append("pts")
    if not np.array_equal(sc.bits(out["lidar_pos"][i]), sc.bits(np.array(ref["lidar_pos"]))): bad.append("lidar_pos")
    if tuple(out["im_size"][i]) != tuple(ref["im_size"]): bad.append("im_size")
    return bad


@pytest.mark.parametrize("name", [g[0] for g in sc.GROUPS])
def test_campaign_group_equals_the_correctly_rounded_oracle(name, campaign, lsdmod, ctx, oracle):
    """One launch per parameter set, several hundred scans (more workgroups than the device has compute units), stride 1024."""
    g = campaign[name]
    refs = sc.reference(oracle, g, oracle.lib_cr())
    sc.check_bounds(refs)
    packed, lens = sc.pack(g["scans"])
    st, out = run_fs(ctx, lsdmod, packed, lens, g)
    over = any(r["n_lines"] > 360 for r in refs)
    assert st == (lsdmod.LSD_ERR_CAPACITY if over else lsdmod.LSD_OK)
    bad, nan_only = [], 0
    for i, r in enumerate(refs):
        d = diffs(out, i, r)
        if d:
            bad.append((i, g["tags"][i], len(g["scans"][i]), d))
        elif out["lines"][i, :len(r["lines"])].tobytes() != r["lines"].tobytes():
            nan_only += 1
    print("%s: %d scans, %d differ, %d equal but for the sign / payload of a NaN" % (name, len(refs), len(bad), nan_only))
    assert not bad, bad[:10]


def _subset(g, step, offset=0):
    idx = list(range(offset, len(g["scans"]), step))
    return idx, [g["scans"][i] for i in idx]


def test_stale_slots_empty_scans_single_calls_and_permutation(campaign, lsdmod, ctx, oracle):
    """Lengths 1 .. 1024 under one stride with NaN or garbage behind lens[i] and lens[i] = 0 scans in between; the same scans one per
    call at their own stride; the batch permuted."""
    g = campaign["log_fine"]
    idx, scans = _subset(g, 5)
    refs = sc.reference(oracle, g, oracle.lib_cr(), idx)
    rng = np.random.default_rng(5)
    n = len(scans) + len(scans) // 3
    empty = np.zeros(n, bool)
    empty[rng.choice(n, n - len(scans), replace=False)] = True
    packed = np.empty((n, sc.STRIDE, 2))
    packed[0::3] = np.nan; packed[1::3] = 1e300; packed[2::3] = rng.uniform(-7, 7, packed[2::3].shape)
    lens = np.zeros(n, np.int32)
    slot = np.nonzero(~empty)[0]
    for s, j in zip(scans, slot):
        packed[j, :len(s)] = s; lens[j] = len(s)
    st, out = run_fs(ctx, lsdmod, packed, lens, g)
    assert st == (lsdmod.LSD_ERR_CAPACITY if any(r["n_lines"] > 360 for r in refs) else lsdmod.LSD_OK)
    bad = [(k, diffs(out, j, r)) for k, (j, r) in enumerate(zip(slot, refs)) if diffs(out, j, r)]
    assert not bad, bad[:10]
    for j in np.nonzero(empty)[0]:
        assert out["n_lines"][j] == 0 and out["n_pts"][j] == 0 and not out["lidar_pos"][j].any() and not out["im_size"][j].any(), j
    # one per call, at the scan's own length as stride
    for k in range(0, len(scans), 7):
        s = scans[k]
        st1, one = run_fs(ctx, lsdmod, np.ascontiguousarray(s[None]), [len(s)], g)
        j = slot[k]
        assert st1 in (lsdmod.LSD_OK, lsdmod.LSD_ERR_CAPACITY)
        assert one["n_lines"][0] == out["n_lines"][j] and one["n_pts"][0] == out["n_pts"][j]
        nl, npt = min(one["n_lines"][0], 360), one["n_pts"][0]
        assert one["lines"][0, :nl].tobytes() == out["lines"][j, :nl].tobytes() and one["pts"][0, :npt].tobytes() == out["pts"][j, :npt].tobytes()
        assert one["lidar_pos"][0].tobytes() == out["lidar_pos"][j].tobytes() and one["im_size"][0].tobytes() == out["im_size"][j].tobytes()
    # permuted
    perm = rng.permutation(n)
    _, shuf = run_fs(ctx, lsdmod, np.ascontiguousarray(packed[perm]), lens[perm], g)
    for a, j in enumerate(perm):
        nl, npt = min(out["n_lines"][j], 360), out["n_pts"][j]
        assert shuf["n_lines"][a] == out["n_lines"][j] and shuf["n_pts"][a] == npt
        assert shuf["lines"][a, :nl].tobytes() == out["lines"][j, :nl].tobytes() and shuf["pts"][a, :npt].tobytes() == out["pts"][j, :npt].tobytes()
        assert shuf["lidar_pos"][a].tobytes() == out["lidar_pos"][j].tobytes() and shuf["im_size"][a].tobytes() == out["im_size"][j].tobytes()


def run_fs_device(ctx, lsdmod, packed, lens, g, pts_cap=sc.PTS_CAP):
    """lsd_enqueue_feature_scan_batch_device on torch tensors prefilled with 0xA5, a guard behind each: what the kernel itself wrote."""
    import torch
    n, stride = packed.shape[:2]
    d_sc, d_len = torch.from_numpy(packed).cuda(), torch.from_numpy(np.ascontiguousarray(lens, np.int32)).cuda()
    size = dict(lines=n * 360 * 80, n_lines=n * 4, pts=n * pts_cap * 24, n_pts=n * 4, lidar_pos=n * 16, im_size=n * 8)
    d = {k: torch.full((b + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for k, b in size.items()}
    ctx._chk(ctx.L.lsd_enqueue_feature_scan_batch_device(ctx.h, d_sc.data_ptr(), d_len.data_ptr(), n, stride, _mp(lsdmod, g), g["limit"],
                                                         g["thre_line"], g["line_dist"], d["lines"].data_ptr(), d["n_lines"].data_ptr(),
                                                         d["pts"].data_ptr(), pts_cap, d["n_pts"].data_ptr(), d["lidar_pos"].data_ptr(),
                                                         d["im_size"].data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    for k, raw in h.items():
        assert (raw[-GUARD:] == 0xA5).all(), "guard behind %s overwritten" % k
    v = lambda k, t: h[k][:size[k]].view(t)
    return dict(lines=v("lines", lsdmod.LINE_DTYPE).reshape(n, 360), n_lines=v("n_lines", np.int32), pts=v("pts", np.float64).reshape(n, pts_cap, 3),
                n_pts=v("n_pts", np.int32), lidar_pos=v("lidar_pos", np.float64).reshape(n, 2), im_size=v("im_size", np.int32).reshape(n, 2))


def test_pts_cap_truncates_and_nothing_is_written_behind(campaign, lsdmod, ctx, oracle):
    """pts_cap = 64: n_pts reports the full count, the first 64 points are the oracle's, and the kernel writes nothing else: the
    unused rest of each scan's slots and the guards behind every array keep their fill (device entry point); the host entry point
    with the same pts_cap leaves its guards alone and returns the same."""
    g = campaign["res05"]
    idx, scans = _subset(g, 4, 1)
    refs = sc.reference(oracle, g, oracle.lib_cr(), idx)
    assert sum(len(r["pts"]) > sc.PTS_CAP_SMALL for r in refs) > 20
    packed, lens = sc.pack(scans)
    out = run_fs_device(ctx, lsdmod, packed, lens, g, pts_cap=sc.PTS_CAP_SMALL)
    st, host = run_fs(ctx, lsdmod, packed, lens, g, pts_cap=sc.PTS_CAP_SMALL)
    assert st == (lsdmod.LSD_ERR_CAPACITY if any(r["n_lines"] > 360 for r in refs) else lsdmod.LSD_OK)
    for o in (out, host):
        bad = [(i, diffs(o, i, r, sc.PTS_CAP_SMALL)) for i, r in enumerate(refs) if diffs(o, i, r, sc.PTS_CAP_SMALL)]
        assert not bad, bad[:10]
    for i, r in enumerate(refs):
        m = min(len(r["pts"]), sc.PTS_CAP_SMALL)
        assert (out["pts"][i, m:].view(np.uint8) == 0xA5).all(), i            # slots behind the last stored point: untouched
        assert (out["lines"][i, min(r["n_lines"], 360):].view(np.uint8) == 0xA5).all(), i


def test_device_entry_point_equals_the_host_entry_point(campaign, lsdmod, ctx):
    g = campaign["edge_coarse"]
    _, scans = _subset(g, 3)
    packed, lens = sc.pack(scans)
    st, out = run_fs(ctx, lsdmod, packed, lens, g)
    assert st in (lsdmod.LSD_OK, lsdmod.LSD_ERR_CAPACITY)
    dev = run_fs_device(ctx, lsdmod, packed, lens, g)
    assert np.array_equal(dev["n_lines"], out["n_lines"]) and np.array_equal(dev["n_pts"], out["n_pts"]) and out["n_lines"].max() > 3
    assert dev["lidar_pos"].tobytes() == out["lidar_pos"].tobytes() and np.array_equal(dev["im_size"], out["im_size"])
    for i in range(len(scans)):
        nl, npt = min(out["n_lines"][i], 360), out["n_pts"][i]
        assert dev["lines"][i, :nl].tobytes() == out["lines"][i, :nl].tobytes() and dev["pts"][i, :npt].tobytes() == out["pts"][i, :npt].tobytes(), i


def test_stride_and_argument_limits(campaign, lsdmod, ctx):
    g = campaign["log_defaults"]
    s = g["scans"][-1]
    assert len(s) == 1024
    st, _ = run_fs(ctx, lsdmod, np.ascontiguousarray(s[None]), [1024], g)
    assert st == lsdmod.LSD_OK
    wide = np.zeros((1, 1025, 2)); wide[0, :1024] = s
    st, _ = run_fs(ctx, lsdmod, wide, [1024], g)
    assert st == lsdmod.LSD_ERR_UNSUPPORTED
    st, _ = run_fs(ctx, lsdmod, np.ascontiguousarray(s[None, :360]), [361], g)
    assert st == lsdmod.LSD_ERR_INVALID
    for res in (0.0, -0.025):
        st, _ = run_fs(ctx, lsdmod, np.ascontiguousarray(s[None]), [1024], dict(g, map_param=g["map_param"][:2] + (res,) + g["map_param"][3:]))
        assert st == lsdmod.LSD_ERR_INVALID


# ---- scan-to-map matching ------------------------------------------------------------------------------------------------------
def _match_diffs(lsdmod, ctx, oracle, c):
    want = oracle.scan_to_map_match(*sc.case_args(c), _lib=oracle.lib_cr()).reshape(-1, 4)
    got = ctx.scan_to_map_match(*sc.case_args(c)).reshape(-1)
    g = np.stack([got["x"], got["y"], got["ang"], got["score"]], 1)
    ne = sc.bits(g) != sc.bits(want)
    return [(int(r), "x y ang score".split()[int(f)], float(g[r, f]), float(want[r, f])) for r, f in zip(*np.nonzero(ne))]


def test_matching_edge_cases_equal_the_correctly_rounded_oracle(lsdmod, ctx, oracle):
    """Every frame of scan_cases.edge_cases() (their conditions are asserted on the oracle's result in test_feature_scan_cpu.py):
    poses, wrapped angles and scores bit for bit.  The kernel's atand / sind / cosd are correctly rounded, like that oracle build's;
    everything else is +, -, *, /, sqrt and round, so nothing is left to a tolerance."""
    bad = {}
    for c in sc.edge_cases():
        d = _match_diffs(lsdmod, ctx, oracle, c)
        if d:
            bad[c["name"]] = d[:5]
    assert not bad, bad


def test_matching_on_feature_scan_output_equals_the_correctly_rounded_oracle(maps, maps_meta, lsdmod, ctx, oracle):
    """Scan lines with FeatureScan's integer end points (the horizontal and vertical branches of line_direction) against a fixture
    map's lines and mapCache, up to 1000 pairs a frame."""
    cases = sc.feature_scan_match_cases(oracle, maps, maps_meta, oracle.lib_cr())
    assert len(cases) >= 6
    bad = {}
    for c in cases:
        d = _match_diffs(lsdmod, ctx, oracle, c)
        if d:
            bad[c["name"]] = (len(d), d[:5])
    assert not bad, bad
