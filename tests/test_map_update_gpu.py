"""The map callback on the device (lsd_enqueue_map_update_device), FeatureAssociation on a map whose line count lives on the device
(lsd_enqueue_localize_live_map_device, lsd_enqueue_localize_resume_live_map_device) and the Localizer's stream-ordered hand-over between
its two map slots (Localizer.set_map_device).  Every comparison is byte equality: the new path runs the same kernels on the same bytes."""
import math
import time

import numpy as np
import pytest

import fa_restatement as fr
from test_localize_resume_gpu import PTS_CAP, REPORT_B, STATE_B, get_log

pytestmark = pytest.mark.gpu
FRAMES = 20


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_of(m):
    """The OccupancyGrid whose callback output is the map m: 0 -> unknown (-1), 255 -> free (0), 1 -> occupied (100)."""
    return np.where(m == 0, -1, np.where(m == 255, 0, 100)).astype(np.int8)


_host = {}


def host_callback(lsdmod, ctx, maps, maps_meta, name):
    """The host mapCallback of a map fixture, once per module: (grid int8 [rows, cols], mapValue, mapCache, structLSD)."""
    if name not in _host:
        g = grid_of(maps[name])
        rows, cols = g.shape
        _host[name] = (g,) + tuple(lsdmod.mapCallback(g.reshape(-1), cols, rows, maps_meta[name]["res"], ctx=ctx))
    return _host[name]


class Outputs:
    """The outputs of one map update, pre-filled with 0xFF so that an unwritten byte shows."""

    def __init__(self, rows, cols, max_lines=512):
        import torch
        ff = lambda count: torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda")
        self.rows, self.cols, self.max_lines = rows, cols, max_lines
        self.map, self.mc, self.lines, self.count, self.line_im = ff(rows * cols), ff(rows * cols * 8), ff(max_lines * 80), ff(4), ff(rows * cols)

    def untouched(self):
        return all((t.cpu().numpy() == 0xFF).all() for t in (self.map, self.mc, self.lines, self.count, self.line_im))

    def check(self, lsdmod, want):
        _, mapValue, mapCache, LSD = want
        n = int(self.count.cpu().numpy().view(np.int32)[0])
        assert n == LSD.len_linesInfo and 0 < n <= self.max_lines
        assert np.array_equal(self.map.cpu().numpy().reshape(self.rows, self.cols), mapValue)
        assert self.mc.cpu().numpy().view(np.float64).tobytes() == mapCache.tobytes()
        assert np.array_equal(self.line_im.cpu().numpy().reshape(self.rows, self.cols), LSD.lineIm)
        rec = self.lines.cpu().numpy().view(lsdmod.LINE_DTYPE)
        got, ref = rec[:n].copy(), LSD.linesInfo.copy()
        got["_pad"] = 0; ref["_pad"] = 0                                        # (tail padding of structLinesInfo: not part of the record)
        assert got.tobytes() == ref.tobytes()
        assert (rec[n:].view(np.uint8) == 0xFF).all()                           # nothing past the count is written


def enqueue_update(lsdmod, ctx, d_grid, out, res):
    import torch
    ctx.enqueue_map_update_device(d_grid.data_ptr(), out.cols, out.rows, res, 2.0, out.map.data_ptr(), out.mc.data_ptr(), out.lines.data_ptr(),
                                  out.max_lines, out.count.data_ptr(), out.line_im.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)


# ---- 1. the callback as one enqueue ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["map1", "f3key"])
def test_map_update_equals_the_host_callback(lsdmod, ctx, maps, maps_meta, name):
    import torch
    want = host_callback(lsdmod, ctx, maps, maps_meta, name)
    rows, cols = want[0].shape
    ctx.reserve_map_update(cols, rows)
    out = Outputs(rows, cols)
    enqueue_update(lsdmod, ctx, dev(want[0]), out, maps_meta[name]["res"])
    torch.cuda.synchronize()
    out.check(lsdmod, want)


def test_two_updates_back_to_back(lsdmod, ctx, maps, maps_meta):
    """Two different grids on one stream with no synchronisation between them: the second leaves the first one's outputs alone."""
    import torch
    names = ("f3key", "map1")
    wants = [host_callback(lsdmod, ctx, maps, maps_meta, n) for n in names]
    outs = [Outputs(*w[0].shape) for w in wants]
    grids = [dev(w[0]) for w in wants]
    torch.cuda.synchronize()
    for name, g, o in zip(names, grids, outs):
        enqueue_update(lsdmod, ctx, g, o, maps_meta[name]["res"])
    torch.cuda.synchronize()
    for w, o in zip(wants, outs):
        o.check(lsdmod, w)


def test_map_callback_device(lsdmod, ctx, maps, maps_meta):
    import torch
    want = host_callback(lsdmod, ctx, maps, maps_meta, "map1")
    rows, cols = want[0].shape
    m, mc, lines, count, line_im = lsdmod.mapCallback_device(dev(want[0]).reshape(-1), cols, rows, maps_meta["map1"]["res"], ctx=ctx, max_lines=64)
    torch.cuda.synchronize()
    assert m.shape == (rows, cols) and mc.shape == (rows, cols) and line_im.shape == (rows, cols) and count.dtype == torch.int32
    n = int(count.cpu()[0])
    assert n == want[3].len_linesInfo == 7
    assert np.array_equal(m.cpu().numpy(), want[1]) and mc.cpu().numpy().tobytes() == want[2].tobytes()
    assert np.array_equal(line_im.cpu().numpy(), want[3].lineIm)
    got, ref = lines.cpu().numpy().reshape(-1).view(lsdmod.LINE_DTYPE)[:n].copy(), want[3].linesInfo.copy()
    got["_pad"] = 0; ref["_pad"] = 0
    assert got.tobytes() == ref.tobytes()


# ---- 2. the count on the device -------------------------------------------------------------------------------------------------------------
class Replay:
    """The data log's first 20 frames through the two one-call entries and the two resumable ones, into 0xFF-filled outputs."""

    def __init__(self, lsdmod, ctx):
        self.lsdmod, self.ctx, self.log = lsdmod, ctx, get_log(lsdmod, ctx, "data")
        self.init = dev(np.array([lsdmod.Context.fa_initial_state()]).view(np.uint8).copy())

    def run(self, n_map=None, cap=None, count=None, resume=False, raw=False, **over):
        """n_map: the entries that take the count from the host; cap + count: the live-map ones, *d_n_map = count."""
        import torch
        lg, cx, L = self.log, self.ctx, self.ctx.L
        d_st = torch.full((FRAMES * STATE_B,), 0xFF, dtype=torch.uint8, device="cuda")
        d_rp = torch.full((FRAMES * REPORT_B,), 0xFF, dtype=torch.uint8, device="cuda")
        d_cnt = None if count is None else dev(np.array([count], np.int32))
        carry = dev(np.array([self.lsdmod.Context.fa_carry_init(odom0=lg.odom[0])]).view(np.uint8).copy())
        nf = np.array([FRAMES], np.int32)
        head = [cx.h, lg.d_mc.data_ptr(), lg.mc.shape[1], lg.mc.shape[0], lg.d_ml.data_ptr()]
        head += [n_map] if cap is None else [cap, over.get("d_n_map", d_cnt.data_ptr())]
        tail = [1, FRAMES, nf.ctypes.data, lg.d_lines.data_ptr(), lg.d_nl.data_ptr(), lg.d_pts.data_ptr(), PTS_CAP, lg.d_np.data_ptr(), lg.d_lp.data_ptr(),
                lg.d_od.data_ptr() + (24 if resume else 0), float(lg.mp[2]), carry.data_ptr() if resume else self.init.data_ptr(), d_st.data_ptr(),
                d_rp.data_ptr(), torch.cuda.current_stream().cuda_stream]
        fn = {(False, False): L.lsd_enqueue_localize_device, (False, True): L.lsd_enqueue_localize_live_map_device,
              (True, False): L.lsd_enqueue_localize_resume_device, (True, True): L.lsd_enqueue_localize_resume_live_map_device}[resume, cap is not None]
        st = fn(*(head + tail))
        torch.cuda.synchronize()
        out = d_st.cpu().numpy().tobytes(), d_rp.cpu().numpy().tobytes(), carry.cpu().numpy().tobytes()
        return (st,) + out if raw else cx._chk(st) or out


@pytest.fixture(scope="module")
def replay(lsdmod, ctx):
    return Replay(lsdmod, ctx)


def test_count_on_the_device(lsdmod, replay):
    n = len(replay.log.ml)
    assert n == 41
    for resume in (False, True):
        before = replay.run(n_map=n, resume=resume)
        want = replay.log.states[:FRAMES].tobytes(), replay.log.reports[:FRAMES].tobytes()      # the one-call replay of the whole log
        assert before[:2] == want
        assert replay.run(cap=512, count=n, resume=resume) == before
        first16 = replay.run(n_map=16, resume=resume)
        assert first16 != before                                                                   # (the case can tell 16 lines from 41)
        assert replay.run(cap=16, count=n, resume=resume) == first16
        none = replay.run(n_map=0, resume=resume)
        assert none != first16
        assert replay.run(cap=512, count=0, resume=resume) == none
        assert replay.run(cap=512, count=-1, resume=resume) == none
        assert replay.run(n_map=n, resume=resume) == before                                        # the old entry, afterwards: the bytes it gave before


# ---- 3. - 6. the Localizer --------------------------------------------------------------------------------------------------------------------
class Case:
    """The data log's first 20 frames on the device, the grids and host callbacks of the maps, and the reference runs the tests share."""

    def __init__(self, lsdmod, ctx, maps, maps_meta):
        self.lsdmod, self.ctx = lsdmod, ctx
        _, self.mp, lid, odom = fr.load_log("data")
        self.lid, self.odom = lid[:FRAMES], odom[:FRAMES + 1]
        self.d_lid, self.d_od = dev(self.lid), dev(self.odom)
        self.host = {n: host_callback(lsdmod, ctx, maps, maps_meta, n) for n in ("mapValue", "f3key", "map1")}
        self.d_grid = {n: dev(h[0]) for n, h in self.host.items()}
        self.param = {"mapValue": tuple(float(v) for v in self.mp), "f3key": tuple(float(v) for v in fr.load_log("f3key")[1]),
                      "map1": (608.0, 480.0, maps_meta["map1"]["res"], -3.0, -2.0)}
        self._plain = None

    def grid_args(self, name):
        p = self.param[name]
        return self.d_grid[name], int(p[0]), int(p[1]), p[2], p[3], p[4]

    def empty_localizer(self, S=1, odom0=None):
        """A Localizer on a map of nothing: whatever it localises against afterwards, a test has put there."""
        return self.lsdmod.Localizer(np.ones((4, 4)), np.zeros(0, self.lsdmod.LINE_DTYPE), self.mp, S, odom0=self.odom[0] if odom0 is None else odom0,
                                     ctx=self.ctx)

    def host_localizer(self, name, S=1, odom0=None, n_lines=None):
        _, _, mc, LSD = self.host[name]
        return self.lsdmod.Localizer(mc, LSD.linesInfo[:n_lines], self.param[name], S, odom0=self.odom[0] if odom0 is None else odom0, ctx=self.ctx)

    def host_swaps(self, swaps):
        """Frame by frame through step(), with host set_map of swaps[t] before frame t: (states, reports, carries)."""
        loc = self.host_localizer("mapValue")
        st, rp = [], []
        for t in range(FRAMES):
            if t in swaps:
                _, _, mc, LSD = self.host[swaps[t]]
                loc.set_map(mc, LSD.linesInfo, self.param[swaps[t]])
            s, r = loc.step(self.lid[None, t:t + 1], self.odom[None, t + 1:t + 2])
            st.append(s[0]); rp.append(r[0])
        return np.concatenate(st).tobytes(), np.concatenate(rp).tobytes(), loc.carries.tobytes()

    def plain(self):
        """No swap at all, on the map from_occupancy_grid makes (once per module)."""
        if self._plain is None:
            g = self.host["mapValue"][0]
            p = self.param["mapValue"]
            loc = self.lsdmod.Localizer.from_occupancy_grid(g.reshape(-1), g.shape[1], g.shape[0], p[2], p[3], p[4], 1, odom0=self.odom[0], ctx=self.ctx)
            st, rp = [], []
            for t in range(FRAMES):
                s, r = loc.step(self.lid[None, t:t + 1], self.odom[None, t + 1:t + 2])
                st.append(s[0]); rp.append(r[0])
            self._plain = np.concatenate(st).tobytes(), np.concatenate(rp).tobytes(), loc.carries.tobytes()
        return self._plain

    def device_run(self, loc, swaps, side=None, frames=range(FRAMES)):
        """Frame by frame through step_device with set_map_device of swaps[t] (on `side`, or the current stream) before frame t and no
        synchronisation anywhere; the tick's outputs are copied on the stream.  Returns (states, reports, carries) after one final wait."""
        import torch
        outs = []
        for t in frames:
            if t in swaps:
                loc.set_map_device(*self.grid_args(swaps[t]), stream=side)
            o = loc.step_device(self.d_lid[None, t:t + 1], self.d_od[None, t + 1:t + 2])
            outs.append((o[0].clone(), o[1].clone()))
        torch.cuda.synchronize()
        return (b"".join(o[0].cpu().numpy().tobytes() for o in outs), b"".join(o[1].cpu().numpy().tobytes() for o in outs), loc.carries.tobytes())


@pytest.fixture(scope="module")
def case(lsdmod, ctx, maps, maps_meta):
    return Case(lsdmod, ctx, maps, maps_meta)


def test_localizer_on_a_device_built_map(lsdmod, case):
    import torch
    loc = case.empty_localizer()
    loc.set_map_device(*case.grid_args("mapValue"))
    st, rp = [], []
    for t in range(FRAMES):
        s, r = loc.step(case.lid[None, t:t + 1], case.odom[None, t + 1:t + 2])
        st.append(s[0]); rp.append(r[0])
    assert (np.concatenate(st).tobytes(), np.concatenate(rp).tobytes(), loc.carries.tobytes()) == case.plain()
    assert loc.map_counts.is_cuda and loc.map_counts.dtype == torch.int32 and int(loc.map_counts.cpu()[0]) == 41
    assert loc.map_param == case.param["mapValue"]


def test_localizer_ragged_robots_on_a_device_built_map(lsdmod, case):
    """3 robots that start on different ticks at different frames of the log, one frame per tick."""
    S, T = 3, FRAMES
    first_tick, starts = [0, 2, 5], [0, 7, 3]
    od0 = np.stack([case.odom[s] for s in starts]); od0[:, 0] = 0.0
    g, p = case.host["mapValue"][0], case.param["mapValue"]
    ref = lsdmod.Localizer.from_occupancy_grid(g.reshape(-1), g.shape[1], g.shape[0], p[2], p[3], p[4], S, odom0=od0, ctx=case.ctx)
    loc = case.empty_localizer(S, od0)
    loc.set_map_device(*case.grid_args("mapValue"))
    for tick in range(T):
        lid = np.zeros((S, 1, 360, 2)); od = np.zeros((S, 1, 3)); nf = np.zeros(S, np.int32)
        for s in range(S):
            t = tick - first_tick[s]
            if 0 <= t and starts[s] + t < FRAMES:
                lid[s, 0] = case.lid[starts[s] + t]; od[s, 0] = case.odom[starts[s] + t + 1]; nf[s] = 1
        a, b = ref.step(lid, od, nf), loc.step(lid, od, nf)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert ref.carries.tobytes() == loc.carries.tobytes() and (loc.carries["frames"] > 0).all()


def test_hand_over_of_the_same_map(lsdmod, case):
    import torch
    side = torch.cuda.Stream()
    loc = case.empty_localizer()
    loc.set_map_device(*case.grid_args("mapValue"))
    assert case.device_run(loc, {8: "mapValue"}, side) == case.plain()


def test_hand_over_to_another_map(lsdmod, case):
    import torch
    side = torch.cuda.Stream()
    want = case.host_swaps({8: "f3key"})
    loc = case.empty_localizer()
    loc.set_map_device(*case.grid_args("mapValue"))
    got = case.device_run(loc, {8: "f3key"}, side)
    assert got == want
    assert loc.map_param == case.param["f3key"] and int(loc.map_counts.cpu()[0]) == 47
    plain = case.plain()
    for k, size in ((0, STATE_B), (1, REPORT_B)):
        assert got[k][:8 * size] == plain[k][:8 * size]                        # ticks enqueued before the update kept the old map
        assert got[k][8 * size:] != plain[k][8 * size:]                        # (and the new map is another one)


def test_two_hand_overs_reuse_a_slot(lsdmod, case):
    """A -> B -> A with ticks between and no synchronisation: the second update goes into the slot the first ticks read."""
    import torch
    side = torch.cuda.Stream()
    want = case.host_swaps({6: "f3key", 12: "mapValue"})
    loc = case.empty_localizer()
    loc.set_map_device(*case.grid_args("mapValue"))
    assert case.device_run(loc, {6: "f3key", 12: "mapValue"}, side) == want
    assert int(loc.map_counts.cpu()[0]) == 41


def test_capacity(lsdmod, case):
    import torch
    ref = case.host_localizer("map1", n_lines=4)
    loc = case.empty_localizer()
    loc.reserve_map(608, 480, lines_cap=4)
    loc.set_map_device(*case.grid_args("map1"))
    a = case.device_run(loc, {}, frames=range(3))
    assert int(loc.map_counts.cpu()[0]) == case.host["map1"][3].len_linesInfo == 7
    st, rp = [], []
    for t in range(3):
        s, r = ref.step(case.lid[None, t:t + 1], case.odom[None, t + 1:t + 2])
        st.append(s[0]); rp.append(r[0])
    assert a == (np.concatenate(st).tobytes(), np.concatenate(rp).tobytes(), ref.carries.tobytes())
    with pytest.raises(lsdmod.LsdError) as e:
        loc.step(case.lid[None, 3:4], case.odom[None, 4:5])
    s, r = ref.step(case.lid[None, 3:4], case.odom[None, 4:5])
    assert e.value.status == lsdmod.LSD_ERR_CAPACITY
    assert e.value.partial[0].tobytes() == s.tobytes() and e.value.partial[1].tobytes() == r.tobytes()


def test_update_and_tick_do_not_synchronise(lsdmod, case):
    import torch
    p = case.param["mapValue"]
    loc = case.empty_localizer()
    loc.reserve_map(int(p[0]), int(p[1]))
    loc.set_map_device(*case.grid_args("mapValue"))                            # warm
    torch.cuda.synchronize()
    a = torch.randn(4096, 4096, device="cuda")

    def burn(count):
        for _ in range(count):
            a @ a
    burn(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    burn(10)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 10                                      # the trial run: seconds per matmul
    count = max(10, min(5000, int(math.ceil(0.08 / per))))                     # ~80 ms of work in front
    done = torch.cuda.Event()
    burn(count)
    done.record()
    if done.query():
        pytest.skip("the stream drained before set_map_device was called (%d matmuls of %.3f ms): the host was too slow to tell" % (count, per * 1e3))
    loc.set_map_device(*case.grid_args("mapValue"))
    o = loc.step_device(case.d_lid[None, 0:1], case.d_od[None, 1:2])
    still_running = not done.query()
    first = o[0].clone(), o[1].clone()
    assert still_running, "set_map_device + step_device returned only after the work in front of them had finished: one of them synchronised"
    rest = case.device_run(loc, {}, frames=range(1, FRAMES))
    got = (first[0].cpu().numpy().tobytes() + rest[0], first[1].cpu().numpy().tobytes() + rest[1], rest[2])
    assert got == case.plain()


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors(lsdmod, ctx, case, replay):
    import torch
    L, INV, UNS = ctx.L, lsdmod.LSD_ERR_INVALID, lsdmod.LSD_ERR_UNSUPPORTED
    g = case.d_grid["map1"]
    out = Outputs(480, 608)
    par = lsdmod.make_params()
    import ctypes as C

    def call(h=ctx.h, grid=g.data_ptr(), cols=608, rows=480, res=0.05, z=2.0, p=C.byref(par), m=out.map.data_ptr(), mc=out.mc.data_ptr(),
             lines=out.lines.data_ptr(), max_lines=512, count=out.count.data_ptr(), li=out.line_im.data_ptr()):
        return L.lsd_enqueue_map_update_device(h, grid, cols, rows, res, z, p, m, mc, lines, max_lines, count, li, None)
    for null in ("h", "grid", "p", "m", "mc", "lines", "count"):
        assert call(**{null: None}) == INV, null
    assert call(grid=g.data_ptr() + 8) == INV and call(m=out.map.data_ptr() + 8) == INV      # the cells move in 16-byte accesses
    assert call(cols=0) == INV and call(rows=-1) == INV and call(max_lines=0) == INV and call(res=0.0) == INV and call(z=-1.0) == INV
    assert call(cols=65536, rows=32768) == UNS                                   # cols * rows = 2^31
    assert L.lsd_reserve_map_update(ctx.h, 65536, 32768) == UNS and L.lsd_reserve_map_update(ctx.h, 0, 480) == INV
    assert L.lsd_reserve_map_update(None, 608, 480) == INV
    torch.cuda.synchronize()
    assert out.untouched()                                                       # nothing ran
    for resume in (False, True):
        for kw, want in ((dict(cap=0, count=41), INV), (dict(cap=-1, count=41), INV), (dict(cap=(1 << 26) // 360 + 1, count=41), UNS),
                         (dict(cap=512, count=41, d_n_map=None), INV)):
            st, states, reports, carry = replay.run(resume=resume, raw=True, **kw)
            assert st == want, kw
            assert set(states) == {0xFF} and set(reports) == {0xFF}              # nothing ran
    # the Python entries: a grid of the wrong size, dtype or device
    loc = case.host_localizer("mapValue")
    before = loc.map_param, loc.map_counts.data_ptr()
    _, cols, rows, res, ox, oy = case.grid_args("map1")
    bad = (g.reshape(-1)[:-1], g.to(torch.uint8), g.cpu(), g.reshape(-1).reshape(608, 480), case.host["map1"][0])
    for d_grid in bad:
        with pytest.raises(lsdmod.LsdError) as e:
            loc.set_map_device(d_grid, cols, rows, res, ox, oy)
        assert e.value.status == INV
        with pytest.raises(lsdmod.LsdError) as e:
            lsdmod.mapCallback_device(d_grid, cols, rows, res, ctx=ctx)
        assert e.value.status == INV
    with pytest.raises(lsdmod.LsdError):
        loc.set_map_device(g, cols, rows, res, ox, oy, stream=0)                 # (a raw handle is not a torch stream)
    with pytest.raises(lsdmod.LsdError) as e:
        loc.set_map_device(g.reshape(-1)[8:8 + cols * (rows - 1)], cols, rows - 1, res, ox, oy)   # the C side's alignment rule
    assert e.value.status == INV
    assert (loc.map_param, loc.map_counts.data_ptr()) == before                  # the Localizer kept its map
    with pytest.raises(lsdmod.LsdError):
        loc.reserve_map(608, 480, lines_cap=0)
    with pytest.raises(lsdmod.LsdError) as e:
        loc.reserve_map(608, 480, lines_cap=(1 << 26) // 360 + 1)
    assert e.value.status == UNS
