"""What the localisation part of the C ABI (csrc/lsd_loc.hip: scan-to-map matching, FeatureScan and the ingest entries, the carry operations,
the six replay-loop entries) refuses, entry by entry: every bad call changes ONE argument of a valid one, is refused on the host with the
status named here -- LSD_ERR_INVALID unless marked -- before anything is enqueued, so that no byte of an output or behind it changes; nothing
here launches a kernel with a bad argument.  One valid call per group at the same shape returns LSD_OK, writes its outputs and leaves the
bytes behind them alone (byte parity of valid calls is the other suites' job).  Everything goes through ctx.L: the test does not care which
file an entry lives in, and every status in it is what the entries returned before they moved."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0x5A                        # bytes behind every output, and what fills both
COLS = ROWS = 8
RESOL, ORI = 0.5, -2.0                         # the lidar at (0, 0) m is at pixel (4, 4)
STRIDE = BEAMS = 4
PTS_CAP = 16
OUTPUTS = dict(states=720, reports=72, carry=768,                                       # the loop's (the resume entries update the carry)
               lines=360 * 80, nl=4, pts=PTS_CAP * 24, npt=4, lp=16, sz=8,              # FeatureScan's
               scans=STRIDE * 16, lens=4, match=4 * 32,                                 # the ingest's, the match's (four scores of one pair)
               crep=48, so=STRIDE * 16, lo=4, pick=4, n_lost=8, srep=48)                # carry-correct's, lost-gather's, seed's


@pytest.fixture(scope="module")
def ctx(lsdmod):
    c = lsdmod.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + off


def a_carry(lsdmod, pose=None):
    cy = np.array([lsdmod.Context.fa_carry_init()])
    if pose is not None:
        cy["state"]["x"][0, :3] = pose
    return cy.view(np.uint8).copy()


@pytest.fixture(scope="module")
def held(lsdmod):
    """The inputs of every call, on the device: an 8 x 8 map cache, one map line, one scan of 4 beams at a stride of 4, one frame of one
    sequence (one scan line, four marked pixels), and the one-record arrays of the carry operations."""
    line = np.zeros(360, lsdmod.LINE_DTYPE)
    line[0] = (0.0, 6.0, 1.0, 0.0, 2.0, 6.0, 6.0, 6.0, 4.0, 0, 0)
    pts = np.zeros((PTS_CAP, 3))
    pts[:4, 0], pts[:4, 1] = (2, 3, 5, 6), 6
    scan = np.array([[[1.0, -0.3], [1.0, -0.1], [1.0, 0.1], [1.0, 0.3]]])
    h = dict(mc=dev(np.full((ROWS, COLS), 0.25)), ml=dev(line[:1].view(np.uint8)), nmap=dev(np.ones(1, np.int32)), map_of=dev(np.zeros(1, np.int32)),
             sc=dev(scan), ln=dev(np.full(1, BEAMS, np.int32)), ranges=dev(scan[:, :, 0].astype(np.float32)),
             ami=dev(np.array([[-0.3, 0.2]], np.float32)), li=dev(line.view(np.uint8)), nl=dev(np.ones(1, np.int32)), pt=dev(pts),
             npt=dev(np.full(1, 4, np.int32)), lp=dev(np.array([4.0, 4.0])), od=dev(np.zeros((2, 3))),
             init=dev(np.array([lsdmod.Context.fa_initial_state()]).view(np.uint8)), pairs=dev(np.zeros(2, np.int32)), key=dev(np.zeros(2, np.int32)),
             poses=dev(np.zeros(3)), no_pose=dev(np.array([-1.0, -1.0, 0.0])), resp=dev(np.zeros(192, np.uint8)), pk=dev(np.zeros(1, np.int32)),
             loc=dev(np.zeros(64, np.uint8)))
    h["tab"] = lsdmod.map_table([lsdmod.map_ref(ptr(h["mc"]), COLS, ROWS, ptr(h["ml"]), 1, (COLS, ROWS, RESOL, ORI, ORI))])
    return h


def outputs(**first):
    """Every output of every entry: CUDA uint8 tensors of the fill pattern, GUARD bytes longer than the output; `first`: what a valid call
    needs at the head of an output it reads as well (a carry)."""
    import torch
    out = {k: torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for k, n in OUTPUTS.items()}
    for k, v in first.items():
        out[k][:len(v)] = torch.from_numpy(v).cuda()
    return out


def untouched(out):
    import torch
    torch.cuda.synchronize()
    return all(bool((t.cpu().numpy() == FILL).all()) for t in out.values())


def wrote(out, *keys):
    """After a valid call: each of `keys` has changed, no other output has, and no byte behind any output has."""
    import torch
    torch.cuda.synchronize()
    for k, t in out.items():
        got, n = t.cpu().numpy(), OUTPUTS[k]
        assert (got[n:] == FILL).all(), "guard of " + k
        assert bool((got[:n] != FILL).any()) == (k in keys), k
    return True


def table(held, n_maps=1, **field):
    tab = held["tab"].copy()
    for k, v in field.items():
        tab[k][0] = v
    return dict(maps=tab, n_maps=n_maps)


# what the table entries (the loops' and FeatureScan's) add; UNSUPPORTED where marked
TABLE_BAD = {
    "maps=null": lambda h: dict(maps=None),
    "n_maps=0": lambda h: dict(n_maps=0),
    "n_maps=65": lambda h: dict(n_maps=65, status="UNSUPPORTED"),
    "d_map_of=null": lambda h: dict(map_of=None),
    "row cols=0": lambda h: table(h, cols=0),
    "row d_map_cache=null": lambda h: table(h, d_map_cache=0),
    "row mapResol=0": lambda h: table(h, mapResol=0.0),
}


def expect(lsdmod, bad):
    return getattr(lsdmod, "LSD_ERR_" + bad.pop("status", "INVALID"))


# --- the six loop entries ---------------------------------------------------------------------------------------------------------------
LOOPS = ("localize", "resume", "live_map", "resume_live_map", "maps", "resume_maps")


def loop_call(lsdmod, cx, entry, held, out, **bad):
    resume, kind = entry.startswith("resume"), entry.replace("resume_", "").replace("resume", "localize")
    a = dict(mc=ptr(held["mc"]), cols=COLS, rows=ROWS, ml=ptr(held["ml"]), n_map=1, d_n_map=ptr(held["nmap"]), maps=held["tab"], n_maps=1,
             map_of=ptr(held["map_of"]), n_seq=1, pitch=1, nf=[1], li=ptr(held["li"]), nl=ptr(held["nl"]), pt=ptr(held["pt"]), pts_cap=PTS_CAP,
             npt=ptr(held["npt"]), lp=ptr(held["lp"]), od=ptr(held["od"]), resol=RESOL, start=ptr(out["carry"]) if resume else ptr(held["init"]),
             st=ptr(out["states"]), rp=ptr(out["reports"]))
    a.update(bad)
    nf = None if a["nf"] is None else np.ascontiguousarray(a["nf"], np.int32)
    frames = (a["n_seq"], a["pitch"], None if nf is None else nf.ctypes.data, a["li"], a["nl"], a["pt"], a["pts_cap"], a["npt"], a["lp"], a["od"])
    tail = (a["start"], a["st"], a["rp"], stream())
    fn = getattr(cx.L, "lsd_enqueue_localize_%sdevice" % {"localize": "resume_" if resume else "", "live_map": "resume_live_map_" if resume else "live_map_",
                                                          "maps": "resume_maps_" if resume else "maps_"}[kind])
    if kind == "maps":
        return fn(cx.h, None if a["maps"] is None else a["maps"].ctypes.data, a["n_maps"], a["map_of"], *frames, *tail)
    one = (cx.h, a["mc"], a["cols"], a["rows"], a["ml"], a["n_map"]) + ((a["d_n_map"],) if kind == "live_map" else ())
    return fn(*one, *frames, a["resol"], *tail)


FRAMES_BAD = {
    "n_seq=0": lambda h: dict(n_seq=0),
    "frames_pitch=0": lambda h: dict(pitch=0),
    "n_frames=null": lambda h: dict(nf=None),
    "n_frames[0]=-1": lambda h: dict(nf=[-1]),
    "n_frames[0]=2": lambda h: dict(nf=[2]),
    "d_lines=null": lambda h: dict(li=None),
    "d_n_lines=null": lambda h: dict(nl=None),
    "d_n_pts=null": lambda h: dict(npt=None),
    "d_lidar_pos=null": lambda h: dict(lp=None),
    "d_odom=null": lambda h: dict(od=None),
    "d_states=null": lambda h: dict(st=None),
    "d_reports=null": lambda h: dict(rp=None),
    "pts_cap=-1": lambda h: dict(pts_cap=-1),
    "pts_cap=16, d_pts=null": lambda h: dict(pt=None),
    "d_init or d_carry=null": lambda h: dict(start=None),
}
ONE_MAP_BAD = {
    "d_map_cache=null": lambda h: dict(mc=None),
    "cols=0": lambda h: dict(cols=0),
    "n_map=-1": lambda h: dict(n_map=-1),
    "n_map=1, d_map_lines=null": lambda h: dict(ml=None),
    "map_resol=0": lambda h: dict(resol=0.0),
    "map_resol=nan": lambda h: dict(resol=math.nan),
    "n_map=186414": lambda h: dict(n_map=186414, status="UNSUPPORTED"),      # x 360 > 2^26: refused before any workspace is sized
}
LIVE_MAP_BAD = {
    "d_n_map=null": lambda h: dict(d_n_map=None),
    "map_lines_cap=0": lambda h: dict(n_map=0),
}
LOOP_BAD = [(e, "frames", k) for e in LOOPS for k in FRAMES_BAD] + [(e, "one_map", k) for e in LOOPS[:4] for k in ONE_MAP_BAD] + \
           [(e, "live_map", k) for e in LOOPS[2:4] for k in LIVE_MAP_BAD] + [(e, "table", k) for e in LOOPS[4:] for k in TABLE_BAD]
RULES = dict(frames=FRAMES_BAD, one_map=ONE_MAP_BAD, live_map=LIVE_MAP_BAD, table=TABLE_BAD)


@pytest.mark.parametrize("entry,rule,bad", LOOP_BAD, ids=["%s-%s" % (e, k) for e, _, k in LOOP_BAD])
def test_loop_entry_refuses(lsdmod, ctx, held, entry, rule, bad):
    out, b = outputs(), RULES[rule][bad](held)
    want = expect(lsdmod, b)
    assert loop_call(lsdmod, ctx, entry, held, out, **b) == want
    assert untouched(out)


@pytest.mark.parametrize("entry", LOOPS)
def test_loop_entry_valid(lsdmod, ctx, held, entry):
    out = outputs(carry=a_carry(lsdmod))
    before = out["carry"].cpu().numpy().tobytes()
    assert loop_call(lsdmod, ctx, entry, held, out) == lsdmod.LSD_OK
    assert wrote(out, "states", "reports", "carry")
    assert (out["carry"].cpu().numpy().tobytes() != before) == entry.startswith("resume")


# --- the two FeatureScan enqueue entries --------------------------------------------------------------------------------------------------
def scan_call(lsdmod, cx, entry, held, out, **bad):
    a = dict(sc=ptr(held["sc"]), ln=ptr(held["ln"]), n=1, stride=STRIDE, resol=RESOL, maps=held["tab"], n_maps=1, map_of=ptr(held["map_of"]), sps=1,
             li=ptr(out["lines"]), nl=ptr(out["nl"]), pt=ptr(out["pts"]), pts_cap=PTS_CAP, npt=ptr(out["npt"]), lp=ptr(out["lp"]), sz=ptr(out["sz"]))
    a.update(bad)
    outs = (3, 0.08, 0.5, a["li"], a["nl"], a["pt"], a["pts_cap"], a["npt"], a["lp"], a["sz"], stream())
    if entry == "maps":
        return cx.L.lsd_enqueue_feature_scan_maps_device(cx.h, a["sc"], a["ln"], a["n"], a["stride"], None if a["maps"] is None else a["maps"].ctypes.data,
                                                         a["n_maps"], a["map_of"], a["sps"], *outs)
    return cx.L.lsd_enqueue_feature_scan_batch_device(cx.h, a["sc"], a["ln"], a["n"], a["stride"], lsdmod.lsd_map_param(COLS, ROWS, a["resol"], ORI, ORI),
                                                      *outs)


SCAN_BAD = dict({"%s=null" % k: (lambda h, k=k: {k: None}) for k in ("sc", "ln", "li", "nl", "pt", "npt", "lp", "sz")}, **{
    "n_scans=0": lambda h: dict(n=0),
    "stride=0": lambda h: dict(stride=0),
    "pts_cap=-1": lambda h: dict(pts_cap=-1),
    "stride=capacity+1": lambda h: dict(stride=h["cap"] + 1, status="UNSUPPORTED"),
})
SCAN_MAP_BAD = {"mapResol=0": lambda h: dict(resol=0.0), "mapResol=nan": lambda h: dict(resol=math.nan)}
SCAN_TABLE_BAD = dict(TABLE_BAD, **{"scans_per_seq=0": lambda h: dict(sps=0)})
SCAN_CASES = [(e, k) for e in ("batch", "maps") for k in SCAN_BAD] + [("batch", k) for k in SCAN_MAP_BAD] + [("maps", k) for k in SCAN_TABLE_BAD]


@pytest.mark.parametrize("entry,bad", SCAN_CASES, ids=["%s-%s" % c for c in SCAN_CASES])
def test_feature_scan_entry_refuses(lsdmod, ctx, held, entry, bad):
    out, b = outputs(), dict(SCAN_BAD, **SCAN_MAP_BAD, **SCAN_TABLE_BAD)[bad](dict(held, cap=ctx.scan_capacity))
    want = expect(lsdmod, b)
    assert scan_call(lsdmod, ctx, entry, held, out, **b) == want
    assert untouched(out)


@pytest.mark.parametrize("entry", ("batch", "maps"))
def test_feature_scan_entry_valid(lsdmod, ctx, held, entry):
    out = outputs()
    assert scan_call(lsdmod, ctx, entry, held, out) == lsdmod.LSD_OK
    n_lines, n_pts = (int(out[k].cpu().numpy()[:4].view(np.int32)[0]) for k in ("nl", "npt"))
    assert 0 <= n_lines <= 360 and 0 <= n_pts <= PTS_CAP
    assert wrote(out, "nl", "npt", "lp", "sz", *(["lines"] if n_lines else []), *(["pts"] if n_pts else []))


# --- the two ingest entries ---------------------------------------------------------------------------------------------------------------
def ingest_call(lsdmod, cx, entry, held, out, **bad):
    a = dict(raw=ptr(held["sc"]), ranges=ptr(held["ranges"]), ami=ptr(held["ami"]), n=1, beams=BEAMS, sc=ptr(out["scans"]), ln=ptr(out["lens"]),
             stride=STRIDE)
    a.update(bad)
    rest = (a["n"], a["beams"], None, a["sc"], a["ln"], a["stride"], stream())
    if entry == "raw":
        return cx.L.lsd_enqueue_scan_ingest_device(cx.h, a["raw"], *rest)
    return cx.L.lsd_enqueue_laserscan_ingest_device(cx.h, a["ranges"], a["ami"], *rest)


INGEST_BAD = {
    "n_beams=5": lambda h, o: dict(beams=5),
    "d_scans+8": lambda h, o: dict(sc=ptr(o["scans"], 8)),
    "d_scans=null": lambda h, o: dict(sc=None),
    "d_lens=null": lambda h, o: dict(ln=None),
    "stride=capacity+1": lambda h, o: dict(stride=h["cap"] + 1, status="UNSUPPORTED"),
}
RAW_BAD = {"d_raw+8": lambda h, o: dict(raw=ptr(h["sc"], 8)), "d_raw=null": lambda h, o: dict(raw=None)}
LASER_BAD = {"d_ranges=null": lambda h, o: dict(ranges=None), "d_angle_min_inc=null": lambda h, o: dict(ami=None)}
INGEST_CASES = [(e, k) for e in ("raw", "laser") for k in INGEST_BAD] + [("raw", k) for k in RAW_BAD] + [("laser", k) for k in LASER_BAD]


@pytest.mark.parametrize("entry,bad", INGEST_CASES, ids=["%s-%s" % c for c in INGEST_CASES])
def test_ingest_entry_refuses(lsdmod, ctx, held, entry, bad):
    out = outputs()
    b = dict(INGEST_BAD, **RAW_BAD, **LASER_BAD)[bad](dict(held, cap=ctx.scan_capacity), out)
    want = expect(lsdmod, b)
    assert ingest_call(lsdmod, ctx, entry, held, out, **b) == want
    assert untouched(out)


@pytest.mark.parametrize("entry", ("raw", "laser"))
def test_ingest_entry_valid(lsdmod, ctx, held, entry):
    out = outputs()
    assert ingest_call(lsdmod, ctx, entry, held, out) == lsdmod.LSD_OK
    assert wrote(out, "scans", "lens")


# --- scan-to-map matching -----------------------------------------------------------------------------------------------------------------
def match_call(lsdmod, cx, held, out, **bad):
    a = dict(mc=ptr(held["mc"]), cols=COLS, ml=ptr(held["ml"]), sl=ptr(held["li"]), pt=ptr(held["pt"]), n_points=4, pairs=ptr(held["pairs"]), n_pairs=1,
             d_out=ptr(out["match"]))
    a.update(bad)
    pos = lsdmod.lsd_position
    return cx.L.lsd_enqueue_scan_to_map_match_device(cx.h, a["mc"], a["cols"], ROWS, a["ml"], a["sl"], a["pt"], a["n_points"], pos(4.0, 4.0, 0.0),
                                                     pos(4.0, 4.0, 0.0), a["pairs"], a["n_pairs"], 1.0, 60.0, a["d_out"], stream())


MATCH_BAD = dict({"%s=null" % k: (lambda k=k: {k: None}) for k in ("mc", "ml", "sl", "pairs", "d_out")}, **{
    "cols=0": lambda: dict(cols=0),
    "n_pairs=0": lambda: dict(n_pairs=0),
    "n_points=-1": lambda: dict(n_points=-1),
    "n_points=1, d_pts=null": lambda: dict(n_points=1, pt=None),
    "n_pairs=2^28+1": lambda: dict(n_pairs=(1 << 28) + 1, status="UNSUPPORTED"),
})


@pytest.mark.parametrize("bad", list(MATCH_BAD))
def test_match_entry_refuses(lsdmod, ctx, held, bad):
    out, b = outputs(), MATCH_BAD[bad]()
    want = expect(lsdmod, b)
    assert match_call(lsdmod, ctx, held, out, **b) == want
    assert untouched(out)


def test_match_entry_valid(lsdmod, ctx, held):
    out = outputs()
    assert match_call(lsdmod, ctx, held, out) == lsdmod.LSD_OK
    assert wrote(out, "match")


# --- the carry operations -----------------------------------------------------------------------------------------------------------------
def rebase_call(lsdmod, cx, out, carry=True, n_seq=1, frm=(RESOL, ORI, ORI), to=(RESOL / 2, ORI, ORI)):
    return cx.L.lsd_enqueue_fa_carry_rebase_device(cx.h, ptr(out["carry"]) if carry else None, n_seq, None, 0, lsdmod.lsd_map_frame(*frm),
                                                   lsdmod.lsd_map_frame(*to), stream())


REBASE_BAD = dict({"%s mapResol=%r" % (w, v): (lambda w=w, v=v: {w: (v, ORI, ORI)}) for w in ("frm", "to") for v in (0.0, math.inf, math.nan)},
                  **{"carry=null": lambda: dict(carry=False), "n_seq=0": lambda: dict(n_seq=0)})


@pytest.mark.parametrize("bad", list(REBASE_BAD))
def test_rebase_refuses(lsdmod, ctx, bad):
    out = outputs()
    assert rebase_call(lsdmod, ctx, out, **REBASE_BAD[bad]()) == lsdmod.LSD_ERR_INVALID
    assert untouched(out)


def test_rebase_valid_and_between_identical_frames(lsdmod, ctx):
    import torch
    cy = a_carry(lsdmod, pose=(3.0, 4.0, 10.0))
    out = outputs(carry=cy)
    assert rebase_call(lsdmod, ctx, out, to=(RESOL, ORI, ORI)) == lsdmod.LSD_OK            # the same frame: no launch
    torch.cuda.synchronize()
    assert out["carry"].cpu().numpy()[:768].tobytes() == cy.tobytes()
    assert rebase_call(lsdmod, ctx, out) == lsdmod.LSD_OK
    assert wrote(out, "carry")
    assert out["carry"].cpu().numpy()[:768].tobytes() != cy.tobytes()


def correct_call(lsdmod, cx, held, out, par=(1.0, 1.0, 1.0, 0.0), s=None, **bad):
    a = dict(cy=ptr(out["carry"]), pitch=1, pp=24, key=None)
    a.update(bad)
    return cx.L.lsd_enqueue_fa_carry_correct_device(cx.h, a["cy"], 1, a["pitch"], ptr(held["poses"]), a["pp"], ptr(held["resp"]), a["key"], 0,
                                                    lsdmod.lsd_fa_correct(*par), ptr(out["crep"]), stream() if s is None else s)


def one_of_four(i, v):
    return tuple(v if k == i else 1.0 for k in range(4))


CORRECT_BAD = dict({"%s=%r" % (n, v): (lambda h, o, i=i, v=v: dict(par=one_of_four(i, v)))
                    for i, n in enumerate(("cov_scale", "floor_xy", "floor_ang", "gate")) for v in (-1.0, math.nan)}, **{
    "pose_pitch=16": lambda h, o: dict(pp=16),
    "pose_pitch=28": lambda h, o: dict(pp=28),
    "frames_pitch=0": lambda h, o: dict(pitch=0),
    "frames_pitch=4097": lambda h, o: dict(pitch=4097),
    "d_carry+4": lambda h, o: dict(cy=ptr(o["carry"], 4)),
    "d_key+2": lambda h, o: dict(key=ptr(h["key"], 2)),
})


@pytest.mark.parametrize("bad", list(CORRECT_BAD))
def test_carry_correct_refuses(lsdmod, ctx, held, bad):
    out = outputs()
    assert correct_call(lsdmod, ctx, held, out, **CORRECT_BAD[bad](held, out)) == lsdmod.LSD_ERR_INVALID
    assert untouched(out)


def test_carry_correct_valid(lsdmod, ctx, held):
    out = outputs(carry=a_carry(lsdmod))
    assert correct_call(lsdmod, ctx, held, out) == lsdmod.LSD_OK
    assert wrote(out, "carry", "crep")


def lost_call(lsdmod, cx, held, out, max_lost=1):
    return cx.L.lsd_enqueue_fa_lost_gather_device(cx.h, ptr(out["carry"]), 1, 1, ptr(held["no_pose"]), 24, ptr(held["sc"]), ptr(held["ln"]), STRIDE, None,
                                                  0, max_lost, ptr(out["so"]), ptr(out["lo"]), ptr(out["pick"]), ptr(out["n_lost"]), stream())


def seed_call(lsdmod, cx, held, out, n_pick=1):
    return cx.L.lsd_enqueue_fa_carry_seed_device(cx.h, ptr(out["carry"]), 1, 1, ptr(held["pk"]), n_pick, ptr(held["loc"]), None, lsdmod.fa_seed(),
                                                 ptr(out["srep"]), stream())


def test_lost_gather_and_seed_refuse(lsdmod, ctx, held):
    """(tests/fa_relocate_host.cpp walks every clause of their rules: one refusal each here)"""
    out = outputs()
    assert lost_call(lsdmod, ctx, held, out, max_lost=0) == lsdmod.LSD_ERR_INVALID
    assert seed_call(lsdmod, ctx, held, out, n_pick=0) == lsdmod.LSD_ERR_INVALID
    assert untouched(out)


def test_lost_gather_and_seed_valid(lsdmod, ctx, held):
    out = outputs(carry=a_carry(lsdmod))                                    # (no pose, and the slot's pose is the carry's: the sequence is lost)
    assert lost_call(lsdmod, ctx, held, out) == lsdmod.LSD_OK
    assert wrote(out, "carry", "so", "lo", "pick", "n_lost")
    assert out["n_lost"].cpu().numpy()[:8].view(np.int32).tolist() == [1, 1]
    assert seed_call(lsdmod, ctx, held, out) == lsdmod.LSD_OK               # (the locate record is not an accepted one: a report, no seed)
    assert wrote(out, "carry", "so", "lo", "pick", "n_lost", "srep")


# --- a host convenience whose device entry refuses after the uploads are queued ---------------------------------------------------------------
def host_scan(lsdmod, cx, stride, resol):
    sc = np.zeros((1, stride, 2))
    sc[0, :BEAMS] = [[1.0, -0.3], [1.0, -0.1], [1.0, 0.1], [1.0, 0.3]]
    ln = np.full(1, BEAMS, np.int32)
    o = dict(lines=np.full(360 * 80, FILL, np.uint8), nl=np.full(4, FILL, np.uint8), pts=np.full(PTS_CAP * 24, FILL, np.uint8),
             npt=np.full(4, FILL, np.uint8), lp=np.full(16, FILL, np.uint8), sz=np.full(8, FILL, np.uint8))
    st = cx.L.lsd_feature_scan_batch(cx.h, sc.ctypes.data, ln.ctypes.data, 1, stride, lsdmod.lsd_map_param(COLS, ROWS, resol, ORI, ORI), 3, 0.08, 0.5,
                                     *(o[k].ctypes.data for k in ("lines", "nl", "pts")), PTS_CAP, *(o[k].ctypes.data for k in ("npt", "lp", "sz")))
    return st, o


@pytest.mark.parametrize("bad,status", [("mapResol=0", "INVALID"), ("stride=capacity+1", "UNSUPPORTED")])
def test_host_feature_scan_refused_by_its_device_entry(lsdmod, ctx, bad, status):
    st, o = host_scan(lsdmod, ctx, STRIDE if bad == "mapResol=0" else ctx.scan_capacity + 1, 0.0 if bad == "mapResol=0" else RESOL)
    assert st == getattr(lsdmod, "LSD_ERR_" + status)
    assert all((v == FILL).all() for v in o.values())
    st, o = host_scan(lsdmod, ctx, STRIDE, RESOL)                         # the context is as good as before
    assert st == lsdmod.LSD_OK
    assert all((o[k] != FILL).any() for k in ("nl", "npt", "lp", "sz"))


# --- lsd_synchronize waits for the stream of the last enqueue, whichever entry it was ---------------------------------------------------------
def test_synchronize_follows_a_carry_correct(lsdmod, ctx, held):
    """lsd_synchronize "blocks until the stream used by the last enqueue is idle": an ingest on one stream, then a carry-correct on another,
    busy one; once lsd_synchronize has returned, an event recorded behind the carry-correct has happened.  Before the localisation entries
    ended in enqueue_on, the four carry operations did not move the context's last stream and this assertion -- the only one of this file --
    failed: lsd_synchronize waited for the ingest's idle stream."""
    import torch
    a = torch.randn(4096, 4096, device="cuda")
    (a @ a).sum().item()                                                    # (the first product's set-up is not part of the load below)
    first, second, ev = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
    out = outputs(carry=a_carry(lsdmod))
    torch.cuda.synchronize()
    with torch.cuda.stream(first):
        assert ingest_call(lsdmod, ctx, "raw", held, out) == lsdmod.LSD_OK
    first.synchronize()
    with torch.cuda.stream(second):
        for _ in range(40):                                                 # tens of milliseconds in front of the carry-correct
            a = (a @ a) * 1e-3
        assert correct_call(lsdmod, ctx, held, out, s=second.cuda_stream) == lsdmod.LSD_OK
        ev.record(second)
    assert ctx.L.lsd_synchronize(ctx.h) == lsdmod.LSD_OK
    done = ev.query()
    torch.cuda.synchronize()
    assert done
