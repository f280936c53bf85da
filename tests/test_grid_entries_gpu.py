"""What the four scan-taking device entries of the grid stack (csrc/lsd_grid.hip: lsd_enqueue_grid_integrate_device, _match_device,
_match_mr_device, _response_device) refuse about their shared leading arguments -- the scans, the lengths, the poses and their pitch, the
frame and the range -- is ONE rule: every such argument is refused by every entry with LSD_ERR_INVALID before anything is enqueued, so
that no byte of an output or behind it changes.  One valid call per entry at the same shape equals the restatements of
tests/grid_*_cases.py byte for byte, so the refusals are not the harness's.  Every bad call is refused on the host: nothing here launches
a kernel with a bad argument."""
import math

import numpy as np
import pytest

import grid_cases as gc
import grid_match_cases as gm
import grid_match_mr_cases as mr
import grid_response_cases as gr

pytestmark = pytest.mark.gpu

GUARD = 256                                    # bytes behind every output
FILL = 0x5A
COLS = ROWS = 8
RESOL, RANGE_MAX, BLOCK = 0.05, 3.0, 2
ENTRIES = ("integrate", "match", "match_mr", "response")
OUTPUTS = dict(pa=4 * COLS * ROWS, hi=4 * COLS * ROWS, rec=56, stats=16, resp=192, vol=4 * 3 * 3)      # bytes of one scan's


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


@pytest.fixture(scope="module")
def setup(oracle):
    """The case -- one scan of 4 beams at a stride of 4 on an 8 x 8 grid --, its restatements, computed once, and its inputs on the device."""
    pose = (3.0, 4.0, 0.0)
    corr = gm.random_plane(np.random.default_rng(5), COLS, ROWS, 0.6)
    case = gm.match_case("entries", corr, RESOL, RANGE_MAX, [gm.beams_at_cells(pose, [(6, 4), (3, 7), (1, 4), (5, 6)], RESOL)], [pose], gm.search(1, 1))
    case = gr.rcase("entries", mr.with_block(case, BLOCK), gr.params(1, 1, 0))
    assert case["scans"].shape == (1, 4, 2) and case["lens"].tolist() == [4]
    start = np.full((ROWS, COLS), 0x5A5A5A5A, np.uint32)                  # the planes' fill: the integration adds to it
    want = dict(zip(("pa", "hi"), gc.run_case(case, pass_counts=start, hit_counts=start)[:2]))
    want["rec"] = gm.run_match_case(case)[0]
    want["mr_rec"], want["stats"] = mr.run_mr_case(case)[:2]
    want["resp"], want["vol"] = gr.run_case(case)[:2]
    assert want["rec"].tobytes() == want["mr_rec"].tobytes() == case["records"].tobytes()
    assert {k: want[k].nbytes for k in OUTPUTS} == OUTPUTS
    held = dict(sc=dev(case["scans"]), ln=dev(case["lens"]), po=dev(case["poses"]), co=dev(case["corr"]), cs=dev(mr.coarse_plane(case["corr"], BLOCK)),
                re=dev(case["records"].view(np.uint8)))
    return case, want, held


def outputs():
    """Every output of the four entries, the planes included: CUDA uint8 tensors of the fill pattern, GUARD bytes longer than the output."""
    import torch
    return {k: torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for k, n in OUTPUTS.items()}


def untouched(out):
    return all(bool((t.cpu().numpy() == FILL).all()) for t in out.values())


def enqueue(lsdmod, cx, entry, case, held, out, **bad):
    """The entry on the case, with the leading arguments in `bad` replaced; the status."""
    a = dict(sc=held["sc"].data_ptr(), ln=held["ln"].data_ptr(), n=1, stride=4, po=held["po"].data_ptr(), pitch=24, cols=COLS, rows=ROWS, resol=RESOL,
             range_max=RANGE_MAX)
    a.update(bad)
    lead = (cx.h, a["sc"], a["ln"], a["n"], a["stride"], a["po"], a["pitch"])
    mp, co = lsdmod.lsd_map_param(a["cols"], a["rows"], a["resol"], 0.0, 0.0), held["co"].data_ptr()
    se, rp = lsdmod.grid_search(case["search"]), lsdmod.grid_response(case["response"])
    o = {k: t.data_ptr() for k, t in out.items()}
    if entry == "integrate":
        return cx.L.lsd_enqueue_grid_integrate_device(*lead, mp, a["range_max"], o["pa"], o["hi"], stream())
    if entry == "match":
        return cx.L.lsd_enqueue_grid_match_device(*lead, mp, a["range_max"], co, se, o["rec"], stream())
    if entry == "match_mr":
        return cx.L.lsd_enqueue_grid_match_mr_device(*lead, mp, a["range_max"], co, held["cs"].data_ptr(), BLOCK, se, o["rec"], o["stats"], stream())
    return cx.L.lsd_enqueue_grid_response_device(*lead, held["re"].data_ptr(), mp, a["range_max"], co, case["search"]["ang_step"], rp, o["resp"],
                                                 o["vol"], stream())


# the shared bad arguments: what replaces the valid ones, given the device tensors and the context's scan capacity
BAD = {
    "n_scans=-1": lambda held, cap: dict(n=-1),
    "stride=0": lambda held, cap: dict(stride=0),
    "stride=capacity+1": lambda held, cap: dict(stride=cap + 1),
    "cols=0": lambda held, cap: dict(cols=0),
    "cols=65536": lambda held, cap: dict(cols=65536),
    "resol=0": lambda held, cap: dict(resol=0.0),
    "resol=nan": lambda held, cap: dict(resol=math.nan),
    "range_max=nan": lambda held, cap: dict(range_max=math.nan),
    "range_max=32767*resol": lambda held, cap: dict(range_max=32767 * RESOL),
    "pose_pitch=16": lambda held, cap: dict(pitch=16),
    "pose_pitch=28": lambda held, cap: dict(pitch=28),
    "d_scans+8": lambda held, cap: dict(sc=held["sc"].data_ptr() + 8),
    "d_poses+4": lambda held, cap: dict(po=held["po"].data_ptr() + 4),
    "d_scans=null": lambda held, cap: dict(sc=None),
    "d_lens=null": lambda held, cap: dict(ln=None),
    "d_poses=null": lambda held, cap: dict(po=None),
}


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("entry", ENTRIES)
def test_shared_argument_is_refused_by_every_entry(lsdmod, ctx, setup, entry, bad):
    import torch
    case, _, held = setup
    out = outputs()
    st = enqueue(lsdmod, ctx, entry, case, held, out, **BAD[bad](held, ctx.scan_capacity))
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_ERR_INVALID
    assert untouched(out)


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_call_equals_the_restatement(lsdmod, ctx, setup, entry):
    import torch
    case, want, held = setup
    out = outputs()
    st = enqueue(lsdmod, ctx, entry, case, held, out)
    torch.cuda.synchronize()
    assert st == lsdmod.LSD_OK
    written = {"integrate": dict(pa="pa", hi="hi"), "match": dict(rec="rec"), "match_mr": dict(rec="mr_rec", stats="stats"),
               "response": dict(resp="resp", vol="vol")}[entry]
    for k, t in out.items():
        got, n = t.cpu().numpy(), OUTPUTS[k]
        assert (got[n:] == FILL).all(), k
        if k in written:
            assert got[:n].tobytes() == want[written[k]].tobytes(), k
        else:
            assert (got[:n] == FILL).all(), k
