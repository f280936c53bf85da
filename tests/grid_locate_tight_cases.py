"""The tight global localisation (csrc/k_gridlocate_tight.hip): the rule restated on the helpers of
tests/grid_locate_cases.py, and a small added campaign on grids of at most 61 x 47 cells, levels <= 5, at most 65 headings.

The restatement is the definition.  Like the one it extends it scores EVERY node of every level densely and states the sets G_h as masks
over those arrays, so what the device never visits -- a node that did not fit the list, a level below an overflow -- is still defined here.
The rule (include/lsd_hip.h), with L_H the existing rule's L and G_H its F_H, for h = H .. 1:
  expand   G_(h-1) = the existing children of G_h with U_(h-1) >= L_h; at h = 1 they are the candidates (L_0 = L_1)
  probe    (h - 1 >= 1, PROBE) per heading: the node of G_(h-1) with the largest U, among equals the smallest Q nbx + P, of the whole set;
           from it the greedy descent to a candidate of score S_a; L_(h-1) = max(L_h, max_a S_a)
  retry    (RETRY, |G_(h-1)| > max_nodes) G_(h-1) rebuilt once with U_(h-1) >= L_(h-1); first_count, bit h - 1 of retried; no second probe
  overflow |G_(h-1)| > max_nodes for some h - 1 >= 1 after the retry where there was one, or |G_H| > max_nodes

A case class is a predicate on the restatement's own TRACE, never on what the device gives; max_nodes of a case is chosen from the
restatement's counts, never from a run of the device.
"""
import functools
import math

import numpy as np

import grid_locate_cases as lc
import grid_match_cases as gm

PROBE, RETRY = 1, 2
TIGHTS = (0, 1, 2, 3)
TIGHT_STATS_DTYPE = np.dtype([("top_nodes", "u4"), ("frontier", "u4", (9,)), ("scored", "u4"), ("retried", "u4"), ("bound", "u4", (9,)),
                              ("first_count", "u4", (9,)), ("reserved", "u4", (2,))])
assert TIGHT_STATS_DTYPE.itemsize == 128
UNLIMITED = 1 << 24


# ---- the search ------------------------------------------------------------------------------------------------------------------------
def dense(scan, n, resol, range_max, corr, p):
    """What does not depend on max_nodes, score_floor or `tight`: nb(a), the headings and U of every node of every level
    ([n_ang, nby, nbx] per level), from the helpers of the existing restatement."""
    H, nx, ny, n_ang, x0, y0 = p["levels"], p["nx"], p["ny"], p["n_ang"], p["x0"], p["y0"]
    dims = [((nx + (1 << h) - 1) >> h, (ny + (1 << h) - 1) >> h) for h in range(H + 1)]
    thetas = [p["ang0"] + float(a) * p["ang_step"] for a in range(n_ang)]
    offs = [lc.offsets(scan, int(n), thetas[a], resol, range_max) for a in range(n_ang)]
    nb = [len(o) for o in offs]
    U = None
    if any(nb):
        planes = [lc.plane(corr, h) for h in range(H + 1)]
        U = [np.stack([lc.node_sums(planes[h], h, offs[a], x0, y0, *dims[h]) for a in range(n_ang)]) for h in range(H + 1)]
    return dict(nb=nb, thetas=thetas, dims=dims, U=U)


def descend(U, dims, a, h0, Q, P):
    """The greedy descent of the existing rule from the node (Q, P) of level h0: S of the candidate it ends at."""
    for h in range(h0, 0, -1):
        kids = [(int(U[h - 1][a, 2 * Q + dq, 2 * P + dp]), -dq, -dp) for dq in (0, 1) for dp in (0, 1)
                if 2 * Q + dq < dims[h - 1][1] and 2 * P + dp < dims[h - 1][0]]
        _, dq, dp = max(kids)                                       # the largest U, among equals the smallest (Q, P)
        Q, P = 2 * Q - dq, 2 * P - dp
    return int(U[0][a, Q, P])


def children(G, dims_below):
    return np.repeat(np.repeat(G, 2, axis=1), 2, axis=2)[:, :dims_below[1], :dims_below[0]]


def search(d, p, tight, wrong_tie=False):
    """(record LOCATE_DTYPE scalar, statistics TIGHT_STATS_DTYPE scalar, trace) of one scan's dense() under the parameters p and the flag
    word `tight`.  wrong_tie: the probe starts from the LARGEST index among equals -- NOT the rule; one test shows the difference."""
    H, nx, ny, n_ang, x0, y0, cap = p["levels"], p["nx"], p["ny"], p["n_ang"], p["x0"], p["y0"], p["max_nodes"]
    rec = np.zeros((), lc.LOCATE_DTYPE)
    st = np.zeros((), TIGHT_STATS_DTYPE)
    rec["x"], rec["y"] = -1.0, -1.0
    U, dims, nb = d["U"], d["dims"], d["nb"]
    t = dict(flags=lc.EMPTY, levels={}, n_best=0, frontier={}, nb=nb)
    if U is None:
        rec["flags"] = lc.EMPTY
        return rec, st, t
    la = [descend(U, dims, a, H, *divmod(int(np.argmax(U[H][a])), dims[H][0])) for a in range(n_ang)]
    L = max(max(la), p["score_floor"])
    st["top_nodes"] = n_ang * dims[H][0] * dims[H][1]
    scored = int(st["top_nodes"])
    G = U[H] >= L
    st["bound"][H] = L
    st["frontier"][H] = t["frontier"][H] = int(G.sum())
    overflow = H >= 1 and int(G.sum()) > cap                        # no retry: no bound was raised yet
    for h in range(H, 0, -1):
        if overflow:
            break
        kids = children(G, dims[h - 1])
        scored += int(kids.sum())
        Gn = kids & (U[h - 1] >= L)
        if h - 1 >= 1:
            lv = dict(L_in=L, probes={}, ties={}, first=int(Gn.sum()), retried=False)
            if tight & PROBE:
                for a in range(n_ang):
                    if not Gn[a].any():
                        continue                                    # a heading without a node has no probe
                    u = np.where(Gn[a], U[h - 1][a], -1).reshape(-1)
                    best = np.flatnonzero(u == u.max())
                    idx = int(best[-1] if wrong_tie else best[0])   # the rule: the smallest Q nbx + P
                    lv["ties"][a] = len(best)
                    lv["probes"][a] = descend(U, dims, a, h - 1, *divmod(idx, dims[h - 1][0]))
                L = max([L] + list(lv["probes"].values()))
            st["bound"][h - 1] = L
            lv.update(L_out=L, rebuilt=int((kids & (U[h - 1] >= L)).sum()), alive=[bool(Gn[a].any()) for a in range(n_ang)])
            if tight & RETRY and int(Gn.sum()) > cap:
                st["first_count"][h - 1] = int(Gn.sum())
                st["retried"] |= 1 << (h - 1)
                scored += int(kids.sum())
                Gn = kids & (U[h - 1] >= L)
                lv["retried"] = True
            t["levels"][h - 1] = lv
            st["frontier"][h - 1] = t["frontier"][h - 1] = int(Gn.sum())
            overflow = int(Gn.sum()) > cap
        else:
            st["frontier"][0] = t["frontier"][0] = int(Gn.sum())
            st["bound"][0] = L
        G = Gn
    st["scored"] = scored
    rec["lower_bound"] = L
    t.update(L=L, la=la, S=U[0])
    if overflow:
        rec["flags"] = t["flags"] = lc.OVERFLOW
        return rec, st, t
    if not G.any():
        rec["flags"] = t["flags"] = lc.NOT_FOUND
        return rec, st, t
    S = np.where(G, U[0], -1)
    lin = int(np.argmax(S))
    a, rem = divmod(lin, ny * nx)
    q, pp = divmod(rem, nx)
    S_win = int(S.reshape(-1)[lin])
    ok = nb[a] >= p["min_beams"] and S_win * p["min_den"] >= 255 * nb[a] * p["min_num"]
    rec["score"], rec["n_beams"], rec["cx"], rec["cy"], rec["a"], rec["n_best"] = S_win, nb[a], x0 + pp, y0 + q, a, int((S == S_win).sum())
    rec["flags"] = lc.ACCEPTED if ok else lc.REJECTED
    if ok:
        rec["x"], rec["y"], rec["ang"] = float(x0 + pp), float(y0 + q), d["thetas"][a]
    t.update(flags=int(rec["flags"]), winner=(a, q, pp), score=S_win, n_best=int(rec["n_best"]))
    return rec, st, t


def dense_case(c, levels=None):
    p = c["par"] if levels is None else dict(c["par"], levels=levels)
    return [dense(c["scans"][n], c["lens"][n], c["resol"], c["range_max"], c["corr"], p) for n in range(len(c["lens"]))]


def run_dense(ds, p, tight, wrong_tie=False):
    """(records [n], statistics [n], traces) of the scans whose dense() is ds."""
    got = [search(d, p, tight, wrong_tie) for d in ds]
    return np.array([g[0] for g in got], lc.LOCATE_DTYPE), np.array([g[1] for g in got], TIGHT_STATS_DTYPE), [g[2] for g in got]


def locate_tight(scans, lens, resol, range_max, corr, p, tight):
    """(records, statistics) as lc.locate gives them, under the tight rule."""
    ds = [dense(scans[n], lens[n], resol, range_max, corr, p) for n in range(len(lens))]
    return run_dense(ds, p, tight)[:2]


# ---- the campaign ----------------------------------------------------------------------------------------------------------------------
def ring(k, r, phase=0.0):
    """k distinct whole-cell offsets near a circle of r cells: a room seen from its middle."""
    out = []
    for i in range(4 * k):
        a = phase + 2 * math.pi * i / (4 * k)
        o = (int(round(r * math.cos(a) * (1 + 0.13 * (i % 3)))), int(round(r * math.sin(a) * (1 - 0.11 * (i % 2)))))
        if o not in out and o != (0, 0):
            out.append(o)
    return out[::4][:k] if len(out[::4]) >= k else out[:k]


def decoy_plane(cols, rows, cells, pose, period=16, extent=40, bright=255):
    """The decoy of the issue: a low-index region with one bright cell per `period` x `period` cells -- every window of plane_H with 2^H >=
    period holds one, so plane_H is saturated there while plane_(H-1) is not -- and the real room, the scan's own cells around `pose`, at a
    higher index."""
    corr = np.zeros((rows, cols), np.uint8)
    for y in range(7 % period, min(extent, rows), period):
        for x in range(5 % period, min(extent, cols), period):
            corr[y, x] = bright
    for ox, oy in cells:
        corr[pose[1] + oy, pose[0] + ox] = bright
    return corr


def counts_of(ds, p):
    """Every count a choice of max_nodes could sit at: the frontiers, the first counts and the rebuilt counts of every scan, unlimited."""
    q = dict(p, max_nodes=UNLIMITED)
    seen = set()
    for tight in TIGHTS:
        for _, st, t in (search(d, q, tight) for d in ds):
            seen.update(int(v) for v in st["frontier"][1:])
            for lv in t["levels"].values():
                seen.update((lv["first"], lv["rebuilt"]))
    return sorted(v for v in seen if v >= 1)


def choose_max_nodes(c, pred):
    """The smallest max_nodes at or one below a count of the restatement at which pred({tight: (records, statistics, traces)}) holds."""
    ds = dense_case(c)
    for m in sorted({v - d for v in counts_of(ds, c["par"]) for d in (0, 1) if v - d >= 1}):
        p = dict(c["par"], max_nodes=m)
        if pred({tight: run_dense(ds, p, tight) for tight in TIGHTS}):
            return m
    raise AssertionError("no max_nodes makes the case %s what it is meant to be" % c["name"])


def flags_of(res, tight, scan=0):
    return int(res[tight][0][scan]["flags"])


def probe_rescues(res):
    return flags_of(res, 0) == lc.OVERFLOW and flags_of(res, PROBE) != lc.OVERFLOW and int(res[PROBE][1][0]["retried"]) == 0


def retry_rescues(res):
    return flags_of(res, 0) == flags_of(res, PROBE) == flags_of(res, RETRY) == lc.OVERFLOW and flags_of(res, 3) != lc.OVERFLOW


def retry_fails(res):
    st = res[3][1][0]
    if flags_of(res, 3) != lc.OVERFLOW or not st["frontier"].any():
        return False
    return bool(st["retried"] >> int(np.flatnonzero(st["frontier"])[0]) & 1)      # the level the search stopped at had its retry


def top_overflows(res):
    for t in TIGHTS:
        st = res[t][1][0]
        if flags_of(res, t) != lc.OVERFLOW or st["retried"] or np.count_nonzero(st["frontier"]) != 1:
            return False
    return True


@functools.lru_cache(maxsize=None)
def campaign():
    """The added cases, deterministic."""
    cases = []
    rng = np.random.default_rng(20251020)
    resol = 0.05
    # the decoy plane: rescue by the probe, rescue by the retry alone
    for v in range(3):
        cells = ring(10 + v, 7 + v, 0.3 * v)
        pose = (46 - v, 33 - 2 * v)
        corr = decoy_plane(61, 47 - v, cells, pose)
        beams = [gm.beams_at_cells((0.0, 0.0), cells, resol)]
        p = lc.whole(corr, ang0=(0.0, -10.0, -20.0)[v], ang_step=(20.0, 10.0, 20.0)[v], n_ang=(1, 3, 2)[v], levels=4 + (v == 2), min_den=2)
        for name, pred in (("probe_rescue", probe_rescues), ("retry_rescue", retry_rescues)):
            c = lc.case("%s_%d" % (name, v), corr, resol, 1.5, beams, dict(p))
            c["par"]["max_nodes"] = choose_max_nodes(c, pred)
            cases.append(c)
    # ambiguous planes: the retry runs and the level still does not fit; and max_nodes below |G_H|
    for v in range(3):
        corr = gm.random_plane(rng, 61 - 2 * v, 47, 0.8)
        c = lc.case("retry_fails_%d" % v, corr, resol, 1.5, [lc.random_beams(rng, 7 + 2 * v)], lc.whole(corr, ang_step=15.0, n_ang=2 + v, levels=3 + v % 2))
        c["par"]["max_nodes"] = choose_max_nodes(c, retry_fails)
        cases.append(c)
        c = dict(c, name="top_overflow_%d" % v, par=dict(c["par"]))
        c["par"]["max_nodes"] = choose_max_nodes(c, top_overflows)
        cases.append(c)
    # a tie for the heading's best node: two clusters whose blocks of level H - 1 give the same U and whose best candidates differ.  The
    # low-index cluster's two cells are one cell further apart than the beams, the high-index cluster's exactly as far
    for v in range(3):
        corr = np.zeros((47, 61), np.uint8)
        gap = 6 + v
        corr[9 + v, 8], corr[9 + v, 8 + gap + 1] = 200, 200
        corr[36 - v, 44], corr[36 - v, 44 + gap] = 200, 200
        corr[20, 30] = 90                                           # what the top-level descent of this plane ends at least as good as
        beams = [gm.beams_at_cells((0.0, 0.0), [(-(gap // 2), 0), (gap - gap // 2, 0)], resol)]
        cases.append(lc.case("head_tie_%d" % v, corr, resol, 1.0, beams, lc.whole(corr, levels=4 + (v == 1), min_den=2)))
    # a heading without a surviving node (the room is seen at one heading only); a probe that does not raise L
    for v in range(3):
        cells = ring(9 + v, 6 + v, 0.2 + v)
        corr = decoy_plane(61 - v, 47, cells, (40 + v, 30), extent=0)
        corr[np.nonzero(gm.random_plane(rng, 61 - v, 47, 0.03))] = 60
        beams = [gm.beams_at_cells((0.0, 0.0), cells, resol)]
        cases.append(lc.case("lone_heading_%d" % v, corr, resol, 1.5, beams, lc.whole(corr, ang0=-90.0, ang_step=45.0, n_ang=3 + 2 * v, levels=3 + v, min_den=2)))
    # score_floor above every probe and every first descent (at S_win: the descents of these planes all end below it), and above S_win
    v = 0
    while v < 3:
        corr = gm.random_plane(rng, 55, 43 + v, 0.5)
        c = lc.case("floor_over_probes_%d" % v, corr, resol, 1.5, [lc.random_beams(rng, 13 + v)], lc.whole(corr, ang_step=9.0, n_ang=2, levels=3 + v % 2))
        ds = dense_case(c)
        s_win = int(run_dense(ds, c["par"], 0)[0][0]["score"])
        c["par"]["score_floor"] = s_win
        t = run_dense(ds, c["par"], 3)[2][0]
        if s_win <= max(t["la"] + [s for lv in t["levels"].values() for s in lv["probes"].values()]):
            continue                                                # a descent found the winner: not this class
        cases.append(c)
        cases.append(dict(c, name="floor_over_win_%d" % v, par=dict(c["par"], score_floor=s_win + 1)))
        v += 1
    # 1025 beams, once: a raised scan capacity
    corr = gm.random_plane(rng, 61, 47)
    b = lc.random_beams(rng, 1025)
    cases.append(lc.case("nb1025", corr, resol, 1.5, [b], lc.whole(corr, ang0=15.0, ang_step=41.5, n_ang=2, levels=4), capacity=2048))
    # an empty scan between two others, on the decoy plane at the probe's max_nodes
    for v in range(3):
        base = cases[2 * v]                                          # probe_rescue_v
        scans = [base["scans"][0][:base["lens"][0]], [], base["scans"][0][:base["lens"][0] - 2 - v]]
        cases.append(lc.case("empty_between_%d" % v, base["corr"], resol, 1.5, scans, dict(base["par"])))
    return cases


CLASSES = ["rescue_by_probe", "rescue_by_retry", "overflow_after_retry", "top_overflow", "head_tie", "heading_without_node", "probe_not_raising",
           "probe_raising", "floor_above_probes", "floor_above_win", "nb_1025", "empty_between", "levels_5"]
ONCE = {"nb_1025"}


def classes_of(c, res, wrong):
    """The classes the case reaches: res = {tight: (records, statistics, traces)}, wrong = the statistics of tight = 3 with the probe's
    tie broken the wrong way."""
    got = set()
    p = c["par"]
    if p["levels"] == 5:
        got.add("levels_5")
    for i in range(len(c["lens"])):
        f = {t: int(res[t][0][i]["flags"]) for t in TIGHTS}
        st = {t: res[t][1][i] for t in TIGHTS}
        tr = {t: res[t][2][i] for t in TIGHTS}
        if f[0] == lc.EMPTY:
            if 0 < i < len(c["lens"]) - 1:
                got.add("empty_between")
            continue
        if 1025 in tr[0]["nb"]:
            got.add("nb_1025")
        if f[0] == lc.OVERFLOW and f[PROBE] != lc.OVERFLOW:
            got.add("rescue_by_probe")
        if f[PROBE] == lc.OVERFLOW and f[3] != lc.OVERFLOW:
            got.add("rescue_by_retry")
            h = int(st[3]["retried"]).bit_length() - 1
            assert st[3]["first_count"][h] > p["max_nodes"] >= st[3]["frontier"][h] and st[PROBE]["frontier"][h] == st[3]["first_count"][h]
        if f[3] == lc.OVERFLOW and st[3]["retried"]:
            h = int(np.flatnonzero(st[3]["frontier"])[0])
            if st[3]["retried"] >> h & 1:
                got.add("overflow_after_retry")
                assert st[3]["first_count"][h] >= st[3]["frontier"][h] > p["max_nodes"]
        if f[3] == lc.OVERFLOW and st[3]["frontier"][p["levels"]] > p["max_nodes"] and p["levels"] >= 1:
            got.add("top_overflow")
            assert not st[3]["retried"] and not st[3]["frontier"][:p["levels"]].any() and not st[3]["bound"][:p["levels"]].any()
        for lv in tr[3]["levels"].values():
            if any(n >= 2 for n in lv["ties"].values()) and wrong[i]["bound"].tobytes() != st[3]["bound"].tobytes():
                got.add("head_tie")
            if any(lv["alive"]) and not all(lv["alive"]):
                got.add("heading_without_node")
                assert len(lv["probes"]) == sum(lv["alive"])
            if lv["probes"]:
                got.add("probe_raising" if lv["L_out"] > lv["L_in"] else "probe_not_raising")
        probes = [s for lv in tr[3]["levels"].values() for s in lv["probes"].values()]
        if probes and p["score_floor"] > max(probes + tr[3]["la"]) and f[3] not in (lc.NOT_FOUND, lc.OVERFLOW):
            got.add("floor_above_probes")
        if f[3] == lc.NOT_FOUND and p["score_floor"] == int(tr[3]["S"].max()) + 1:
            got.add("floor_above_win")
    return got


@functools.lru_cache(maxsize=None)
def expected():
    """Per case of the added campaign {tight: (records, statistics, traces)} and the statistics of tight = 3 under the wrong tie: computed
    once, shared, never changed."""
    out = []
    for c in campaign():
        ds = dense_case(c)
        out.append(({t: run_dense(ds, c["par"], t) for t in TIGHTS}, run_dense(ds, c["par"], 3, wrong_tie=True)[1]))
    return out


@functools.lru_cache(maxsize=None)
def expected_existing():
    """The same for the campaign of tests/grid_locate_cases.py."""
    out = []
    for c in lc.campaign():
        ds = dense_case(c)
        out.append({t: run_dense(ds, c["par"], t) for t in TIGHTS})
    return out
