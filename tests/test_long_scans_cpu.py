"""What the long-scan campaign (tests/scan_cases_long.py) reaches, under the oracle alone, and the interface the long lidars get:
the two C entries, the n_beams keyword of the three constructors, the tick's input bytes.  tests/test_long_scans_gpu.py holds
k_rdp_long.hip to the same campaign bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest

import scan_cases as sc
import scan_cases_long as scl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def campaign():
    return scl.campaign()


@pytest.fixture(scope="module")
def refs(campaign, oracle):
    out = [sc.reference(oracle, g, oracle.lib_cr()) for g in campaign]
    for r in out:
        scl.check_bounds(r)
    return out


def test_campaign_size_and_lengths(campaign):
    n = sum(len(g["scans"]) for g in campaign)
    assert 300 <= n <= 600, n
    for g in campaign:
        assert sorted({len(s) for s in g["scans"]}) == sorted(scl.SHORT_LENGTHS + scl.LONG_LENGTHS)
        assert set(scl.by_stride(g)) == {scl.SHORT_STRIDE} | set(scl.LONG_LENGTHS)
    assert min(scl.LONG_LENGTHS) == 1025 and max(scl.LONG_LENGTHS) == 4096 and scl.SHORT_STRIDE > sc.STRIDE
    assert len({t for g in campaign for t in g["tags"]}) >= 14


def test_campaign_reaches_the_cluster_cases(campaign):
    joined = dropped = joined_behind_a_drop = 0
    for g in campaign:
        for s in g["scans"]:
            if len(s) <= 1024:
                continue
            cl, d, j = scl.walk(s, g["limit"])
            joined += j
            dropped += d > 0 and len(cl) > 0
            joined_behind_a_drop += sc.clusters(s, g["limit"])[2]
    assert joined > 0 and dropped > 0 and joined_behind_a_drop > 0, (joined, dropped, joined_behind_a_drop)


def test_campaign_reaches_the_record_and_pixel_limits(campaign, refs):
    over = under = many_pts = 0
    for g, rs in zip(campaign, refs):
        for s, r in zip(g["scans"], rs):
            if len(s) > 1024:
                over += r["n_lines"] > 360
                under += r["n_lines"] <= 360
            many_pts += len(r["pts"]) > sc.PTS_CAP_SMALL
    assert over > 0 and under > over and many_pts > 0, (over, under, many_pts)


def test_campaign_reaches_split_points_in_the_first_and_the_last_chunk(campaign):
    first = last = 0
    for g in campaign:
        for s in g["scans"]:
            if len(s) <= 1024:
                continue
            sp = scl.split_points(s, g["limit"], g["thre_line"])
            first += bool((sp < 64).any())
            last += bool((sp >= len(s) - 64).any())
    assert first > 0 and last > 0, (first, last)


def test_header_and_symbol_list(lsdmod):
    h = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    assert re.search(r"^#define\s+LSD_SCAN_MAX_LEN\s+4096\s*$", h, re.M)
    assert re.search(r"^int\s+lsd_set_scan_capacity\(lsd_ctx \*ctx, int readings\);", h, re.M)
    assert re.search(r"^int\s+lsd_scan_capacity\(const lsd_ctx \*ctx\);", h, re.M)
    assert "lsd_set_scan_capacity" in lsdmod.EXPORTED_SYMBOLS and "lsd_scan_capacity" in lsdmod.EXPORTED_SYMBOLS
    assert lsdmod.LSD_SCAN_MAX_LEN == 4096
    assert callable(lsdmod.Context.set_scan_capacity) and isinstance(lsdmod.Context.scan_capacity, property)


def test_constructors_take_n_beams_last(lsdmod):
    for f in (lsdmod.Localizer.__init__, lsdmod.Localizer.from_occupancy_grid, lsdmod.FleetLocalizer.__init__):
        p = list(inspect.signature(f).parameters.values())
        assert p[-1].name == "n_beams" and p[-1].default == 360, f


def test_tick_input_bytes_per_slot(lsdmod):
    t = lsdmod._Ticks
    assert t._IN_B == 5788 and t._in_b(360) == 5788
    for n in (1, 360, 1081, 4096):
        assert t._in_b(n) == 16 * n + 28


def test_n_beams_outside_the_range_is_refused_before_anything_else(lsdmod):
    for n, code in ((0, lsdmod.LSD_ERR_INVALID), (-5, lsdmod.LSD_ERR_INVALID), (4097, lsdmod.LSD_ERR_UNSUPPORTED)):
        with pytest.raises(lsdmod.LsdError) as e:
            lsdmod._check_n_beams(n)
        assert e.value.status == code
    assert lsdmod._check_n_beams(4096) == 4096 and lsdmod._check_n_beams(1) == 1
