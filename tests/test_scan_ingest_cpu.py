"""Scan ingestion without a device: the plain restatement of the ingest rules (tests/scan_ingest.py) is the host filter that
Localizer.step used to run (lidar_frames, lidar_frames_batch) on every frame of the three logs; the built library and the Python mirror
have the new entries; the LaserScan angle's single-precision rule is one a test can tell from the double-precision expression."""
import ctypes as C

import numpy as np
import pytest

import fa_restatement as fr
import scan_ingest as si


@pytest.mark.parametrize("name", ["data", "f3key", "f4key"])
def test_restatement_is_the_host_filter(lsdmod, name):
    lid = fr.load_log(name)[2]
    assert lid.shape == (fr.LOG_FRAMES[name], 360, 2)
    scans, lens = si.ingest_pairs(lid)
    assert (lens < 360).all() and (lens > 0).all()                             # every frame has infinite ranges: the filter is never a no-op
    for got_scans, got_lens in (lsdmod.lidar_frames(lid), lsdmod.lidar_frames_batch(lid)):
        assert got_scans.dtype == np.float64 and got_scans.tobytes() == scans.tobytes()     # byte for byte, the zero tail included
        assert got_lens.dtype == np.int32 and np.array_equal(got_lens, lens)


def test_restatement_corner_cases():
    raw = np.zeros((3, 5, 2)); raw[..., 1] = np.arange(5)
    raw[0, :, 0] = [1.0, np.inf, -np.inf, np.nan, 2.0]
    raw[1, :, 0] = np.inf
    raw[2, :, 0] = [3.0, 4.0, 5.0, 6.0, np.inf]
    scans, lens = si.ingest_pairs(raw, stride=7, take=[1, 1, 0])
    assert list(lens) == [4, 0, 0] and scans.shape == (3, 7, 2)
    assert np.array_equal(scans[0, :4, 1], [0, 2, 3, 4]) and np.isnan(scans[0, 2, 0]) and scans[0, 1, 0] == -np.inf
    assert not scans[0, 4:].view(np.uint8).any() and not scans[1:].view(np.uint8).any()
    sc, ln = si.ingest_laserscan(np.array([[1.5, np.inf, 2.5]], np.float32), np.array([[0.25, 0.5]], np.float32))
    assert list(ln) == [2] and np.array_equal(sc[0], [[1.5, 0.25], [2.5, 1.25], [0.0, 0.0]])


def test_library_exports_and_python_mirror(lsdmod):
    lib = lsdmod.load_library()
    for name in ("lsd_enqueue_scan_ingest_device", "lsd_enqueue_laserscan_ingest_device"):
        assert name in lsdmod.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.lsd_enqueue_scan_ingest_device.argtypes) == 9 and len(lib.lsd_enqueue_laserscan_ingest_device.argtypes) == 10
    for name in ("enqueue_scan_ingest_device", "enqueue_laserscan_ingest_device"):
        assert callable(getattr(lsdmod.Context, name))
    assert callable(lsdmod.Localizer.step_device)


def test_single_precision_angle_is_distinguishable():
    """angle_min + i * angle_increment in float (the callback's fields) against the same float32 constants widened to double first."""
    a_min, a_inc = np.float32(-3.12414), np.float32(0.0174533)
    single = np.array([si.laserscan_angle(a_min, a_inc, i) for i in range(360)])
    double = np.array([float(a_min) + i * float(a_inc) for i in range(360)])
    assert (single != double).sum() == 357
    assert np.abs(single - double).max() < 1e-6                                # a rounding, not another formula
