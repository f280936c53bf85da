"""The fleet entries without a GPU: the lsd_map_ref record (its layout in include/lsd_hip.h, in ctypes and in MAP_REF_DTYPE), the three
exported symbols, and the argument checks of the Python side that need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lsd_enqueue_feature_scan_maps_device", "lsd_enqueue_localize_maps_device", "lsd_enqueue_localize_resume_maps_device")
# offsets on the LP64 targets the library is built for: three pointers, three ints (+ 4 bytes of padding), three doubles
OFFSETS = {"d_map_cache": 0, "d_map_lines": 8, "d_n_map": 16, "cols": 24, "rows": 28, "n_map": 32, "mapResol": 40, "mapOriX": 48, "mapOriY": 56}


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return g


def header_map_ref_fields():
    """(is a pointer, type, names) of the member declarations of lsd_map_ref, in the header's order."""
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    body = re.search(r"typedef struct lsd_map_ref \{(.*?)\} lsd_map_ref;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*([\w\s,]+)$", decl)
        if m:
            out.append((bool(m.group(2)), m.group(1), [n.strip() for n in m.group(3).split(",")]))
    return out


def test_map_ref_layout_matches_the_header(lsdmod):
    scalars = {"int": C.c_int, "double": C.c_double}
    fields = []
    for ptr, typ, names in header_map_ref_fields():
        fields += [(n, C.c_void_p if ptr else scalars[typ]) for n in names]
    assert [n for n, _ in fields] == list(OFFSETS)
    ct = type("lsd_map_ref_h", (C.Structure,), {"_fields_": fields})
    dt = lsdmod.MAP_REF_DTYPE
    assert C.sizeof(ct) == C.sizeof(lsdmod.lsd_map_ref) == dt.itemsize == 64
    for n, t in fields:
        assert getattr(ct, n).offset == getattr(lsdmod.lsd_map_ref, n).offset == dt.fields[n][1] == OFFSETS[n], n
        assert C.sizeof(t) == dt.fields[n][0].itemsize, n
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    assert int(re.search(r"#define LSD_MAX_MAPS (\d+)", src).group(1)) == lsdmod.LSD_MAX_MAPS == 64


def test_entries_are_exported(built, lsdmod):
    lib = lsdmod.load_library()
    for name in ENTRIES:
        assert name in lsdmod.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == (20 if "feature_scan" in name else 18)
    src = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(lsd_ctx \*ctx" % name, src), name


def test_map_ref_and_table(lsdmod):
    r = lsdmod.map_ref(0x1000, 7, 5, 0x2000, 3, (7, 5, 0.05, -1.5, 2.25))
    assert r.dtype == lsdmod.MAP_REF_DTYPE
    assert (r["d_map_cache"], r["d_map_lines"], r["d_n_map"], r["cols"], r["rows"], r["n_map"]) == (0x1000, 0x2000, 0, 7, 5, 3)
    assert (r["mapResol"], r["mapOriX"], r["mapOriY"]) == (0.05, -1.5, 2.25)
    live = lsdmod.map_ref(0x1000, 7, 5, None, 0, (7, 5, 0.05, 0, 0), d_n_map=0x3000)
    assert live["d_map_lines"] == 0 and live["d_n_map"] == 0x3000
    tab = lsdmod.map_table([r, live])
    assert tab.dtype == lsdmod.MAP_REF_DTYPE and tab.shape == (2,) and tab.flags.c_contiguous
    assert tab[0].tobytes() == r.tobytes() and tab[1].tobytes() == live.tobytes()
    as_c = lsdmod.lsd_map_ref.from_buffer_copy(tab[0].tobytes())          # the bytes are the C record's
    assert (as_c.d_map_cache, as_c.d_map_lines, as_c.d_n_map, as_c.cols, as_c.rows, as_c.n_map) == (0x1000, 0x2000, None, 7, 5, 3)
    assert (as_c.mapResol, as_c.mapOriX, as_c.mapOriY) == (0.05, -1.5, 2.25)
    assert lsdmod.map_table(tab) is not None and lsdmod.map_table(tab[::1]).tobytes() == tab.tobytes()


def test_fleet_map_ids(lsdmod):
    ids = lsdmod.fleet_map_ids([2, 0, -1, 1], 3)
    assert ids.dtype == np.int32 and ids.tolist() == [2, 0, -1, 1]
    assert lsdmod.fleet_map_ids(np.array([[0, 1]]), 2, count=2).tolist() == [0, 1]
    for bad, n_maps, count in (([0, 3], 3, None), ([-2], 3, None), ([0, 1], 3, 3)):
        with pytest.raises(lsdmod.LsdError) as e:
            lsdmod.fleet_map_ids(bad, n_maps, count)
        assert e.value.status == lsdmod.LSD_ERR_INVALID


def test_fleet_localizer_refuses_bad_tables_before_touching_the_device(lsdmod):
    """The checks FleetLocalizer makes before its first allocation: no map, too many maps, an id outside the table, no robot."""
    m = (np.zeros((4, 4)), np.zeros(0, lsdmod.LINE_DTYPE), (4, 4, 0.025, 0.0, 0.0))
    for maps, map_of, status in (([], [0], lsdmod.LSD_ERR_INVALID), ([m] * 65, [0], lsdmod.LSD_ERR_UNSUPPORTED),
                                 ([m], [1], lsdmod.LSD_ERR_INVALID), ([m], [-2], lsdmod.LSD_ERR_INVALID), ([m], [], lsdmod.LSD_ERR_INVALID)):
        with pytest.raises(lsdmod.LsdError) as e:
            lsdmod.FleetLocalizer(maps, map_of)
        assert e.value.status == status
