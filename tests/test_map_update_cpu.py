"""The device-side map update without a device: the header declares the new entries, the built library exports them with C linkage,
the ctypes signatures of the Python mirror have the header's argument counts, and the mirror has the new calls."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsd_enqueue_map_update_device", "lsd_reserve_map_update", "lsd_enqueue_localize_live_map_device",
       "lsd_enqueue_localize_resume_live_map_device")


def header_arguments(name):
    """The argument list of `name`'s declaration in include/lsd_hip.h, comments removed, split at the commas."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsd_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, "include/lsd_hip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_mirrored(lsdmod, name):
    args = header_arguments(name)
    lib = lsdmod.load_library()
    assert name in lsdmod.EXPORTED_SYMBOLS
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args), (len(fn.argtypes), args)
    syms = subprocess.run(["nm", "-D", "--defined-only", lsdmod.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert name in {l.split()[-1] for l in syms.splitlines() if l.strip()}          # the plain name: C linkage


def test_live_map_entries_carry_the_old_arguments():
    """int n_map becomes int map_lines_cap, const int32_t *d_n_map; every other argument keeps its place and type."""
    for old, new in (("lsd_enqueue_localize_device", "lsd_enqueue_localize_live_map_device"),
                     ("lsd_enqueue_localize_resume_device", "lsd_enqueue_localize_resume_live_map_device")):
        a, b = header_arguments(old), header_arguments(new)
        assert a[5] == "int n_map" and b[5:7] == ["int map_lines_cap", "const int32_t *d_n_map"]
        assert a[:5] == b[:5] and a[6:] == b[7:]
    assert header_arguments("lsd_enqueue_map_update_device") == [
        "lsd_ctx *ctx", "const int8_t *d_grid", "int cols", "int rows", "double res", "double z_occ_max_dis", "const lsd_params *p",
        "uint8_t *d_map", "double *d_map_cache", "lsd_line *d_lines", "int max_lines", "int32_t *d_count", "uint8_t *d_line_im", "void *stream"]
    assert header_arguments("lsd_reserve_map_update") == ["lsd_ctx *ctx", "int cols", "int rows"]


def test_python_mirror(lsdmod):
    for name in ("enqueue_map_update_device", "reserve_map_update", "enqueue_localize_live_map_device", "enqueue_localize_resume_live_map_device"):
        assert callable(getattr(lsdmod.Context, name))
    for name in ("set_map_device", "reserve_map", "set_map"):
        assert callable(getattr(lsdmod.Localizer, name))
    assert isinstance(lsdmod.Localizer.map_counts, property)
    assert list(inspect.signature(lsdmod.Localizer.set_map_device).parameters) == [
        "self", "d_grid", "oriMapCol", "oriMapRow", "mapResol", "mapOriX", "mapOriY", "stream"]
    assert list(inspect.signature(lsdmod.Localizer.reserve_map).parameters) == ["self", "cols", "rows", "lines_cap"]
    assert inspect.signature(lsdmod.Localizer.reserve_map).parameters["lines_cap"].default == 512
    assert list(inspect.signature(lsdmod.mapCallback_device).parameters)[:6] == ["d_grid", "oriMapCol", "oriMapRow", "mapResol", "ctx", "stream"]
