"""lsd_set_fused_lines (lines written by the region stage): the setter is declared, exported and bound.  No GPU."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setter_is_bound():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    lsdmod = importlib.import_module("linesegmentdetector-slam_amd")
    hdr = open(os.path.join(ROOT, "include", "lsd_hip.h")).read()
    assert "lsd_set_fused_lines" in lsdmod.EXPORTED_SYMBOLS and "int lsd_set_fused_lines(lsd_ctx *ctx, int on);" in hdr
    assert callable(lsdmod.Context.set_fused_lines)
