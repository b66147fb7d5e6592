"""The depth images' share of the C ABI on a GPU-less host: the two 32-byte structures, the two symbols, the
enumerators as the header states them, and the CLI's usage text (no compute calls here)."""
import ctypes as C
import os
import re
import subprocess

from volumerenderercl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")


def test_struct_sizes_and_offsets():
    assert C.sizeof(_lib.DepthParams) == 32 and C.sizeof(_lib.DepthInfo) == 32
    for i, name in enumerate(("mode", "threshold", "refineSteps", "x0", "y0", "w", "h", "reserved")):
        assert getattr(_lib.DepthParams, name).offset == 4 * i
    for i, name in enumerate(("mode", "work_items", "empty_skip", "reserved")):
        assert getattr(_lib.DepthInfo, name).offset == 4 * i
    assert C.sizeof(_lib.LaunchInfo) == 128   # (vrhip_last_launch_info keeps its size)


def test_symbols_load():
    lib = _lib.load()
    for name in ("vrhip_render_depth", "vrhip_last_depth_info"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # no renderer: refused, not dereferenced
    assert lib.vrhip_render_depth(None, 8, 8, C.byref(_lib.DepthParams()), None, None, None, 0) == _lib.ERR_INVALID
    assert lib.vrhip_last_depth_info(None, C.byref(_lib.DepthInfo())) == _lib.ERR_INVALID


def test_enumerators_match_the_header():
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for name, value in (("DEPTH_ISO", 0), ("DEPTH_MAX", 1), ("DEPTH_OPACITY", 2), ("DEPTH_MISS", 0),
                        ("DEPTH_NO_HIT", 1), ("DEPTH_HIT", 2)):
        m = re.search(r"\bVRHIP_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == value == getattr(_lib, name)


def test_usage_text_names_depth():
    res = subprocess.run([EXE, "--depth-refine", "3"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render")
    for opt in ("--depth iso V | max | opacity A", "--depth-refine N", "--depth-rect X Y W H"):
        assert opt in res.stderr
