"""The isosurface extraction's share of the C ABI on a GPU-less host: the 48- and 32-byte structures, the three
symbols, the enumerators as the header states them, and the CLI's usage text (no compute calls here)."""
import ctypes as C
import os
import re
import subprocess

from volumerenderercl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")


def test_struct_sizes_and_offsets():
    assert C.sizeof(_lib.MeshParams) == 48 and C.sizeof(_lib.MeshInfo) == 32
    for name, off in (("isoValue", 0), ("normals", 4), ("lo", 8), ("hi", 20), ("reserved", 32)):
        assert getattr(_lib.MeshParams, name).offset == off
    for name, off in (("triangles", 0), ("blocks", 8), ("blocks_skipped", 16), ("empty_skip", 24), ("reserved", 28)):
        assert getattr(_lib.MeshInfo, name).offset == off
    assert C.sizeof(_lib.LaunchInfo) == 128 and C.sizeof(_lib.DepthParams) == 32   # (the others keep their sizes)


def test_symbols_load():
    lib = _lib.load()
    for name in ("vrhip_isosurface_count", "vrhip_isosurface_extract", "vrhip_last_mesh_info"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # no renderer: refused, not dereferenced
    n = C.c_uint64(7)
    assert lib.vrhip_isosurface_count(None, C.byref(_lib.MeshParams()), C.byref(n)) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract(None, C.byref(_lib.MeshParams()), None, None, 0, C.byref(n), 0) == _lib.ERR_INVALID
    assert lib.vrhip_last_mesh_info(None, C.byref(_lib.MeshInfo())) == _lib.ERR_INVALID
    assert n.value == 7


def test_enumerators_match_the_header():
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for name, value in (("MESH_NORMALS_NONE", 0), ("MESH_NORMALS_GRADIENT", 1)):
        m = re.search(r"\bVRHIP_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == value == getattr(_lib, name)
    m = re.search(r"#define VRHIP_MESH_BLOCK (\d+)u", text)
    assert m and int(m.group(1)) == _lib.MESH_BLOCK == 8


def test_usage_text_names_mesh():
    res = subprocess.run([EXE, "--mesh-normals"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render")
    for opt in ("--mesh V FILE.stl|.ply", "--mesh-normals", "--mesh-region X0 Y0 Z0 X1 Y1 Z1"):
        assert opt in res.stderr
