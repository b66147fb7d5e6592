"""The indexed isosurface extraction's share of the C ABI on a GPU-less host: the 64-byte info block, the structures
that keep their sizes, the three symbols, a NULL renderer, and the CLI's usage text (no compute calls here)."""
import ctypes as C
import os
import subprocess

from volumerenderercl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")


def test_struct_sizes_and_offsets():
    assert C.sizeof(_lib.IndexedMeshInfo) == 64
    for name, off in (("vertices", 0), ("triangles", 8), ("point_blocks", 16), ("point_blocks_skipped", 24), ("blocks", 32),
                      ("blocks_skipped", 40), ("scratch_bytes", 48), ("empty_skip", 56), ("reserved", 60)):
        assert getattr(_lib.IndexedMeshInfo, name).offset == off
    assert C.sizeof(_lib.MeshParams) == 48 and C.sizeof(_lib.MeshInfo) == 32 and C.sizeof(_lib.LaunchInfo) == 128


def test_symbols_load_and_refuse_a_null_renderer():
    lib = _lib.load()
    for name in ("vrhip_isosurface_count_indexed", "vrhip_isosurface_extract_indexed", "vrhip_last_indexed_mesh_info"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    nv, nt = C.c_uint64(7), C.c_uint64(9)
    p = _lib.MeshParams()
    assert lib.vrhip_isosurface_count_indexed(None, C.byref(p), C.byref(nv), C.byref(nt)) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(None, C.byref(p), None, None, None, 0, 0, C.byref(nv), C.byref(nt), 0) == _lib.ERR_INVALID
    assert lib.vrhip_last_indexed_mesh_info(None, C.byref(_lib.IndexedMeshInfo())) == _lib.ERR_INVALID
    assert (nv.value, nt.value) == (7, 9)


def test_header_states_the_structure():
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    at = text.index("typedef struct vrhip_indexed_mesh_info {")
    body = text[at:text.index("} vrhip_indexed_mesh_info;", at)]
    fields = [w.strip(" ;\n") for line in body.splitlines()[1:] for w in line.split("uint64_t")[-1].split("uint32_t")[-1].split(",")]
    assert fields == [n for n, _ in _lib.IndexedMeshInfo._fields_]


def test_usage_text_names_mesh_indexed(tmp_path):
    for args in (["--mesh-indexed"], ["--mesh", "0.5", "out.stl", "--mesh-indexed"]):
        res = subprocess.run([EXE, "--synth", "shells", "32", "UCHAR"] + args, capture_output=True, text=True, timeout=60,
                             cwd=str(tmp_path))
        assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render")
        assert "[--mesh-indexed]" in res.stderr and "--mesh V FILE.stl|.ply" in res.stderr
        assert not os.listdir(str(tmp_path))
