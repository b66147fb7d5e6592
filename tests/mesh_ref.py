"""ctypes loader of tests/ref/mesh_ref.c, the scalar CPU restatement of the isosurface extraction
(vrhip_isosurface_count / vrhip_isosurface_extract).  TEST INFRASTRUCTURE ONLY.  The library is compiled on first use
with the CFLAGS line of oracle/Makefile (no fp contraction), next to its source, linked to the oracle's library (the
included tests/ref/iso_ref.c refers to it), and rebuilt when a source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import vro
from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "ref", "mesh_ref.c")
_DEPS = [_SRC, os.path.join(_HERE, "ref", "iso_ref.c")]
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libmeshref.so")
_ORACLE_DIR = os.path.join(_ROOT, "oracle", "_build")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
BLOCK = 8


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("tff", C.c_void_p), ("tff_n", C.c_uint32)]


class MeshParams(C.Structure):
    _fields_ = [("isoValue", C.c_float), ("normals", C.c_uint32), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3),
                ("reserved", C.c_uint32 * 4)]


assert C.sizeof(MeshParams) == 48


def build():
    vro.lib()   # (builds the oracle's library when it is missing)
    if os.path.exists(_LIB_PATH) and all(os.path.getmtime(_LIB_PATH) >= os.path.getmtime(d) for d in _DEPS):
        return
    os.makedirs(os.path.dirname(_LIB_PATH), exist_ok=True)
    tmp = "%s.%d.tmp" % (_LIB_PATH, os.getpid())
    subprocess.check_call([os.environ.get("CC", "gcc")] + oracle_cflags() +
                          ["-shared", "-o", tmp, _SRC, "-L" + _ORACLE_DIR, "-lvroracle",
                           "-Wl,-rpath,$ORIGIN/../../../oracle/_build", "-lm"])
    os.replace(tmp, _LIB_PATH)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB_PATH)
        L.mesh_extract.restype = C.c_int64
        L.mesh_extract.argtypes = [C.POINTER(Scene), C.POINTER(MeshParams)] + [C.c_void_p] * 4 + [C.c_uint64]
        _lib = L
    return _lib


def extract(vol, fmt, iso, normals=False, region=None, debug=False):
    """The triangle list of vol (ndarray [z, y, x] of the format's dtype) at iso; region = (lo xyz, hi xyz) or None.
    Returns (positions float32 [n, 3, 3], normals float32 [n, 3, 3] or None) and, with debug, per triangle the
    direction from its tetrahedron's inside to its outside vertices (float64 [n, 3], voxel units) and its cube's corner 0
    (uint32 [n, 3], x y z)."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    mp = MeshParams()
    mp.isoValue = iso
    mp.normals = 1 if normals else 0
    if region is not None:
        mp.lo = (C.c_uint32 * 3)(*region[0])
        mp.hi = (C.c_uint32 * 3)(*region[1])
    n = lib().mesh_extract(C.byref(sc), C.byref(mp), None, None, None, None, 0)
    if n < 0:
        raise ValueError("mesh_extract refuses the arguments")
    pos = np.zeros((n, 3, 3), dtype=np.float32)
    nrm = np.zeros((n, 3, 3), dtype=np.float32) if normals else None
    dirs = np.zeros((n, 3), dtype=np.float64) if debug else None
    cubes = np.zeros((n, 3), dtype=np.uint32) if debug else None
    got = lib().mesh_extract(C.byref(sc), C.byref(mp), pos.ctypes.data, nrm.ctypes.data if normals else None,
                             dirs.ctypes.data if debug else None, cubes.ctypes.data if debug else None, n)
    assert got == n
    return (pos, nrm, dirs, cubes) if debug else (pos, nrm)
