"""ctypes loader of tests/ref/morph_ref.c, the scalar CPU restatement of the volume morphology (vrhip_morph_volume).
TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of oracle/Makefile (no fp
contraction), next to its source, and rebuilt when the source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "morph_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libmorphref.so")

UCHAR, USHORT, FLOAT = 0, 1, 2
NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
ERODE, DILATE, OPEN, CLOSE, GRADIENT, TOPHAT, BLACKHAT = range(7)
OP_NAMES = ["erode", "dilate", "open", "close", "gradient", "tophat", "blackhat"]
BOX, BALL = 0, 1
SHAPE_NAMES = ["box", "ball"]
MAX_RADIUS = 8


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32)]


class MorphParams(C.Structure):
    _fields_ = [("op", C.c_uint32), ("shape", C.c_uint32), ("radius", C.c_uint32 * 3), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(MorphParams) == 32


def build():
    if os.path.exists(_LIB_PATH) and os.path.getmtime(_LIB_PATH) >= os.path.getmtime(_SRC):
        return
    os.makedirs(os.path.dirname(_LIB_PATH), exist_ok=True)
    tmp = "%s.%d.tmp" % (_LIB_PATH, os.getpid())
    subprocess.check_call([os.environ.get("CC", "gcc")] + oracle_cflags() + ["-shared", "-o", tmp, _SRC, "-lm"])
    os.replace(tmp, _LIB_PATH)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB_PATH)
        L.morph_compute.restype = C.c_int
        L.morph_compute.argtypes = [C.POINTER(Scene), C.POINTER(MorphParams), C.c_void_p, C.c_int]
        L.morph_element.restype = C.c_uint32
        L.morph_element.argtypes = [C.POINTER(MorphParams), C.POINTER(C.c_int8), C.c_uint32]
        _lib = L
    return _lib


def params(op=ERODE, shape=BALL, radius=(1, 1, 1)):
    p = MorphParams()
    p.op = op
    p.shape = shape
    p.radius[:] = [int(v) for v in radius]
    return p


def element(shape, radius):
    """int8 [n, 3]: the offsets (dx, dy, dz) of the structuring element, z, then y, then x ascending."""
    p = params(ERODE, shape, radius)
    n = lib().morph_element(C.byref(p), None, 0)
    out = np.zeros((n, 3), np.int8)
    assert lib().morph_element(C.byref(p), out.ctypes.data_as(C.POINTER(C.c_int8)), n) == n
    return out


def compute(vol, fmt, op, shape, radius, inside=False):
    """The result volume (ndarray [z, y, x] of the format's dtype) of the op on vol: the bytes are the contract's.
    inside: over the positions inside the volume instead of the clamped positions (the same set of voxels)."""
    vol = np.ascontiguousarray(vol, dtype=NP_DTYPE[fmt])
    assert vol.ndim == 3
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    p = params(op, shape, radius)
    out = np.empty_like(vol)
    if lib().morph_compute(C.byref(sc), C.byref(p), out.ctypes.data, 1 if inside else 0) != 0:
        raise ValueError("morph_compute refuses the arguments")
    return out
