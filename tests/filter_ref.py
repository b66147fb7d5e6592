"""ctypes loader of tests/ref/filter_ref.c, the scalar CPU restatement of the volume filters (vrhip_filter_volume).
TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of oracle/Makefile (no fp
contraction), next to its source, and rebuilt when the source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "filter_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libfilterref.so")

UCHAR, USHORT, FLOAT = 0, 1, 2
NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
SEPARABLE, MEDIAN3 = 0, 1
MAX_RADIUS = 8


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32)]


class FilterParams(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("radius", C.c_uint32 * 3), ("taps", (C.c_float * (MAX_RADIUS + 1)) * 3),
                ("reserved", C.c_uint32 * 4)]


assert C.sizeof(FilterParams) == 140


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
        L.filter_compute.restype = C.c_int
        L.filter_compute.argtypes = [C.POINTER(Scene), C.POINTER(FilterParams), C.c_void_p]
        L.filter_gaussian_taps.restype = C.c_int
        L.filter_gaussian_taps.argtypes = [C.c_double, C.c_uint32, C.POINTER(C.c_float)]
        _lib = L
    return _lib


def params(kind=SEPARABLE, radius=(0, 0, 0), taps=None):
    """taps: three sequences of radius[a] + 1 weights (distance 0 first); entries beyond stay 0."""
    p = FilterParams()
    p.kind = kind
    p.radius[:] = [int(v) for v in radius]
    if taps is not None:
        for a in range(3):
            for k, w in enumerate(taps[a]):
                p.taps[a][k] = float(w)
    return p


def compute(vol, fmt, kind=SEPARABLE, radius=(0, 0, 0), taps=None):
    """The filtered volume (ndarray [z, y, x] of the format's dtype) of vol: the bytes are the contract's."""
    vol = np.ascontiguousarray(vol, dtype=NP_DTYPE[fmt])
    assert vol.ndim == 3
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    p = params(kind, radius, taps)
    out = np.empty_like(vol)
    if lib().filter_compute(C.byref(sc), C.byref(p), out.ctypes.data) != 0:
        raise ValueError("filter_compute refuses the arguments")
    return out


def gaussian_taps(sigma, radius):
    """float32 [9]: the restated vrhip_filter_gaussian_taps."""
    t = (C.c_float * (MAX_RADIUS + 1))()
    if lib().filter_gaussian_taps(float(sigma), int(radius), t) != 0:
        raise ValueError("filter_gaussian_taps refuses the arguments")
    return np.array(t[:], dtype=np.float32)
