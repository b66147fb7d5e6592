"""ctypes loader of tests/ref/stats_ref.c, the scalar CPU restatement of the volume statistics
(vrhip_volume_statistics).  TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of
oracle/Makefile (no fp contraction), next to its source, and rebuilt when the source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "stats_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libstatsref.so")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
BLOCK, SUM_CHUNK, MOMENTS = 8, 256, 1


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32)]


class StatsParams(C.Structure):
    _fields_ = [("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("bins_v", C.c_uint32), ("bins_g", C.c_uint32),
                ("v_lo", C.c_float), ("v_hi", C.c_float), ("g_hi", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class VolumeStats(C.Structure):
    _fields_ = [("voxels", C.c_uint64), ("nan", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64),
                ("gradient_nan", C.c_uint64), ("binned", C.c_uint64), ("min", C.c_float), ("max", C.c_float),
                ("sum", C.c_double), ("sum_sq", C.c_double)]


assert C.sizeof(StatsParams) == 64 and C.sizeof(VolumeStats) == 72


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
        L.stats_compute.restype = C.c_int
        L.stats_compute.argtypes = [C.POINTER(Scene), C.POINTER(StatsParams), C.POINTER(VolumeStats), C.c_void_p]
        _lib = L
    return _lib


def params(bins=(256, 1), window=(0.0, 1.0, 1.0), region=None, moments=False):
    p = StatsParams()
    p.bins_v, p.bins_g = bins
    p.v_lo, p.v_hi, p.g_hi = window
    p.flags = MOMENTS if moments else 0
    if region is not None:
        p.lo[:] = region[0]
        p.hi[:] = region[1]
    return p


def compute(vol, fmt, bins=(256, 1), window=(0.0, 1.0, 1.0), region=None, moments=False):
    """(VolumeStats, hist uint64 [bins_g, bins_v]) of vol (ndarray [z, y, x] of the format's dtype); region =
    (lo xyz, hi xyz) or None.  The bytes of both are the contract's."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    p = params(bins, window, region, moments)
    st = VolumeStats()
    hist = np.full((bins[1], bins[0]), 0xdead, dtype=np.uint64)
    if lib().stats_compute(C.byref(sc), C.byref(p), C.byref(st), hist.ctypes.data) != 0:
        raise ValueError("stats_compute refuses the arguments")
    return st, hist
