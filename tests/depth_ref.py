"""ctypes loader of tests/ref/depth_ref.c, the scalar CPU restatement of the depth images (vrhip_render_depth).
TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of oracle/Makefile (no fp
contraction), next to its source, linked to the oracle's library (vro_powr, vro_tff_linear), and rebuilt when the
source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import vro
from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "ref", "depth_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libdepthref.so")
_ORACLE_DIR = os.path.join(_ROOT, "oracle", "_build")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
ISO, MAX, OPACITY = 0, 1, 2
MISS, NO_HIT, HIT = 0, 1, 2

# depth_ray: cam[3], dir[3], tnear (clamped to >= 0: t_0), tfar, stepSize, offset
RAY_DTYPE = np.dtype([("cam", np.float32, 3), ("dir", np.float32, 3), ("tnear", np.float32), ("tfar", np.float32),
                      ("step", np.float32), ("offset", np.float32)])
assert RAY_DTYPE.itemsize == 40


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("tff", C.c_void_p), ("tff_n", C.c_uint32)]


class DepthParams(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("threshold", C.c_float), ("refineSteps", C.c_uint32), ("x0", C.c_uint32),
                ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("reserved", C.c_uint32)]


def build():
    vro.lib()   # (builds the oracle's library when it is missing)
    if os.path.exists(_LIB_PATH) and os.path.getmtime(_LIB_PATH) >= os.path.getmtime(_SRC):
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
        L.depth_render.restype = C.c_int
        L.depth_render.argtypes = [C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DepthParams),
                                   C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        _lib = L
    return _lib


def render(vol, fmt, tff, cam, rp, rc, mode, threshold=0.5, refine=4, W=64, H=64, rect=None, with_rays=False):
    """The rectangle rect = (x0, y0, w, h) -- None: the whole frame -- of the W x H frame.  vol: ndarray [z, y, x] of the
    format's dtype; tff: RGBA8 table or None (ISO, MAX); cam, rp, rc: ctypes structures with the layout of
    vrhip_camera_params / _rendering_params / _raycast_params.
    Returns (xyzt float32 [h, w, 4], aux float32 [h, w], kind uint8 [h, w]) and, with_rays, the rays as a RAY_DTYPE
    array [h, w] (valid where kind != MISS)."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    if tff is not None:
        tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1)
        sc.tff = tff.ctypes.data
        sc.tff_n = tff.size // 4
    dp = DepthParams()
    dp.mode, dp.threshold, dp.refineSteps = mode, threshold, refine
    if rect is not None:
        dp.x0, dp.y0, dp.w, dp.h = rect
    w, h = (rect[2], rect[3]) if rect is not None else (W, H)
    xyzt = np.zeros((h, w, 4), dtype=np.float32)
    aux = np.zeros((h, w), dtype=np.float32)
    kind = np.zeros((h, w), dtype=np.uint8)
    rays = np.zeros((h, w), dtype=RAY_DTYPE)
    assert C.sizeof(cam) == 128 and C.sizeof(rp) == 64 and C.sizeof(rc) == 32 and C.sizeof(dp) == 32
    r = lib().depth_render(C.byref(sc), C.addressof(cam), C.addressof(rp), C.addressof(rc), C.byref(dp), W, H,
                           xyzt.ctypes.data, aux.ctypes.data, kind.ctypes.data, rays.ctypes.data if with_rays else None)
    if r != 0:
        raise RuntimeError("depth_render failed: %d" % r)
    return (xyzt, aux, kind, rays) if with_rays else (xyzt, aux, kind)
