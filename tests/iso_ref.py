"""ctypes loader of tests/ref/iso_ref.c, the scalar CPU restatement of technique 4 (first-hit isosurface
rendering).  TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of
oracle/Makefile (no fp contraction), next to its source, linked to the oracle's library (vro_powr, vro_tff_linear),
and rebuilt when the source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import vro
from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "ref", "iso_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libisoref.so")
_ORACLE_DIR = os.path.join(_ROOT, "oracle", "_build")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
MISS, NO_HIT, HIT = 0, 1, 2


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("tff", C.c_void_p), ("tff_n", C.c_uint32)]


class IsoParams(C.Structure):
    _fields_ = [("isoValue", C.c_float), ("refineSteps", C.c_uint32), ("reserved", C.c_uint32 * 2)]


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
        L.iso_render_tile.restype = C.c_int
        L.iso_render_tile.argtypes = [C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(IsoParams)] + \
                                     [C.c_uint32] * 6 + [C.c_void_p] * 5
        _lib = L
    return _lib


def render_tile(vol, fmt, tff, cam, rp, rc, iso_value=0.5, refine_steps=4, W=64, H=64, tile=None):
    """Tile (x0, y0, w, h) of the W x H frame.  vol: ndarray [z, y, x] of the format's dtype; cam, rp, rc: ctypes
    structures with the layout of vrhip_camera_params / _rendering_params / _raycast_params.
    Returns (rgba float32 [h, w, 4], kind uint8 [h, w] (MISS / NO_HIT / HIT), hit index k uint32 [h, w],
    t_hit float32 [h, w], march sample counts uint32 [h, w])."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1)
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    sc.tff = tff.ctypes.data
    sc.tff_n = tff.size // 4
    ip = IsoParams()
    ip.isoValue = iso_value
    ip.refineSteps = refine_steps
    x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
    rgba = np.zeros((h, w, 4), dtype=np.float32)
    kind = np.zeros((h, w), dtype=np.uint8)
    k = np.zeros((h, w), dtype=np.uint32)
    t_hit = np.zeros((h, w), dtype=np.float32)
    count = np.zeros((h, w), dtype=np.uint32)
    assert C.sizeof(cam) == 128 and C.sizeof(rp) == 64 and C.sizeof(rc) == 32 and C.sizeof(ip) == 16
    r = lib().iso_render_tile(C.byref(sc), C.addressof(cam), C.addressof(rp), C.addressof(rc), C.byref(ip), W, H,
                              x0, y0, w, h, rgba.ctypes.data, kind.ctypes.data, k.ctypes.data, t_hit.ctypes.data,
                              count.ctypes.data)
    if r != 0:
        raise RuntimeError("iso_render_tile failed: %d" % r)
    return rgba, kind, k, t_hit, count
