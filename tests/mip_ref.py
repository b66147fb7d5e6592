"""ctypes loader of tests/ref/mip_ref.c, the scalar CPU restatement of technique 2 (maximum intensity
projection).  TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of
oracle/Makefile (no fp contraction), next to its source, and rebuilt when the source is newer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "ref", "mip_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libmipref.so")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
MISS, NO_SAMPLE, SAMPLED = 0, 1, 2


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("tff", C.c_void_p), ("tff_n", C.c_uint32)]


def oracle_cflags():
    """The flags oracle/Makefile compiles the oracle with."""
    text = open(os.path.join(_ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^CFLAGS\s*\?=\s*(.+)$", text, flags=re.M)
    assert m, "oracle/Makefile: no CFLAGS line"
    flags = m.group(1).split()
    assert "-ffp-contract=off" in flags
    return flags


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
        L.mip_tff_linear.restype = None
        L.mip_tff_linear.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
        L.mip_pixel.restype = None
        L.mip_pixel.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.mip_render_tile.restype = C.c_int
        L.mip_render_tile.argtypes = [C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + \
                                     [C.c_void_p] * 4
        _lib = L
    return _lib


def _tff(tff):
    return np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1)


def tff_linear(tff, x):
    """The restatement's transfer-function read at every x (float32 array): float32 [n, 4]."""
    tff = _tff(tff)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    out = np.zeros((x.size, 4), dtype=np.float32)
    f = lib().mip_tff_linear
    for i in range(x.size):
        f(tff.ctypes.data, tff.size // 4, C.c_float(x[i]), out[i].ctypes.data)
    return out


def pixel(tff, m, sampled, bg):
    """The restatement's pixel for every maximum m[i] (sampled[i]: the ray took a sample) over bg: float32 [n, 4]."""
    tff = _tff(tff)
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    sampled = np.broadcast_to(np.asarray(sampled, dtype=bool), m.shape)
    bg = np.ascontiguousarray(bg, dtype=np.float32).reshape(4)
    out = np.zeros((m.size, 4), dtype=np.float32)
    f = lib().mip_pixel
    for i in range(m.size):
        f(tff.ctypes.data, tff.size // 4, C.c_float(m[i]), int(sampled[i]), bg.ctypes.data, out[i].ctypes.data)
    return out


def render_tile(vol, fmt, tff, cam, rp, rc, W=64, H=64, tile=None):
    """Tile (x0, y0, w, h) of the W x H frame.  vol: ndarray [z, y, x] of the format's dtype; cam, rp, rc: ctypes
    structures with the layout of vrhip_camera_params / _rendering_params / _raycast_params.
    Returns (rgba float32 [h, w, 4], m float32 [h, w], kind uint8 [h, w] (MISS / NO_SAMPLE / SAMPLED),
    sample counts uint32 [h, w])."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    tff = _tff(tff)
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    sc.tff = tff.ctypes.data
    sc.tff_n = tff.size // 4
    x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
    rgba = np.zeros((h, w, 4), dtype=np.float32)
    m = np.zeros((h, w), dtype=np.float32)
    kind = np.zeros((h, w), dtype=np.uint8)
    count = np.zeros((h, w), dtype=np.uint32)
    assert C.sizeof(cam) == 128 and C.sizeof(rp) == 64 and C.sizeof(rc) == 32
    r = lib().mip_render_tile(C.byref(sc), C.addressof(cam), C.addressof(rp), C.addressof(rc), W, H, x0, y0, w, h,
                              rgba.ctypes.data, m.ctypes.data, kind.ctypes.data, count.ctypes.data)
    if r != 0:
        raise RuntimeError("mip_render_tile failed: %d" % r)
    return rgba, m, kind, count
