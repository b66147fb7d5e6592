"""ctypes loader of tests/ref/slice_ref.c, the scalar CPU restatement of the slice views (vrhip_render_slices).
TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of oracle/Makefile (no fp
contraction), next to its source, and rebuilt when the source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from .mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "slice_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libsliceref.so")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
MAX, MIN, MEAN = 0, 1, 2
TF, VALUE = 0, 1


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("tff", C.c_void_p), ("tff_n", C.c_uint32)]


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
        L.slice_fetch.restype = C.c_float
        L.slice_fetch.argtypes = [C.POINTER(Scene), C.c_int, C.c_float, C.c_float, C.c_float]
        L.slice_tff_linear.restype = None
        L.slice_tff_linear.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
        L.slice_pixel.restype = None
        L.slice_pixel.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.slice_render_tile.restype = C.c_int
        L.slice_render_tile.argtypes = [C.POINTER(Scene), C.c_void_p, C.c_int, C.c_void_p] + [C.c_uint32] * 6 + \
                                       [C.c_void_p] * 3
        _lib = L
    return _lib


def _tff(tff):
    return np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1)


def _scene(vol, fmt, tff):
    """(Scene, the arrays it points into)."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    keep = [vol]
    if tff is not None:
        tff = _tff(tff)
        sc.tff = tff.ctypes.data
        sc.tff_n = tff.size // 4
        keep.append(tff)
    return sc, keep


def fetch(vol, fmt, linear, tex):
    """The restatement's fetch at every texture coordinate tex[i] = (x, y, z) (float32 [n, 3]): float32 [n]."""
    sc, keep = _scene(vol, fmt, None)
    tex = np.ascontiguousarray(tex, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(tex.shape[0], dtype=np.float32)
    f = lib().slice_fetch
    for i in range(tex.shape[0]):
        out[i] = f(C.byref(sc), 1 if linear else 0, C.c_float(tex[i, 0]), C.c_float(tex[i, 1]), C.c_float(tex[i, 2]))
    return out


def tff_linear(tff, x):
    """The restatement's transfer-function read at every x (float32 array): float32 [n, 4]."""
    tff = _tff(tff)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    out = np.zeros((x.size, 4), dtype=np.float32)
    f = lib().slice_tff_linear
    for i in range(x.size):
        f(tff.ctypes.data, tff.size // 4, C.c_float(x[i]), out[i].ctypes.data)
    return out


def pixel(tff, val, taken, output, bg):
    """The restatement's pixel for every reduced value val[i] (taken[i]: a sample was taken) over bg: float32 [n, 4]."""
    tff = _tff(tff)
    val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1)
    taken = np.broadcast_to(np.asarray(taken, dtype=bool), val.shape)
    bg = np.ascontiguousarray(bg, dtype=np.float32).reshape(4)
    out = np.zeros((val.size, 4), dtype=np.float32)
    f = lib().slice_pixel
    for i in range(val.size):
        f(tff.ctypes.data, tff.size // 4, C.c_float(val[i]), int(taken[i]), int(output), bg.ctypes.data, out[i].ctypes.data)
    return out


def render(vol, fmt, tff, sp, linear, bg, W, H, tile=None):
    """One slice at W x H (tile (x0, y0, w, h) of it).  vol: ndarray [z, y, x] of the format's dtype; sp: a ctypes
    structure with the layout of vrhip_slice_params; tff: RGBA8 table or None (VALUE output only).
    Returns (rgba float32 [h, w, 4], reduced values float32 [h, w], samples taken uint32 [h, w])."""
    sc, keep = _scene(vol, fmt, tff)
    assert C.sizeof(sp) == 80
    bg = np.ascontiguousarray(bg, dtype=np.float32).reshape(4)
    x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
    rgba = np.zeros((h, w, 4), dtype=np.float32)
    val = np.zeros((h, w), dtype=np.float32)
    count = np.zeros((h, w), dtype=np.uint32)
    r = lib().slice_render_tile(C.byref(sc), C.addressof(sp), 1 if linear else 0, bg.ctypes.data, W, H, x0, y0, w, h,
                                rgba.ctypes.data, val.ctypes.data, count.ctypes.data)
    if r != 0:
        raise RuntimeError("slice_render_tile failed: %d" % r)
    return rgba, val, count


def render_all(vol, fmt, tff, slices, linear, bg, W, H):
    """Every slice of `slices`: float32 [n, H, W, 4], what vrhip_render_slices writes."""
    return np.stack([render(vol, fmt, tff, sp, linear, bg, W, H)[0] for sp in slices])
