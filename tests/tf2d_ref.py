"""ctypes loader of tests/ref/tf2d_ref.c, the scalar CPU restatement of technique 6 (ray casting through a 2-D
transfer function).  TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of
oracle/Makefile (no fp contraction), next to its source, linked to the oracle's library (vro_powr), and rebuilt when
the source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import vro
from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "ref", "tf2d_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libtf2dref.so")
_ORACLE_DIR = os.path.join(_ROOT, "oracle", "_build")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
MISS, MARCHED = 0, 1


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("table", C.c_void_p), ("n_v", C.c_uint32), ("n_g", C.c_uint32), ("g_hi", C.c_float)]


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
        L.tf2d_render_tile.restype = C.c_int
        L.tf2d_render_tile.argtypes = [C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + \
                                      [C.c_void_p] * 5
        L.tf2d_lookup.restype = None
        L.tf2d_lookup.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                  C.POINTER(C.c_float)]
        _lib = L
    return _lib


def _table(table):
    table = np.ascontiguousarray(table, dtype=np.uint8)
    assert table.ndim == 3 and table.shape[2] == 4
    return table


def lookup(table, g_hi, s, m):
    """The restatement's lookup of table [n_g, n_v, 4] at (s, m): float32 [4]."""
    table = _table(table)
    out = (C.c_float * 4)()
    lib().tf2d_lookup(table.ctypes.data, table.shape[1], table.shape[0], float(g_hi), float(s), float(m), out)
    return np.array(out[:], dtype=np.float32)


def render_tile(vol, fmt, table, g_hi, cam, rp, rc, W=64, H=64, tile=None):
    """Tile (x0, y0, w, h) of the W x H frame.  vol: ndarray [z, y, x] of the format's dtype; table: uint8
    [n_g, n_v, 4]; cam, rp, rc: ctypes structures with the layout of vrhip_camera_params / _rendering_params /
    _raycast_params.  Returns (rgba float32 [h, w, 4], kind uint8 [h, w] (MISS / MARCHED), and per pixel, uint32
    [h, w]: the samples taken, those of them with c.a != 0, those that read a column of the table which is not
    transparent in every row)."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    table = _table(table)
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    sc.table = table.ctypes.data
    sc.n_v, sc.n_g = table.shape[1], table.shape[0]
    sc.g_hi = g_hi
    x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
    rgba = np.zeros((h, w, 4), dtype=np.float32)
    kind = np.zeros((h, w), dtype=np.uint8)
    samples = np.zeros((h, w), dtype=np.uint32)
    visible = np.zeros((h, w), dtype=np.uint32)
    marginal = np.zeros((h, w), dtype=np.uint32)
    assert C.sizeof(cam) == 128 and C.sizeof(rp) == 64 and C.sizeof(rc) == 32
    r = lib().tf2d_render_tile(C.byref(sc), C.addressof(cam), C.addressof(rp), C.addressof(rc), W, H, x0, y0, w, h,
                               rgba.ctypes.data, kind.ctypes.data, samples.ctypes.data, visible.ctypes.data,
                               marginal.ctypes.data)
    if r != 0:
        raise RuntimeError("tf2d_render_tile failed: %d" % r)
    return rgba, kind, samples, visible, marginal
