"""ctypes loader of tests/ref/preint_ref.c, the scalar CPU restatement of technique 8 (ray casting with
pre-integrated classification).  TEST INFRASTRUCTURE ONLY.  The library is compiled on first use with the CFLAGS line of
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
_SRC = os.path.join(_HERE, "ref", "preint_ref.c")
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libpreintref.so")
_ORACLE_DIR = os.path.join(_ROOT, "oracle", "_build")

UCHAR, USHORT, FLOAT = 0, 1, 2
_NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
MISS, MARCHED = 0, 1


class Scene(C.Structure):
    _fields_ = [("voxels", C.c_void_p), ("res", C.c_uint32 * 3), ("format", C.c_int32),
                ("tff", C.c_void_p), ("n", C.c_uint32)]


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
        L.pre_render_tile.restype = C.c_int
        L.pre_render_tile.argtypes = [C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + \
                                     [C.c_void_p] * 7 + [C.c_uint32]
        L.pre_slab.restype = C.c_int
        L.pre_slab.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float)]
        L.pre_tff_linear.restype = None
        L.pre_tff_linear.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.POINTER(C.c_float)]
        _lib = L
    return _lib


def entries(tff):
    """The table as the renderer holds it: uint8 [n, 4] -> float32 [n, 4], c / 255.0f."""
    tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1, 4)
    return (tff.astype(np.float32) / np.float32(255.0)).astype(np.float32)


def slab(E, sf, sb, raw=False):
    """The restatement's classification of the slab between the values sf and sb with the float32 [n, 4] entries E:
    float32 (Cbar.rgb, abar)."""
    E = np.ascontiguousarray(E, dtype=np.float32)
    out = (C.c_float * 4)()
    r = lib().pre_slab(E.ctypes.data, E.shape[0], 1 if raw else 0, float(sf), float(sb), out)
    assert r == 0
    return np.array(out[:], dtype=np.float32)


def tff_linear(E, x, raw=False):
    """The ray caster's transfer-function read (tff_linear) of the float32 [n, 4] entries E at x."""
    E = np.ascontiguousarray(E, dtype=np.float32)
    out = (C.c_float * 4)()
    lib().pre_tff_linear(E.ctypes.data, E.shape[0], 1 if raw else 0, float(x), out)
    return np.array(out[:], dtype=np.float32)


def render_tile(vol, fmt, tff, cam, rp, rc, W=64, H=64, tile=None, max_values=0, positions=False):
    """Tile (x0, y0, w, h) of the W x H frame.  vol: ndarray [z, y, x] of the format's dtype; tff: uint8 [n, 4]; cam,
    rp, rc: ctypes structures with the layout of vrhip_camera_params / _rendering_params / _raycast_params.  Returns
    (rgba float32 [h, w, 4], kind uint8 [h, w] (MISS / MARCHED), and per pixel, uint32 [h, w]: the samples taken, the
    slabs with abar != 0, the slabs that can read an entry which is not transparent; with max_values > 0 also float32
    [h, w, max_values], the first sample values of every ray (NaN-filled beyond the ray's samples); with positions also
    float32 [h, w, max_values, 3], their texture coordinates (x, y, z) in [0, 1])."""
    vol = np.ascontiguousarray(vol, dtype=_NP_DTYPE[fmt])
    assert vol.ndim == 3
    tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1, 4)
    sc = Scene()
    sc.voxels = vol.ctypes.data
    sc.res = (C.c_uint32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
    sc.format = fmt
    sc.tff = tff.ctypes.data
    sc.n = tff.shape[0]
    x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
    rgba = np.zeros((h, w, 4), dtype=np.float32)
    kind = np.zeros((h, w), dtype=np.uint8)
    samples = np.zeros((h, w), dtype=np.uint32)
    visible = np.zeros((h, w), dtype=np.uint32)
    marginal = np.zeros((h, w), dtype=np.uint32)
    values = np.full((h, w, max(1, max_values)), np.nan, dtype=np.float32)
    pos = np.full((h, w, max(1, max_values), 3), np.nan, dtype=np.float32)
    assert C.sizeof(cam) == 128 and C.sizeof(rp) == 64 and C.sizeof(rc) == 32
    r = lib().pre_render_tile(C.byref(sc), C.addressof(cam), C.addressof(rp), C.addressof(rc), W, H, x0, y0, w, h,
                              rgba.ctypes.data, kind.ctypes.data, samples.ctypes.data, visible.ctypes.data,
                              marginal.ctypes.data, values.ctypes.data if max_values else None,
                              pos.ctypes.data if max_values and positions else None, max_values)
    if r != 0:
        raise RuntimeError("pre_render_tile failed: %d" % r)
    if max_values and positions:
        return rgba, kind, samples, visible, marginal, values, pos
    if max_values:
        return rgba, kind, samples, visible, marginal, values
    return rgba, kind, samples, visible, marginal
