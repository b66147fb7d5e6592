"""ctypes loader of tests/ref/mesh_indexed_ref.c, the scalar CPU restatement of the indexed isosurface extraction
(vrhip_isosurface_count_indexed / vrhip_isosurface_extract_indexed).  TEST INFRASTRUCTURE ONLY.  Built like
tests/mesh_ref.py builds its library: the oracle's CFLAGS (no fp contraction), next to the source, rebuilt when a
source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import vro
from tests import mesh_ref
from tests.mesh_ref import FLOAT, UCHAR, USHORT, MeshParams, Scene  # noqa: F401
from tests.mip_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ref", "mesh_indexed_ref.c")
_DEPS = [_SRC, os.path.join(_HERE, "ref", "mesh_ref.c"), os.path.join(_HERE, "ref", "iso_ref.c")]
_LIB_PATH = os.path.join(_HERE, "ref", "_build", "libmeshindexedref.so")
_ORACLE_DIR = os.path.join(os.path.dirname(_HERE), "oracle", "_build")


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
        L.mesh_extract_indexed.restype = C.c_int
        L.mesh_extract_indexed.argtypes = ([C.POINTER(Scene), C.POINTER(MeshParams)] + [C.c_void_p] * 3 +
                                           [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)])
        _lib = L
    return _lib


def extract(vol, fmt, iso, normals=False, region=None):
    """The indexed mesh of vol (ndarray [z, y, x] of the format's dtype) at iso; region = (lo xyz, hi xyz) or None.
    Returns (vertices float32 [m, 3], normals float32 [m, 3] or None, indices uint32 [n, 3], point_blocks)."""
    vol = np.ascontiguousarray(vol, dtype=mesh_ref._NP_DTYPE[fmt])
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
    counts = (C.c_uint64 * 3)()
    if lib().mesh_extract_indexed(C.byref(sc), C.byref(mp), None, None, None, 0, 0, counts) != 0:
        raise ValueError("mesh_extract_indexed refuses the arguments")
    m, n, blocks = int(counts[0]), int(counts[1]), int(counts[2])
    vtx = np.zeros((m, 3), dtype=np.float32)
    nrm = np.zeros((m, 3), dtype=np.float32) if normals else None
    idx = np.zeros((n, 3), dtype=np.uint32)
    rc = lib().mesh_extract_indexed(C.byref(sc), C.byref(mp), vtx.ctypes.data, nrm.ctypes.data if normals else None,
                                    idx.ctypes.data, m, n, counts)
    assert rc == 0 and (int(counts[0]), int(counts[1]), int(counts[2])) == (m, n, blocks)
    return vtx, nrm, idx, blocks


# ---- the volumes tests/test_mesh_indexed_ref.py and tests/test_gpu_mesh_indexed.py share (tests/test_gpu_mesh.py's)

def quantise(f, fmt):
    if fmt == UCHAR:
        return np.round(f * 255).astype(np.uint8)
    if fmt == USHORT:
        return np.round(f * 65535).astype(np.uint16)
    return f.astype(np.float32)


def noise(res, fmt, seed=5):
    """Seeded noise, smoothed once along every axis: values in [0, 1] with structure down to a voxel, whatever the shape."""
    f = np.random.default_rng(seed).random((res[2] + 2, res[1] + 2, res[0] + 2))
    for ax in range(3):
        f = (np.take(f, range(0, f.shape[ax] - 2), ax) + np.take(f, range(1, f.shape[ax] - 1), ax) +
             np.take(f, range(2, f.shape[ax]), ax)) / 3.0
    return quantise(f.astype(np.float32), fmt)


def ball(n=40, fmt=UCHAR, centre=(19.3, 20.1, 19.6), radius=13.0):
    """1 at the centre, falling to exactly 0 at `radius` and beyond: whole cells of the grid are all 0, others all high."""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return quantise(np.clip(1.0 - d / radius, 0.0, 1.0).astype(np.float32), fmt)


def exact_iso_volume(res=(17, 10, 9), iso=0.5, seed=11):
    """FLOAT noise in which every fifth voxel that was near `iso` is exactly `iso`: t = 0 on all edges of such a point."""
    vol = noise(res, FLOAT, seed)
    near = np.abs(vol - np.float32(iso)) < 0.04
    pick = near & (np.arange(vol.size).reshape(vol.shape) % 5 == 0)
    vol[pick] = np.float32(iso)
    assert pick.sum() > 5
    return vol


def normalised(vol, fmt):
    """The grid's point values s = (float)raw * inv_max, in np.float32."""
    inv = {UCHAR: np.float32(1.0) / np.float32(255.0), USHORT: np.float32(1.0) / np.float32(65535.0), FLOAT: np.float32(1.0)}[fmt]
    with np.errstate(all="ignore"):
        return vol.astype(np.float32) * inv


def crossed_edges(vol, fmt, iso, region=None):
    """The number of eligible crossed lattice edges, counted apart from any extraction: seven shifted comparisons of
    the inside array, P over lo <= P < hi on an axis whose bit of d is set and over lo <= P <= hi on the others."""
    with np.errstate(all="ignore"):
        inside = normalised(vol, fmt) >= np.float32(iso)
    res = vol.shape[::-1]
    lo = list(region[0]) if region else [0, 0, 0]
    hi = [min(h, r - 1) for h, r in zip(region[1] if region else res, res)]
    if any(h <= l for l, h in zip(lo, hi)):
        return 0
    total = 0
    for d in range(1, 8):
        bits = [(d >> ax) & 1 for ax in range(3)]
        p = tuple(slice(lo[ax], hi[ax] + 1 - bits[ax]) for ax in (2, 1, 0))           # [z, y, x]
        q = tuple(slice(lo[ax] + bits[ax], hi[ax] + 1) for ax in (2, 1, 0))
        total += int((inside[p] != inside[q]).sum())
    return total
