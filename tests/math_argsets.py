"""Argument sets for the fp32 building blocks (vr_device_math.h, the TF reads of vr_sampling.h).

Shared by tests/test_gpu_device_math.py (device against oracle, bit for bit, every point) and
tests/test_oracle_math.py (oracle against float64, on D and N).  Everything is built from bit patterns,
deterministic and seeded.  A case is (op, tag, args, table): op a name of vro.MATH_OPS, tag one of
  "E"  every binade: zeros, denormals, infinities, NaNs,
  "D"  the domain the kernels reach, every k-th bit pattern with k prime,
  "N"  +-128 ulps around the branch constants of the source,
args uint32 [count, n_in] (floats as bit patterns), table an index into tables() or None.
"""
import functools

import numpy as np

U32 = np.uint32
F32 = np.float32
TARGET = 2_000_000          # points of D per function

# 1 / rate for the sampling rates the suite uses, and the specular exponent (volumeraycast.cl:290, :864)
POWR_RATES = (0.5, 0.7, 1.0, 1.5, 2.0, 3.1, 0)   # 0 stands for the specular exponent
POWR_Y = [F32(1) / F32(r) if r else F32(40) for r in POWR_RATES]
TABLE_SIZES = (1, 3, 255, 256, 257, 1024, 4096)   # vrhip_set_transfer_function accepts 1..4096
TWO_PI_F = F32(2.0 * float(F32(3.14159274101257)))   # vr_pathtrace.hip dir_phase_function


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32)


def flt(u):
    return np.ascontiguousarray(u, dtype=U32).view(F32)


def next_prime(n):
    n = max(int(n), 2)
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


def strided(lo, hi, target, salt=0):
    """Every k-th bit pattern of [lo, hi] (bit patterns of non-negative floats), k prime, ~target points,
    both ends included.  salt picks another prime."""
    k = next_prime((hi - lo) // target + 1 + salt)
    a = np.arange(lo, hi + 1, k, dtype=np.int64)
    return np.unique(np.concatenate([a, [hi]])).astype(U32)


def ulps_around(c, n=128):
    """bit patterns within n ulps of the float32 nearest c, walking through zero to the other sign"""
    b = int(bits(F32(c))[0])
    mag, neg = b & 0x7fffffff, bool(b >> 31)
    k = np.arange(mag - n, mag + n + 1, dtype=np.int64)       # signed magnitude, < 0: across zero
    out = np.where(k >= 0, k, -k) | (np.where((k >= 0) != neg, 0, 1) << 31)
    if mag < n:   # both zeros
        out = np.concatenate([out, [0, 0x80000000]])
    return np.unique(out[(out & 0x7fffffff) <= 0x7f800000]).astype(U32)


@functools.lru_cache(maxsize=None)
def E():
    """For each of the 256 exponent fields and both signs: the first 64 mantissas, the last 64, 192 random ones.
    Laid out [sign, exponent, 320]."""
    rng = np.random.default_rng(0xE)
    m = np.empty((2, 256, 320), dtype=np.uint32)
    m[..., :64] = np.arange(64)
    m[..., 64:128] = 0x7fffff - np.arange(64)
    m[..., 128:] = rng.integers(0, 1 << 23, size=(2, 256, 192))
    s = np.arange(2, dtype=np.uint32)[:, None, None] << 31
    e = np.arange(256, dtype=np.uint32)[None, :, None] << 23
    out = (s | e | m).reshape(-1).astype(U32)
    out.setflags(write=False)
    return out


def E_shuffled(seed):
    return np.random.default_rng(seed).permutation(E())


def uint_specials():
    p = 1 << np.arange(32, dtype=np.int64)
    v = np.concatenate([[0, 1], p, p - 1, p + 1, np.arange(0xffffff7f, 0x100000000, dtype=np.int64)])
    return np.unique(v[(v >= 0) & (v <= 0xffffffff)]).astype(U32)


def uint_strided(target=TARGET, salt=0):
    k = next_prime((1 << 32) // target + 1 + salt)
    return np.concatenate([np.arange(0, 1 << 32, k, dtype=np.int64).astype(U32), uint_specials()])


def map_uint_float(v):
    """v / 2^32 rounded once to fp32 (random.cl:44-47 with (float)UINT_MAX == 2^32)"""
    return (np.asarray(v, dtype=np.float64) / 4294967296.0).astype(F32)


ONE = 0x3f800000


def unit_dense(target, salt=0):
    """[0, 1], every k-th bit pattern"""
    return strided(0, ONE, target, salt)


def col(*arrays):
    return np.ascontiguousarray(np.stack([np.asarray(a, dtype=U32) for a in arrays], axis=1))


def with_const(a, c):
    return col(a, np.full(len(a), bits(F32(c))[0], dtype=U32))


# ----------------------------------------------------------------------------------------------- tables

@functools.lru_cache(maxsize=None)
def tables():
    """[(tff uint8 [n, 4], prefix uint32 [n])]: seeded random RGBA8 with runs of zero opacity, so that the
    skip test takes both outcomes; the prefix sum is the inclusive sum of the alpha bytes."""
    out = []
    for n in TABLE_SIZES:
        rng = np.random.default_rng(1000 + n)
        t = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
        run = max(n // 8, 1)
        zero = ((np.arange(n) // run) % 2) == 0      # alternate runs: zero opacity, random opacity
        t[zero, 3] = 0
        prefix = np.cumsum(t[:, 3].astype(np.uint64)).astype(U32)
        t.setflags(write=False)
        prefix.setflags(write=False)
        out.append((t, prefix))
    return out


def tf_neighbourhoods(n):
    """+-64 ulps around every i / n and (i + 1/2) / n (sizes <= 257; a few i for the larger ones)"""
    idx = np.arange(n + 1) if n <= 257 else np.array([0, 1, n // 2, n - 1, n])
    pts = np.concatenate([idx / n, (idx[:-1] + 0.5) / n if n <= 257 else (idx + 0.5) / n])
    return np.unique(np.concatenate([ulps_around(p, 64) for p in pts]))


# ------------------------------------------------------------------------------------------------ cases

def _logf():
    yield "D", strided(1, ONE, TARGET)
    v = uint_strided()
    yield "D", bits(F32(1) - map_uint_float(v))          # log(1 - u) of the free-path length
    k = [0.70710678 * 2.0 ** k for k in range(-3, 2)] + [2.0 ** -126, 1.0]
    yield "N", np.concatenate([ulps_around(c) for c in k])
    yield "E", E()


def _sincosf():
    yield "D", strided(0, int(bits(F32(2 * np.pi))[0]), TARGET)
    yield "D", bits(TWO_PI_F * map_uint_float(uint_strided()))     # phi of the phase function
    k = [(j + 0.5) * np.pi / 2 for j in range(5)] + [0.0, 2 * np.pi]
    yield "N", np.concatenate([ulps_around(c) for c in k])
    yield "E", E()


def _acosf():
    pos = strided(0, ONE, TARGET // 2)
    yield "D", np.concatenate([pos, pos | U32(0x80000000)])
    yield "N", np.concatenate([ulps_around(c) for c in (0.5, -0.5, 1.0, -1.0, 0.0)])
    yield "E", E()


def _powr():
    for j, y in enumerate(POWR_Y):
        yield "D", with_const(unit_dense(TARGET // len(POWR_Y), salt=j), y)
        # the x at which y * log(x) crosses -87 (below 2^-149 for the small y: then the smallest denormals)
        x0 = np.exp(-87.0 / float(y))
        n = [ulps_around(x0) if x0 > 1e-44 else np.arange(0, 257, dtype=U32), ulps_around(1.0)]
        yield "N", with_const(np.concatenate(n), y)
        yield "E", with_const(E(), y)


def _atan2f():
    rng = np.random.default_rng(0xA2)
    d = rng.standard_normal((1_000_000, 3)).astype(F32)
    d = d * (F32(1) / np.sqrt((d * d).sum(axis=1, dtype=F32)))[:, None]
    yield "D", col(bits(d[:, 2]), bits(d[:, 0]))                   # (dir.z, dir.x)
    g = E()[::80]                                                  # 2048 values: 4 of every binade and sign
    assert g.size == 2048
    yield "E", col(np.repeat(g, 2048), np.tile(g, 2048))
    for c in (2.41421356, 0.41421356):                             # vr_atan_pos's switches, as y / x
        for x in (1.0, 3.0, -1.0, -3.0):
            y = ulps_around(float(F32(c)) * abs(x))
            yield "N", with_const(np.concatenate([y, y | U32(0x80000000)]), x)


@functools.lru_cache(maxsize=None)
def vectors():
    rng = np.random.default_rng(0x3D)
    n = 1_000_000
    e = rng.integers(127 - 20, 127 + 21, size=(n, 3)).astype(U32)
    v = (rng.integers(0, 2, size=(n, 3)).astype(U32) << 31) | (e << 23) | rng.integers(0, 1 << 23, size=(n, 3)).astype(U32)
    z = np.array([[a, b, c] for a in (0, 0x80000000) for b in (0, 0x80000000) for c in (0, 0x80000000)], dtype=U32)
    den = rng.integers(0, 1 << 23, size=(1024, 3)).astype(U32) | (rng.integers(0, 2, size=(1024, 3)).astype(U32) << 31)
    big = (rng.integers(127 + 60, 255, size=(1024, 3)).astype(U32) << 23) | rng.integers(0, 1 << 23, size=(1024, 3)).astype(U32)
    big |= rng.integers(0, 2, size=(1024, 3)).astype(U32) << 31
    every = col(E(), E_shuffled(1), E_shuffled(2))
    return v, np.concatenate([z, den, big]), every


def _vec3():
    v, edge, every = vectors()
    yield "D", v
    yield "N", edge
    yield "E", every


def _dot3():
    v, edge, every = vectors()
    yield "D", np.concatenate([v, v[::-1]], axis=1)
    yield "N", np.concatenate([edge, edge[::-1]], axis=1)
    yield "E", np.concatenate([every, col(E_shuffled(3), E_shuffled(4), E_shuffled(5))], axis=1)


SPECIAL = np.array([0, 0x80000000, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
                    0x7f800001, 0xff800001, 0x00000001, 0x80000001, 0x7f7fffff, 0xff7fffff, 0x3f000000], dtype=U32)


def _cmp2():
    a, b = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")     # NaN in either position, +-0 against -+0
    yield "N", col(a.ravel(), b.ravel())
    yield "E", col(E(), E_shuffled(6))


def _cmp3():
    a, b, c = np.meshgrid(SPECIAL, SPECIAL, SPECIAL, indexing="ij")
    yield "N", col(a.ravel(), b.ravel(), c.ravel())
    yield "E", col(E(), E_shuffled(7), E_shuffled(8))


def _lerpf():
    rng = np.random.default_rng(0x1E)
    n = 1 << 18
    p = (rng.integers(0, 256, size=n).astype(F32) / F32(255))
    q = (rng.integers(0, 256, size=n).astype(F32) / F32(255))
    yield "D", col(bits(p), bits(q), bits(rng.random(n, dtype=F32)))
    yield "E", col(E(), E_shuffled(9), E_shuffled(10))


def _rng():
    yield "D", uint_strided()


def _rng3():
    rng = np.random.default_rng(0x33)
    yield "D", rng.integers(0, 1 << 32, size=(1 << 20, 3), dtype=np.uint64).astype(U32)
    gx, gy, seed = np.meshgrid(np.arange(64), np.arange(64), [0, 1, 2, 0xffffffff], indexing="ij")
    yield "N", col(gx.ravel(), gy.ravel(), seed.ravel())          # pixels and seeds as make_ray passes them


def _map_uint_float():
    yield "D", uint_strided()


def _tf_plain(ti, n):
    yield "D", unit_dense(TARGET // len(TABLE_SIZES), salt=ti)
    yield "N", tf_neighbourhoods(n)


def _tf_raw(ti, n):
    yield from _tf_plain(ti, n)
    yield "E", E()


def _skip(ti, n):
    rng = np.random.default_rng(0x5C + ti)
    for tag, x in _tf_raw(ti, n):
        mx = flt(x)
        other = rng.permutation(mx)
        with np.errstate(invalid="ignore"):
            near = (mx - rng.random(mx.size, dtype=F32) * F32(2.0 / n)).astype(F32)   # often inside one run
            lo, hi = np.minimum(mx, other), np.maximum(mx, other)
        yield tag, np.concatenate([col(bits(near), x), col(bits(lo), bits(hi)), col(bits(other), x)])


def cases(ops=None):
    """Yields (op, tag, args uint32 [count, n_in], table index or None)."""
    plain = {"logf": _logf, "sincosf": _sincosf, "acosf": _acosf, "powr": _powr, "atan2f": _atan2f,
             "normalize3": _vec3, "len3": _vec3, "dot3": _dot3, "vmin": _cmp2, "vmax": _cmp2, "vclamp": _cmp3,
             "lerpf": _lerpf, "rng": _rng, "rng3": _rng3, "map_uint_float": _map_uint_float}
    table = {"tff_linear": _tf_plain, "tff_alpha": _tf_plain, "tff_linear_raw": _tf_raw, "tff_alpha_raw": _tf_raw,
             "prefix_nearest": _tf_raw, "skip_test": _skip}
    for op, gen in plain.items():
        if ops is None or op in ops:
            for tag, a in gen():
                a = np.ascontiguousarray(a, dtype=U32)
                yield op, tag, a.reshape(len(a), -1), None
    for op, gen in table.items():
        if ops is None or op in ops:
            for ti, n in enumerate(TABLE_SIZES):
                for tag, a in gen(ti, n):
                    a = np.ascontiguousarray(a, dtype=U32)
                    yield op, tag, a.reshape(len(a), -1), ti
