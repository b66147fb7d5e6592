"""Pins tests/ref/filter_ref.c, the scalar restatement of the volume filters, on the CPU: against a numpy-float32
formulation of the three passes with explicit operation order and clamped index arrays, against np.sort of the 27
clamp-gathered neighbours, the identity round trip of every UCHAR and USHORT value, the premises of the two skip rules
and the Gaussian tap helper."""
import numpy as np
import pytest

from tests import filter_ref as fr

F32 = np.float32
FMTS = (fr.UCHAR, fr.USHORT, fr.FLOAT)
FMT_MAX = {fr.UCHAR: 255, fr.USHORT: 65535}


def _volume(fmt, shape, seed, special=False):
    rng = np.random.default_rng(seed)
    if fmt == fr.FLOAT:
        v = rng.uniform(-1.5, 2.5, shape).astype(F32)
        if special:
            flat = v.reshape(-1)
            idx = rng.choice(flat.size, 12, replace=False)
            flat[idx[:3]] = np.nan
            flat[idx[3:5]] = np.inf
            flat[idx[5:7]] = -np.inf
            flat[idx[7:10]] = -0.0
            flat[idx[10:]] = 0.0
        return v
    return rng.integers(0, FMT_MAX[fmt] + 1, shape).astype(fr.NP_DTYPE[fmt])


def _taps(rng, radius):
    return [rng.uniform(-0.6, 0.8, r + 1).astype(F32) for r in radius]


def _np_pass(f, axis, R, w):
    """One pass on the float32 field f [z, y, x] along x (axis 0), y (1) or z (2): every operation a float32 numpy
    operation of its own, in the contract's order; neighbours through clamped index arrays."""
    ax = 2 - axis
    n = f.shape[ax]
    idx = np.arange(n)
    acc = F32(w[0]) * f
    for k in range(1, R + 1):
        lo = np.take(f, np.clip(idx - k, 0, n - 1), axis=ax)
        hi = np.take(f, np.clip(idx + k, 0, n - 1), axis=ax)
        acc = acc + F32(w[k]) * (lo + hi)
    assert acc.dtype == F32
    return acc


def _np_separable(vol, fmt, radius, taps):
    with np.errstate(all="ignore"):
        if fmt == fr.FLOAT:
            s = vol.astype(F32)
        else:
            s = vol.astype(F32) * (F32(1.0) / F32(FMT_MAX[fmt]))
        c = s
        for a in range(3):
            c = _np_pass(c, a, radius[a], taps[a])
        if fmt == fr.FLOAT:
            bits = c.view(np.uint32).copy()
            bits[np.isnan(c)] = 0x7fc00000
            bits[c == 0] = 0
            return bits.view(F32)
        mx = F32(FMT_MAX[fmt])
        q = c * mx
        q = np.where(q > 0, q, F32(0))
        q = np.where(q < mx, q, mx)
        return np.rint(q).astype(fr.NP_DTYPE[fmt])   # (round half to even)


def _same(a, b, fmt):
    if fmt == fr.FLOAT:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape,radius", [((7, 11, 13), (2, 1, 3)), ((5, 9, 3), (8, 8, 8)), ((9, 5, 15), (0, 4, 0)),
                                          ((3, 3, 3), (0, 0, 0))])
def test_separable_matches_the_numpy_float32_formulation(fmt, shape, radius):
    rng = np.random.default_rng(hash((fmt, shape)) & 0xffff)
    vol = _volume(fmt, shape, 11 + fmt, special=True)
    taps = _taps(rng, radius)
    got = fr.compute(vol, fmt, fr.SEPARABLE, radius, taps)
    assert _same(got, _np_separable(vol, fmt, radius, taps), fmt)
    if radius != (0, 0, 0):
        assert not _same(got, vol, fmt)


def _keys(bits):
    bits = bits.astype(np.uint32)
    nan = (bits & 0x7fffffff) > 0x7f800000
    k = np.where(bits & 0x80000000, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = 0xffffffff
    return k


def _np_median(vol, fmt):
    src = _keys(vol.view(np.uint32)) if fmt == fr.FLOAT else vol.astype(np.uint32)
    d, h, w = src.shape
    zi, yi, xi = np.arange(d), np.arange(h), np.arange(w)
    stack = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                stack.append(src[np.clip(zi + dz, 0, d - 1)][:, np.clip(yi + dy, 0, h - 1)][:, :, np.clip(xi + dx, 0, w - 1)])
    med = np.sort(np.stack(stack), axis=0)[13]
    if fmt != fr.FLOAT:
        return med.astype(fr.NP_DTYPE[fmt])
    bits = np.where(med & 0x80000000, med ^ np.uint32(0x80000000), ~med).astype(np.uint32)
    bits[med == 0xffffffff] = 0x7fc00000
    bits[bits == 0x80000000] = 0
    return bits.view(F32)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", [(7, 11, 13), (1, 9, 2), (4, 4, 4)])
def test_median_matches_np_sort(fmt, shape):
    vol = _volume(fmt, shape, 5 + fmt, special=True)
    got = fr.compute(vol, fmt, fr.MEDIAN3)
    assert _same(got, _np_median(vol, fmt), fmt)


def test_median_key_order_of_special_floats():
    # in key order: -inf < -1 < -0 < +0 < 1 < +inf < NaN (either sign)
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], F32)
    neg_nan = np.array([0xffc00001], np.uint32).view(F32)
    k = _keys(np.concatenate([vals, neg_nan]).view(np.uint32))
    assert (np.diff(k[:7].astype(np.int64)) > 0).all() and k[6] == k[7] == 0xffffffff
    # a row of 3 x 1 x 1 voxels: the neighbourhood of the middle voxel holds every voxel nine times
    for row, want in (((np.nan, 1.0, np.inf), np.inf), ((np.nan, np.nan, 1.0), np.nan), ((-0.0, -0.0, 1.0), 0.0),
                      ((-np.inf, -2.0, np.nan), -2.0)):
        got = fr.compute(np.array(row, F32).reshape(1, 1, 3), fr.FLOAT, fr.MEDIAN3)[0, 0, 1]
        if np.isnan(want):
            assert got.view(np.uint32) == 0x7fc00000
        else:
            assert got.view(np.uint32) == F32(want).view(np.uint32)   # (-0 leaves as +0)


@pytest.mark.parametrize("fmt", (fr.UCHAR, fr.USHORT))
def test_identity_taps_return_every_raw_value(fmt):
    n = FMT_MAX[fmt] + 1
    vol = np.arange(n, dtype=fr.NP_DTYPE[fmt]).reshape(1, n // 64, 64) if fmt == fr.USHORT else \
        np.arange(n, dtype=fr.NP_DTYPE[fmt]).reshape(1, 4, 64)
    got = fr.compute(vol, fmt, fr.SEPARABLE, (0, 0, 0), [[1.0], [1.0], [1.0]])
    assert np.array_equal(got, vol)


def test_identity_taps_on_floats_keep_the_words_but_canonical_ones():
    vol = _volume(fr.FLOAT, (3, 4, 5), 3, special=True)
    got = fr.compute(vol, fr.FLOAT, fr.SEPARABLE, (0, 0, 0), [[1.0], [1.0], [1.0]])
    want = vol.view(np.uint32).copy()
    want[np.isnan(vol)] = 0x7fc00000
    want[vol == 0] = 0
    assert np.array_equal(got.view(np.uint32), want)


@pytest.mark.parametrize("fmt", FMTS)
def test_skip_premises(fmt):
    rng = np.random.default_rng(1)
    # zeros in, zeros out, whatever the (finite, signed) taps: the separable skip
    zeros = np.zeros((5, 6, 7), fr.NP_DTYPE[fmt])
    if fmt == fr.FLOAT:
        zeros[::2] = -0.0
    got = fr.compute(zeros, fmt, fr.SEPARABLE, (8, 3, 1), _taps(rng, (8, 3, 1)))
    assert not got.view(np.uint32 if fmt == fr.FLOAT else got.dtype).any()
    # a constant neighbourhood has the constant as its median, raw value for raw value: the median skip
    for c in (0, 1, 77, 200):
        const = np.full((4, 5, 6), c, fr.NP_DTYPE[fmt]) if fmt != fr.FLOAT else np.full((4, 5, 6), c * 0.37 - 3.0, F32)
        assert _same(fr.compute(const, fmt, fr.MEDIAN3), const, fmt)
    # ... while a constant is NOT a fixed point of normalised fp32 taps in general: other constants are fetched
    if fmt == fr.FLOAT:
        hits = 0
        for sigma in (0.7, 1.1, 1.9, 2.6):
            w = fr.gaussian_taps(sigma, 4)[:5]
            const = np.full((3, 3, 3), 0.3, F32)
            hits += not _same(fr.compute(const, fmt, fr.SEPARABLE, (4, 4, 4), [w, w, w]), const, fmt)
        assert hits > 0


def test_gaussian_taps():
    for sigma, radius in ((0.5, 1), (1.0, 3), (1.5, 4), (2.7, 8), (40.0, 8), (0.05, 2), (1.0, 0)):
        got = fr.gaussian_taps(sigma, radius)
        k = np.arange(radius + 1, dtype=np.float64)
        t = np.exp(-(k * k) / (2.0 * sigma * sigma))
        s = t[0]
        tail = 0.0
        for v in t[1:]:
            tail = tail + v
        want = (t / (s + 2.0 * tail)).astype(F32)
        assert got.size == 9 and (got[radius + 1:] == 0).all()
        # within one fp32 ulp of the float64 evaluation
        ulp = np.spacing(np.maximum(np.abs(want), np.finfo(F32).tiny).astype(F32))
        assert (np.abs(got[:radius + 1].astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (sigma, radius)
        # symmetric by construction (one weight for both sides); the full kernel sums to 1 within 2^-22
        full = float(got[0]) + 2.0 * float(np.sum(got[1:radius + 1].astype(np.float64)))
        assert abs(full - 1.0) <= 2.0 ** -22, (sigma, radius, full)
    with pytest.raises(ValueError):
        fr.gaussian_taps(0.0, 1)
    with pytest.raises(ValueError):
        fr.gaussian_taps(1.0, 9)


def test_refused_arguments():
    vol = np.zeros((2, 2, 2), np.uint8)
    with pytest.raises(ValueError):
        fr.compute(vol, fr.UCHAR, fr.SEPARABLE, (9, 0, 0), [[1.0] * 9] * 3)
    with pytest.raises(ValueError):
        fr.compute(vol, fr.UCHAR, fr.MEDIAN3, (1, 0, 0))
    with pytest.raises(ValueError):
        fr.compute(vol, fr.UCHAR, fr.SEPARABLE, (1, 0, 0), [[1.0, float("nan")], [1.0], [1.0]])
