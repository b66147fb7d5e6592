"""Pins tests/ref/morph_ref.c, the CPU restatement of the volume morphology, on a GPU-less host: against an
independent numpy formulation (sliding windows over an edge-padded array of keys), against scipy.ndimage where it
imports, the clamped form against the inside-the-volume form, the element's counts and symmetry, the ordering erosion
<= open <= f <= close <= dilation, idempotence, BOX as three 1-D passes, and the FLOAT rules."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from tests import morph_ref as mr

F32 = np.float32
SHAPES = [(5, 7, 3), (13, 4, 9), (2, 1, 6)]             # (x, y, z)
RADII = [(1, 1, 1), (2, 0, 3), (8, 8, 8), (3, 1, 0), (4, 2, 1)]
FMTS = [mr.UCHAR, mr.USHORT, mr.FLOAT]


def _random(res, fmt, seed=1, special=False):
    rng = np.random.default_rng(seed)
    shape = (res[2], res[1], res[0])
    if fmt == mr.UCHAR:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if fmt == mr.USHORT:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    v = (rng.random(shape, dtype=F32) * 4.0 - 1.5).astype(F32)
    if special and v.size >= 12:
        flat = v.reshape(-1)
        idx = rng.choice(flat.size, 8, replace=False)
        flat[idx[0]] = np.nan
        flat[idx[1]] = np.array([0xffc00123], np.uint32).view(F32)[0]
        flat[idx[2]] = np.inf
        flat[idx[3]] = -np.inf
        flat[idx[4:6]] = -0.0
        flat[idx[6:]] = 0.0
    return v


def _keys(vol):
    """uint32 keys of a volume: the raw integer, or the order-preserving key of a float word."""
    if vol.dtype != F32:
        return vol.astype(np.uint32)
    bits = vol.view(np.uint32)
    key = np.where(bits & 0x80000000, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where((bits & 0x7fffffff) > 0x7f800000, np.uint32(0xffffffff), key)


def _unkeys(key, dtype):
    if dtype != F32:
        return key.astype(dtype)
    bits = np.where(key & 0x80000000, key ^ np.uint32(0x80000000), ~key).astype(np.uint32)
    bits = np.where(key == 0xffffffff, np.uint32(0x7fc00000), bits)
    return np.where(bits == 0x80000000, np.uint32(0), bits).astype(np.uint32).view(F32)


def _footprint(shape, radius):
    """bool [2 Rz + 1, 2 Ry + 1, 2 Rx + 1] from the header's inequality, written independently of the C code."""
    rx, ry, rz = radius
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    if shape == mr.BOX:
        return np.ones(dz.shape, bool)
    px, py, pz = max(rx, 1) ** 2, max(ry, 1) ** 2, max(rz, 1) ** 2
    return dx * dx * py * pz + dy * dy * px * pz + dz * dz * px * py <= px * py * pz


def _np_extreme(vol, shape, radius, is_max):
    rx, ry, rz = radius
    key = np.pad(_keys(vol), ((rz, rz), (ry, ry), (rx, rx)), mode="edge")
    win = sliding_window_view(key, (2 * rz + 1, 2 * ry + 1, 2 * rx + 1))
    sel = win[..., _footprint(shape, radius)]
    return _unkeys(sel.max(-1) if is_max else sel.min(-1), vol.dtype)


def _np_diff(a, b):
    """a - b by the contract's store: integers as they are; FLOAT one fp32 subtraction, a zero of either sign stored
    +0 and any NaN 0x7fc00000 (the special-value volumes give inf - inf, NaN operands and -0 results)."""
    if a.dtype != F32:
        return a - b
    with np.errstate(invalid="ignore"):
        c = (a - b).astype(F32)
    bits = c.view(np.uint32).copy()
    bits[np.isnan(c)] = 0x7fc00000
    bits[c == 0] = 0
    return bits.view(F32)


def _bits(a):
    return a.view(np.uint32) if a.dtype == F32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", [mr.BOX, mr.BALL])
def test_against_numpy_windows(fmt, shape):
    for res in SHAPES:
        vol = _random(res, fmt, seed=sum(res), special=True)
        for radius in RADII:
            e = _np_extreme(vol, shape, radius, False)
            d = _np_extreme(vol, shape, radius, True)
            assert _same(mr.compute(vol, fmt, mr.ERODE, shape, radius), e), (res, radius)
            assert _same(mr.compute(vol, fmt, mr.DILATE, shape, radius), d), (res, radius)
            assert _same(mr.compute(vol, fmt, mr.OPEN, shape, radius), _np_extreme(e, shape, radius, True)), (res, radius)
            assert _same(mr.compute(vol, fmt, mr.CLOSE, shape, radius), _np_extreme(d, shape, radius, False)), (res, radius)
            o, c = _np_extreme(e, shape, radius, True), _np_extreme(d, shape, radius, False)
            assert _same(mr.compute(vol, fmt, mr.GRADIENT, shape, radius), _np_diff(d, e)), (res, radius)
            assert _same(mr.compute(vol, fmt, mr.TOPHAT, shape, radius), _np_diff(vol, o)), (res, radius)
            assert _same(mr.compute(vol, fmt, mr.BLACKHAT, shape, radius), _np_diff(c, vol)), (res, radius)


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for fmt in (mr.UCHAR, mr.USHORT, mr.FLOAT):
        for res in SHAPES:
            vol = _random(res, fmt, seed=7)   # (finite values: scipy compares floats, not keys)
            for shape in (mr.BOX, mr.BALL):
                for radius in RADII:
                    fp = _footprint(shape, radius)
                    assert _same(mr.compute(vol, fmt, mr.ERODE, shape, radius), ndi.grey_erosion(vol, footprint=fp, mode="nearest"))
                    assert _same(mr.compute(vol, fmt, mr.DILATE, shape, radius), ndi.grey_dilation(vol, footprint=fp, mode="nearest"))


@pytest.mark.parametrize("fmt", FMTS)
def test_clamped_form_equals_inside_form(fmt):
    for res in SHAPES:
        vol = _random(res, fmt, seed=3, special=True)
        for shape in (mr.BOX, mr.BALL):
            for radius in RADII:
                for op in range(7):
                    assert _same(mr.compute(vol, fmt, op, shape, radius), mr.compute(vol, fmt, op, shape, radius, inside=True)), (
                        res, shape, radius, op)


def test_element_counts_order_and_symmetry():
    for radius, n in (((1, 1, 1), 7), ((2, 2, 2), 33), ((4, 4, 4), 257), ((8, 8, 8), 2109), ((2, 0, 3), 19), ((0, 0, 0), 1)):
        assert len(mr.element(mr.BALL, radius)) == n, radius
    assert sorted(map(tuple, mr.element(mr.BALL, (1, 1, 1)))) == sorted(
        [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    for shape in (mr.BOX, mr.BALL):
        for radius in RADII + [(0, 0, 0), (0, 8, 1)]:
            e = mr.element(shape, radius)
            if shape == mr.BOX:
                assert len(e) == np.prod([2 * r + 1 for r in radius])
            assert len(e) == _footprint(shape, radius).sum()
            s = set(map(tuple, e.tolist()))
            assert len(s) == len(e) and all((-x, -y, -z) in s for x, y, z in s)          # symmetric
            assert all((abs(x) - (x != 0), abs(y), abs(z)) in s and (abs(x), abs(y) - (y != 0), abs(z)) in s and
                       (abs(x), abs(y), abs(z) - (z != 0)) in s for x, y, z in s)      # down-closed in |o|
            order = [(z, y, x) for x, y, z in e.tolist()]
            assert order == sorted(order)                                                # z, y, x ascending


@pytest.mark.parametrize("fmt", FMTS)
def test_ordering_and_idempotence(fmt):
    for res in SHAPES:
        vol = _random(res, fmt, seed=11)   # (finite: the ordering is of keys, compared as values here)
        for shape in (mr.BOX, mr.BALL):
            for radius in RADII:
                e, d, o, c = (mr.compute(vol, fmt, op, shape, radius) for op in (mr.ERODE, mr.DILATE, mr.OPEN, mr.CLOSE))
                ke, kd, ko, kc, kf = (_keys(a).astype(np.int64) for a in (e, d, o, c, vol))
                assert (ke <= ko).all() and (ko <= kf).all() and (kf <= kc).all() and (kc <= kd).all(), (res, shape, radius)
                assert _same(mr.compute(o, fmt, mr.OPEN, shape, radius), o), (res, shape, radius)
                assert _same(mr.compute(c, fmt, mr.CLOSE, shape, radius), c), (res, shape, radius)
                if fmt != mr.FLOAT:   # so the differences never wrap
                    assert _same(mr.compute(vol, fmt, mr.TOPHAT, shape, radius), vol - o)
                    assert _same(mr.compute(vol, fmt, mr.BLACKHAT, shape, radius), c - vol)
                    assert _same(mr.compute(vol, fmt, mr.GRADIENT, shape, radius), d - e)


@pytest.mark.parametrize("fmt", FMTS)
def test_box_is_three_passes(fmt):
    for res in SHAPES:
        vol = _random(res, fmt, seed=5, special=True)
        for radius in RADII:
            for op in (mr.ERODE, mr.DILATE):
                step = vol
                for a in range(3):
                    r1 = [0, 0, 0]
                    r1[a] = radius[a]
                    step = mr.compute(step, fmt, op, mr.BOX, r1)
                assert _same(step, mr.compute(vol, fmt, op, mr.BOX, radius)), (res, radius, op)


def test_float_rules():
    w = lambda *bits: np.array(bits, np.uint32).view(F32).reshape(1, 1, -1)
    nan_payload, pinf, ninf, nzero, pzero = 0xffc00123, 0x7f800000, 0xff800000, 0x80000000, 0
    one = np.array([1.0], F32).view(np.uint32)[0]
    # every NaN is the largest key: the dilation next to it is the canonical NaN, the erosion ignores it
    vol = w(one, nan_payload, pinf)
    assert list(_bits(mr.compute(vol, mr.FLOAT, mr.DILATE, mr.BOX, (1, 0, 0))).ravel()) == [0x7fc00000] * 3
    assert list(_bits(mr.compute(vol, mr.FLOAT, mr.ERODE, mr.BOX, (1, 0, 0))).ravel()) == [one, one, pinf]
    # -0 sorts below +0 and either is stored +0; the identity element canonicalises the stored word only
    vol = w(nzero, pzero, nan_payload, ninf)
    assert list(_bits(mr.compute(vol, mr.FLOAT, mr.ERODE, mr.BALL, (0, 0, 0))).ravel()) == [0, 0, 0x7fc00000, ninf]
    assert list(_bits(mr.compute(vol[..., :2], mr.FLOAT, mr.GRADIENT, mr.BOX, (1, 0, 0))).ravel()) == [0, 0]
    # inf - inf stores 0x7fc00000; inf - finite stays inf
    vol = w(pinf, pinf, one)
    assert list(_bits(mr.compute(vol, mr.FLOAT, mr.GRADIENT, mr.BOX, (1, 0, 0))).ravel()) == [0x7fc00000, pinf, pinf]
    # the top hat reads the source's raw word: a NaN with a payload gives the canonical NaN
    vol = w(one, nan_payload, one)
    assert list(_bits(mr.compute(vol, mr.FLOAT, mr.TOPHAT, mr.BOX, (1, 0, 0))).ravel()) == [0, 0x7fc00000, 0]


def test_refusals():
    vol = np.zeros((2, 2, 2), np.uint8)
    for radius in ((9, 0, 0), (0, 0, 9)):
        with pytest.raises(ValueError):
            mr.compute(vol, mr.UCHAR, mr.ERODE, mr.BOX, radius)
    with pytest.raises(ValueError):
        mr.compute(vol, mr.UCHAR, 7, mr.BOX, (1, 1, 1))
    with pytest.raises(ValueError):
        mr.compute(vol, mr.UCHAR, mr.ERODE, 2, (1, 1, 1))
