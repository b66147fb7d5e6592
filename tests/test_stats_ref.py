"""tests/ref/stats_ref.c, the restatement the GPU statistics are compared with bit for bit, pinned without a GPU against
an independent vectorised numpy-float32 formulation of the header's contract: counts, value and gradient bins on
random volumes of every voxel type, the count identity, region additivity, the 1-D table as the 2-D table's column
sum, the closed upper end of the window, FLOAT volumes with NaN, infinities and values outside [0, 1], the double sums
against math.fsum, and the constant-block rule the device's skip relies on."""
import math

import numpy as np
import pytest

from tests import stats_ref
from tests.stats_ref import FLOAT, UCHAR, USHORT

F = np.float32
INV_MAX = {UCHAR: F(1.0) / F(255.0), USHORT: F(1.0) / F(65535.0), FLOAT: F(1.0)}


def _random(res, fmt, seed=1):
    rng = np.random.default_rng(seed)
    shape = (res[2], res[1], res[0])
    if fmt == UCHAR:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if fmt == USHORT:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return rng.random(shape, dtype=np.float32)


def _numpy_stats(vol, fmt, bins, window, region=None):
    """The contract in whole-array float32 numpy: (counts dict, hist)."""
    bv, bg = bins
    v_lo, v_hi, g_hi = (F(w) for w in window)
    with np.errstate(all="ignore"):
        s = vol.astype(F) * INV_MAX[fmt]
        pad = np.pad(s, 1, mode="edge")                     # the neighbour clamped to the volume
        gx = pad[1:-1, 1:-1, 2:] - pad[1:-1, 1:-1, :-2]
        gy = pad[1:-1, 2:, 1:-1] - pad[1:-1, :-2, 1:-1]
        gz = pad[2:, 1:-1, 1:-1] - pad[:-2, 1:-1, 1:-1]
        m = F(0.5) * np.sqrt((gx * gx + gy * gy) + gz * gz, dtype=F)
        if region is not None:
            (x0, y0, z0), (x1, y1, z1) = region
            s, m = s[z0:z1, y0:y1, x0:x1], m[z0:z1, y0:y1, x0:x1]
        s, m = s.ravel(), m.ravel()
        nan = np.isnan(s)
        below = ~nan & (s < v_lo)
        above = ~nan & ~below & (s > v_hi)
        inside = ~nan & ~below & ~above
        k_v = F(bv) / (v_hi - v_lo)
        u = (s[inside] - v_lo) * k_v
        i = np.where(u >= F(bv), bv - 1, np.minimum(u, F(bv)).astype(np.int64))
        mi = m[inside]
        if bg > 1:
            gnan = np.isnan(mi)
            k_g = F(bg) / g_hi
            w = mi[~gnan] * k_g
            j = np.where(w >= F(bg), bg - 1, np.minimum(w, F(bg)).astype(np.int64))
            i = i[~gnan]
        else:
            gnan = np.zeros(mi.shape, bool)
            j = np.zeros(i.shape, np.int64)
    hist = np.bincount(j * bv + i, minlength=bv * bg).astype(np.uint64).reshape(bg, bv)
    return dict(voxels=s.size, nan=int(nan.sum()), below=int(below.sum()), above=int(above.sum()),
                gradient_nan=int(gnan.sum()), binned=int(i.size)), hist


def _counts(st):
    return {k: int(getattr(st, k)) for k in ("voxels", "nan", "below", "above", "gradient_nan", "binned")}


def _identity(st, hist):
    assert st.voxels == st.nan + st.below + st.above + st.gradient_nan + st.binned
    assert st.binned == int(hist.sum())


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
@pytest.mark.parametrize("bins,window", [((256, 1), (0.0, 1.0, 1.0)), ((64, 64), (0.1, 0.9, 0.4)), ((7, 5), (0.25, 0.5, 2.0)),
                                         ((1, 1), (0.0, 1.0, 1.0))], ids=["256x1", "64x64", "7x5", "1x1"])
def test_counts_and_bins_against_numpy(fmt, bins, window):
    vol = _random((19, 10, 11), fmt, seed=3 + fmt)
    for region in (None, ((3, 1, 2), (17, 9, 11)), ((8, 8, 8), (9, 9, 9))):
        st, hist = stats_ref.compute(vol, fmt, bins, window, region)
        counts, nh = _numpy_stats(vol, fmt, bins, window, region)
        assert _counts(st) == counts, (region, _counts(st), counts)
        assert np.array_equal(hist, nh), region
        _identity(st, hist)
        assert (st.min, st.max, st.sum, st.sum_sq) == (0.0, 0.0, 0.0, 0.0)   # no moments asked for


def test_regions_that_tile_the_volume_add_up():
    vol = _random((21, 9, 12), USHORT, seed=8)
    bins, window = (32, 16), (0.05, 0.95, 0.6)
    whole_st, whole = stats_ref.compute(vol, USHORT, bins, window)
    for axis, cut in ((0, 13), (1, 8), (2, 5)):
        lo_hi = [[0, 0, 0], [21, 9, 12]]
        a_hi, b_lo = list(lo_hi[1]), list(lo_hi[0])
        a_hi[axis] = b_lo[axis] = cut
        sa, ha = stats_ref.compute(vol, USHORT, bins, window, (lo_hi[0], a_hi))
        sb, hb = stats_ref.compute(vol, USHORT, bins, window, (b_lo, lo_hi[1]))
        assert np.array_equal(ha + hb, whole), axis
        assert {k: v + _counts(sb)[k] for k, v in _counts(sa).items()} == _counts(whole_st)


def test_one_gradient_bin_is_the_column_sum():
    vol = _random((17, 8, 9), UCHAR, seed=4)
    st2, h2 = stats_ref.compute(vol, UCHAR, (128, 32), (0.0, 1.0, 0.5))
    st1, h1 = stats_ref.compute(vol, UCHAR, (128, 1), (0.0, 1.0, 0.5))
    assert st2.gradient_nan == 0 and np.array_equal(h2.sum(axis=0, dtype=np.uint64).reshape(1, -1), h1)
    assert h2[-1].sum() > 0   # the open-ended top bin holds the steep voxels of noise


def test_window_ends():
    """s == v_hi lies in the last bin, s == v_lo in the first; just outside: above and below."""
    vol = np.array([0.25, 0.75, np.nextafter(F(0.75), F(1)), np.nextafter(F(0.25), F(0)), 0.5], dtype=F).reshape(1, 1, 5)
    st, hist = stats_ref.compute(vol, FLOAT, (4, 1), (0.25, 0.75, 1.0))
    assert hist.tolist() == [[1, 0, 1, 1]] and (st.below, st.above, st.binned) == (1, 1, 3)
    vol8 = np.array([0, 255, 128], dtype=np.uint8).reshape(1, 1, 3)
    st, hist = stats_ref.compute(vol8, UCHAR, (256, 1), (0.0, 1.0, 1.0))
    assert hist[0, 0] == 1 and hist[0, 255] == 1 and hist[0, 128] == 1 and st.binned == 3


def test_float_specials():
    rng = np.random.default_rng(11)
    vol = (rng.random((9, 10, 12), dtype=np.float32) * 3.0 - 1.0).astype(F)   # values in [-1, 2]
    vol[2, 3, 4] = np.nan
    vol[5, 5, 5] = np.inf
    vol[5, 5, 7] = np.inf
    vol[5, 5, 6] = 0.5         # between them: inf - inf, a NaN gradient
    vol[7, 1, 1] = -np.inf
    vol[0, 0, 0] = 3e38        # its neighbours' squares overflow: the open-ended top bin
    for bins, window in (((16, 8), (0.0, 1.0, 1.5)), ((16, 1), (-1.0, 2.0, 1.0)), ((5, 3), (-1e38, 2e38, 3e38))):
        st, hist = stats_ref.compute(vol, FLOAT, bins, window, moments=True)
        counts, nh = _numpy_stats(vol, FLOAT, bins, window)
        assert _counts(st) == counts and np.array_equal(hist, nh), bins
        _identity(st, hist)
        assert st.nan == 1 and st.min == -np.inf and st.max == np.inf
        assert math.isnan(st.sum) and st.sum_sq == np.inf   # (inf + -inf; the squares of infinities)
    st, _ = stats_ref.compute(vol, FLOAT, (16, 8), (0.0, 1.0, 1.5))
    assert st.gradient_nan >= 1
    # nothing but NaN: no minimum, no maximum
    st, hist = stats_ref.compute(np.full((2, 3, 4), np.nan, F), FLOAT, (8, 2), (0.0, 1.0, 1.0), moments=True)
    assert (st.nan, st.binned, st.min, st.max, st.sum, st.sum_sq) == (24, 0, np.inf, -np.inf, 0.0, 0.0) and not hist.any()


def _tree_sums(s):
    """The contract's order in float64 numpy, one addition at a time, for the whole volume s [z, y, x] (NaNs add
    nothing): a lane's column from 0.0, the xor butterfly, the blocks of a chunk ascending, the chunks ascending.
    Returns (sum, sum_sq, additions on the longest path from a voxel to the total)."""
    d, h, w = s.shape
    pad = np.full(((d + 7) // 8 * 8, (h + 7) // 8 * 8, (w + 7) // 8 * 8), np.nan)
    pad[:d, :h, :w] = s
    lanes_of = np.arange(64)
    totals, chunks, n_in_chunk = [0.0, 0.0], [0.0, 0.0], 0
    for bz in range(pad.shape[0] // 8):
        for by in range(pad.shape[1] // 8):
            for bx in range(pad.shape[2] // 8):
                blk = pad[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
                for which, vals in enumerate((blk, blk * blk)):
                    lanes = np.zeros(64)
                    for z in range(8):
                        layer = vals[z].ravel()        # index y * 8 + x: the lane
                        lanes = np.where(np.isnan(layer), lanes, lanes + layer)
                    for k in (1, 2, 4, 8, 16, 32):
                        lanes = lanes + lanes[lanes_of ^ k]
                    chunks[which] = chunks[which] + float(lanes[0])
                n_in_chunk += 1
                if n_in_chunk == stats_ref.SUM_CHUNK:
                    totals = [totals[0] + chunks[0], totals[1] + chunks[1]]
                    chunks, n_in_chunk = [0.0, 0.0], 0
    n_blocks = pad.size // 512
    if n_in_chunk:
        totals = [totals[0] + chunks[0], totals[1] + chunks[1]]
    depth = 8 + 6 + min(n_blocks, stats_ref.SUM_CHUNK) + (n_blocks + stats_ref.SUM_CHUNK - 1) // stats_ref.SUM_CHUNK
    return totals[0], totals[1], depth


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_sums_follow_the_order_and_stay_near_fsum(fmt):
    """The double sums are the contract's tree bit for bit, and close to the exact sum: the values are >= 0, so every
    partial sum is at most the total and each of the `depth` additions on the path from a voxel to the total errs by
    at most half an ulp of the total -- depth / 2 ulp in all (a plain loop over the voxels: voxels / 2).  20 x 17 x 9
    is 3 x 3 x 2 blocks with a partial one on every axis: depth 33, a few ulp.  8 x 8 x 2400 is 300 blocks: two
    chunks."""
    for res in ((20, 17, 9), (8, 8, 2400)):
        vol = _random(res, fmt, seed=21)
        st, _ = stats_ref.compute(vol, fmt, moments=True)
        s = (vol.astype(F) * INV_MAX[fmt]).astype(np.float64)
        tree, tree_sq, depth = _tree_sums(s)
        assert st.sum == tree and st.sum_sq == tree_sq
        exact, exact_sq = math.fsum(s.ravel()), math.fsum((s * s).ravel())   # (the squares of floats are exact in double)
        assert depth == (33 if res[2] == 9 else 8 + 6 + 256 + 2)
        assert abs(st.sum - exact) <= depth / 2 * math.ulp(exact) and abs(st.sum_sq - exact_sq) <= depth / 2 * math.ulp(exact_sq)
        assert st.min == s.min() and st.max == s.max()
    # a region: the same order over the region's own block grid, voxels outside it adding nothing
    vol = _random((20, 17, 9), fmt, seed=22)
    s = (vol.astype(F) * INV_MAX[fmt]).astype(np.float64)
    st, _ = stats_ref.compute(vol, fmt, region=((9, 3, 0), (20, 16, 8)), moments=True)
    masked = np.full(s.shape, np.nan)
    masked[0:8, 3:16, 9:20] = s[0:8, 3:16, 9:20]
    tree, tree_sq, _ = _tree_sums(masked[:8, :, 8:])       # the region's blocks start at block (1, 0, 0) and end at z = 8
    assert st.sum == tree and st.sum_sq == tree_sq


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_constant_block_rule(fmt):
    """What the device's skip of a constant block writes is what the fetched path gives.  Counts: every voxel in the one
    value bin of fl(c * inv_max) (or below / above) and gradient bin 0, for any finite c.  Moments, for c == 0 (either
    sign): block sums +0.0 and min = max = +0 -- so a volume of zero blocks sums to +0.0 bit for bit.  And n * c is exact
    while n * c * c is not in general, which is why other constants are fetched."""
    dtype = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: F}[fmt]
    for c in {UCHAR: (0, 37, 255), USHORT: (0, 12345, 65535), FLOAT: (0.0, -0.0, 0.3, -7.5, 3e38)}[fmt]:
        vol = np.full((9, 17, 10), c, dtype=dtype)
        s = F(vol[0, 0, 0]) * INV_MAX[fmt]
        for bins, window in (((64, 16), (0.0, 1.0, 0.25)), ((3, 2), (0.2, 0.5, 1e-30)), ((5, 1), (-8.0, 0.31, 1.0))):
            for region in (None, ((1, 2, 3), (9, 16, 9))):
                st, hist = stats_ref.compute(vol, fmt, bins, window, region)
                n = st.voxels
                v_lo, v_hi = F(window[0]), F(window[1])
                if s < v_lo:
                    assert (st.below, st.binned) == (n, 0)
                elif s > v_hi:
                    assert (st.above, st.binned) == (n, 0)
                else:
                    u = (s - v_lo) * (F(bins[0]) / (v_hi - v_lo))
                    i = bins[0] - 1 if u >= F(bins[0]) else int(u)
                    assert st.binned == n and hist[0, i] == n and st.gradient_nan == 0
    zero = np.zeros((9, 17, 10), dtype=dtype)
    if fmt == FLOAT:
        zero[::2, 1::3, ::5] = -0.0
    st, _ = stats_ref.compute(zero, fmt, moments=True)
    assert _bits(st.sum) == 0 and _bits(st.sum_sq) == 0
    assert F(st.min).view(np.uint32) == 0 and F(st.max).view(np.uint32) == 0
    # the counter-example: 343 voxels of one value.  n * c is exact whatever the order; n * c * c is no double
    c = F(0.1)
    block = np.full((8, 8, 8), c, dtype=F)
    st, _ = stats_ref.compute(block, FLOAT, region=((0, 0, 0), (7, 7, 7)), moments=True)
    assert st.sum == 343.0 * float(c)
    mant = int(c.view(np.uint32) & 0x7fffff | 0x800000)
    assert (343 * mant * mant) % 2 == 1 and (343 * mant * mant).bit_length() > 53


def test_refusals():
    vol = _random((9, 9, 9), UCHAR)
    inf, nan = float("inf"), float("nan")
    bad = [dict(bins=(0, 1)), dict(bins=(4097, 1)), dict(bins=(1, 0)), dict(bins=(16, 257)), dict(bins=(4096, 17)),
           dict(window=(nan, 1.0, 1.0)), dict(window=(0.0, inf, 1.0)), dict(window=(0.5, 0.5, 1.0)), dict(window=(0.6, 0.5, 1.0)),
           dict(window=(-3e38, 3e38, 1.0)), dict(window=(0.0, 1e-45, 1.0)),
           dict(bins=(4, 2), window=(0.0, 1.0, 0.0)), dict(bins=(4, 2), window=(0.0, 1.0, -1.0)),
           dict(bins=(4, 2), window=(0.0, 1.0, inf)), dict(bins=(4, 2), window=(0.0, 1.0, nan)),
           dict(bins=(4, 2), window=(0.0, 1.0, 1e-45)),
           dict(region=((0, 0, 0), (10, 9, 9))), dict(region=((5, 0, 0), (4, 9, 9))), dict(region=((0, 0, 0), (9, 0, 9))),
           dict(region=((1, 0, 0), (0, 0, 0)))]
    for kw in bad:
        with pytest.raises(ValueError):
            stats_ref.compute(vol, UCHAR, **kw)
    # g_hi is not looked at with one gradient bin; an empty region is a table of zeros
    st, hist = stats_ref.compute(vol, UCHAR, (4, 1), (0.0, 1.0, nan))
    assert st.binned == 729
    st, hist = stats_ref.compute(vol, UCHAR, (4, 2), region=((3, 3, 3), (3, 9, 9)), moments=True)
    assert st.voxels == 0 and not hist.any() and (st.min, st.max) == (np.inf, -np.inf)
