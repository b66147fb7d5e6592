"""A plain reference for the tables the renderer derives from the cell grids and the transfer function
(vr_cells.hip: per-cell opacity bound, empty bit, macro-cell bound, leap radii), the inputs that put them on
their edges, and the assertions tests/test_gpu_cell_tables.py (device) and tests/test_cell_tables_ref.py (a
numpy stand-in for the device, no GPU) make about them.

Per cell with finite extrema (mn, mx) within +-FLT_MAX / 2, density interval [x_lo, x_hi] = the extrema over the
format's maximum, computed in float64, rounded to fp32 and widened by 4 ulps at each end:
  A  the oracle's opacity (vro.math_batch "tff_alpha") maximised over the two ends and over every entry centre
     (i + 0.5) / n inside the interval with its +-2-ulp neighbours: the read is piecewise linear, so this is
     the largest opacity a sample in the cell can read.  A bound below A is unsound.
  E  the largest alpha entry over [floor(x_lo n - 0.5) - 2, floor(x_hi n - 0.5) + 3] (float64), clamped to the
     table.  The kernel reads floor - 1 .. floor + 2 of an fp32 index whose absolute error is below 1 for
     n <= 4096, so its window lies inside this one: a bound above E * 1.000001 is needlessly loose.
"""
import numpy as np

from oracle import vro

UCHAR, USHORT, FLOAT = 0, 1, 2
MAXV = {UCHAR: 255.0, USHORT: 65535.0, FLOAT: 1.0}
NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
HALF_MAX = float(np.finfo(np.float32).max) / 2
LEVELS, MAX_RADIUS, MACRO = 7, 15, 4
MARGIN = np.float32(1.000001)


def _step(x, n, towards):
    x = np.asarray(x, np.float32)
    for _ in range(n):
        x = np.nextafter(x, np.float32(towards))
    return x


def cell_minmax(vol, shift):
    """(min, max) of the voxels [E c - 1, E c + E + 1]^3 of every cell, clipped to the volume; a cell with a NaN
    voxel is (-inf, +inf) -- what test_cell_grid_bounds / test_cell_grids_float_range pin for the device."""
    E = 1 << shift
    v = vol.astype(np.float32)
    cz, cy, cx = (-(-s // E) for s in v.shape)
    out = np.empty((cz, cy, cx, 2), np.float32)
    for k in range(cz):
        zs = v[max(E * k - 1, 0):E * k + E + 2]
        for j in range(cy):
            ys = zs[:, max(E * j - 1, 0):E * j + E + 2]
            for i in range(cx):
                box = ys[:, :, max(E * i - 1, 0):E * i + E + 2]
                out[k, j, i] = (-np.inf, np.inf) if np.isnan(box).any() else (box.min(), box.max())
    return out


def _range_max(values, lo, hi):
    """max(values[lo .. hi]) per element (inclusive; -inf where lo > hi), one slice per distinct pair."""
    out = np.full(lo.shape, -np.inf, np.float64)
    pairs, inv = np.unique(np.stack([lo.ravel(), hi.ravel()], 1), axis=0, return_inverse=True)
    res = np.array([values[a:b + 1].max() if a <= b else -np.inf for a, b in pairs], np.float64)
    out.ravel()[:] = res[inv.ravel()]
    return out


def _alpha(tff, x):
    return vro.math_batch("tff_alpha", np.ascontiguousarray(x, np.float32).reshape(-1, 1), tff=tff) \
        .view(np.float32)[:, 0].astype(np.float64)


def reference(mm, fmt, tff):
    """finite [cells] bool, A and E [cells] float64 (meaningless where not finite) for the (min, max) pairs mm."""
    tff = np.ascontiguousarray(tff, np.uint8).reshape(-1, 4)
    n = tff.shape[0]
    mn, mx = mm[..., 0].astype(np.float64).ravel(), mm[..., 1].astype(np.float64).ravel()
    with np.errstate(invalid="ignore"):
        finite = (mn <= mx) & (np.abs(mn) <= HALF_MAX) & (np.abs(mx) <= HALF_MAX)
    x_lo = _step(np.where(finite, mn, 0.0) / MAXV[fmt], 4, -np.inf)
    x_hi = _step(np.where(finite, mx, 0.0) / MAXV[fmt], 4, np.inf)
    # A: the ends, and the breakpoints inside with their neighbours
    centres = ((np.arange(n, dtype=np.float64) + 0.5) / n).astype(np.float32)
    around = np.stack([_alpha(tff, _step(centres, k, -np.inf)) for k in (2, 1, 0)] +
                      [_alpha(tff, _step(centres, k, np.inf)) for k in (1, 2)]).max(axis=0)
    first = np.searchsorted(centres, x_lo, side="left")
    last = np.searchsorted(centres, x_hi, side="right") - 1
    A = np.maximum(np.maximum(_alpha(tff, x_lo), _alpha(tff, x_hi)), _range_max(around, first, last))
    # E: the widest window of entries a correct kernel can read
    entries = (tff[:, 3].astype(np.float32) / np.float32(255.0)).astype(np.float64)
    w_lo = np.clip(np.floor(x_lo.astype(np.float64) * n - 0.5) - 2, 0, n - 1).astype(np.int64)
    w_hi = np.clip(np.floor(x_hi.astype(np.float64) * n - 0.5) + 3, 0, n - 1).astype(np.int64)
    E = _range_max(entries, w_lo, w_hi)
    return finite, A, E


def unpack_bits(words, n_cells):
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool).ravel()
    return bits[:n_cells], bits[n_cells:]


def macro_reference(bound):
    cz, cy, cx = bound.shape
    out = np.empty(tuple(-(-s // MACRO) for s in bound.shape), np.float32)
    for Z in range(out.shape[0]):
        for Y in range(out.shape[1]):
            for X in range(out.shape[2]):
                out[Z, Y, X] = bound[MACRO * Z:MACRO * Z + MACRO, MACRO * Y:MACRO * Y + MACRO,
                                     MACRO * X:MACRO * X + MACRO].max()
    return out


def leap_reference(macro):
    """[LEVELS, ccz, ccy, ccx] bytes by brute force: 0 where the macro cell is not free at level j (bound >= j / 8 in
    fp32), else 1 + the largest R <= 15 with every existing macro cell within Chebyshev distance R free."""
    cz, cy, cx = macro.shape
    out = np.zeros((LEVELS,) + macro.shape, np.uint8)
    for j in range(1, LEVELS + 1):
        free = macro < np.float32(j / 8.0)
        for Z, Y, X in zip(*np.nonzero(free)):
            R = 0
            while R < MAX_RADIUS:
                r = R + 1
                if not free[max(Z - r, 0):Z + r + 1, max(Y - r, 0):Y + r + 1, max(X - r, 0):X + r + 1].all():
                    break
                R = r
            out[j - 1, Z, Y, X] = 1 + R
    return out


def check_bounds(bound, mm, fmt, tff, what=""):
    """Soundness and tightness of the per-cell bounds; returns (finite, A, E) for the callers' own counts."""
    finite, A, E = reference(mm, fmt, tff)
    b = bound.astype(np.float32).ravel()
    bad = finite & ~(b.astype(np.float64) >= A)
    assert not bad.any(), "%s: %d bounds below the opacity a sample can read, first cell %d: %r < %r" % (
        what, bad.sum(), np.argmax(bad), b[np.argmax(bad)], A[np.argmax(bad)])
    limit = E.astype(np.float32) * MARGIN
    bad = finite & ~(b <= limit)
    assert not bad.any(), "%s: %d bounds above the envelope, first cell %d: %r > %r" % (
        what, bad.sum(), np.argmax(bad), b[np.argmax(bad)], limit[np.argmax(bad)])
    bad = finite & (E == 0) & (b != 0)
    assert not bad.any(), "%s: %d cells that read only zero entries have a bound above 0" % (what, bad.sum())
    bad = ~finite & (b != np.float32(2.0))
    assert not bad.any(), "%s: %d cells that can sample a non-finite value have a bound other than 2" % (what, bad.sum())
    return finite, A, E


def check_empty(words, mm, fmt, tff, what=""):
    """The empty bits of the (min, max) grid mm: set only where nothing can be read, set wherever only zero entries
    can be read, never on a non-finite cell, and no bit for a cell that does not exist."""
    finite, A, E = reference(mm, fmt, tff)
    n_cells = finite.size
    assert words.size == (n_cells + 31) // 32
    bits, beyond = unpack_bits(words, n_cells)
    assert not beyond.any(), "%s: bits set beyond the last cell" % what
    bad = bits & finite & (A != 0)
    assert not bad.any(), "%s: %d cells marked empty whose samples can read opacity" % (what, bad.sum())
    bad = bits & ~finite
    assert not bad.any(), "%s: %d non-finite cells marked empty" % (what, bad.sum())
    bad = finite & (E == 0) & ~bits
    assert not bad.any(), "%s: %d cells that read only zero entries are not marked empty" % (what, bad.sum())
    return bits, finite, A, E


def check_macro_and_leaps(bound, macro, leap, what=""):
    np.testing.assert_array_equal(macro, macro_reference(bound), err_msg=what + ": macro bounds")
    want = leap_reference(macro)
    np.testing.assert_array_equal(leap, want, err_msg=what + ": leap radii")
    assert not leap[:, macro >= np.float32(2.0)].any(), what + ": a macro cell with bound 2 is free"
    return want


# ---- a numpy fp32 stand-in for the device (the check of the checks; never the reference)

def device_standin(mm, fmt, tff, widen=(1, 2), margin=True, always_two=False):
    """Bound and empty bit per cell the way a device kernel forms them in fp32: the index window floor - widen[0] ..
    floor + widen[1] around the fp32 table coordinates of the extrema, times 1.000001.  widen=(0, 1), margin=False
    and always_two=True are the deliberately wrong variants."""
    tff = np.ascontiguousarray(tff, np.uint8).reshape(-1, 4)
    n = tff.shape[0]
    f32 = np.float32
    mn, mx = mm[..., 0].astype(f32).ravel(), mm[..., 1].astype(f32).ravel()
    inv = f32(1.0) / f32(MAXV[fmt])
    fn = f32(n)
    with np.errstate(over="ignore", invalid="ignore"):
        ok = (mn <= mx) & (np.abs(mn) <= f32(HALF_MAX)) & (np.abs(mx) <= f32(HALF_MAX))
        flo = np.floor((mn * inv) * fn - f32(0.5)) - f32(widen[0])
        fhi = np.floor((mx * inv) * fn - f32(0.5)) + f32(widen[1])
    flo = np.where(ok, np.clip(flo, 0, n - 1), 0).astype(np.int64)
    fhi = np.where(ok, np.clip(fhi, 0, n - 1), 0).astype(np.int64)
    entries = (tff[:, 3].astype(f32) / f32(255.0)).astype(np.float64)
    b = _range_max(entries, flo, fhi).astype(f32)
    if margin:
        b = b * MARGIN
    b = np.where(ok, b, f32(2.0)).astype(f32)
    if always_two:
        b = np.full_like(b, 2.0)
    bits = np.zeros(((b.size + 31) // 32) * 32, bool)
    bits[:b.size] = b == 0
    words = (bits.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
    return b.reshape(mm.shape[:-1]), words


# ---- inputs

def comb_tff(n, seed=0):
    """Alpha zero except: isolated single non-zero entries over the first half of the table, and over the second half
    a non-zero plateau cut by isolated zero gaps 1, 2, 3, 4 and 5 entries wide.  Returns (tff, features): features
    are the entries where opacity starts or stops."""
    rng = np.random.default_rng(1000 + seed)
    t = np.zeros((n, 4), np.uint8)
    t[:, :3] = rng.integers(20, 256, (n, 3))
    half = n // 2
    teeth = np.arange(max(half // 12, 1), half - 8, max(half // 6, 24))
    t[teeth, 3] = rng.integers(1, 256, teeth.size)
    t[half:, 3] = rng.integers(1, 256, n - half)
    # (the teeth three times over and the middles of the zero stretches between them: half the slabs lie by a tooth)
    features = 3 * list(teeth) + list((teeth[:-1] + teeth[1:]) // 2) + [half]
    pos = half + max(half // 12, 8)
    for width in (1, 2, 3, 4, 5):
        t[pos:pos + width, 3] = 0
        features += [pos, pos + width]
        pos += max(half // 7, 16)
    assert pos < n
    return t, np.array(features)


KIND_SETS = [(0, 1, 2, 3), (0, 1), (2, 3), (0,), (0, 1, 2), (1, 3)]


def knife_edge_volume(fmt, res, n, features, seed=0, spread=8):
    """Voxels drawn from {(i + 0.5) / n, its fp32 (or integer) neighbours above and below, i / n} for the entries i
    and i + 1, i within `spread` of a feature of the table; one feature, offset and subset of the four kinds
    (KIND_SETS) per slab of 16 x 20 voxels in x and y, so that many cells see one or two slabs only and their
    extrema are now a centre, now its neighbour on either side, now an entry's edge."""
    rng = np.random.default_rng(2000 + seed)
    x, y, z = res
    sx, sy = -(-x // 16), -(-y // 20)
    base = features[rng.integers(0, features.size, (sy, sx))] + rng.integers(-spread, spread + 1, (sy, sx))
    base = np.clip(base, 0, n - 2)
    i0 = np.repeat(np.repeat(base, 20, axis=0), 16, axis=1)[:y, :x]
    i = (i0[None, :, :] + rng.integers(0, 2, (z, y, x))).astype(np.float64)
    sets = np.array([[k[j % len(k)] for j in range(12)] for k in KIND_SETS])[rng.integers(0, len(KIND_SETS), (sy, sx))]
    sets = np.repeat(np.repeat(sets, 20, axis=0), 16, axis=1)[:y, :x]            # [y, x, 12]
    kind = np.take_along_axis(np.broadcast_to(sets, (z, y, x, 12)), rng.integers(0, 12, (z, y, x, 1)), axis=3)[..., 0]
    if fmt == FLOAT:
        c = ((i + 0.5) / n).astype(np.float32)
        v = np.select([kind == 0, kind == 1, kind == 2], [c, _step(c, 1, np.inf), _step(c, 1, -np.inf)],
                      (i / n).astype(np.float32))
        return v.astype(np.float32)
    m = MAXV[fmt]
    c = np.round((i + 0.5) / n * m)
    v = np.select([kind == 0, kind == 1, kind == 2], [c, c + 1, c - 1], np.round(i / n * m))
    return np.clip(v, 0, m).astype(NP_DTYPE[fmt])


def blob_volume(long_axis="x"):
    """1050 x 70 x 33 UCHAR (33 x 3 x 2 macro cells of 32 voxels, a partial one last on every axis), zero except for
    a strong blob in the first macro cell, a weak one in the last -- partial -- macro cell and a weak one off to a
    side near the middle of the second half: with blob_tff() the leap-radius bytes 0, 1, 2, 7, 14, 15 and 16 occur."""
    v = np.zeros((33, 70, 1050), np.uint8)
    v[3:6, 4:7, 3:6] = 250          # macro cell (0, 0, 0)
    v[20:23, 40:43, 1040:1045] = 90    # macro cell (32, 1, 0): cells 130 of 132
    v[30:32, 66:69, 900:903] = 130   # macro cell (28, 2, 0), in the last rows and slices
    if long_axis == "y":
        v = np.ascontiguousarray(v.transpose(0, 2, 1))
    return v


def blob_tff(n=1024):
    """Opacity i / n: nothing at density 0, each blob blocks the levels below its own opacity."""
    t = np.zeros((n, 4), np.uint8)
    t[:, 0] = 200
    t[:, 1] = np.arange(n) % 256
    t[:, 2] = 60
    t[:, 3] = np.arange(n) * 255 // max(n - 1, 1)
    return t


TF_SIZES = (1, 2, 3, 255, 257, 1000, 4095, 4096)
NOISE_RES = (70, 33, 50)
KNIFE_RES = (64, 40, 36)
# (format, entries, seed, table): "comb" = comb_tff, "saw" = saw_tff
# (the seeds: the first for which the reference alone finds a tenth of the coarse cells reading only zero entries)
KNIFE_CASES = [(FLOAT, 1024, 8, "comb"), (FLOAT, 1000, 4, "comb"), (USHORT, 1024, 8, "comb"), (USHORT, 257, 10, "comb"),
               (FLOAT, 1000, 4, "saw"), (USHORT, 1024, 5, "saw")]


def sized_tff(n):
    """The default stops on n entries (opacity 0 up to a tenth of the range); the one entry of n = 1 is opaque."""
    from volumerenderercl_amd import frontend
    if n == 1:
        return np.array([[200, 40, 20, 120]], np.uint8)
    return frontend.tff_from_stops(n=n)


def edge_tff(n, only_first=False):
    """The palettes' tables of tests/test_gpu_float_range.py: the default stops with opaque coloured TF[0] and
    TF[n-1] -- what every value outside [0, 1] reads -- or opacity at TF[0] alone."""
    if only_first:
        t = np.zeros((n, 4), np.uint8)
        t[0] = [220, 30, 30, 200]
        return t
    t = sized_tff(n).copy()
    t[0] = [200, 40, 20, 120]
    t[-1] = [20, 60, 230, 90]
    return t


def saw_tff(n, seed=0):
    """Opacity 1 / 255 with every sixth entry opaque.  Features: the entries one above and two below an opaque one,
    so that a slab of knife_edge_volume(spread=0) -- entries i and i + 1 -- has the opaque entry just outside the
    entries its values lie in: only a sample a few ulps beyond the cell's extrema reads it."""
    rng = np.random.default_rng(3000 + seed)
    t = np.zeros((n, 4), np.uint8)
    t[:, :3] = rng.integers(20, 256, (n, 3))
    t[:, 3] = 1
    t[::6, 3] = 255
    i = np.arange(6, n - 8, 6)
    return t, np.concatenate([i + 1, i + 4])


def knife_case(fmt, n, seed, table="comb"):
    tff, features = (comb_tff if table == "comb" else saw_tff)(n, seed)
    return knife_edge_volume(fmt, KNIFE_RES, n, features, seed, spread=8 if table == "comb" else 0), tff


# volumes whose fine grid (cells of 4 voxels) has a cell count of 0, 1, 31, 32, 33, 63 mod 64: (res, cells)
WORD_CASES = [((32, 15, 16), 128), ((18, 27, 44), 385), ((11, 36, 50), 351), ((16, 14, 24), 96),
              ((20, 19, 34), 225), ((12, 20, 66), 255)]
