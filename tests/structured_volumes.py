"""Seeded 3-D patchworks for the volume operators that skip blocks of 8^3 voxels on the word of the cell grid
(vrhip_filter_volume, vrhip_morph_volume, vrhip_volume_statistics, the isosurface calls), and the skip predictors:
which blocks each operator skips, from a [cz, cy, cx, 2] array of (min, max) pairs, written from the operators'
contracts (the header comments of vr_filter.hip, vr_morph.hip, vr_stats.hip, vr_mesh.hip).
TEST INFRASTRUCTURE ONLY, no GPU.  tests/test_structured_volumes_ref.py shows on the CPU restatements alone that the
inputs are fit and the predictors sound; tests/test_gpu_structured_volumes.py holds the kernels to both.

A patchwork is a volume cut into boxes by 2-4 cut positions per axis, each at a multiple of 8 or 1, 2 or 3 voxels
off one (a cell answers for the voxels [8 c - 1, 8 c + 9]: its rim straddles such a cut).  A box is noise or one
constant of a small palette; a box copies a neighbour's content with some probability, so constants span cuts, and
different constants meet without noise between them.  FLOAT: zeros of both signs, one box of +inf, and one NaN and
one -inf strictly inside the largest constant box.

All arrays are [z, y, x]; radii, margins, regions and resolutions are (x, y, z), as the API takes them."""
import functools

import numpy as np

UCHAR, USHORT, FLOAT = 0, 1, 2
NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
FMTS = [UCHAR, USHORT, FLOAT]
FMT_IDS = ["uchar", "ushort", "float"]
F32 = np.float32
INV_MAX = {UCHAR: F32(1) / F32(255), USHORT: F32(1) / F32(65535), FLOAT: F32(1)}
B = 8   # voxels per block and axis, and per coarse cell up to 2048 voxels per axis (shift 3)

# (x, y, z): partial cells on every axis; whole multiples of 8; a single layer of blocks with a ninth voxel; the same
# along x; the long case, for margins of 8 and 16 voxels
SHAPES = [(37, 21, 29), (40, 24, 32), (43, 18, 9), (9, 44, 26), (72, 16, 24)]
LONG = (72, 16, 24)
PALETTE = {UCHAR: [0, 77, 255], USHORT: [0, 300, 65535]}
# FLOAT constants: +0, a box of mixed +-0 ("pm0"), three finite values; +inf is given to one box afterwards
FLOAT_PALETTE = [0.0, "pm0", 0.3, 2.5, -1.5]
# The seeds: per case one for which tests/test_structured_volumes_ref.py's conditions hold on the reference's
# own cells (the generator is tuned, never the thresholds).
_INT_SEEDS = {(37, 21, 29): 278, (40, 24, 32): 264, (43, 18, 9): 646, (9, 44, 26): 328, (72, 16, 24): 589}
_FLOAT_SEEDS = {(37, 21, 29): 517, (40, 24, 32): 15, (43, 18, 9): 469, (9, 44, 26): 487, (72, 16, 24): 13}
SEEDS = {(res, fmt): (_FLOAT_SEEDS if fmt == FLOAT else _INT_SEEDS)[res] for res in SHAPES for fmt in FMTS}
COPY = 0.9   # the chance that a box takes a neighbour's content


def shape_id(res):
    return "x".join(map(str, res))


def cuts_of(res, seed):
    """2-4 cut positions per axis (x, y, z): box k of an axis is [cut[k-1], cut[k]).  Every cut lies at 8 m + d,
    d in -3 .. 3."""
    rng = np.random.default_rng(10007 * seed + 17)
    out = []
    for n in res:
        cand = sorted({B * m + d for m in range(n // B + 2) for d in range(-3, 4) if 1 <= B * m + d <= n - 1})
        k = int(rng.integers(2, 5))
        k = min(k, len(cand))
        out.append(sorted(int(c) for c in rng.choice(cand, k, replace=False)))
    return out


def _noise(rng, shape, fmt):
    if fmt == UCHAR:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if fmt == USHORT:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return (rng.random(shape, dtype=np.float32) * 4.0 - 1.5).astype(F32)   # values outside [0, 1]


@functools.lru_cache(maxsize=None)
def _patchwork(res, fmt, seed):
    rng = np.random.default_rng(seed)
    cuts = cuts_of(res, seed)
    edges = [[0] + c + [n] for c, n in zip(cuts, res)]           # x, y, z
    nbox = [len(e) - 1 for e in edges]
    palette = FLOAT_PALETTE if fmt == FLOAT else PALETTE[fmt]
    content = {}                                                 # (k, j, i) -> "noise" or a palette entry
    weights = np.array([1.0 / res[0], 1.0 / res[1], 1.0 / res[2]])
    for k in range(nbox[2]):
        for j in range(nbox[1]):
            for i in range(nbox[0]):
                prev = [(k, j, i - 1), (k, j - 1, i), (k - 1, j, i)]
                have = [a for a in range(3) if prev[a] in content]
                if have and rng.random() < COPY:      # a neighbour's content, the short axes first: constants span cuts
                    w = weights[have] / weights[have].sum()
                    content[(k, j, i)] = content[prev[have[int(rng.choice(len(have), p=w))]]]
                elif rng.random() < 0.3:
                    content[(k, j, i)] = "noise"
                elif rng.random() < 0.5:
                    content[(k, j, i)] = palette[0]              # zero is what the smoothing skips
                else:
                    content[(k, j, i)] = palette[int(rng.integers(1, len(palette)))]
    vol = np.zeros((res[2], res[1], res[0]), NP_DTYPE[fmt])

    def box(key):
        k, j, i = key
        return (slice(edges[2][k], edges[2][k + 1]), slice(edges[1][j], edges[1][j + 1]), slice(edges[0][i], edges[0][i + 1]))

    def dims(key):
        return [s.stop - s.start for s in box(key)]

    info = {"cuts": cuts, "content": content, "nan_at": None, "ninf_at": None, "inf_box": None}
    if fmt == FLOAT:
        # +inf: the box that holds the most whole cells with their rims (a fetched block of constant inf needs one)
        def cells_inside(key):
            n = 1
            for s, size in zip(box(key), vol.shape):
                lo = -(-(s.start + (1 if s.start else 0)) // B)
                hi = ((s.stop - (2 if s.stop < size else 0)) // B) if s.stop < size else -(-size // B)
                n *= max(hi - lo, 0)
            return n
        # (the smallest such box, or failing that the largest box)
        keys = sorted(content, key=lambda q: (cells_inside(q) == 0, int(np.prod(dims(q))) * (1 if cells_inside(q) else -1), q))
        info["inf_box"] = keys[0]
        content[keys[0]] = np.inf
    for key, c in content.items():
        part = vol[box(key)]
        if isinstance(c, str) and c == "noise":
            part[...] = _noise(rng, part.shape, fmt)
        elif isinstance(c, str):   # zeros of both signs
            part[...] = np.where(rng.random(part.shape) < 0.5, F32(-0.0), F32(0.0))
        else:
            part[...] = c
    if fmt == FLOAT:
        finite = [q for q, c in content.items() if not isinstance(c, str) and np.isfinite(c) and min(dims(q)) >= 3]
        finite.sort(key=lambda q: (-int(np.prod(dims(q))), q))
        assert finite, "no constant box with an interior"
        s = box(finite[0])
        mid = [int(rng.integers(a.start + 1, a.stop - 1)) for a in s]
        other = list(mid)
        ax = int(np.argmax(dims(finite[0])))
        other[ax] = mid[ax] + 1 if mid[ax] + 1 < s[ax].stop - 1 else mid[ax] - 1   # (next to it: one neighbourhood lost)
        vol[tuple(mid)] = np.nan
        vol[tuple(other)] = -np.inf
        info["nan_at"], info["ninf_at"] = tuple(mid), tuple(other)
    vol.setflags(write=False)
    return vol, info


def patchwork(res, fmt, seed=None):
    """The patchwork of resolution res (x, y, z): a read-only ndarray [z, y, x] of the format's dtype.  seed None: the
    committed seed of the case."""
    return _patchwork(tuple(res), fmt, SEEDS[(tuple(res), fmt)] if seed is None else seed)[0]


def patchwork_info(res, fmt, seed=None):
    """What patchwork() planted: cuts (x, y, z), content per box (z, y, x index), nan_at / ninf_at (z, y, x), inf_box."""
    return _patchwork(tuple(res), fmt, SEEDS[(tuple(res), fmt)] if seed is None else seed)[1]


# ---- predictors

def block_grid(res):
    """Blocks per axis, (z, y, x)."""
    return tuple(-(-n // B) for n in res[::-1])


def constant_cells(cells):
    """(is a finite constant, its value) per cell.  A cell with a NaN holds (-inf, +inf); zeros of both signs compare
    equal."""
    mn, mx = cells[..., 0], cells[..., 1]
    with np.errstate(invalid="ignore"):
        return (mn == mx) & np.isfinite(mn), mn


KINDS = ("x", "y", "z", "edge", "corner")


def _kind(dz, dy, dx):
    n = (dz != 0) + (dy != 0) + (dx != 0)
    if n == 0:
        return "self"
    if n == 1:
        return "x" if dx else ("y" if dy else "z")
    return "edge" if n == 2 else "corner"


def covering_constant(cells, res, margin, zero_only=False, ignore=None):
    """Blocks [bz, by, bx] whose covering cells all hold one finite constant: the block's voxels dilated by margin
    (x, y, z) voxels per axis and clamped to the volume, the cells (shift 3) that hold one of those.  zero_only: the
    constant is a zero.  ignore: a kind of neighbouring cell (KINDS) that is left out -- "its margin set to 0"."""
    ok, val = constant_cells(cells)
    nb = block_grid(res)
    assert cells.shape[:3] == nb, (cells.shape, nb)
    c0, c1 = [], []
    for ax in range(3):                     # z, y, x
        n, m = res[2 - ax], int(margin[2 - ax])
        b = np.arange(nb[ax])
        c0.append(np.maximum(B * b - m, 0) >> 3)
        c1.append(np.minimum(B * b + B - 1 + m, n - 1) >> 3)
    reach = max(int((c1[ax] - c0[ax]).max()) for ax in range(3))
    bz, by, bx = np.meshgrid(*[np.arange(n) for n in nb], indexing="ij")
    own = val
    skip = ok.copy()
    if zero_only:
        skip &= own == 0
    rng = range(-reach, reach + 1)
    for dz in rng:
        for dy in rng:
            for dx in rng:
                if ignore is not None and _kind(dz, dy, dx) == ignore:
                    continue
                idx = [bz + dz, by + dy, bx + dx]
                inside = np.ones(nb, bool)
                for ax in range(3):
                    lo = c0[ax].reshape([-1 if a == ax else 1 for a in range(3)])
                    hi = c1[ax].reshape([-1 if a == ax else 1 for a in range(3)])
                    inside &= (idx[ax] >= lo) & (idx[ax] <= hi)
                if not inside.any():
                    continue
                cz, cy, cx = (np.clip(idx[ax], 0, nb[ax] - 1) for ax in range(3))
                with np.errstate(invalid="ignore"):
                    good = ok[cz, cy, cx] & (val[cz, cy, cx] == own)
                skip &= ~inside | good
    return skip


def filter_skipped(cells, res, radius, median, ignore=None):
    """vrhip_filter_volume: the block dilated by the radius per axis; the smoothing skips zeros only,
    the median any finite constant (its radius is 1 on every axis)."""
    return covering_constant(cells, res, (1, 1, 1) if median else radius, zero_only=not median, ignore=ignore)


def morph_skipped(cells, res, radius, sweep, ignore=None):
    """vrhip_morph_volume, sweep 1 or 2: the block dilated by sweep * radius per axis, any finite
    constant.  A margin of 0 reaches no neighbour."""
    return covering_constant(cells, res, tuple(sweep * int(r) for r in radius), ignore=ignore)


def _region(res, region):
    lo, hi = region if region is not None else ((0, 0, 0), tuple(res))
    return [int(v) for v in lo], [int(v) for v in hi]


def _block_mask(res, first, last):
    """Blocks first[ax] .. last[ax] (x, y, z; inclusive) as a mask [bz, by, bx]; empty where last < first."""
    nb = block_grid(res)
    m = np.ones(nb, bool)
    for ax in range(3):
        b = np.arange(nb[2 - ax])
        m &= ((b >= first[ax]) & (b <= last[ax])).reshape([-1 if a == 2 - ax else 1 for a in range(3)])
    return m


def stats_skipped(cells, res, fmt, window, moments, region=None):
    """vrhip_volume_statistics: (counted, constant, window) masks [bz, by, bx].  Counted: the blocks
    that hold a voxel of the region.  Without moments a block whose cell lies outside the value window is skipped as
    out of window; else a block whose cell is one finite constant is skipped as constant -- with moments only a zero."""
    lo, hi = _region(res, region)
    if any(h <= l for l, h in zip(lo, hi)):
        counted = np.zeros(block_grid(res), bool)
    else:
        counted = _block_mask(res, [l // B for l in lo], [(h - 1) // B for h in hi])
    ok, val = constant_cells(cells)
    with np.errstate(invalid="ignore", over="ignore"):
        s_min = cells[..., 0].astype(F32) * INV_MAX[fmt]
        s_max = cells[..., 1].astype(F32) * INV_MAX[fmt]
        outside = (s_max < F32(window[0])) | (s_min > F32(window[1]))
    win = counted & outside & (not moments)
    const = counted & ~win & ok & ((val == 0) if moments else True)
    return counted, const, win


def _mesh_proves(cells, fmt, iso):
    with np.errstate(invalid="ignore", over="ignore"):
        s_min = cells[..., 0].astype(F32) * INV_MAX[fmt]
        s_max = cells[..., 1].astype(F32) * INV_MAX[fmt]
        return (s_max < F32(iso)) | (s_min >= F32(iso))


def mesh_skipped(cells, res, fmt, iso, region=None):
    """vrhip_isosurface_count / _extract: (counted, skipped) masks [bz, by, bx].  Counted: the blocks
    of 8^3 cubes that hold a cube of the region; skipped: the one cell proves every point outside (s < isoValue) or
    every point inside (s >= isoValue)."""
    lo, hi = _region(res, region)
    hi = [min(h, n - 1) for h, n in zip(hi, res)]
    if any(h <= l for l, h in zip(lo, hi)):
        counted = np.zeros(block_grid(res), bool)
    else:
        counted = _block_mask(res, [l // B for l in lo], [(h - 1) // B for h in hi])
    return counted, counted & _mesh_proves(cells, fmt, iso)


def mesh_points_skipped(cells, res, fmt, iso, region=None):
    """The indexed extraction's point blocks: (counted, skipped).  Counted: the blocks of 8^3 grid
    points that own an edge of the region -- those that hold a point lo <= P <= hi, but for the one whose only such
    point is hi itself."""
    lo, hi = _region(res, region)
    hi = [min(h, n - 1) for h, n in zip(hi, res)]
    if any(h <= l for l, h in zip(lo, hi)):
        counted = np.zeros(block_grid(res), bool)
    else:
        counted = _block_mask(res, [l // B for l in lo], [h // B for h in hi])
        if all(h % B == 0 for h in hi):
            counted[hi[2] // B, hi[1] // B, hi[0] // B] = False
    return counted, counted & _mesh_proves(cells, fmt, iso)


# ---- bounds from the voxels alone: no cell grid, a box of voxels per block

def _box_constant(v, zero_only):
    if v.dtype == F32:
        if not np.isfinite(v).all():
            return False
    c = v.flat[0]
    return bool((v == c).all()) and (not zero_only or c == 0)


def extent_bounds(vol, margin, zero_only=False):
    """(lower, upper) masks [bz, by, bx] for a block-constant skip with margin (x, y, z).  Upper: the block's own
    dilated, clamped extent is one finite constant in the source (a sound kernel skips nothing else).  Lower: the
    extent rounded out to whole cells and widened by their rim, [8 c0 - 1, 8 c1 + 9], is (a kernel whose cells answer
    for no more than that must skip it)."""
    res = vol.shape[::-1]
    nb = block_grid(res)
    lower, upper = np.zeros(nb, bool), np.zeros(nb, bool)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                tight, wide = [], []
                for b, n, m in zip((bz, by, bx), vol.shape, margin[::-1]):
                    lo, hi = max(B * b - int(m), 0), min(B * b + B - 1 + int(m), n - 1)
                    tight.append(slice(lo, hi + 1))
                    wide.append(slice(max(B * (lo >> 3) - 1, 0), B * (hi >> 3) + B + 2))
                upper[bz, by, bx] = _box_constant(vol[tuple(tight)], zero_only)
                lower[bz, by, bx] = _box_constant(vol[tuple(wide)], zero_only)
    return lower, upper


def block_views(vol, rim_lo, rim_hi):
    """Per block (bz, by, bx) the voxels [8 b - rim_lo, 8 b + 7 + rim_hi] clipped to the volume."""
    nb = block_grid(vol.shape[::-1])
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                s = tuple(slice(max(B * b - rim_lo, 0), B * b + B + rim_hi) for b in (bz, by, bx))
                yield (bz, by, bx), vol[s]


def voxel_cells(vol, rim_lo, rim_hi):
    """(min, max) pairs [bz, by, bx, 2] of block_views(): rim (1, 2) is the cells' own extent (cell_tables_ref.
    cell_minmax), (0, 0) a block's voxels, (0, 1) a block's grid points, (1, 1) a block's voxels with the neighbours
    their central differences read.  A box with a NaN is (-inf, +inf)."""
    out = np.empty(block_grid(vol.shape[::-1]) + (2,), F32)
    for at, v in block_views(vol, rim_lo, rim_hi):
        v = v.astype(F32)
        out[at] = (-np.inf, np.inf) if np.isnan(v).any() else (v.min(), v.max())
    return out


# ---- the calls both test files make, and the restatements' results, computed once per process

RADII = [(1, 1, 1), (3, 0, 1), (0, 2, 0)]
LONG_FILTER_RADIUS, LONG_MORPH_RADIUS = (8, 1, 0), (8, 8, 8)
STATS_BINS = [(256, 1), (64, 16)]
# isoValues (normalised): one equal to a palette constant -- its cells are all inside, the >= edge --, one strictly
# between two palette constants
ISO_VALUES = {UCHAR: [F32(77) * INV_MAX[UCHAR], F32(0.5)], USHORT: [F32(300) * INV_MAX[USHORT], F32(0.5)],
              FLOAT: [F32(0.3), F32(1.0)]}
# the value window's lower edge equals a palette constant: that constant is in the window, the zeros are below it
STATS_WINDOW = {UCHAR: (float(ISO_VALUES[UCHAR][0]), 1.0, 0.5), USHORT: (float(ISO_VALUES[USHORT][0]), 1.0, 0.5),
                FLOAT: (float(F32(0.3)), 2.0, 0.5)}
WHOLE_WINDOW = (0.0, 1.0, 0.5)


def filter_radii(res):
    return RADII + ([LONG_FILTER_RADIUS] if tuple(res) == LONG else [])


def morph_radii(res):
    # (0, 0, 0): the block's own cell decides alone -- a cell of constant inf must not
    return RADII + [(0, 0, 0)] + ([LONG_MORPH_RADIUS] if tuple(res) == LONG else [])


def region_of(res):
    """A region (lo, hi) that cuts through the blocks on every face of the volume."""
    return (3, 2, 1), (res[0] - 2, res[1] - 3, res[2] - 1)


def taps_of(radius, seed=6):
    rng = np.random.default_rng(seed + 100 * radius[0] + 10 * radius[1] + radius[2])
    return [rng.uniform(-0.7, 0.9, r + 1).astype(F32) for r in radius]


@functools.lru_cache(maxsize=None)
def filter_want(res, fmt, radius):
    """The restatement's filtered patchwork, read-only; radius None: the median."""
    from tests import filter_ref as fr
    vol = patchwork(res, fmt)
    out = fr.compute(vol, fmt, fr.MEDIAN3) if radius is None else fr.compute(vol, fmt, fr.SEPARABLE, radius, taps_of(radius))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def morph_want(res, fmt, op, shape, radius):
    from tests import morph_ref as mr
    out = mr.compute(patchwork(res, fmt), fmt, op, shape, radius)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_cells(res, fmt):
    from tests.cell_tables_ref import cell_minmax
    out = cell_minmax(patchwork(res, fmt), 3)
    out.setflags(write=False)
    return out


def bits(a):
    return a.view(np.uint32) if a.dtype == F32 else a


def block_slices(mask):
    """The voxel slices [z, y, x] of every block set in mask (beyond the volume they are clipped by the indexing)."""
    return [tuple(slice(B * b, B * b + B) for b in at) for at in np.argwhere(mask)]
