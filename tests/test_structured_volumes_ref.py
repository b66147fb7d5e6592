"""The patchworks of tests/structured_volumes.py are fit to test the operators' block skipping, and the skip predictors
are sound -- shown on the CPU restatements and on the reference's own cells (tests/cell_tables_ref.cell_minmax), no GPU.

Soundness: wherever a predictor says "skipped", the restatement (which knows nothing of cells) gives what the skip
writes -- the constant or 0 for the filters and the morphology, one bin without a gradient for the statistics, no
triangle for the mesh.  Non-vacuity: the skipping is decided in every direction, by every kind of neighbouring cell,
on partial cells, next to two constants that meet, next to inf and NaN.  The thresholds are conditions on the
generator (its seeds are tuned until they hold), not measurements."""
import numpy as np
import pytest

from tests import filter_ref as fr
from tests import mesh_ref
from tests import morph_ref as mr
from tests import stats_ref
from tests import structured_volumes as sv
from tests.structured_volumes import FLOAT, FMT_IDS, FMTS, SHAPES, UCHAR, USHORT

CASES = [(res, fmt) for res in SHAPES for fmt in FMTS]
CASE_IDS = ["%s-%s" % (sv.shape_id(res), FMT_IDS[fmt]) for res, fmt in CASES]
MORPH_OPS = [mr.ERODE, mr.GRADIENT, mr.OPEN, mr.BLACKHAT]
R1 = (1, 1, 1)


def _fill(vol, want, mask, zero, what):
    """At every block of mask `want` holds the source's constant (zero: 0), stored as the skip stores it (+0)."""
    for s in sv.block_slices(mask):
        src, out = vol[s], want[s]
        c = src.flat[0]
        fill = np.zeros((), vol.dtype) if zero or c == 0 else c
        assert (sv.bits(out) == sv.bits(np.asarray(fill, vol.dtype))).all(), (what, s, c, out.flat[0])


@pytest.mark.parametrize("res,fmt", CASES, ids=CASE_IDS)
def test_filter_and_morph_rules_are_sound(res, fmt):
    vol, cells = sv.patchwork(res, fmt), sv.reference_cells(res, fmt)
    _fill(vol, sv.filter_want(res, fmt, None), sv.filter_skipped(cells, res, None, True), False, "median")
    for radius in sv.filter_radii(res):
        _fill(vol, sv.filter_want(res, fmt, radius), sv.filter_skipped(cells, res, radius, False), True, ("separable", radius))
    for radius in sv.morph_radii(res):
        first, second = sv.morph_skipped(cells, res, radius, 1), sv.morph_skipped(cells, res, radius, 2)
        assert not (second & ~first).any()   # (twice the margin proves no more)
        for shape in (mr.BOX, mr.BALL):
            for op in MORPH_OPS:
                mask = second if op in (mr.OPEN, mr.BLACKHAT) else first
                _fill(vol, sv.morph_want(res, fmt, op, shape, radius), mask, op in (mr.GRADIENT, mr.BLACKHAT),
                      (mr.OP_NAMES[op], mr.SHAPE_NAMES[shape], radius))


def _block_region(at, res, region):
    lo, hi = region if region else ((0, 0, 0), res)
    b = at[::-1]   # x, y, z
    return tuple(max(8 * b[a], lo[a]) for a in range(3)), tuple(min(8 * b[a] + 8, hi[a]) for a in range(3))


@pytest.mark.parametrize("res,fmt", CASES, ids=CASE_IDS)
def test_stats_rule_is_sound(res, fmt):
    """The restatement on the voxels of a skipped block alone: out of window, all below or all above; constant, one bin
    of gradient row 0 (or one counter), and with moments only zeros."""
    vol, cells = sv.patchwork(res, fmt), sv.reference_cells(res, fmt)
    seen = {"constant": 0, "window": 0}
    for window in (sv.WHOLE_WINDOW, sv.STATS_WINDOW[fmt]):
        for moments in (False, True):
            for region in (None, sv.region_of(res)):
                counted, const, win = sv.stats_skipped(cells, res, fmt, window, moments, region)
                assert not (const & win).any() and not ((const | win) & ~counted).any()
                if moments:
                    assert not win.any()
                for mask, kind in ((const, "constant"), (win, "window")):
                    for at in np.argwhere(mask):
                        lo, hi = _block_region(tuple(at), res, region)
                        st, hist = stats_ref.compute(vol, fmt, (64, 16), window, (lo, hi), moments)
                        n = int(np.prod([h - l for l, h in zip(lo, hi)]))
                        assert st.voxels == n > 0 and st.nan == 0 and st.gradient_nan == 0
                        assert sorted([st.below, st.above, st.binned])[:2] == [0, 0], (kind, at)
                        if kind == "window":
                            assert st.binned == 0
                        else:
                            assert not hist[1:].any() and np.count_nonzero(hist[0]) == (1 if st.binned else 0)
                            if moments:
                                assert st.min == 0 and st.max == 0 and st.sum == 0 and st.sum_sq == 0
                        seen[kind] += 1
    assert seen["constant"] > 0 and (seen["window"] > 0 or fmt != UCHAR)


@pytest.mark.parametrize("res,fmt", CASES, ids=CASE_IDS)
def test_mesh_rule_is_sound(res, fmt):
    vol, cells = sv.patchwork(res, fmt), sv.reference_cells(res, fmt)
    skipped_some = False
    for iso in sv.ISO_VALUES[fmt]:
        for region in (None, sv.region_of(res)):
            counted, skipped = sv.mesh_skipped(cells, res, fmt, iso, region)
            pcounted, pskipped = sv.mesh_points_skipped(cells, res, fmt, iso, region)
            assert not (skipped & ~counted).any() and not (pskipped & ~pcounted).any() and not (counted & ~pcounted).any()
            lo, hi = region if region else ((0, 0, 0), res)
            for at in np.argwhere(skipped):
                b = tuple(at)[::-1]
                part = (tuple(max(8 * b[a], lo[a]) for a in range(3)), tuple(min(8 * b[a] + 9, hi[a], res[a]) for a in range(3)))
                assert mesh_ref.extract(vol, fmt, iso, region=part)[0].shape[0] == 0, (iso, at)
            # a skipped point block owns no crossed edge: all its points, and the ends of their edges, lie on one side
            for at in np.argwhere(pskipped):
                s = tuple(slice(8 * b, 8 * b + 9) for b in at)
                with np.errstate(invalid="ignore"):
                    inside = vol[s].astype(np.float32) * sv.INV_MAX[fmt] >= iso
                assert inside.all() or not inside.any(), (iso, at)
            skipped_some = skipped_some or (skipped.any() and (counted & ~skipped).any())
    assert skipped_some


# ---- non-vacuity

@pytest.mark.parametrize("res,fmt", CASES, ids=CASE_IDS)
def test_every_case_skips_and_fetches(res, fmt):
    cells = sv.reference_cells(res, fmt)
    masks = {"smoothing": sv.filter_skipped(cells, res, R1, False), "median": sv.filter_skipped(cells, res, None, True),
             "morph": sv.morph_skipped(cells, res, R1, 1)}
    for name, m in masks.items():
        assert 0.2 <= m.mean() <= 0.8, (name, int(m.sum()), m.size)
    if res == sv.LONG:
        assert sv.filter_skipped(cells, res, sv.LONG_FILTER_RADIUS, False).any()
        assert sv.morph_skipped(cells, res, sv.LONG_MORPH_RADIUS, 1).any()     # a margin of 8
        assert sv.morph_skipped(cells, res, sv.LONG_MORPH_RADIUS, 2).any()     # ... and of 16
    if fmt == FLOAT:
        z, y, x = sv.patchwork_info(res, fmt)["nan_at"]
        vol = sv.patchwork(res, fmt)
        assert np.isnan(vol[z, y, x]) and np.isneginf(vol[sv.patchwork_info(res, fmt)["ninf_at"]])
        for m in masks.values():
            assert not m[z // 8, y // 8, x // 8]   # the NaN's own cell is fetched
        assert np.isposinf(cells[z // 8, y // 8, x // 8, 1]) and np.isneginf(cells[z // 8, y // 8, x // 8, 0])


def _extent_values(vol, at):
    """The distinct values over block `at` dilated by one voxel, rounded out to whole cells with their rims."""
    s = []
    for b, n in zip(at, vol.shape):
        lo, hi = max(8 * b - 1, 0), min(8 * b + 8, n - 1)
        s.append(slice(max(8 * (lo >> 3) - 1, 0), 8 * (hi >> 3) + 10))
    return np.unique(vol[tuple(s)])


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_every_direction_decides_somewhere(fmt):
    """Over the case list: every kind of neighbouring cell turns some block's decision alone; a skipped block lies on
    the high edge of an axis whose last cell is partial; a fetched block sees two constants and nothing else; FLOAT: a
    fetched block of constant inf; and the cuts take every offset -3 .. 3 from a multiple of 8 on every axis."""
    turned = {k: 0 for k in sv.KINDS}
    high_edge = two_constants = inf_block = 0
    offsets = [set(), set(), set()]
    palette = {float(np.float32(p)) for p in (sv.PALETTE[fmt] if fmt != FLOAT else [0.0, 0.3, 2.5, -1.5])}
    for res in SHAPES:
        vol, cells = sv.patchwork(res, fmt), sv.reference_cells(res, fmt)
        full = sv.morph_skipped(cells, res, R1, 1)
        for k in sv.KINDS:   # skipped with that kind's cells left out, fetched with them in force
            turned[k] += int((sv.morph_skipped(cells, res, R1, 1, ignore=k) & ~full).sum())
        nb = sv.block_grid(res)
        for ax in range(3):
            if res[2 - ax] % 8:
                high_edge += int(np.take(full, nb[ax] - 1, axis=ax).sum())
        for at in np.argwhere(~full):
            u = _extent_values(vol, tuple(at)).astype(np.float64)
            two_constants += int(u.size == 2 and all(float(v) in palette for v in u))
        inf_cell = np.isposinf(cells[..., 0]) & np.isposinf(cells[..., 1])
        inf_block += int((inf_cell & ~full & ~sv.filter_skipped(cells, res, None, True)).sum())
        for ax, cuts in enumerate(sv.patchwork_info(res, fmt)["cuts"]):
            assert 2 <= len(cuts) <= 4 and all(0 < c < res[ax] for c in cuts)
            offsets[ax] |= {(c + 3) % 8 - 3 for c in cuts}
    assert all(n > 0 for n in turned.values()), turned
    assert high_edge > 0 and two_constants > 0
    assert inf_block > 0 or fmt != FLOAT
    assert all(o == set(range(-3, 4)) for o in offsets), offsets


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_iso_values_and_window_sit_on_the_palette(fmt):
    inv = sv.INV_MAX[fmt]
    s = sorted(float(np.float32(p) * inv) for p in (sv.PALETTE[fmt] if fmt != FLOAT else [0.0, 0.3, 2.5, -1.5]))
    on, between = (float(v) for v in sv.ISO_VALUES[fmt])
    assert on in s and between not in s and any(a < between < b for a, b in zip(s, s[1:]))
    assert sv.STATS_WINDOW[fmt][0] in s
    # ... and the constant on the edge is inside: its cells are skipped as constant, not as out of window
    for res in SHAPES:
        cells = sv.reference_cells(res, fmt)
        _, const, win = sv.stats_skipped(cells, res, fmt, sv.STATS_WINDOW[fmt], False)
        ok, val = sv.constant_cells(cells)
        edge = ok & (val.astype(np.float32) * inv == np.float32(on))
        assert not (edge & win).any() and (edge <= const).all()


def test_the_generator_is_seeded():
    a = sv._patchwork.__wrapped__((37, 21, 29), USHORT, 5)[0]
    b = sv._patchwork.__wrapped__((37, 21, 29), USHORT, 5)[0]
    c = sv._patchwork.__wrapped__((37, 21, 29), USHORT, 6)[0]
    assert np.array_equal(a, b) and not np.array_equal(a, c) and a.dtype == np.uint16 and a.shape == (29, 21, 37)


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_voxel_bounds_bracket_the_predictors(fmt):
    """The two bounds the GPU tests take from the voxels alone do bracket the predictor on the reference's cells."""
    for res in SHAPES:
        vol, cells = sv.patchwork(res, fmt), sv.reference_cells(res, fmt)
        for margin, zero_only in ((R1, False), (R1, True), ((3, 0, 1), False), ((0, 4, 0), True), ((6, 0, 2), False)):
            lower, upper = sv.extent_bounds(vol, margin, zero_only)
            got = sv.covering_constant(cells, res, margin, zero_only)
            assert not (lower & ~got).any() and not (got & ~upper).any(), (res, margin, zero_only)
