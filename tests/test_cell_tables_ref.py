"""The check of the checks of tests/test_gpu_cell_tables.py, without a GPU: a numpy fp32 stand-in for the device's
bound formula (tests/cell_tables_ref.device_standin) passes every assertion on the inputs the GPU tests use, and
three deliberately wrong variants of it are each caught -- the envelope is wide enough for a correct kernel and
narrow enough for a wrong one.  The inputs alone are checked for the edges they are meant to hit."""
import numpy as np
import pytest

from tests import cell_tables_ref as ctr
from tests import common, scenes
from tests.cell_tables_ref import FLOAT, UCHAR, USHORT


def _inputs():
    for fmt, n, seed, table in ctr.KNIFE_CASES:
        vol, tff = ctr.knife_case(fmt, n, seed, table)
        yield "knife %s fmt %d n %d" % (table, fmt, n), fmt, vol, tff
    for fmt in (UCHAR, USHORT, FLOAT):
        vol = common.noise_volume(ctr.NOISE_RES, fmt, seed=40 + fmt, smooth=False)
        for n in ctr.TF_SIZES:
            yield "noise fmt %d n %d" % (fmt, n), fmt, vol, ctr.sized_tff(n)
    for palette in scenes.FLOAT_PALETTES:
        vol = scenes.float_volume(palette, (40, 33, 30), seed=17)
        for n, first in ((1024, False), (257, True), (3, False)):
            yield "%s n %d" % (palette, n), FLOAT, vol, ctr.edge_tff(n, only_first=first)


@pytest.fixture(scope="module")
def inputs():
    out = []
    grids = {}
    for name, fmt, vol, tff in _inputs():
        key = (id(vol), vol.shape, fmt, name.split(" n ")[0])
        if key not in grids:
            grids[key] = {s: ctr.cell_minmax(vol, s) for s in (3, 2)}
        out.append((name, fmt, grids[key], tff))
    return out


def _run(inputs, **variant):
    """Names of the inputs on which the stand-in (or a variant of it) fails an assertion."""
    failed = []
    for name, fmt, grids, tff in inputs:
        try:
            for shift in (3, 2):
                b, words = ctr.device_standin(grids[shift], fmt, tff, **variant)
                ctr.check_bounds(b, grids[shift], fmt, tff, name)
                ctr.check_empty(words, grids[shift], fmt, tff, name)
        except AssertionError as e:
            failed.append((name, str(e).split(":")[1][:60] if ":" in str(e) else str(e)[:60]))
    return failed


def test_a_correct_formula_passes_every_assertion(inputs):
    assert _run(inputs) == []


def test_a_window_narrowed_by_one_entry_is_caught(inputs):
    failed = _run(inputs, widen=(0, 1))
    assert any("below the opacity" in why or "marked empty" in why for _, why in failed), failed


def test_a_narrowed_window_without_the_margin_is_caught(inputs):
    failed = _run(inputs, widen=(0, 1), margin=False)
    assert any("below the opacity" in why or "marked empty" in why for _, why in failed), failed


def test_a_bound_that_is_always_two_is_caught(inputs):
    failed = _run(inputs, always_two=True)
    assert len(failed) == len(inputs), failed
    assert all("above the envelope" in why for _, why in failed), failed


@pytest.mark.parametrize("fmt,n,seed", [c[:3] for c in ctr.KNIFE_CASES if c[3] == "comb"])
def test_knife_edge_inputs_reach_both_edges(fmt, n, seed):
    vol, tff = ctr.knife_case(fmt, n, seed)
    for shift in (3, 2):
        finite, A, E = ctr.reference(ctr.cell_minmax(vol, shift), fmt, tff)
        assert finite.all()
        assert (E == 0).mean() >= 0.05, (shift, (E == 0).mean())
        assert ((A > 0) & (A < E)).sum() > 0
        assert (A <= E * 1.000001).all()


@pytest.mark.parametrize("axis", ["x", "y"])
def test_blob_volume_reaches_every_radius(axis):
    vol = ctr.blob_volume(axis)
    tff = ctr.blob_tff()
    mm = ctr.cell_minmax(vol, 3)
    bound, _ = ctr.device_standin(mm, UCHAR, tff)
    macro = ctr.macro_reference(bound)
    assert sorted(macro.shape) == [2, 3, 33]
    leap = ctr.leap_reference(macro)
    assert set(np.unique(leap)) >= {0, 1, 2, 7, 14, 15, 16}
    assert {len(np.unique(leap[j])) for j in range(7)} != {1}
    assert len({leap[j].tobytes() for j in range(7)}) >= 3      # the levels differ


@pytest.mark.parametrize("res,count", ctr.WORD_CASES)
def test_word_case_volumes_have_the_cell_counts(res, count):
    assert np.prod([-(-r // 4) for r in res]) == count
    assert count % 64 in (0, 1, 31, 32, 33, 63)
