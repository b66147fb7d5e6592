"""The CPU side of tests/test_gpu_random_techniques.py (no GPU): the restatement of technique 6 holds against the
oracle on the random scene space, not only on hand-picked scenes; the case lists of the GPU file are not mostly empty
frames; the generator's extras are what they are said to be.  The kernel-argument structs come from
tests/scenes.py oracle_params, which the GPU file checks byte for byte against the renderer's own for every case."""
import numpy as np
import pytest

from oracle import vro
from tests import depth_ref, iso_ref, mip_ref, preint_ref, scenes, tf2d_ref
from tests.test_gpu_random_techniques import DEPTH_MODE_ID, N_CASES, SEED_BASES, depth_mode_of, scene_kw
from volumerenderercl_amd import frontend

SHOWS = 0.01               # a case shows something: at least 1 % of its pixels meet the technique's condition
ENOUGH = (3 * N_CASES + 3) // 4     # ... and three quarters of a technique's cases must


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_extras_are_what_they_say():
    for case in range(N_CASES):
        vol, fmt, tff, view, kw, W, H, ex, _ = scenes.technique_case(SEED_BASES["tf2d"], case)
        lo, hi = scenes.value_range(vol, fmt)
        assert lo <= ex["iso"] <= hi and ex["refine"] in (0, 1, 4)
        assert ex["depth_mode"] in scenes.DEPTH_MODES and ex["g_hi"] in (0.05, 0.12, 0.3)
        t = ex["table"]
        assert t.dtype == np.uint8 and t.ndim == 3 and t.shape[0] in (1, 2, 5, 8, 16) and t.shape[1] in (7, 64, 256)
        assert t.shape[2] == 4 and np.array_equal(t[0, :, :3], t[-1, :, :3])   # rows differ in alpha alone
        assert 33 <= W <= 149 and 33 <= H <= 119 and all(17 <= n <= 69 for n in vol.shape)
        again = scenes.technique_case(SEED_BASES["tf2d"], case)
        assert np.array_equal(again[7]["table"], t) and again[7]["iso"] == ex["iso"]      # seeded: the same every run
    tables = [scenes.technique_case(SEED_BASES["tf2d"], c)[7]["table"] for c in range(N_CASES)]
    assert any(np.any(np.all(t[..., 3] == 0, axis=1)) and t.shape[0] > 1 for t in tables)   # a wholly transparent row
    assert sum(bool(np.any(np.all(t[..., 3] == 0, axis=0))) for t in tables) >= N_CASES // 2   # ... columns


def test_oracle_params_takes_a_view_matrix():
    from tests import common
    m = common.views()["rot30"]
    a = scenes.oracle_params((40, 33, 21), "rot30", {"rate": 2.0})
    b = scenes.oracle_params((40, 33, 21), [float(x) for x in m], {"rate": 2.0})
    for x, y in zip(a, b):
        assert bytes(x) == bytes(y)


@pytest.mark.parametrize("case", range(12))
def test_rows_all_equal_is_the_oracles_technique_0_on_random_scenes(case):
    """tests/test_tf2d_ref.py test_rows_all_equal_is_the_oracles_technique_0 carried to clip boxes, slice thickness,
    orthographic cameras and eyes inside the box: every row of the table the scene's 1-D table, useGradient off
    (technique 0 honours it, technique 6 ignores it) -- the restatement's frame is the oracle's technique-0 frame with
    object-order ESS off, bit for bit."""
    rng = np.random.default_rng(71261021 + case)
    vol, fmt, tff, view, kw, W, H = scenes.random_scene(rng)
    kw = dict(kw, gradient_bg=False)
    cam, rp, rc, pt = scenes.oracle_params(vol.shape[::-1], view, kw, seed=kw["seed"])
    ref, st, _ = vro.render_tile(vol, fmt, tff, cam, rp, rc, pt, use_ess=False, W=W, H=H)
    n_g = (1, 2, 7)[case % 3]
    img, kind, samples, _, _ = tf2d_ref.render_tile(vol, fmt, frontend.tf2d_from_1d(tff, n_g), 0.3, cam, rp, rc, W=W, H=H)
    bad = np.any(_bits(img) != _bits(ref), axis=-1)
    assert not bad.any(), "seed 71261021 + %d: %d pixels differ, first (row, column) %s" % (case, bad.sum(), np.argwhere(bad)[0])
    assert st["samples_taken"] == int(samples.sum()) and st["rays_hit"] == int(np.sum(kind != tf2d_ref.MISS))


def _fractions(name):
    """Per case of the GPU file's list: the fraction of pixels that meet the technique's condition (and, technique 6,
    the fraction of the samples that read columns which are transparent in every row)."""
    shown, clear = [], []
    for case in range(N_CASES):
        mode = depth_mode_of(case) if name == "depth" else None
        vol, fmt, tff, view, kw, W, H, ex, _ = scenes.technique_case(SEED_BASES[name], case, depth_mode=mode)
        cam, rp, rc, _ = scenes.oracle_params(vol.shape[::-1], view, scene_kw(name, kw), seed=kw["seed"])
        if name == "mip":
            met = mip_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H)[2] == mip_ref.SAMPLED
        elif name == "iso":
            met = iso_ref.render_tile(vol, fmt, tff, cam, rp, rc, iso_value=ex["iso"], refine_steps=ex["refine"], W=W,
                                      H=H)[1] == iso_ref.HIT
        elif name == "tf2d":
            _, _, samples, visible, marginal = tf2d_ref.render_tile(vol, fmt, ex["table"], ex["g_hi"], cam, rp, rc, W=W, H=H)
            met = visible > 0
            clear.append(1.0 - float(marginal.sum()) / max(1, int(samples.sum())))
        elif name == "preint":
            met = preint_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H)[3] > 0
        else:
            met = depth_ref.render(vol, fmt, tff, cam, rp, rc, DEPTH_MODE_ID[mode], ex["depth_threshold"], ex["refine"],
                                   W=W, H=H)[2] == depth_ref.HIT
        shown.append(float(met.mean()))
    return shown, clear


@pytest.mark.parametrize("name", sorted(SEED_BASES))
def test_the_case_lists_are_not_mostly_empty(name):
    """MIP: rays that sampled; ISO and the depth modes: hits; techniques 6 and 8: pixels with a visible sample.  For
    technique 6 also: in a third of the cases more than half of the samples read all-transparent columns -- the cases
    where the search stage and the cell bound have work to do."""
    shown, clear = _fractions(name)
    n = sum(f >= SHOWS for f in shown)
    print("%s: %d of %d cases show something; fractions %s" % (name, n, N_CASES, " ".join("%.3f" % f for f in shown)))
    assert n >= ENOUGH, (name, n, shown)
    if name == "tf2d":
        busy = sum(f > 0.5 for f in clear)
        print("tf2d: %d cases with more than half of the samples in transparent columns; %s" % (
            busy, " ".join("%.2f" % f for f in clear)))
        assert 3 * busy >= N_CASES, (busy, clear)
    if name == "depth":   # every mode on its own eight cases
        for k, mode in enumerate(scenes.DEPTH_MODES):
            assert sum(f >= SHOWS for f in shown[k::3]) >= 6, (mode, shown[k::3])
