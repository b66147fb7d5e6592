"""Seeded random scenes (tests/scenes.py random_scene + random_extras: odd non-cubic volumes, slice thickness, empty
slabs, random tables, eyes inside and outside the box, orthographic cameras, clip boxes, five sampling rates, both
filters, odd viewports) through the techniques that had hand-written scenes only: MIP (2), first-hit isosurface (4),
2-D transfer function (6), pre-integrated classification (8) and the depth images.  Each kernel against its CPU
restatement with a difference of exactly 0 in the raw fp32 bits, object-order ESS on and off; the renderer's
kernel-argument structs against tests/scenes.py oracle_params byte for byte, so that tests/test_random_scenes_ref.py
(no GPU) speaks about the same scenes; on every third case the counted kernels and the counter identities the
technique's own file states; on every fourth one batch of three cameras over a random tile subset.

None of random_scene's keys is one these techniques reject (illumination is 0 or 1, there is no AO, showEss, imgEss,
environment map, iteration > 0 or multi-channel volume -- the lists of test_rejections in tests/test_gpu_mip.py,
_iso.py, _tf2d.py and _preint.py), so all of them are kept; "ess" picks the switch for the batch, the frames
themselves are rendered with it on AND off.  useGradient is set where the scene draws it: all four ignore it."""
import numpy as np
import pytest

from tests import common, depth_ref, iso_ref, mip_ref, preint_ref, scenes, tf2d_ref
from volumerenderercl_amd import TECH_ISO, TECH_MIP, TECH_PREINT, TECH_RAYCAST, TECH_TF2D, VolumeRenderCL

pytestmark = pytest.mark.gpu

N_CASES = 24
# one seed base per technique (tests/test_random_scenes_ref.py runs the restatements alone on the same lists)
SEED_BASES = {"mip": 21261021, "iso": 41261021, "tf2d": 61261021, "preint": 81261021, "depth": 91261021}
TECHNIQUE = {"mip": TECH_MIP, "iso": TECH_ISO, "tf2d": TECH_TF2D, "preint": TECH_PREINT, "depth": TECH_RAYCAST}
DEPTH_MODE_ID = {"iso": depth_ref.ISO, "max": depth_ref.MAX, "opacity": depth_ref.OPACITY}


def depth_mode_of(case):
    return scenes.DEPTH_MODES[case % 3]


def scene_kw(name, kw):
    """The scene's keys as oracle_params reads them, with the technique."""
    return dict(kw, technique=TECHNIQUE[name])


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _setup(vr, name, vol, fmt, tff, view, kw, ex):
    vr.loadVolumeArrays([vol], fmt, thickness=kw.get("thickness", (1.0, 1.0, 1.0)))
    vr.setTransferFunction(tff)
    if name == "tf2d":
        vr.setTransferFunction2D(ex["table"], ex["g_hi"])
    vr.setTechnique(TECHNIQUE[name])
    vr.setStatsEnabled(False)
    vr.setIllumination(kw["illum"])
    vr.setLinearInterpolation(kw["linear"])
    vr.setCamOrtho(kw["ortho"])
    vr.setUseGradient(kw["gradient_bg"])
    vr.updateSamplingRate(kw["rate"])
    vr.setBBox(*kw.get("bbox", (-1, -1, -1, 1, 1, 1)))
    if "background" in kw:
        vr.setBackground(kw["background"])          # (alpha becomes 0 like in the reference)
    else:
        vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    vr.setIsoValue(ex["iso"])
    vr.setIsoRefinement(ex["refine"])
    vr.setObjEss(True)
    vr.updateView(view)
    vr.setSeed(kw["seed"])
    vr.setIteration(0)


def _defaults(vr):
    """Every switch a case may have moved, back to its default."""
    vr.setTechnique(TECH_RAYCAST)
    vr.setStatsEnabled(False)
    vr.setIllumination(1)
    vr.setLinearInterpolation(True)
    vr.setCamOrtho(False)
    vr.setUseGradient(False)
    vr.updateSamplingRate(1.5)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    vr.setIsoValue(0.5)
    vr.setIsoRefinement(4)
    vr.setObjEss(True)
    vr.setIteration(0)


def _same_params(vr, res, view, kw):
    """tests/test_gpu_parity.py's check: the renderer-free builder gives the product's own structs, byte for byte."""
    mine = scenes.oracle_params(res, view, kw, seed=vr.params()[1].seed)
    mine[1].iteration = vr.params()[1].iteration
    for a, b in zip(mine, vr.params()):
        assert bytes(a) == bytes(b), type(a).__name__


def _restate(vr, name, vol, fmt, tff, ex, W, H):
    """The restatement's result for the renderer's current parameters; [0] is the frame."""
    cam, rp, rc, _ = common.to_oracle_params(*vr.params())
    rp.iteration = 0
    if name == "mip":
        return mip_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H)
    if name == "iso":
        ip = vr.isoParams()
        return iso_ref.render_tile(vol, fmt, tff, cam, rp, rc, iso_value=ip.isoValue, refine_steps=ip.refineSteps, W=W, H=H)
    if name == "tf2d":
        return tf2d_ref.render_tile(vol, fmt, ex["table"], ex["g_hi"], cam, rp, rc, W=W, H=H)
    return preint_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H)


def _differ(img, ref, what):
    bad = np.any(_bits(img) != _bits(ref), axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (row, column) %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _frames_both_ess(vr, name, W, H, ref, what):
    for ess in (True, False):
        vr.setObjEss(ess)
        img = vr.runRaycastNoGL(W, H)
        li = vr.lastLaunchInfo()
        assert li["technique"] == TECHNIQUE[name] and li["empty_skip"] == int(ess), li
        assert li["frames"] == 1 and li["views"] == 0 and li["work_items"] == ((W + 7) // 8) * ((H + 7) // 8), li
        _differ(img, ref, "%s, ESS %s" % (what, ess))


def _counted(vr, name, W, H, ref, what):
    """The counted kernels, ESS off and on: the uncounted frames, and the identities of tests/test_gpu_iso.py
    test_ignored_fields_and_counters (all zero), tests/test_gpu_tf2d.py test_counters and tests/test_gpu_preint.py
    test_ess_on_equals_ess_off.  (tests/test_gpu_mip.py states none for technique 2: the frames alone.)"""
    vr.setStatsEnabled(True)
    try:
        stats = {}
        for ess in (False, True):
            vr.setObjEss(ess)
            _differ(vr.runRaycastNoGL(W, H), ref[0], "%s, counted, ESS %s" % (what, ess))
            stats[ess] = vr.getStats()
            if name in ("tf2d", "preint"):
                assert vr.lastLaunchInfo()["instrumented"] == 1
    finally:
        vr.setStatsEnabled(False)
    off, on = stats[False], stats[True]
    if name == "iso":
        assert off == dict.fromkeys(off, 0) and on == dict.fromkeys(on, 0)
    if name in ("tf2d", "preint"):
        img, kind, samples, visible, marginal = ref[:5]
        assert off["samples_taken"] == int(samples.sum()) and off["bricks_skipped"] == 0
        assert off["samples_shaded"] == on["samples_shaded"] == int(marginal.sum())
        assert on["samples_taken"] + on["bricks_skipped"] == int(samples.sum())
        hit = int(np.sum((kind == tf2d_ref.MARCHED) & (img[..., 3] > 0)))
        assert off["rays_hit"] == on["rays_hit"] == hit
        for st in (off, on):
            assert st["samples_shaded"] <= st["samples_taken"]
            assert st["samples_nominal"] == 0 and st["bricks_visited"] == 0


def _batch(vr, rng, view, kw, W, H, what):
    """One render_batch of three frames -- three random views, three seeds, tiles of 16 or 32, a random subset --
    against the same regions of the frames rendered alone (tests/test_gpu_parity.py
    test_randomised_batches_of_tile_subsets_equal_their_frames)."""
    import torch
    views = [scenes.random_view(rng) for _ in range(3)]
    seeds = [int(v) for v in rng.integers(1, 1 << 32, size=3)]
    T = int(rng.choice([16, 32]))
    tx, ty = (W + T - 1) // T, (H + T - 1) // T
    ids = np.sort(rng.choice(tx * ty, size=int(rng.integers(1, tx * ty + 1)), replace=False)).astype(np.uint32)
    vr.setObjEss(kw["ess"])
    singles = []
    for v, s in zip(views, seeds):
        vr.updateView(v)
        vr.setSeed(s)
        singles.append(vr.runRaycastNoGL(W, H))
    vr.updateView(view)
    vr.setSeed(kw["seed"])
    out = torch.full((3, len(ids), T, T, 4), -7.0, dtype=torch.float32, device="cuda")
    vr.render_batch(W, H, seeds, out.data_ptr(), tile_w=T, tile_h=T, tile_ids=ids, views=views)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    li = vr.lastLaunchInfo()
    assert li["frames"] == 3 and li["views"] == 1 and li["empty_skip"] == int(kw["ess"]), li
    for f in range(3):
        for k, t in enumerate(ids):
            x0, y0 = (int(t) % tx) * T, (int(t) // tx) * T
            w, h = min(T, W - x0), min(T, H - y0)
            assert _same(got[f, k, :h, :w], singles[f][y0:y0 + h, x0:x0 + w]), "%s: frame %d tile %d" % (what, f, int(t))


def _technique_case(vr, name, case):
    vol, fmt, tff, view, kw, W, H, ex, rng = scenes.technique_case(SEED_BASES[name], case)
    what = "%s seed %d + %d" % (name, SEED_BASES[name], case)
    _setup(vr, name, vol, fmt, tff, view, kw, ex)
    try:
        _same_params(vr, vol.shape[::-1], view, scene_kw(name, kw))
        ref = _restate(vr, name, vol, fmt, tff, ex, W, H)
        assert not np.isnan(ref[0]).any()
        _frames_both_ess(vr, name, W, H, ref[0], what)
        if case % 3 == 0:
            _counted(vr, name, W, H, ref, what)
        if case % 4 == 0:
            _batch(vr, rng, view, kw, W, H, what)
    finally:
        _defaults(vr)


@pytest.mark.parametrize("case", range(N_CASES))
def test_randomised_scenes_mip(vr, case):
    _technique_case(vr, "mip", case)


@pytest.mark.parametrize("case", range(N_CASES))
def test_randomised_scenes_iso(vr, case):
    _technique_case(vr, "iso", case)


@pytest.mark.parametrize("case", range(N_CASES))
def test_randomised_scenes_tf2d(vr, case):
    _technique_case(vr, "tf2d", case)


@pytest.mark.parametrize("case", range(N_CASES))
def test_randomised_scenes_preint(vr, case):
    _technique_case(vr, "preint", case)


def _depth_equal(got, ref, what):
    """tests/test_gpu_depth.py's _equal: xyzt, aux and kind, bit for bit."""
    for label, g, r in zip(("xyzt", "aux", "kind"), got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, label)
        gb, rb = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == np.float32 else (g, r)
        bad = gb != rb
        assert not bad.any(), "%s: %s differs in %d places, first at %s" % (what, label, bad.sum(), np.argwhere(bad)[0])


@pytest.mark.parametrize("case", range(N_CASES))
def test_randomised_scenes_depth(vr, case):
    """render_depth against tests/ref/depth_ref.c, the mode cycling through iso, max and opacity; on every fourth case
    a random rectangle of the frame as well."""
    mode = depth_mode_of(case)
    vol, fmt, tff, view, kw, W, H, ex, rng = scenes.technique_case(SEED_BASES["depth"], case, depth_mode=mode)
    what = "depth %s seed %d + %d" % (mode, SEED_BASES["depth"], case)
    thr, refine = ex["depth_threshold"], ex["refine"]
    _setup(vr, "depth", vol, fmt, tff, view, kw, ex)
    try:
        _same_params(vr, vol.shape[::-1], view, scene_kw("depth", kw))
        cam, rp, rc, _ = common.to_oracle_params(*vr.params())
        rects = [None]
        if case % 4 == 0:
            x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
            rects.append((x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))))
        for rect in rects:
            ref = depth_ref.render(vol, fmt, tff, cam, rp, rc, DEPTH_MODE_ID[mode], thr, refine, W=W, H=H, rect=rect)
            w, h = (rect[2], rect[3]) if rect else (W, H)
            for ess in (True, False):
                vr.setObjEss(ess)
                got = vr.render_depth(W, H, mode, thr, refine, rect=rect)
                di = vr.lastDepthInfo()
                assert di == {"mode": DEPTH_MODE_ID[mode], "work_items": ((w + 7) // 8) * ((h + 7) // 8),
                              "empty_skip": int(ess)}, di
                _depth_equal(got, ref, "%s, rect %s, ESS %s" % (what, rect, ess))
    finally:
        _defaults(vr)
