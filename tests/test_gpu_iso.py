"""Technique 4, first-hit isosurface rendering (vr_iso.hip), against its CPU restatement (tests/ref/iso_ref.c, pinned
to the oracle by tests/test_iso_ref.py) with a difference of exactly 0: frames of every voxel type, filter, shading
mode, camera kind and rate with object-order ESS on and off (the skipping must not change a bit), the positions of
the hit in the lookahead, the thresholds where `<` and `<=` differ, every entry point that renders, the rejections,
the renderer's state after an isosurface, the C++ class and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common, iso_ref, mip_ref
from volumerenderercl_amd import (FLOAT, TECH_ISO, TECH_MIP, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT,
                                  VolumeRenderCL, frontend)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")
SEEDS = [3499211612, 581869302, 3890346734, 3586334585, 545404204]
RES = (48, 40, 36)
BG = [0.1, 0.9, 0.5, 0.25]
BOX = ((-0.5, -0.7, -0.3), (0.6, 0.4, 0.8))
VIEWS = common.views()
ALONG_X = frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 0), -90.0), (0.0, 0.0, 2.0))


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits_one_nan(a):
    """The fp32 bit patterns, every NaN as one pattern.  For shaded frames of volumes with non-finite voxels ONLY
    (test_float_volumes): which NaN an invalid operation makes (inf - inf in a gradient next to infinite voxels) is
    the processor's choice, not the definition's -- there a NaN must be a NaN, no more."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _load(vr, vol, fmt, tff, thickness=(1.0, 1.0, 1.0)):
    vr.loadVolumeArrays([vol], fmt, thickness)
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_ISO)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = BG


def _conf(vr, view="rot30", linear=True, ortho=False, rate=1.0, box=None, ess=True, seed=SEEDS[0], iso=0.5, refine=4,
          illum=1):
    vr.setLinearInterpolation(linear)
    vr.setCamOrtho(ortho)
    vr.updateSamplingRate(rate)
    bl, tr = box if box else ((-1, -1, -1), (1, 1, 1))
    vr.setBBox(*bl, *tr)
    vr.setObjEss(ess)
    vr.updateView(VIEWS[view] if isinstance(view, str) else view)
    vr.setSeed(seed)
    vr.setIteration(0)
    vr.setIllumination(illum)
    vr.setIsoValue(iso)
    vr.setIsoRefinement(refine)


def _ref(vr, vol, fmt, tff, W, H, tile=None):
    """The restatement's (rgba, kind, k, t_hit, count) for the renderer's current parameters."""
    cam, rp, rc, _ = common.to_oracle_params(*vr.params())
    rp.iteration = 0
    ip = vr.isoParams()
    return iso_ref.render_tile(vol, fmt, tff, cam, rp, rc, iso_value=ip.isoValue, refine_steps=ip.refineSteps, W=W, H=H,
                               tile=tile)


def _both_ess(vr, vol, fmt, tff, W, H, what, bits=_bits, **conf):
    """The frame with ESS on and off: both equal the restatement.  Returns the restatement's result."""
    ref = None
    for ess in (True, False):
        _conf(vr, ess=ess, **conf)
        img = vr.runRaycastNoGL(W, H)
        li = vr.lastLaunchInfo()
        assert li["technique"] == 4 and li["empty_skip"] == int(ess) and li["frames"] == 1 and li["views"] == 0, li
        assert li["work_items"] == ((W + 7) // 8) * ((H + 7) // 8), li
        assert li["prepass"] == li["phase1_waves"] == li["phase2_waves"] == li["footprint"] == li["samples"] == 0, li
        if ref is None:
            ref = _ref(vr, vol, fmt, tff, W, H)
        bad = np.any(bits(img) != bits(ref[0]), axis=-1)
        assert not bad.any(), "%s, ESS %s: %d pixels differ, first at %s" % (what, ess, bad.sum(), np.argwhere(bad)[0])
    return ref


def _random_volume(fmt, res, seed):
    """Uniform random voxels: no structure for the skipping to lean on.  A third of the volume is left low so that
    rays differ."""
    rng = np.random.default_rng(seed)
    x, y, z = res
    f = rng.random((z, y, x), dtype=np.float32)
    f[:, :, : x // 3] *= 0.25
    if fmt == UCHAR:
        return np.round(f * 255).astype(np.uint8)
    if fmt == USHORT:
        return np.round(f * 65535).astype(np.uint16)
    return f


CAMERAS = {
    "perspective": dict(view="rot30"),
    "orthographic": dict(view="close", ortho=True),
    "inside": dict(view="inside"),
    "clip_box": dict(view="rot30", box=BOX),
}


@pytest.mark.parametrize("illum", [0, 1], ids=["flat", "shaded"])
@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_frames_equal_restatement(vr, fmt, linear, illum):
    """Every camera kind x rates 0.5, 1, 2 on a structured and on a uniform random volume."""
    tff = common.tffs()["opaque"]
    W, H = 80, 56
    for name, vol, iso in (("noise", common.noise_volume(RES, fmt, seed=5, smooth=False), 0.3),
                           ("random", _random_volume(fmt, RES, 9), 0.8)):
        _load(vr, vol, fmt, tff)
        hits = 0
        for cam, ckw in CAMERAS.items():
            for rate in (0.5, 1.0, 2.0):
                ref = _both_ess(vr, vol, fmt, tff, W, H, "%s %s rate %g" % (name, cam, rate), linear=linear, rate=rate,
                                iso=iso, illum=illum, **ckw)
                hit = ref[1] == iso_ref.HIT
                hits += int(hit.sum() > 100)
                if illum and hit.sum() > 100:   # shading varies over the surface
                    assert np.unique(ref[0][hit][:, :3], axis=0).shape[0] > 20
        assert hits >= 9


# ---- where the hit falls in the lookahead

def test_hit_at_the_first_sample(vr):
    """Camera inside the solid, and a clip box through it: k = 0, no refinement, the box caps the surface."""
    vol = np.full((RES[2], RES[1], RES[0]), 200, np.uint8)
    vol[:, :, :4] = 0
    tff = common.tffs()["opaque"]
    _load(vr, vol, UCHAR, tff)
    for cam in ("inside", "clip_box"):
        for linear in (True, False):
            ref = _both_ess(vr, vol, UCHAR, tff, 72, 56, cam, linear=linear, iso=0.5, **CAMERAS[cam])
            hit = ref[1] == iso_ref.HIT
            assert (hit & (ref[2] == 0)).sum() > 500


def test_hit_across_lookahead_rounds(vr):
    """A slab seen along x by an orthographic camera (rate 1: two samples per voxel): the jitter spreads the hit index
    over k = 15, 16 and 17 -- the last position of the first round of 16 and the first two of the second, where
    t_{k-1} comes from the round before -- and, for a deeper slab, over 31, 32, 33."""
    tff = common.tffs()["opaque"]
    for start, want in ((7, (15, 16, 17)), (15, (31, 32, 33))):
        vol = np.zeros((40, 40, 48), np.float32)
        vol[:, :, start:] = 1.0
        _load(vr, vol, FLOAT, tff)
        for linear in (True, False):
            ref = _both_ess(vr, vol, FLOAT, tff, 64, 64, "slab %d" % start, view=ALONG_X, ortho=True, linear=linear,
                            rate=1.0, iso=0.75 if linear else 0.5, refine=4)
            ks = set(np.unique(ref[2][ref[1] == iso_ref.HIT]).tolist())
            assert set(want) <= ks, (start, linear, sorted(ks))


def test_mixed_wave(vr):
    """A small opaque blob across the image plane of an orthographic camera inside an otherwise empty volume: in the
    waves over its rim some lanes hit at k = 0 and their neighbours march to tfar."""
    vol = np.zeros((40, 40, 40), np.uint8)
    vol[20:26, 17:23, 18:24] = 255
    tff = common.tffs()["opaque"]
    _load(vr, vol, UCHAR, tff)
    W, H = 64, 64
    ref = _both_ess(vr, vol, UCHAR, tff, W, H, "blob", view="inside", ortho=True, linear=False, iso=0.5)
    kind, k = ref[1], ref[2]
    first = (kind == iso_ref.HIT) & (k == 0)
    nohit = kind == iso_ref.NO_HIT
    assert first.any() and nohit.any()
    mixed = 0
    for y in range(0, H, 8):
        for x in range(0, W, 8):
            mixed += bool(first[y:y + 8, x:x + 8].any() and nohit[y:y + 8, x:x + 8].any())
    assert mixed >= 2


# ---- isoValue

def test_iso_equal_to_the_constant_volume(vr):
    """Every cell's bound EQUALS isoValue: `bound < iso` must not skip (a `<=` would lose every hit); one ulp above,
    nothing hits."""
    tff = common.tffs()["opaque"]
    for fmt, val, iso in ((FLOAT, np.float32(0.6171875), 0.6171875),
                          (UCHAR, np.uint8(51), float(np.float32(51) * (np.float32(1) / np.float32(255))))):
        vol = np.full((RES[2], RES[1], RES[0]), val)
        _load(vr, vol, fmt, tff)
        for linear in (True, False):
            ref = _both_ess(vr, vol, fmt, tff, 72, 56, "constant", linear=linear, iso=iso)
            assert (ref[1] == iso_ref.HIT).sum() > 500
            above = float(np.nextafter(np.float32(iso), np.float32(2)))
            ref = _both_ess(vr, vol, fmt, tff, 72, 56, "constant, one ulp above", linear=linear, iso=above)
            assert not (ref[1] == iso_ref.HIT).any()
            assert np.all(_bits(ref[0]) == _bits(np.asarray(BG, np.float32)))


def test_iso_above_zero_and_negative(vr):
    vol = common.noise_volume(RES, UCHAR, seed=5, smooth=False)
    tff = common.tffs()["opaque"]
    _load(vr, vol, UCHAR, tff)
    ref = _both_ess(vr, vol, UCHAR, tff, 72, 56, "above the maximum", iso=1.25)
    assert np.all(_bits(ref[0]) == _bits(np.asarray(BG, np.float32))) and (ref[1] == iso_ref.NO_HIT).any()
    for iso in (0.0, -0.5):   # nearest: border reads are 0 >= isoValue, every ray that samples hits at k = 0
        for linear in (False, True):
            ref = _both_ess(vr, vol, UCHAR, tff, 72, 56, "iso %g" % iso, linear=linear, iso=iso)
            sampled = ref[1] != iso_ref.MISS
            assert sampled.any() and np.all(ref[1][sampled] == iso_ref.HIT) and np.all(ref[2][sampled] == 0)
    rng = np.random.default_rng(3)
    fvol = rng.normal(-2.0, 1.5, (RES[2], RES[1], RES[0])).astype(np.float32)   # FLOAT values outside [0, 1]
    _load(vr, fvol, FLOAT, tff)
    for linear in (True, False):
        for iso in (-1.0, -3.5, 1.5):
            ref = _both_ess(vr, fvol, FLOAT, tff, 72, 56, "float iso %g" % iso, linear=linear, iso=iso)
            assert (ref[1] == iso_ref.HIT).any()


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("kind", ["nan", "inf_and_huge"])
def test_float_volumes(vr, kind, linear):
    rng = np.random.default_rng(21)
    z, y, x = RES[2], RES[1], RES[0]
    vol = rng.random((z, y, x), dtype=np.float32) * np.float32(0.5)
    vol[:, :, 30:] += np.float32(0.5)
    if kind == "nan":
        vol[rng.random((z, y, x)) < 0.02] = np.nan
        vol[4:12, 6:20, 10:30] = np.nan   # a block of cells that hold nothing else
    else:
        vol[rng.random((z, y, x)) < 0.01] = np.inf
        vol[rng.random((z, y, x)) < 0.01] = -np.inf
        vol[20:, 20:, 20:] *= np.float32(3.0e38)
        vol[20:, 20:, 30:] *= np.float32(-1.0)
    tff = common.tffs()["opaque"]
    _load(vr, vol, FLOAT, tff)
    for cam in ("perspective", "inside"):
        for iso in (0.7, -1.0e30 if kind == "nan" else 1.0e38):
            for illum in (0, 1):   # (shaded: the gradient next to a non-finite voxel may be NaN, in both alike)
                ref = _both_ess(vr, vol, FLOAT, tff, 80, 56, "%s %s" % (kind, cam), bits=_bits_one_nan if illum else _bits,
                                linear=linear, iso=iso, illum=illum, **CAMERAS[cam])
                assert (ref[1] == iso_ref.HIT).any()
                assert illum or np.isfinite(ref[0]).all()


@pytest.mark.parametrize("refine", [0, 1, 4, 16])
def test_refine_steps(vr, refine):
    vol = common.noise_volume(RES, USHORT, seed=5, smooth=False)
    tff = common.tffs()["opaque"]
    _load(vr, vol, USHORT, tff)
    for linear in (True, False):
        ref = _both_ess(vr, vol, USHORT, tff, 80, 56, "refine %d" % refine, linear=linear, rate=0.5, iso=0.3,
                        refine=refine)
        assert ((ref[1] == iso_ref.HIT) & (ref[2] > 0)).sum() > 200


@pytest.mark.parametrize("fmt,res,size,thickness", [
    (UCHAR, (45, 38, 33), (90, 60), (1.0, 1.0, 1.0)),     # no multiple of 4 or of the cell edge; no multiple of 8
    (FLOAT, (45, 38, 33), (90, 60), (1.0, 1.3, 2.0)),     # ... on an anisotropic grid
    (USHORT, (40, 32, 1), (96, 60), (1.0, 1.0, 1.0)),     # one voxel thick
    (FLOAT, (1, 37, 29), (61, 64), (1.0, 1.0, 1.0)),
], ids=["odd_uchar", "odd_float_aniso", "thin_z_ushort", "thin_x_float"])
def test_odd_sizes(vr, fmt, res, size, thickness):
    vol = _random_volume(fmt, res, 4)
    tff = common.tffs()["opaque"]
    _load(vr, vol, fmt, tff, thickness)
    for linear in (True, False):
        for cam in ("perspective", "orthographic"):
            _both_ess(vr, vol, fmt, tff, size[0], size[1], "%s %s" % (cam, linear), linear=linear, iso=0.7,
                      **CAMERAS[cam])


def test_ignored_fields_and_counters(vr):
    vol = common.noise_volume(RES, UCHAR, seed=5, smooth=False)
    tff = common.tffs()["default"]
    _load(vr, vol, UCHAR, tff)
    W, H = 72, 56
    plain = _both_ess(vr, vol, UCHAR, tff, W, H, "plain", iso=0.3)[0]
    vr.setUseGradient(True)
    vr.setContours(True)
    vr.setAerial(True)
    try:
        vr.setStatsEnabled(True)
        _conf(vr, iso=0.3)
        assert _same(vr.runRaycastNoGL(W, H), plain)
        assert vr.getStats() == dict.fromkeys(vr.getStats(), 0)   # the work counters stay zero
    finally:
        vr.setStatsEnabled(False)
        vr.setUseGradient(False)
        vr.setContours(False)
        vr.setAerial(False)
    away = frontend.view_matrix(frontend.DEFAULT_ROTATION, (6.0, 0.0, 2.0))
    ref = _both_ess(vr, vol, UCHAR, tff, W, H, "away", view=away, iso=0.3)
    assert np.all(_bits(ref[0]) == _bits(np.asarray(BG, np.float32)))


# ---- entry points

def _dev(shape, fill=-7.0):
    import torch
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def _sync_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_entry_points(vr):
    import torch
    from volumerenderercl_amd import tiles
    vol = common.noise_volume(RES, USHORT, seed=8, smooth=False)
    tff = common.tffs()["opaque"]
    _load(vr, vol, USHORT, tff)
    W, H, T = 90, 60, 16
    conf = dict(iso=0.3, refine=4, illum=1)
    _conf(vr, **conf)
    full = vr.runRaycastNoGL(W, H)
    assert _same(full, _ref(vr, vol, USHORT, tff, W, H)[0])

    # every tile of the frame: the tile subset equals the full frame's pixels (pixels beyond the frame stay untouched)
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    ids = np.arange(tiles_x * tiles_y, dtype=np.uint32)
    out = _dev((len(ids), T, T, 4))
    vr.render_tiles(W, H, T, T, ids, out.data_ptr())
    got = _sync_np(out)
    li = vr.lastLaunchInfo()
    assert li["technique"] == 4 and li["frames"] == 1 and li["empty_skip"] == 1, li

    def crops(frame, tid):
        tx, ty = int(tid) % tiles_x, int(tid) // tiles_x
        h, w = min(T, H - ty * T), min(T, W - tx * T)
        return frame[ty * T: ty * T + h, tx * T: tx * T + w], (h, w)

    for k, tid in enumerate(ids):
        want, (h, w) = crops(full, tid)
        assert _same(got[k, :h, :w], want), "tile %d" % tid
        assert np.all(got[k, h:] == -7.0) and np.all(got[k, :, w:] == -7.0)

    # 8-bit frames: the quantised float frame, and the frame buffer's bytes afterwards
    _conf(vr, **conf)
    q = vr.render_frame_rgba8(W, H)
    assert np.array_equal(q, frontend.quantise_rgba8(full))
    q2 = np.zeros((H, W, 4), np.uint8)
    vr._check(vr.lib.vrhip_frame_rgba8(vr.handle, W, H, q2.ctypes.data, 0))
    assert np.array_equal(q2, q)

    # batches: 4 seeds, then 4 cameras, equal 4 single frames -- whole frames and a tile subset a stride apart
    views = [VIEWS["default"], VIEWS["rot30"], VIEWS["close"], VIEWS["inside"]]
    sub = np.array([0, 3, 5, 8, 11, 17, 23], dtype=np.uint32)
    for ess in (True, False):
        for use_views in (False, True):
            vs = views if use_views else [VIEWS["rot30"]] * 4
            singles = []
            for v, s in zip(vs, SEEDS):
                _conf(vr, view=v, seed=s, ess=ess, **conf)
                singles.append(vr.runRaycastNoGL(W, H))
            assert not _same(singles[0], singles[1])
            _conf(vr, ess=ess, **conf)
            out = _dev((4, H, W, 4))
            vr.render_batch(W, H, SEEDS[:4], out.data_ptr(), views=vs if use_views else None)
            got = _sync_np(out)
            li = vr.lastLaunchInfo()
            assert li["technique"] == 4 and li["frames"] == 4 and li["views"] == int(use_views), li
            assert li["empty_skip"] == int(ess) and li["work_items"] == 4 * ((W + 7) // 8) * ((H + 7) // 8), li
            for f in range(4):
                assert _same(got[f], singles[f]), "frame %d (views %s, ESS %s)" % (f, use_views, ess)
            stride = (len(sub) + 2) * T * T
            out = _dev((4, stride, 4))
            vr.render_batch(W, H, SEEDS[:4], out.data_ptr(), tile_w=T, tile_h=T, tile_ids=sub, frame_stride=stride,
                            views=vs if use_views else None)
            got = _sync_np(out)
            for f in range(4):
                tl = got[f, : len(sub) * T * T].reshape(len(sub), T, T, 4)
                for k, tid in enumerate(sub):
                    want, (h, w) = crops(singles[f], tid)
                    assert _same(tl[k, :h, :w], want), "frame %d tile %d" % (f, tid)
                assert np.all(got[f, len(sub) * T * T:] == -7.0)
            if use_views and ess:   # 8-bit batches
                q = vr.render_batch(W, H, SEEDS[:4], views=vs, rgba8=True)
                assert np.array_equal(_sync_np(q).reshape(4, H, W, 4), frontend.quantise_rgba8(np.stack(singles)))
    # a frame of the views batch against the restatement itself
    _conf(vr, view=views[2], seed=SEEDS[2], **conf)
    assert _same(vr.runRaycastNoGL(W, H), _ref(vr, vol, USHORT, tff, W, H)[0])
    assert vr.getLastExecTime() > 0.0

    # TileDriver on one rank
    _conf(vr, **conf)
    dev = torch.device("cuda")
    drv = tiles.TileDriver(vr, tiles.TileSplit(W, H, T, T, 1, 0), dev)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    assert _same(_sync_np(drv.render_frame(frame)), full)


# ---- rejections, and the renderer after an isosurface

def _unsupported(vr, call):
    with pytest.raises(RuntimeError) as e:
        call()
    assert str(e.value).strip(), "no message"
    assert vr.lib.vrhip_last_error(vr.handle), "no message"
    return str(e.value)


def test_rejections(vr):
    from volumerenderercl_amd import _lib
    vol = common.noise_volume((32, 32, 32), UCHAR, seed=1)
    tff = common.tffs()["default"]
    _load(vr, vol, UCHAR, tff)
    _conf(vr, iso=0.3)
    W, H = 48, 40
    good = vr.runRaycastNoGL(W, H)
    assert _same(good, _ref(vr, vol, UCHAR, tff, W, H)[0])

    def frame_rc():
        vr._push_params()
        return vr.lib.vrhip_render_frame(vr.handle, W, H, None, 0)

    for illum in (2, 3, 4, 5):
        vr.setIllumination(illum)
        assert frame_rc() == _lib.ERR_UNSUPPORTED, illum
        _unsupported(vr, lambda: vr.runRaycastNoGL(W, H))
    vr.setIllumination(1)
    for setter, name in ((vr.setImgEss, "imgEss"), (vr.setShowESS, "showEss"), (vr.setAmbientOcclusion, "useAO")):
        setter(True)
        try:
            assert frame_rc() == _lib.ERR_UNSUPPORTED, name
            _unsupported(vr, lambda: vr.runRaycastNoGL(W, H))
        finally:
            setter(False)
    vr.setIteration(3)
    assert frame_rc() == _lib.ERR_UNSUPPORTED
    _unsupported(vr, lambda: vr.runRaycastNoGL(W, H))
    vr.setIteration(0)
    vr.setEnvironmentMap(np.full((4, 8, 4), 0.5, np.float32))
    try:
        assert frame_rc() == _lib.ERR_UNSUPPORTED
        _unsupported(vr, lambda: vr.runRaycastNoGL(W, H))
    finally:
        vr.setEnvironmentMap(None)
    # sets of samples, traffic counters
    sd = np.asarray(SEEDS[:2], np.uint32)
    vr._push_params()
    assert vr.lib.vrhip_render_samples(vr.handle, W, H, 0, 0, None, 0, sd.ctypes.data_as(C.c_void_p), 2, 0, None,
                                       0) == _lib.ERR_UNSUPPORTED
    _unsupported(vr, lambda: vr.render_samples(W, H, SEEDS[:2]))
    vr.setIteration(0)
    n = C.c_uint64()
    assert vr.lib.vrhip_count_touched(vr.handle, W, H, C.byref(n), None, 0) == _lib.ERR_UNSUPPORTED
    _unsupported(vr, lambda: vr.countTouched(W, H))
    _unsupported(vr, lambda: vr.countFetched(W, H))
    _unsupported(vr, lambda: vr.countTouchedTiles(W, H, 16, 16, [0, 1]))
    # invalid parameters: VRHIP_ERR_INVALID at render time, and only with technique 4 selected
    for iso, refine in ((float("nan"), 4), (float("inf"), 4), (-float("inf"), 4), (0.3, 17)):
        vr.setIsoValue(iso)
        vr.setIsoRefinement(refine)
        assert frame_rc() == _lib.ERR_INVALID, (iso, refine)
        with pytest.raises(ValueError):
            vr.runRaycastNoGL(W, H)
        vr.setTechnique(TECH_MIP)
        assert frame_rc() == _lib.OK
        vr.setTechnique(TECH_ISO)
    # the renderer still renders
    _conf(vr, iso=0.3)
    assert _same(vr.runRaycastNoGL(W, H), good)
    # RG / RGBA volumes
    for ch in (2, 4):
        multi = np.stack([vol] * ch, axis=-1)
        vr.loadVolumeArrays([multi], UCHAR, channels=ch)
        vr.setTransferFunction(tff)
        _conf(vr, iso=0.3)
        assert frame_rc() == _lib.ERR_UNSUPPORTED
        _unsupported(vr, lambda: vr.runRaycastNoGL(W, H))
    # technique 3 stays unassigned
    _load(vr, vol, UCHAR, tff)
    for tech in (3, 5):
        vr.setTechnique(tech)
        with pytest.raises(ValueError, match="Unknown rendering technique."):
            vr.runRaycastNoGL(W, H)
    vr.setTechnique(TECH_RAYCAST)


def test_state(vr):
    """Techniques 0, 1 and 2 rendered after technique-4 frames on the same renderer still match the oracle or the MIP
    restatement, and the isosurface follows a new transfer function, new voxels, a new time step and a new isoValue:
    nothing goes stale."""
    fmt = UCHAR
    vol = common.noise_volume(RES, fmt, seed=12, smooth=False)
    vol2 = _random_volume(fmt, RES, 13)
    tff, tff2 = common.tffs()["default"], common.tffs()["opaque"]
    W, H = 80, 64
    r = VolumeRenderCL()
    r.initialize()
    try:
        r.loadVolumeArrays([vol, vol2], fmt)
        r.setTransferFunction(tff)
        r.setStatsEnabled(False)
        r.params()[1].backgroundColor[:] = BG

        def iso(v, t, what, value=0.3):
            r.setTechnique(TECH_ISO)
            _conf(r, ess=True, iso=value)
            img = r.runRaycastNoGL(W, H)
            ref = _ref(r, v, fmt, t, W, H)
            assert (ref[1] == iso_ref.HIT).sum() > 50, what
            assert _same(img, ref[0]), what
            return img

        def mip(v, t, what):
            r.setTechnique(TECH_MIP)
            _conf(r, ess=True)
            img = r.runRaycastNoGL(W, H)
            cam, rp, rc, _ = common.to_oracle_params(*r.params())
            rp.iteration = 0
            assert _same(img, mip_ref.render_tile(v, fmt, t, cam, rp, rc, W=W, H=H)[0]), what

        def oracle(tech, v, t, what, ess=True):
            r.setTechnique(tech)
            _conf(r, ess=ess, rate=1.5)
            img = r.runRaycastNoGL(W, H)
            r.setIteration(0)
            ref = common.oracle_frame(r, v, fmt, t, W, H, use_ess=ess)[0]
            assert float(np.abs(img - ref).max()) == 0.0, what

        a = iso(vol, tff, "first")
        oracle(TECH_RAYCAST, vol, tff, "ray caster after the isosurface")
        iso(vol, tff, "isosurface after the ray caster")
        oracle(TECH_PATHTRACE, vol, tff, "path tracer after the isosurface")
        mip(vol, tff, "MIP after the isosurface")
        oracle(TECH_RAYCAST, vol, tff, "ray caster, no ESS", ess=False)
        b = iso(vol, tff, "new isoValue", value=0.45)
        assert not _same(a, b)
        r.setTransferFunction(tff2)
        c = iso(vol, tff2, "new TF", value=0.45)
        assert not _same(b, c)
        oracle(TECH_RAYCAST, vol, tff2, "ray caster, new TF")
        r.setTimestep(1)
        iso(vol2, tff2, "time step 1", value=0.8)
        mip(vol2, tff2, "MIP, time step 1")
        r.setTimestep(0)
        r.loadVolumeArrays([vol2], fmt)
        r.setTransferFunction(tff2)
        r.params()[1].backgroundColor[:] = BG
        iso(vol2, tff2, "new voxels", value=0.8)
        oracle(TECH_RAYCAST, vol2, tff2, "ray caster, new voxels")
        twin = r.shareVolumes()   # a twin that shares the voxels reads the owner's cell grid or its own
        try:
            twin.setTechnique(TECH_ISO)
            twin.setStatsEnabled(False)
            twin.params()[1].backgroundColor[:] = BG
            _conf(twin, ess=True, iso=0.8)
            assert _same(twin.runRaycastNoGL(W, H), _ref(twin, vol2, fmt, tff2, W, H)[0])
            assert twin.lastLaunchInfo()["empty_skip"] == 1
        finally:
            twin.close()
    finally:
        r.close()


# ---- C++ class and CLI

def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_iso")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_iso.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "frames.f32")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    W, H = 56, 40
    a, b, c, d = np.fromfile(out, dtype=np.float32).reshape(4, H, W, 4)
    tff = np.zeros((256, 4), np.uint8)
    tff[:, 0] = np.arange(256)
    tff[:, 1] = 255 - np.arange(256)
    tff[:, 2] = 40
    tff[:, 3] = np.arange(256)
    vr.synthVolume("sphere", (32, 32, 32), UCHAR)
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_ISO)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    view = [2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1]
    _conf(vr, view=view, rate=1.5, seed=77, iso=0.4, refine=6, illum=1)
    mine = vr.runRaycastNoGL(W, H)
    vol = vr.downloadVolume(0)
    ref = _ref(vr, vol, UCHAR, tff, W, H)
    assert _same(mine, ref[0]) and (ref[1] == iso_ref.HIT).sum() > 100
    assert _same(a, mine) and _same(b, mine)           # ESS on, ESS off; the second frame is iteration 0 again
    _conf(vr, view=view, rate=1.5, seed=77, iso=0.4, refine=6, illum=0)
    assert _same(c, vr.runRaycastNoGL(W, H)) and not _same(c, mine)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIllumination(1)
    vr.setIteration(0)
    assert _same(d, vr.runRaycastNoGL(W, H)) and not _same(d, mine)
    vr.setIteration(0)


def _cli(args, tmp_path, name, W, H, dtype=np.float32, suffix=".frames.rgba.f32"):
    out = str(tmp_path / name)
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return np.fromfile(out + suffix, dtype=dtype).reshape(-1, H, W, 4)


CLI_SCENE = ["--synth", "shells", 32, "UCHAR", "--iso", 0.35, "--iso-refine", 3, "--seed", 1234]


def _python_cli_scene(vr):
    """The renderer set up as `vrhip_render` sets itself up for CLI_SCENE; returns (voxels, transfer function)."""
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    tff = frontend.tff_from_stops()
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_ISO)
    vr.setStatsEnabled(False)
    vr.setBackground((1.0, 1.0, 1.0))   # (as the CLI sets it: alpha 0)
    return vr.downloadVolume(0), tff


def test_cli_iso_single_frames(vr, tmp_path):
    """vrhip_render --iso V --iso-refine N without a camera path: the frame-after-frame path through runRaycastNoGL,
    which leaves the iteration at 0 -- two frames in a row (the second would be refused at iteration 1), shaded and
    flat, equal the Python frame and the restatement with a difference of 0; the same two frames over two and three
    tile ranks (--ranks N --loopback) equal the single renderer's."""
    W, H = 72, 56
    view = VIEWS["rot30"]
    args = CLI_SCENE + ["--size", W, H, "--view"] + [repr(float(np.float32(v))) for v in view] + ["--frames", 2]
    vol, tff = _python_cli_scene(vr)
    for illum in (1, 0):
        one = _cli(args + ["--illum", illum], tmp_path, "single%d" % illum, W, H, suffix=".rgba.f32")[0]
        _conf(vr, view=view, rate=1.5, seed=1234, iso=0.35, refine=3, illum=illum)
        img = vr.runRaycastNoGL(W, H)
        ref = _ref(vr, vol, UCHAR, tff, W, H)
        assert (ref[1] == iso_ref.HIT).sum() > 100 and (ref[1] != iso_ref.HIT).any()
        assert _same(img, ref[0]) and _same(one, ref[0]), illum
        for ranks, tile in ((2, 16), (3, 32)):
            got = _cli(args + ["--illum", illum, "--ranks", ranks, "--loopback", "--tile", tile], tmp_path,
                       "ranks%d_%d" % (ranks, illum), W, H, suffix=".rgba.f32")[0]
            assert _same(got, one), (illum, ranks)
    vr.setTechnique(TECH_RAYCAST)


def test_cli_iso_orbit(vr, tmp_path):
    """vrhip_render --iso --orbit: an 8-view turntable in launch sets of 4 -- on one renderer and over two tile ranks
    -- equals the frame-by-frame run and the Python frames of the same views and seeds; --rgba8 writes their
    quantised bytes."""
    W, H, n = 72, 56, 8
    base = CLI_SCENE + ["--size", W, H, "--orbit", 0, 1, 0, n]
    one = _cli(base, tmp_path, "one", W, H)
    assert one.shape[0] == n and not np.array_equal(one[0], one[1])
    fpl = _cli(base + ["--frames-per-launch", 4, "--rgba8"], tmp_path, "fpl", W, H)
    assert _same(fpl, one)
    q = np.fromfile(str(tmp_path / "fpl") + ".frames.rgba.u8", dtype=np.uint8).reshape(n, H, W, 4)
    assert np.array_equal(q, frontend.quantise_rgba8(one))
    ranks = _cli(base + ["--frames-per-launch", 4, "--ranks", 2, "--loopback", "--tile", 16], tmp_path, "ranks", W, H)
    assert _same(ranks, one)
    vol, tff = _python_cli_scene(vr)
    for f, view in enumerate(frontend.orbit_views((0, 1, 0), n)):
        _conf(vr, view=view, rate=1.5, seed=1234, iso=0.35, refine=3)
        img = vr.runRaycastNoGL(W, H)
        assert _same(img, one[f]), "view %d" % f
        if f == 0:
            ref = _ref(vr, vol, UCHAR, tff, W, H)
            assert _same(img, ref[0]) and (ref[1] == iso_ref.HIT).sum() > 100
    vr.setTechnique(TECH_RAYCAST)


@pytest.mark.parametrize("extra", [["--mip"], ["--pathtrace"], ["--ao"], ["--show-ess"], ["--img-ess"],
                                   ["--env", "none.hdr"], ["--iso-refine", 17], None],
                         ids=["mip", "pathtrace", "ao", "show_ess", "img_ess", "env", "refine_17", "refine_without_iso"])
def test_cli_iso_usage_errors(tmp_path, extra):
    """What does not combine with --iso ends with the usage text before anything is loaded; so does --iso-refine
    without --iso."""
    args = CLI_SCENE + extra if extra else ["--synth", "shells", 32, "UCHAR", "--iso-refine", 3]
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", str(tmp_path / "bad")], capture_output=True,
                         text=True, timeout=60)
    assert res.returncode != 0 and res.stderr.startswith("usage: vrhip_render"), res.stderr
    assert "--iso V [--iso-refine N]" in res.stderr
