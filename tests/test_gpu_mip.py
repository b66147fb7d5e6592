"""Technique 2, maximum intensity projection (vr_mip.hip), against its CPU restatement (tests/ref/mip_ref.c, pinned
to the oracle by tests/test_mip_ref.py) with a difference of exactly 0: frames of every voxel type, filter, camera
kind and rate with object-order ESS on and off (the skipping must not change a bit), every entry point that
renders, the rejections, the renderer's state after a projection, the C++ class and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from tests import common, mip_ref
from volumerenderercl_amd import FLOAT, TECH_MIP, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")
SEEDS = [3499211612, 581869302, 3890346734, 3586334585, 545404204]
RES = (48, 40, 36)
BG = [0.1, 0.9, 0.5, 0.25]
BOX = ((-0.5, -0.7, -0.3), (0.6, 0.4, 0.8))
VIEWS = common.views()


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


def _load(vr, vol, fmt, tff, thickness=(1.0, 1.0, 1.0)):
    vr.loadVolumeArrays([vol], fmt, thickness)
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_MIP)
    vr.setIllumination(1)          # ignored
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = BG


def _conf(vr, view="rot30", linear=True, ortho=False, rate=1.0, box=None, ess=True, seed=SEEDS[0]):
    vr.setLinearInterpolation(linear)
    vr.setCamOrtho(ortho)
    vr.updateSamplingRate(rate)
    bl, tr = box if box else ((-1, -1, -1), (1, 1, 1))
    vr.setBBox(*bl, *tr)
    vr.setObjEss(ess)
    vr.updateView(VIEWS[view] if isinstance(view, str) else view)
    vr.setSeed(seed)
    vr.setIteration(0)


def _ref(vr, vol, fmt, tff, W, H, tile=None):
    cam, rp, rc, _ = common.to_oracle_params(*vr.params())
    rp.iteration = 0
    return mip_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H, tile=tile)


def _both_ess(vr, vol, fmt, tff, W, H, what, **conf):
    """The frame with ESS on and off: both equal the restatement.  Returns the restatement's frame."""
    ref = None
    for ess in (True, False):
        _conf(vr, ess=ess, **conf)
        img = vr.runRaycastNoGL(W, H)
        li = vr.lastLaunchInfo()
        assert li["technique"] == 2 and li["empty_skip"] == int(ess) and li["frames"] == 1 and li["views"] == 0, li
        assert li["prepass"] == li["phase1_waves"] == li["phase2_waves"] == li["footprint"] == 0, li
        if ref is None:
            ref = _ref(vr, vol, fmt, tff, W, H)[0]
        bad = np.any(_bits(img) != _bits(ref), axis=-1)
        assert not bad.any(), "%s, ESS %s: %d pixels differ, first at %s" % (what, ess, bad.sum(), np.argwhere(bad)[0])
    return ref


def _random_volume(fmt, res, seed):
    """Uniform random voxels: no structure for the skipping to lean on, every cell's bound close to every ray's
    maximum -- the worst case for an interpolation overshoot.  A quarter of the volume is left low so that rays differ."""
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


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_frames_equal_restatement(vr, fmt, linear):
    """Every camera kind x rates 0.5, 1, 2 on a structured and on a uniform random volume."""
    tff = common.tffs()["opaque"]
    W, H = 96, 64
    for name, vol in (("noise", common.noise_volume(RES, fmt, seed=5, smooth=False)),
                      ("random", _random_volume(fmt, RES, 9))):
        _load(vr, vol, fmt, tff)
        pictures = 0
        for cam, ckw in CAMERAS.items():
            for rate in (0.5, 1.0, 2.0):
                ref = _both_ess(vr, vol, fmt, tff, W, H, "%s %s rate %g" % (name, cam, rate), linear=linear, rate=rate,
                                **ckw)
                pictures += np.unique(ref.reshape(-1, 4), axis=0).shape[0] > 50
        assert pictures >= 9


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("kind", ["constant", "beyond_unit", "nan", "inf_and_huge"])
def test_float_volumes(vr, kind, linear):
    rng = np.random.default_rng(21)
    z, y, x = RES[2], RES[1], RES[0]
    if kind == "constant":          # the bound equals the maximum everywhere
        vol = np.full((z, y, x), 0.6171875, np.float32)
    elif kind == "beyond_unit":     # values outside [0, 1], both signs, and an all-negative block
        vol = rng.normal(0.3, 1.5, (z, y, x)).astype(np.float32)
        vol[: z // 2, :, : x // 2] = -np.abs(vol[: z // 2, :, : x // 2]) - 0.5
    elif kind == "nan":
        vol = rng.random((z, y, x), dtype=np.float32)
        vol[rng.random((z, y, x)) < 0.02] = np.nan
        vol[4:12, 6:20, 10:30] = np.nan   # a block of cells that hold nothing else
    else:
        vol = rng.random((z, y, x), dtype=np.float32)
        vol[rng.random((z, y, x)) < 0.01] = np.inf
        vol[rng.random((z, y, x)) < 0.01] = -np.inf
        vol[20:, 20:, 20:] *= np.float32(3.0e38)
        vol[20:, 20:, 30:] *= np.float32(-1.0)
    tff = common.tffs()["opaque"]
    _load(vr, vol, FLOAT, tff)
    for cam in ("perspective", "inside"):
        ref = _both_ess(vr, vol, FLOAT, tff, 96, 64, "%s %s" % (kind, cam), linear=linear, rate=1.0, **CAMERAS[cam])
        assert np.isfinite(ref).all()


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
            _both_ess(vr, vol, fmt, tff, size[0], size[1], "%s %s" % (cam, linear), linear=linear, rate=1.0,
                      **CAMERAS[cam])


def test_ignored_fields_and_empty_frames(vr):
    """illumType, useGradient, contours, aerial are ignored; a view that misses the box and an empty volume give the
    background."""
    vol = common.noise_volume(RES, UCHAR, seed=5, smooth=False)
    tff = common.tffs()["default"]
    _load(vr, vol, UCHAR, tff)
    W, H = 72, 56
    plain = _both_ess(vr, vol, UCHAR, tff, W, H, "plain")
    vr.setIllumination(5)
    vr.setUseGradient(True)
    vr.setContours(True)
    vr.setAerial(True)
    try:
        _conf(vr)
        assert _same(vr.runRaycastNoGL(W, H), plain)
    finally:
        vr.setIllumination(1)
        vr.setUseGradient(False)
        vr.setContours(False)
        vr.setAerial(False)
    away = frontend.view_matrix(frontend.DEFAULT_ROTATION, (6.0, 0.0, 2.0))
    ref = _both_ess(vr, vol, UCHAR, tff, W, H, "away", view=away)
    assert np.all(_bits(ref) == _bits(np.asarray(BG, np.float32)))
    empty = np.zeros_like(vol)
    _load(vr, empty, UCHAR, tff)
    ref = _both_ess(vr, empty, UCHAR, tff, W, H, "empty")
    assert np.all(_bits(ref) == _bits(np.asarray(BG, np.float32)))


# ---- entry points

def _dev(shape, fill=-7.0):
    import torch
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def _sync_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_entry_points(vr):
    vol = common.noise_volume(RES, USHORT, seed=8, smooth=False)
    tff = common.tffs()["opaque"]
    _load(vr, vol, USHORT, tff)
    W, H, T = 90, 60, 16
    _conf(vr)
    full = vr.runRaycastNoGL(W, H)
    assert _same(full, _ref(vr, vol, USHORT, tff, W, H)[0])

    # a scattered tile subset equals the crops of the frame (pixels beyond the frame stay untouched)
    tiles_x = (W + T - 1) // T
    ids = np.array([0, 3, 5, 8, 11, 17, 23], dtype=np.uint32)
    out = _dev((len(ids), T, T, 4))
    vr.render_tiles(W, H, T, T, ids, out.data_ptr())
    got = _sync_np(out)
    li = vr.lastLaunchInfo()
    assert li["technique"] == 2 and li["frames"] == 1 and li["empty_skip"] == 1, li

    def crops(frame, k, tid):
        tx, ty = int(tid) % tiles_x, int(tid) // tiles_x
        h, w = min(T, H - ty * T), min(T, W - tx * T)
        return frame[ty * T: ty * T + h, tx * T: tx * T + w], (h, w)

    for k, tid in enumerate(ids):
        want, (h, w) = crops(full, k, tid)
        assert _same(got[k, :h, :w], want), "tile %d" % tid
        assert np.all(got[k, h:] == -7.0) and np.all(got[k, :, w:] == -7.0)

    # 8-bit frames: the quantised float frame, and the frame buffer's bytes afterwards
    _conf(vr)
    q = vr.render_frame_rgba8(W, H)
    assert np.array_equal(q, frontend.quantise_rgba8(full))
    q2 = np.zeros((H, W, 4), np.uint8)
    vr._check(vr.lib.vrhip_frame_rgba8(vr.handle, W, H, q2.ctypes.data, 0))
    assert np.array_equal(q2, q)

    # batches: 5 seeds, then 5 cameras, equal 5 single frames -- whole frames and a tile subset a stride apart
    views = [VIEWS["default"], VIEWS["rot30"], VIEWS["close"], VIEWS["inside"],
             frontend.view_matrix(frontend.DEFAULT_ROTATION, (6.0, 0.0, 2.0))]
    for ess in (True, False):
        for use_views in (False, True):
            vs = views if use_views else [VIEWS["rot30"]] * 5
            singles = []
            for v, s in zip(vs, SEEDS):
                _conf(vr, view=v, seed=s, ess=ess)
                singles.append(vr.runRaycastNoGL(W, H))
            assert not _same(singles[0], singles[1])
            _conf(vr, ess=ess)
            out = _dev((5, H, W, 4))
            vr.render_batch(W, H, SEEDS, out.data_ptr(), views=vs if use_views else None)
            got = _sync_np(out)
            li = vr.lastLaunchInfo()
            assert li["technique"] == 2 and li["frames"] == 5 and li["views"] == int(use_views), li
            assert li["empty_skip"] == int(ess) and li["work_items"] == 5 * ((W + 7) // 8) * ((H + 7) // 8), li
            for f in range(5):
                assert _same(got[f], singles[f]), "frame %d (views %s, ESS %s)" % (f, use_views, ess)
            stride = (len(ids) + 2) * T * T
            out = _dev((5, stride, 4))
            vr.render_batch(W, H, SEEDS, out.data_ptr(), tile_w=T, tile_h=T, tile_ids=ids, frame_stride=stride,
                            views=vs if use_views else None)
            got = _sync_np(out)
            for f in range(5):
                tiles = got[f, : len(ids) * T * T].reshape(len(ids), T, T, 4)
                for k, tid in enumerate(ids):
                    want, (h, w) = crops(singles[f], k, tid)
                    assert _same(tiles[k, :h, :w], want), "frame %d tile %d" % (f, tid)
                assert np.all(got[f, len(ids) * T * T:] == -7.0)
    # the first frame of the views batch against the restatement itself
    _conf(vr, view=views[2], seed=SEEDS[2])
    assert _same(vr.runRaycastNoGL(W, H), _ref(vr, vol, USHORT, tff, W, H)[0])
    assert vr.getLastExecTime() > 0.0


# ---- rejections, and the renderer after a projection

def _unsupported(vr, call):
    with pytest.raises(RuntimeError) as e:
        call()
    assert str(e.value).strip(), "no message"
    assert vr.lib.vrhip_last_error(vr.handle), "no message"
    return str(e.value)


def test_rejections(vr):
    import ctypes as C
    from volumerenderercl_amd import _lib
    vol = common.noise_volume((32, 32, 32), UCHAR, seed=1)
    tff = common.tffs()["default"]
    _load(vr, vol, UCHAR, tff)
    _conf(vr)
    W, H = 48, 40
    good = vr.runRaycastNoGL(W, H)

    def frame_rc():
        vr._push_params()
        return vr.lib.vrhip_render_frame(vr.handle, W, H, None, 0)

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
    # environment map
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
    # the renderer still renders
    _conf(vr)
    assert _same(vr.runRaycastNoGL(W, H), good)
    # RG / RGBA volumes
    for ch in (2, 4):
        multi = np.stack([vol] * ch, axis=-1)
        vr.loadVolumeArrays([multi], UCHAR, channels=ch)
        vr.setTransferFunction(tff)
        _conf(vr)
        assert frame_rc() == _lib.ERR_UNSUPPORTED
        _unsupported(vr, lambda: vr.runRaycastNoGL(W, H))
    # an unknown technique is still an error of its own
    _load(vr, vol, UCHAR, tff)
    vr.setTechnique(3)
    with pytest.raises(ValueError, match="Unknown rendering technique."):
        vr.runRaycastNoGL(W, H)
    vr.setTechnique(TECH_RAYCAST)


def test_other_techniques_after_a_projection(vr):
    """Techniques 0 and 1 rendered after technique-2 frames on the same renderer still match the oracle, and the
    projection follows a new transfer function, new voxels and a new time step: nothing it builds goes stale or
    poisons the others."""
    from oracle import vro
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

        def mip(v, t, what):
            r.setTechnique(TECH_MIP)
            _conf(r, ess=True)
            img = r.runRaycastNoGL(W, H)
            assert _same(img, _ref(r, v, fmt, t, W, H)[0]), what

        def raycast(v, t, what, ess):
            r.setTechnique(TECH_RAYCAST)
            _conf(r, ess=ess, rate=1.5)
            img = r.runRaycastNoGL(W, H)
            r.setIteration(0)
            ref = common.oracle_frame(r, v, fmt, t, W, H, use_ess=ess)[0]
            assert float(np.abs(img - ref).max()) == 0.0, what

        def pathtrace(v, t, what):
            r.setTechnique(TECH_PATHTRACE)
            _conf(r, ess=True)
            img = r.runRaycastNoGL(W, H)
            r.setIteration(0)
            ref = common.oracle_frame(r, v, fmt, t, W, H)[0]
            assert float(np.abs(img - ref).max()) == 0.0, what

        mip(vol, tff, "first")
        raycast(vol, tff, "ray caster after MIP", True)
        mip(vol, tff, "MIP after the ray caster")
        pathtrace(vol, tff, "path tracer after MIP")
        raycast(vol, tff, "ray caster, no ESS", False)
        r.setTransferFunction(tff2)
        mip(vol, tff2, "new TF")
        raycast(vol, tff2, "ray caster, new TF", True)
        r.setTimestep(1)
        mip(vol2, tff2, "time step 1")
        pathtrace(vol2, tff2, "path tracer, time step 1")
        r.setTimestep(0)
        r.loadVolumeArrays([vol2], fmt)
        r.setTransferFunction(tff2)
        r.params()[1].backgroundColor[:] = BG
        mip(vol2, tff2, "new voxels")
        raycast(vol2, tff2, "ray caster, new voxels", True)
        # a twin that shares the voxels projects from the owner's cell grid or its own
        twin = r.shareVolumes()
        try:
            twin.setTechnique(TECH_MIP)
            twin.setStatsEnabled(False)
            twin.params()[1].backgroundColor[:] = BG
            _conf(twin, ess=True)
            assert _same(twin.runRaycastNoGL(W, H), _ref(twin, vol2, fmt, tff2, W, H)[0])
            assert twin.lastLaunchInfo()["empty_skip"] == 1
        finally:
            twin.close()
    finally:
        r.close()


# ---- C++ class and CLI

def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_mip")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_mip.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "frames.f32")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    W, H = 56, 40
    a, b, c = np.fromfile(out, dtype=np.float32).reshape(3, H, W, 4)
    tff = np.zeros((256, 4), np.uint8)
    tff[:, 0] = np.arange(256)
    tff[:, 1] = 255 - np.arange(256)
    tff[:, 2] = 40
    tff[:, 3] = np.arange(256)
    vr.synthVolume("sphere", (32, 32, 32), UCHAR)
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_MIP)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    _conf(vr, view=[2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1], rate=1.5, seed=77)
    vr.setIllumination(1)
    mine = vr.runRaycastNoGL(W, H)
    vol = vr.downloadVolume(0)
    assert _same(mine, _ref(vr, vol, UCHAR, tff, W, H)[0])
    assert _same(a, mine) and _same(b, mine)
    assert np.unique(mine.reshape(-1, 4), axis=0).shape[0] > 50
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)
    assert _same(c, vr.runRaycastNoGL(W, H)) and not _same(c, mine)
    vr.setIteration(0)


def _cli(args, tmp_path, name, W, H, dtype=np.float32, suffix=".frames.rgba.f32"):
    out = str(tmp_path / name)
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return np.fromfile(out + suffix, dtype=dtype).reshape(-1, H, W, 4)


def test_cli_mip_orbit(vr, tmp_path):
    """vrhip_render --mip --orbit: an 8-view turntable in launch sets of 4 equals the frame-by-frame run and the
    Python frames of the same views and seeds; --rgba8 writes their quantised bytes."""
    W, H, n = 72, 56, 8
    base = ["--synth", "shells", 32, "UCHAR", "--size", W, H, "--mip", "--seed", 1234, "--orbit", 0, 1, 0, n]
    one = _cli(base, tmp_path, "one", W, H)
    assert one.shape[0] == n and not np.array_equal(one[0], one[1])
    fpl = _cli(base + ["--frames-per-launch", 4, "--rgba8"], tmp_path, "fpl", W, H)
    assert _same(fpl, one)
    q = np.fromfile(str(tmp_path / "fpl") + ".frames.rgba.u8", dtype=np.uint8).reshape(n, H, W, 4)
    assert np.array_equal(q, frontend.quantise_rgba8(one))
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.setTechnique(TECH_MIP)
    vr.setStatsEnabled(False)
    vr.setBackground((1.0, 1.0, 1.0))   # (as the CLI sets it: alpha 0)
    for f, view in enumerate(frontend.orbit_views((0, 1, 0), n)):
        _conf(vr, view=view, rate=1.5, seed=1234)
        assert _same(vr.runRaycastNoGL(W, H), one[f]), "view %d" % f
    vr.setTechnique(TECH_RAYCAST)


def test_cli_two_modes_one_scene(vr, tmp_path):
    """One tiny scene through two of vrhip_render's output modes, one after the other -- rendered frames (--mip --orbit)
    and slice views -- with no option of a third mode (depth, mesh, statistics) given: each run's files are the Python
    arrays of the same scene."""
    W, H, n = 40, 24, 3
    scene = ["--synth", "sphere", 32, "UCHAR", "--size", W, H]
    frames = _cli(scene + ["--mip", "--seed", 1234, "--orbit", 0, 1, 0, n], tmp_path, "frames", W, H)
    slices = _cli(scene + ["--slice-axis", "Z", 0.25, "--slice-stack", 2], tmp_path, "slices", W, H)
    assert frames.shape[0] == n and slices.shape[0] == 2
    for name in ("frames", "slices"):   # the last frame again, alone
        last = np.fromfile(str(tmp_path / name) + ".rgba.f32", dtype=np.float32).reshape(H, W, 4)
        assert _same(last, (frames if name == "frames" else slices)[-1])
        assert not os.path.exists(str(tmp_path / name) + ".depth.f32")
    vr.synthVolume("sphere", (32, 32, 32), UCHAR)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.setStatsEnabled(False)
    vr.setBackground((1.0, 1.0, 1.0))   # (as the CLI sets it: alpha 0)
    _conf(vr, view=frontend.view_matrix(), rate=1.5, seed=1234)   # (the whole box, linear filtering)
    want = vr.render_slices(W, H, frontend.slice_stack(frontend.axis_slice("z", 0.0), 2, 2.0))
    assert _same(slices, want) and np.unique(want.reshape(-1, 4), axis=0).shape[0] > 1
    vr.setTechnique(TECH_MIP)
    for f, view in enumerate(frontend.orbit_views((0, 1, 0), n)):
        _conf(vr, view=view, rate=1.5, seed=1234)
        assert _same(vr.runRaycastNoGL(W, H), frames[f]), "view %d" % f
    assert np.unique(frames.reshape(-1, 4), axis=0).shape[0] > 1
    vr.setTechnique(TECH_RAYCAST)
