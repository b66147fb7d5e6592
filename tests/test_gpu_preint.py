"""Technique 8, ray casting with pre-integrated classification (vr_preint.hip), against its CPU restatement
(tests/ref/preint_ref.c, pinned by tests/test_preint_ref.py) with a difference of exactly 0: frames of every voxel
type, filter, shading mode, projection, sampling rate and table size; object-order ESS on against off, bit for bit,
with the skipping shown to happen; the scene a per-cell skip rule gets wrong; the point of the feature on the device's
frame; every entry point that renders; the rejections; the renderer's state around technique-8 frames; the counters."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common, preint_ref
from tests.test_preint_ref import crossing_rays, peak_scene
from volumerenderercl_amd import FLOAT, TECH_PREINT, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, _lib, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [3499211612, 581869302, 3890346734]
BG = [0.1, 0.9, 0.5, 0.25]
VIEWS = common.views()
SIZE_A, SIZE_B = (40, 32), (37, 29)   # partial 8 x 8 patches on both


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits_one_nan(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _as(fmt, f):
    if fmt == UCHAR:
        return np.round(np.clip(f, 0, 1) * 255).astype(np.uint8)
    if fmt == USHORT:
        return np.round(np.clip(f, 0, 1) * 65535).astype(np.uint16)
    return f.astype(np.float32)


def _ball(fmt, res=(32, 32, 32)):
    """Value = distance from the centre / 1.2 in box units, on res = (x, y, z) voxels: a shell of every value."""
    gx, gy, gz = [(np.arange(n) + 0.5) * 2.0 / n - 1.0 for n in res]
    zz, yy, xx = np.meshgrid(gz, gy, gx, indexing="ij")
    return _as(fmt, np.clip(np.sqrt(xx * xx + yy * yy + zz * zz) / 1.2, 0, 1))


def peak_tff(n=256, at=0.5, width=2, alpha=255):
    t = np.zeros((n, 4), np.uint8)
    t[:, 0] = np.linspace(30, 250, n)
    t[:, 1] = np.linspace(220, 40, n)
    t[:, 2] = 90
    lo = max(0, min(n - width, int(at * n) - width // 2))
    t[lo:lo + width, 3] = alpha
    return t


def step_tff(n=256, at=0.45):
    t = peak_tff(n)
    t[:, 3] = 0
    t[int(at * n):, 3] = 90
    return t


def _setup(vr, vol, fmt, tff):
    vr.loadVolumeArrays([vol], fmt)
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_PREINT)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = BG


def _conf(vr, view="rot30", linear=True, ortho=False, rate=1.0, ess=True, seed=SEEDS[0], illum=1, bbox=None):
    vr.setLinearInterpolation(linear)
    vr.setCamOrtho(ortho)
    vr.updateSamplingRate(rate)
    vr.setBBox(*(bbox or (-1, -1, -1, 1, 1, 1)))
    vr.setObjEss(ess)
    vr.updateView(VIEWS[view] if isinstance(view, str) else view)
    vr.setSeed(seed)
    vr.setIteration(0)
    vr.setIllumination(illum)


def _ref(vr, vol, fmt, tff, W, H, tile=None, max_values=0):
    cam, rp, rc, _ = common.to_oracle_params(*vr.params())
    rp.iteration = 0
    return preint_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H, tile=tile, max_values=max_values)


def _both_ess(vr, vol, fmt, tff, size, what, bits=_bits, **conf):
    """The frame with ESS on and off: both equal the restatement.  Returns the restatement's result."""
    W, H = size
    ref = None
    for ess in (True, False):
        _conf(vr, ess=ess, **conf)
        img = vr.runRaycastNoGL(W, H)
        li = vr.lastLaunchInfo()
        assert li["technique"] == 8 and li["empty_skip"] == int(ess) and li["frames"] == 1 and li["views"] == 0, li
        assert li["work_items"] == ((W + 7) // 8) * ((H + 7) // 8), li
        if ref is None:
            ref = _ref(vr, vol, fmt, tff, W, H)
        bad = np.any(bits(img) != bits(ref[0]), axis=-1)
        assert not bad.any(), "%s, ESS %s: %d pixels differ, first at %s" % (what, ess, bad.sum(), np.argwhere(bad)[0])
    return ref


@pytest.mark.parametrize("illum", [0, 1], ids=["flat", "shaded"])
@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_frames_equal_restatement(vr, fmt, linear, illum):
    """An unstructured non-cubic volume with one axis below a micro-brick (40 x 24 x 3) and the default table at
    37 x 29, perspective; the ball at 32^3 with the narrow peak at 40 x 32, orthographic."""
    noise = common.noise_volume((40, 24, 3), fmt, seed=4, smooth=False)
    tff = frontend.tff_from_stops()
    _setup(vr, noise, fmt, tff)
    ref = _both_ess(vr, noise, fmt, tff, SIZE_B, "noise", linear=linear, illum=illum, view="close", seed=SEEDS[1])
    assert 0 < ref[3].sum() and np.any(ref[0][..., 3] > 0)
    ball = _ball(fmt)
    _setup(vr, ball, fmt, peak_tff())
    ref = _both_ess(vr, ball, fmt, peak_tff(), SIZE_A, "peak", linear=linear, illum=illum, ortho=True, rate=0.5)
    assert 0 < ref[3].sum() < ref[2].sum()


@pytest.mark.parametrize("rate", [0.5, 1.5, 4.0])
def test_sampling_rates_and_a_camera_inside_the_box(vr, rate):
    fmt = UCHAR
    vol = _ball(fmt, (40, 24, 17))
    tff = step_tff()
    _setup(vr, vol, fmt, tff)
    _both_ess(vr, vol, fmt, tff, SIZE_A, "rate %g" % rate, rate=rate)
    inside = list(VIEWS["rot30"])
    inside[3], inside[7], inside[11] = 0.1, -0.2, 0.3    # the eye inside the box: t_0 = 0
    ref = _both_ess(vr, vol, fmt, tff, SIZE_B, "inside, rate %g" % rate, rate=rate, view=inside, seed=SEEDS[2])
    assert np.all(ref[1] == preint_ref.MARCHED)


@pytest.mark.parametrize("n", [1, 2, 256, 4096])
def test_table_sizes(vr, n):
    fmt = USHORT
    vol = _ball(fmt, (24, 24, 24))
    rng = np.random.default_rng(n)
    tff = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    if n > 2:
        tff[rng.random(n) < 0.5, 3] = 0
    _setup(vr, vol, fmt, tff)
    ref = _both_ess(vr, vol, fmt, tff, SIZE_B, "n %d" % n, rate=1.5, illum=0)
    assert ref[3].sum() > 0


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
def test_float_volume_outside_unit_range_with_inf_and_nan(vr, linear):
    vol = (common.noise_volume((29, 24, 21), FLOAT, seed=9, smooth=False) * 3.0 - 1.0).astype(np.float32)
    vol[10, 14, 18] = np.nan
    vol[3, 5, 7] = np.inf
    vol[15, 20, 2] = -np.inf
    tff = peak_tff(64, at=0.4, width=6, alpha=200)
    tff[0, 3] = 120   # entry 0 is what a NaN reads: not transparent
    _setup(vr, vol, FLOAT, tff)
    for illum in (0, 1):
        _both_ess(vr, vol, FLOAT, tff, SIZE_B, "float", bits=_bits_one_nan, linear=linear, illum=illum)


def _scenes():
    ball = _ball(UCHAR)
    opaque = peak_tff()
    opaque[:, 3] = 230
    clear = peak_tff()
    clear[:, 3] = 0
    return {"peak": (ball, peak_tff()), "step": (ball, step_tff()), "transparent": (ball, clear), "opaque": (ball, opaque)}


@pytest.mark.parametrize("scene", ["peak", "step", "transparent", "opaque"])
def test_ess_on_equals_ess_off(vr, scene):
    """... in every bit, and both equal the restatement.  On the peak scene the skipping happens: samples are stepped
    over and fewer values are fetched.  A transparent table: no ray is hit, the frame is the background."""
    vol, tff = _scenes()[scene]
    _setup(vr, vol, UCHAR, tff)
    W, H = SIZE_A
    vr.setStatsEnabled(True)
    try:
        frames, stats = {}, {}
        for ess in (False, True):
            _conf(vr, ess=ess, rate=1.5)
            frames[ess] = vr.runRaycastNoGL(W, H)
            stats[ess] = vr.getStats()
            assert vr.lastLaunchInfo()["instrumented"] == 1
        img, kind, samples, visible, marginal = _ref(vr, vol, UCHAR, tff, W, H)
        assert _same(frames[True], frames[False]) and _same(frames[False], img)
        off, on = stats[False], stats[True]
        assert off["samples_taken"] == int(samples.sum()) and off["bricks_skipped"] == 0
        assert off["samples_shaded"] == on["samples_shaded"] == int(marginal.sum())
        assert on["samples_taken"] + on["bricks_skipped"] == int(samples.sum())
        hit = int(np.sum((kind == preint_ref.MARCHED) & (img[..., 3] > 0)))
        assert off["rays_hit"] == on["rays_hit"] == hit
        for st in (off, on):
            assert st["samples_shaded"] <= st["samples_taken"]
        if scene == "peak":
            assert on["bricks_skipped"] > 0 and on["samples_taken"] < off["samples_taken"] and hit > 0
        if scene == "transparent":
            assert hit == 0 and off["samples_shaded"] == 0
            # the background's colour everywhere; its alpha where the ray misses the box, the accumulated 0 elsewhere
            assert np.all(_bits(frames[True])[..., :3] == _bits(np.array(BG[:3], np.float32)))
            assert np.all(frames[True][..., 3] == np.where(kind == preint_ref.MARCHED, np.float32(0), np.float32(BG[3])))
    finally:
        vr.setStatsEnabled(False)
    # the uncounted kernels
    _both_ess(vr, vol, UCHAR, tff, SIZE_A, scene, rate=1.5)


def test_two_transparent_cells_whose_hull_is_not(vr):
    """0.2 on one side of a plane, 0.8 on the other, the peak at 0.5 between them; an orthographic camera looks along
    the plane's normal (z) at samplingRate 0.04, a step of 10.7 voxels against cells of 4 voxels whose (min, max) cover a
    one-voxel halo.  On the rays whose jitter puts one sample in the cell layer z 8..11 and the next in z 20..23, both
    cells hold one value -- each alone reads transparent entries only -- and the hull of the two reads the peak: the
    case a rule that tests each cell separately gets wrong.  The premise is not taken on trust: the cells the renderer
    built are downloaded, every sample of the restatement is put into its cell, and the slabs whose two cells are each
    transparent while their hull is not are counted.  Those rays must show the peak, ESS on equals ESS off, and the
    switch must actually have left samples out."""
    vol = np.full((32, 32, 32), 0.2, np.float32)
    vol[16:, :, :] = 0.8    # [z, y, x]
    vol = _as(UCHAR, vol)
    tff = peak_tff()
    n = tff.shape[0]
    _setup(vr, vol, UCHAR, tff)
    W, H = SIZE_A
    conf = dict(view="default", ortho=True, linear=True, illum=0, rate=0.04)
    frames = {}
    vr.setStatsEnabled(True)
    try:
        for ess in (True, False):
            _conf(vr, ess=ess, **conf)
            frames[ess] = vr.runRaycastNoGL(W, H)
            skipped = vr.getStats()["bricks_skipped"]
            assert (skipped > 0) == ess
    finally:
        vr.setStatsEnabled(False)
    img, kind, samples, visible, marginal, values, pos = _ref_positions(vr, vol, UCHAR, tff, W, H, 8)
    assert samples.max() <= 8
    assert _same(frames[True], frames[False]) and _same(frames[False], img)
    # the renderer's own cells (the fine grid: the one the kernel reads), with their halo
    cells, shift = vr.downloadCells(fine=True)
    E = 1 << shift
    assert E == 4 and cells.shape[:3] == (8, 8, 8)
    with np.errstate(invalid="ignore"):
        vox = np.floor(pos * 32.0)
        inside = ~np.isnan(pos[..., 0]) & np.all((vox >= 0) & (vox <= 31), axis=-1)   # (border cells: left out)
        # (a sample within a twentieth of a voxel of a cell face may be looked up in the neighbour: left out too)
        frac = pos * 32.0 / E - np.floor(pos * 32.0 / E)
        inside &= np.all((frac > 0.0125) & (frac < 0.9875), axis=-1)
    c = np.where(inside[..., None], vox // E, 0).astype(np.int64)
    mm = cells[c[..., 2], c[..., 1], c[..., 0]] / np.float32(255.0)    # [h, w, k, 2]

    def entries(lo, hi):
        u0, u1 = lo * np.float32(n) - np.float32(0.5), hi * np.float32(n) - np.float32(0.5)
        return np.clip(np.floor(u0), 0, n - 1).astype(np.int64), np.clip(np.floor(u1) + 1, 0, n - 1).astype(np.int64)

    nz = np.concatenate([[0], np.cumsum(tff[:, 3] != 0)])
    i0, i1 = entries(mm[..., 0], mm[..., 1])
    alone = inside & (nz[i1 + 1] == nz[i0])                                 # the cell alone is transparent
    h0, h1 = np.minimum(i0[..., :-1], i0[..., 1:]), np.maximum(i1[..., :-1], i1[..., 1:])
    hull = nz[h1 + 1] == nz[h0]                                             # ... the hull of two neighbours
    trap = alone[..., :-1] & alone[..., 1:] & ~hull
    rays = np.any(trap, axis=-1)
    assert rays.sum() >= 50, rays.sum()
    # each such cell pair holds 0.2 on one side and 0.8 on the other, and so do the two samples
    k = np.argwhere(trap)
    a, b = values[k[:, 0], k[:, 1], k[:, 2]], values[k[:, 0], k[:, 1], k[:, 2] + 1]
    assert np.all(np.minimum(a, b) < 0.3) and np.all(np.maximum(a, b) > 0.7)
    assert np.all(frames[True][..., 3][rays] > 0) and np.all(crossing_rays(values, tff)[rays])


def _ref_positions(vr, vol, fmt, tff, W, H, max_values):
    cam, rp, rc, _ = common.to_oracle_params(*vr.params())
    rp.iteration = 0
    return preint_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H, max_values=max_values, positions=True)


def test_the_peak_between_two_samples_is_seen_on_the_device(vr):
    """Conditions A and B of tests/test_preint_ref.py on the device's frames: technique 8 shows the peak on every ray
    with two consecutive samples either side of it; technique 0 at the same rate misses it on some."""
    vol, tff = peak_scene()
    _setup(vr, vol, UCHAR, tff)
    vr.params()[1].backgroundColor[:] = [0, 0, 0, 0]
    try:
        W, H = SIZE_A
        _conf(vr, rate=0.5, illum=0)
        pre = vr.runRaycastNoGL(W, H)
        ref = _ref(vr, vol, UCHAR, tff, W, H, max_values=96)
        assert _same(pre, ref[0])
        R = crossing_rays(ref[5], tff)
        assert R.sum() > 100 and np.all(pre[..., 3][R] > 0)
        vr.setTechnique(TECH_RAYCAST)
        _conf(vr, rate=0.5, illum=0, ess=False)
        t0 = vr.runRaycastNoGL(W, H)
        vr.setIteration(0)
        assert np.sum(t0[..., 3][R] == 0) >= 1
    finally:
        vr.setTechnique(TECH_PREINT)
        vr.params()[1].backgroundColor[:] = BG


def _dev(shape, fill=-7.0):
    import torch
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def _sync_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_entry_points(vr):
    fmt = USHORT
    ball = _ball(fmt)
    tff = peak_tff(width=8, alpha=120)
    _setup(vr, ball, fmt, tff)
    W, H, T = 48, 32, 16
    _conf(vr, rate=1.5)
    full = vr.runRaycastNoGL(W, H)
    assert _same(full, _ref(vr, ball, fmt, tff, W, H)[0]) and np.any(full[..., 3] > 0)
    # tiles
    tiles_x = (W + T - 1) // T
    ids = np.array([0, 2, 4, 5], dtype=np.uint32)
    out = _dev((len(ids), T, T, 4))
    vr.render_tiles(W, H, T, T, ids, out.data_ptr())
    got = _sync_np(out)
    assert vr.lastLaunchInfo()["technique"] == 8
    for k, tid in enumerate(ids):
        tx, ty = int(tid) % tiles_x, int(tid) // tiles_x
        assert _same(got[k], full[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]), tid
    # an 8-bit frame: the float frame through the project's one quantiser
    _conf(vr, rate=1.5)
    assert np.array_equal(vr.render_frame_rgba8(W, H), frontend.quantise_rgba8(full))
    # batches: three seeds with one camera, three frames with two cameras
    singles = []
    views = [VIEWS["rot30"], VIEWS["close"], VIEWS["rot30"]]
    for v, s in zip(views, SEEDS):
        _conf(vr, view=v, seed=s, rate=1.5)
        singles.append(vr.runRaycastNoGL(W, H))
    one_view = []
    for s in SEEDS:
        _conf(vr, seed=s, rate=1.5)
        one_view.append(vr.runRaycastNoGL(W, H))
    _conf(vr, rate=1.5)
    out = _dev((3, H, W, 4))
    vr.render_batch(W, H, SEEDS[:3], out.data_ptr())
    got = _sync_np(out)
    li = vr.lastLaunchInfo()
    assert li["technique"] == 8 and li["frames"] == 3 and li["views"] == 0, li
    for f in range(3):
        assert _same(got[f], one_view[f]), f
    out = _dev((3, H, W, 4))
    vr.render_batch(W, H, SEEDS[:3], out.data_ptr(), views=views)
    got = _sync_np(out)
    li = vr.lastLaunchInfo()
    assert li["technique"] == 8 and li["frames"] == 3 and li["views"] == 1, li
    for f in range(3):
        assert _same(got[f], singles[f]), f
    assert not _same(singles[0], singles[1])


def test_cli_preint_is_the_python_routes_frame(vr, tmp_path):
    """The C++ route (vrhip_render --preint, through VolumeRenderCL::setTechnique(TECH_PREINT); tests/cxx/
    caller_preint.cpp is its compile-only mirror) writes the Python route's frame; two frames per launch of an orbit
    equal the frames one by one."""
    W, H = 48, 32
    view = VIEWS["rot30"]
    exe = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")
    scene = ["--synth", "shells", 32, "UCHAR", "--seed", 1234, "--size", W, H, "--preint", "--view"] + \
            [repr(float(np.float32(v))) for v in view]

    def cli(args, name, suffix=".rgba.f32"):
        out = str(tmp_path / name)
        res = subprocess.run([exe] + [str(a) for a in scene + args] + ["--out", out], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        return np.fromfile(out + suffix, dtype=np.float32).reshape(-1, H, W, 4)

    one = cli([], "one")[0]
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    tff = frontend.tff_from_stops()
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_PREINT)
    vr.setStatsEnabled(False)
    vr.setBackground((1.0, 1.0, 1.0))
    _conf(vr, view=view, rate=1.5, seed=1234)
    img = vr.runRaycastNoGL(W, H)
    assert _same(one, img) and np.any(img[..., 3] > 0)
    assert _same(img, _ref(vr, vr.downloadVolume(0), UCHAR, tff, W, H)[0])
    orbit = ["--orbit", 0, 1, 0, 4]
    a = cli(orbit, "orbit", suffix=".frames.rgba.f32")
    b = cli(orbit + ["--frames-per-launch", 2], "orbit_fpl", suffix=".frames.rgba.f32")
    assert a.shape[0] == 4 and _same(a, b) and not _same(a[0], a[1])
    vr.setTechnique(TECH_RAYCAST)


def test_rejections(vr):
    vol = common.noise_volume((32, 32, 32), UCHAR, seed=1)
    tff = common.tffs()["default"]
    _setup(vr, vol, UCHAR, tff)
    _conf(vr)
    W, H = SIZE_A
    good = vr.runRaycastNoGL(W, H)

    def frame_rc():
        vr._push_params()
        return vr.lib.vrhip_render_frame(vr.handle, W, H, None, 0)

    def unsupported(call):
        assert frame_rc() == _lib.ERR_UNSUPPORTED
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value).strip()

    for illum in (2, 3, 4, 5):
        vr.setIllumination(illum)
        unsupported(lambda: vr.runRaycastNoGL(W, H))
    vr.setIllumination(1)
    for setter in (vr.setImgEss, vr.setShowESS, vr.setAmbientOcclusion):
        setter(True)
        try:
            unsupported(lambda: vr.runRaycastNoGL(W, H))
        finally:
            setter(False)
    vr.setIteration(3)
    unsupported(lambda: vr.runRaycastNoGL(W, H))
    vr.setIteration(0)
    vr.setEnvironmentMap(np.full((4, 8, 4), 0.5, np.float32))
    try:
        unsupported(lambda: vr.runRaycastNoGL(W, H))
    finally:
        vr.setEnvironmentMap(None)
    sd = np.asarray(SEEDS[:2], np.uint32)
    vr._push_params()
    assert vr.lib.vrhip_render_samples(vr.handle, W, H, 0, 0, None, 0, sd.ctypes.data_as(C.c_void_p), 2, 0, None,
                                       0) == _lib.ERR_UNSUPPORTED
    n = C.c_uint64()
    assert vr.lib.vrhip_count_touched(vr.handle, W, H, C.byref(n), None, 0) == _lib.ERR_UNSUPPORTED
    assert vr.lib.vrhip_count_fetched(vr.handle, W, H, C.byref(n)) == _lib.ERR_UNSUPPORTED
    ids = np.array([0, 1], np.uint32)
    assert vr.lib.vrhip_count_touched_tiles(vr.handle, W, H, 16, 16, ids.ctypes.data_as(C.c_void_p), 2,
                                            C.byref(n)) == _lib.ERR_UNSUPPORTED
    _conf(vr)
    assert _same(vr.runRaycastNoGL(W, H), good)
    # RG / RGBA volumes
    for ch in (2, 4):
        vr.loadVolumeArrays([np.stack([vol] * ch, axis=-1)], UCHAR, channels=ch)
        vr.setTransferFunction(tff)
        _conf(vr)
        unsupported(lambda: vr.runRaycastNoGL(W, H))
    # 7 is unassigned, like 3 and 5
    _setup(vr, vol, UCHAR, tff)
    for tech in (3, 5, 7):
        vr.setTechnique(tech)
        with pytest.raises(ValueError, match="Unknown rendering technique."):
            vr.runRaycastNoGL(W, H)
    vr.setTechnique(TECH_RAYCAST)
    # no transfer function: VRHIP_ERR_NODATA
    r = VolumeRenderCL()
    r.initialize()
    try:
        r.loadVolumeArrays([vol], UCHAR)
        r.setTechnique(TECH_PREINT)
        r._push_params()
        assert r.lib.vrhip_render_frame(r.handle, W, H, None, 0) == _lib.ERR_NODATA
        assert r.lib.vrhip_last_error(r.handle) == b"No transfer function set."
    finally:
        r.close()


def test_state():
    """Technique-0 frames -- single ones and a progressive accumulation (iterations 0 and 1) -- a slice and a depth
    image, before technique-8 frames and with technique-8 frames in between, are bit-identical to those of a renderer
    that never rendered technique 8; vrhip_set_transfer_function between two technique-8 frames takes effect.  (The
    library has ONE frame buffer, which every technique's frame overwrites and which iteration k > 0 accumulates onto:
    an accumulation is started after the technique-8 frame, as setTechnique's reset of the iteration makes a caller do;
    one that CONTINUES over a frame of another technique reads that frame, whatever the technique.)"""
    fmt = UCHAR
    vol = common.noise_volume((37, 29, 21), fmt, seed=12, smooth=False)
    tff, tff2 = common.tffs()["default"], common.tffs()["opaque"]
    W, H = SIZE_B

    def others(r, interleave):
        out = []
        for ess in (True, False):
            if interleave:                            # a technique-8 frame right before every accumulation
                r.setTechnique(TECH_PREINT)
                _conf(r, ess=ess, rate=1.5)
                r.runRaycastNoGL(W, H)
            r.setTechnique(TECH_RAYCAST)
            _conf(r, ess=ess, rate=1.5)
            out.append(r.runRaycastNoGL(W, H))        # iteration 0
            out.append(r.runRaycastNoGL(W, H))        # iteration 1: accumulates onto the first
            r.setIteration(0)
        out.append(r.render_slices(W, H, frontend.axis_slice(2, 0.1)))
        out.append(r.render_depth(W, H, "opacity", threshold=0.3)[0])
        return out

    plain = VolumeRenderCL()
    plain.initialize()
    r = VolumeRenderCL()
    r.initialize()
    try:
        for x in (plain, r):
            x.loadVolumeArrays([vol], fmt)
            x.setStatsEnabled(False)
            x.setTransferFunction(tff)
            x.params()[1].backgroundColor[:] = BG
        want = others(plain, False)
        before = others(r, False)
        r.setTechnique(TECH_PREINT)
        _conf(r)
        a = r.runRaycastNoGL(W, H)
        assert _same(a, _ref(r, vol, fmt, tff, W, H)[0])
        across = others(r, True)
        for p, q, w in zip(before, across, want):
            assert _same(p, w) and _same(q, w)
        # a new table shows in the next technique-8 frame: the integral tables are rebuilt
        r.setTechnique(TECH_PREINT)
        r.setTransferFunction(tff2)
        _conf(r)
        b = r.runRaycastNoGL(W, H)
        assert not _same(a, b) and _same(b, _ref(r, vol, fmt, tff2, W, H)[0])
        r.setTransferFunction(tff)
        _conf(r)
        assert _same(r.runRaycastNoGL(W, H), a)
    finally:
        r.close()
        plain.close()
