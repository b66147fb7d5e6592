"""FLOAT volumes of raw values outside [0, 1] -- CT values, values on both sides of [0, 1], values far above
2^31 / n, all-negative fields and fields sprinkled with NaN, +-inf, -0.0, denormals and +-3e38 -- through every
path of the HIP kernels, against the oracle at the suite's bar (TOL, work counters equal), and every
work-skipping device against the frame without it.  The palettes: tests/scenes.float_volume."""
import os

import numpy as np
import pytest

from oracle import vro
from tests import common, scenes
from tests.scenes import FLOAT_PALETTES
from tests.test_gpu_parity import SEED, TOL, _setup
from tests.test_oracle_float_range import _bricks_ref
from volumerenderercl_amd import FLOAT, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _tff(n):
    """The default TF's stops on a table of n entries, with opaque coloured edges: TF[0] and TF[n-1] -- what every
    value outside [0, 1] reads -- differ from each other and from their neighbours."""
    t = frontend.tff_from_stops(n=n)
    t[0] = [200, 40, 20, 120]
    t[-1] = [20, 60, 230, 90]
    return t


def _edge0_tff(n):
    """Opacity only at TF[0]: every cell whose range lies above 0 is empty -- unless a fetch in it can be NaN or
    +-inf, which reads TF[0]."""
    t = np.zeros((n, 4), np.uint8)
    t[0] = [220, 30, 30, 200]
    return t


def _same(got, ref, what=""):
    """Equal within TOL, NaN where the oracle has NaN (assert_array_equal treats NaN as equal)."""
    if TOL == 0:
        np.testing.assert_array_equal(got, ref, err_msg=what)
    else:
        np.testing.assert_allclose(got, ref, rtol=0, atol=TOL, equal_nan=True, err_msg=what)


def _compare(vr, vol, tff, W, H, ess=True, pathtrace=False):
    """tests/test_gpu_parity._compare for frames that may hold NaN: instrumented kernels (image + the six work
    counters) and production kernels, both against the oracle."""
    it = vr.params()[1].iteration
    vr.setStatsEnabled(True)
    got = vr.runRaycastNoGL(W, H)
    gstats = vr.getStats()
    seed = vr.params()[1].seed
    vr.setIteration(it)
    ref, rstats, _ = common.oracle_frame(vr, vol, FLOAT, tff, W, H, use_ess=ess)
    _same(got, ref, "instrumented")
    if pathtrace:
        gstats = dict(gstats, bricks_visited=0, bricks_skipped=0, samples_nominal=0)
    assert gstats == rstats
    vr.setStatsEnabled(False)
    pinned = vr._fixed_seed
    vr.setSeed(seed)
    prod = vr.runRaycastNoGL(W, H)
    vr.setSeed(pinned)
    vr.setIteration(it)
    _same(prod, ref, "production")
    return got, ref, gstats


RAYCAST_MODES = [
    ("rot30", {}),
    ("rot30", {"ess": False, "illum": 0}),
    ("close", {"illum": 2}),
    ("rot30", {"illum": 3, "contours": True}),
    ("close", {"illum": 4, "ess": False}),
    ("inside", {"illum": 5, "aerial": True}),
    ("rot30", {"ao": True, "illum": 0}),
    ("rot30", {"linear": False}),
    ("close", {"show_ess": True, "illum": 0, "background": (0.25, 0.5, 1.0, 1.0)}),
]


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("mode", range(len(RAYCAST_MODES)))
@pytest.mark.parametrize("palette", FLOAT_PALETTES)
def test_raycast_float_range_matches_oracle(vr, palette, mode, n):
    view, kw = RAYCAST_MODES[mode]
    res = (36, 33, 30)
    vol = scenes.float_volume(palette, res, seed=5 + mode)
    tff = _tff(n)
    _setup(vr, vol, FLOAT, tff, common.views()[view], **kw)
    try:
        _, _, st = _compare(vr, vol, tff, 64, 48, ess=kw.get("ess", True))
        assert st["rays_hit"] > 0
    finally:
        _setup(vr, vol, FLOAT, tff, common.views()["rot30"])


@pytest.mark.parametrize("palette,tff,ess", [(p, "edge", True) for p in FLOAT_PALETTES] +
                         [("specials", "transparent", False), ("specials", "edge0", False),
                          ("specials", "edge0", True), ("straddle", "edge0", False)])
def test_empty_runs_float_range_are_exact(palette, tff, ess, monkeypatch):
    """Empty-run skipping forced on (VRHIP_EMPTY_SKIP=1) against the renderer without it (VRHIP_NO_EMPTY_SKIP=1):
    image and work counters bit-equal, and equal to the oracle.  With a fully transparent TF or one opaque only
    at TF[0], a cell holding NaN, +-inf or values beyond FLT_MAX / 2 must not be taken as empty."""
    res = (72, 64, 56)
    vol = scenes.float_volume(palette, res, seed=17)
    table = {"edge": _tff(1024), "transparent": np.zeros((1024, 4), np.uint8), "edge0": _edge0_tff(1024)}[tff]
    W, H = 96, 72
    outs = []
    monkeypatch.setenv("VRHIP_EMPTY_SKIP", "1")
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("VRHIP_NO_EMPTY_SKIP", env)
        r2 = VolumeRenderCL()
        r2.initialize()
        try:
            _setup(r2, vol, FLOAT, table, common.views()["rot30"], ess=ess)
            r2.setStatsEnabled(True)
            outs.append((r2.runRaycastNoGL(W, H).copy(), r2.getStats()))
            r2.setStatsEnabled(False)
            r2.setIteration(0)
            outs.append((r2.runRaycastNoGL(W, H).copy(), None))
            if not env:
                r2.setIteration(0)
                ref, rstats, _ = common.oracle_frame(r2, vol, FLOAT, table, W, H, use_ess=ess)
        finally:
            r2.close()
    _same(outs[0][0], ref)
    assert outs[0][1] == rstats
    np.testing.assert_array_equal(outs[0][0], outs[2][0])
    assert outs[0][1] == outs[2][1]
    np.testing.assert_array_equal(outs[1][0], outs[3][0])
    _same(outs[1][0], ref)


@pytest.mark.parametrize("palette", FLOAT_PALETTES)
def test_footprint_volume_float_range(vr, palette, monkeypatch):
    """The footprint volume's frames (production kernels) equal the oracle's and those without it."""
    res = (48, 48, 48)
    vol = scenes.float_volume(palette, res, seed=12)
    table = _tff(1024)
    W, H = 80, 64
    _setup(vr, vol, FLOAT, table, common.views()["rot30"])
    vr.setStatsEnabled(False)
    got = vr.runRaycastNoGL(W, H)
    vr.setIteration(0)
    ref, _, _ = common.oracle_frame(vr, vol, FLOAT, table, W, H)
    _same(got, ref)
    monkeypatch.setenv("VRHIP_NO_FOOTPRINT", "1")
    r2 = VolumeRenderCL()
    r2.initialize()
    try:
        _setup(r2, vol, FLOAT, table, common.views()["rot30"])
        r2.setStatsEnabled(False)
        plain = r2.runRaycastNoGL(W, H)
    finally:
        r2.close()
    np.testing.assert_array_equal(got, plain)


@pytest.mark.parametrize("palette", FLOAT_PALETTES)
def test_pathtrace_float_range(vr, palette, monkeypatch):
    """Path tracer: against the oracle, and bit-equal with the majorant grid off (VRHIP_PT_NO_CULL) and with
    leaps off (VRHIP_PT_NO_LEAP)."""
    res = (48, 44, 40)
    vol = scenes.float_volume(palette, res, seed=11)
    table = _tff(1024)
    W, H = 64, 56
    _setup(vr, vol, FLOAT, table, common.views()["rot30"], technique=1, ext=60.0)
    try:
        got, _, st = _compare(vr, vol, table, W, H, pathtrace=True)
        assert st["rays_hit"] > 0
        vr.setIteration(0)
        vr.setStatsEnabled(False)
        prod = vr.runRaycastNoGL(W, H).copy()
    finally:
        _setup(vr, vol, FLOAT, table, common.views()["rot30"])
    for env in ("VRHIP_PT_NO_CULL", "VRHIP_PT_NO_LEAP"):
        monkeypatch.setenv(env, "1")
        r2 = VolumeRenderCL()
        r2.initialize()
        try:
            _setup(r2, vol, FLOAT, table, common.views()["rot30"], technique=1, ext=60.0)
            r2.setStatsEnabled(True)
            np.testing.assert_array_equal(r2.runRaycastNoGL(W, H), got, err_msg=env)
            r2.setIteration(0)
            r2.setStatsEnabled(False)
            np.testing.assert_array_equal(r2.runRaycastNoGL(W, H), prod, err_msg=env)
        finally:
            r2.close()
        monkeypatch.delenv(env)


@pytest.mark.parametrize("palette,nch,kw", [("straddle", 4, {}), ("hu", 2, {"aerial": True}),
                                            ("specials", 2, {"ess": False}), ("specials", 4, {"linear": False}),
                                            ("huge", 2, {}), ("negative", 4, {"ess": False})])
def test_multichannel_float_range(vr, palette, nch, kw):
    """CL_RG / CL_RGBA FLOAT volumes: RG reads the TF at |g|, RGBA uses the voxel as colour and opacity."""
    res = (36, 40, 32)
    vol = scenes.float_volume(palette, res, seed=21, nch=nch)
    if nch == 4:
        # opacity channel kept moderate (finite opacity correction): |v| scaled into [0, 0.2]
        a = np.abs(vol[..., 3])
        vol[..., 3] = np.where(np.isfinite(a), a / np.float32(max(1.0, float(np.nanmax(a[np.isfinite(a)])))),
                               a) * np.float32(0.2)
    table = _tff(1024)
    _setup(vr, vol, FLOAT, table, common.views()["rot30"], **kw)
    try:
        _compare(vr, vol, table, 64, 48, ess=kw.get("ess", True))
    finally:
        _setup(vr, vol[..., 0].copy(), FLOAT, table, common.views()["rot30"])


@pytest.mark.parametrize("palette", FLOAT_PALETTES)
def test_downsample_float_range(vr, palette):
    """downsampleVolume (volumeraycast.cl:966-994) on FLOAT: bit-exact, NaN where the oracle has NaN."""
    vol = scenes.float_volume(palette, (131, 134, 140), seed=8)
    vr.loadVolumeArrays([vol], FLOAT)
    np.testing.assert_array_equal(vr.downsampleVolume(0, 2), vro.downsample(vol, FLOAT, 2))


def test_batch_of_views_float_range(vr):
    """One render_batch(..., views=) call equals its frames rendered one at a time."""
    import torch
    vol = scenes.float_volume("specials", (48, 40, 44), seed=30)
    table = _tff(1024)
    _setup(vr, vol, FLOAT, table, common.views()["rot30"])
    W, H = 72, 56
    views = frontend.orbit_views((0.0, 1.0, 0.0), 5)
    seeds = [SEED + 7 * i for i in range(len(views))]
    vr.setStatsEnabled(False)
    out = torch.zeros((len(views), H, W, 4), dtype=torch.float32, device="cuda")
    vr.render_batch(W, H, seeds, out.data_ptr(), views=views)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for f, (v, s) in enumerate(zip(views, seeds)):
        vr.updateView(v)
        vr.setSeed(s)
        vr.setIteration(0)
        np.testing.assert_array_equal(got[f], vr.runRaycastNoGL(W, H), err_msg="frame %d" % f)
    vr.updateView(common.views()["rot30"])


@pytest.mark.parametrize("palette", FLOAT_PALETTES)
@pytest.mark.parametrize("res", [(64, 64, 64), (130, 40, 77)])
def test_bricks_float_range(vr, palette, res):
    """downloadBricks equals the oracle and the float64 restatement of generateBricks (values compared: -0.0 and
    +0.0 are equal); NaN is ignored."""
    vol = scenes.float_volume(palette, res, seed=3)
    vr.loadVolumeArrays([vol], FLOAT)
    vr.setTransferFunction(_tff(1024))
    got = vr.downloadBricks()
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, vro.generate_bricks(vol, FLOAT))
    np.testing.assert_array_equal(got.astype(np.float64), _bricks_ref(vol))


@pytest.mark.parametrize("palette", FLOAT_PALETTES)
def test_cell_grids_float_range(palette, monkeypatch):
    """Both cell builds (one wave per cell, separable streaming) give the exact extrema of the voxels
    [E c - 1, E c + E + 1]^3; a cell with a NaN voxel is (-inf, +inf) in both."""
    res = (64, 56, 40)
    vol = scenes.float_volume(palette, res, seed=31)
    got = {}
    for name, env in (("wave", "1"), ("stream", None)):
        if env:
            monkeypatch.setenv("VRHIP_CELLS_PER_WAVE", env)
        else:
            monkeypatch.delenv("VRHIP_CELLS_PER_WAVE", raising=False)
        r2 = VolumeRenderCL()
        r2.initialize()
        try:
            r2.loadVolumeArrays([vol], FLOAT)
            r2.setTransferFunction(_tff(1024))
            got[name, 8], _ = r2.downloadCells()
            got[name, 4], _ = r2.downloadCells(fine=True)
        finally:
            r2.close()
    v = vol.astype(np.float32)
    for E in (8, 4):
        cz, cy, cx = got["wave", E].shape[:3]
        want = np.empty_like(got["wave", E])
        for k in range(cz):
            for j in range(cy):
                for i in range(cx):
                    box = v[max(E * k - 1, 0):E * k + E + 2, max(E * j - 1, 0):E * j + E + 2,
                            max(E * i - 1, 0):E * i + E + 2]
                    want[k, j, i] = (-np.inf, np.inf) if np.isnan(box).any() else (box.min(), box.max())
        np.testing.assert_array_equal(got["wave", E], want)
        np.testing.assert_array_equal(got["stream", E], want)


@pytest.mark.parametrize("case", range(16))
def test_randomised_float_range_scenes(vr, case):
    """scenes.random_scene with FLOAT forced, remapped v * scale + offset: scale in {1, 255, 4096, 1e7}, offset in
    {0, -scale / 2, -1024}."""
    rng = np.random.default_rng(20261016 + case)
    vol, fmt, tff, view, kw, W, H = scenes.random_scene(rng)
    if fmt != FLOAT:
        vol = vol.astype(np.float32) / np.float32(255.0 if fmt == 0 else 65535.0)
    scale = [1.0, 255.0, 4096.0, 1e7][case % 4]
    offset = [0.0, -scale / 2, -1024.0][(case // 4) % 3]
    vol = (vol.astype(np.float64) * scale + offset).astype(np.float32)
    _setup(vr, vol, FLOAT, tff, view, **kw)
    try:
        vr.updateOutputImg(W, H)
        _compare(vr, vol, tff, W, H, ess=kw["ess"])
    finally:
        _setup(vr, vol, FLOAT, tff, common.views()["rot30"])


def test_cpp_host_cli_float_hu_matches_oracle(tmp_path):
    """vrhip_render on a FLOAT .dat / .raw of Hounsfield values, equal to the oracle on what the loader read."""
    import subprocess
    from volumerenderercl_amd import datraw
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "volumerenderercl_amd", "vrhip_render")
    res = (40, 36, 30)
    vol = scenes.float_volume("hu", res, seed=41)
    vol.tofile(str(tmp_path / "hu.raw"))
    dat = tmp_path / "hu.dat"
    dat.write_text("ObjectFileName: hu.raw\nResolution: %d %d %d\nSliceThickness: 1.0 1.0 1.0\nFormat: FLOAT\n" % res)
    out = str(tmp_path / "frame")
    W, H = 72, 40
    cmd = [exe, "--dat", str(dat), "--size", str(W), str(H), "--rotate", "1", "1", "0", "30",
           "--seed", str(SEED), "--out", out]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    got = np.fromfile(out + ".rgba.f32", dtype=np.float32).reshape(H, W, 4)
    rd = datraw.DatRawReader()
    rd.read_files(datraw.Properties(str(dat)))
    p = rd.properties()
    data = rd.data()[0].reshape(p.volume_res[2], p.volume_res[1], p.volume_res[0])
    assert data.dtype == np.float32 and data.min() < 0     # out-of-range values reach the kernels
    cam = vro.CameraParams()
    cam.viewMat[:] = frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0))
    cam.bbox_bl[:] = [-1, -1, -1, 0]
    cam.bbox_tr[:] = [1, 1, 1, 0]
    rp = vro.RenderingParams()
    rp.backgroundColor[:] = [1, 1, 1, 0]
    rp.modelScale[:] = vro.calc_scaling(p.volume_res[:3], p.slice_thickness) + [0]
    rp.illumType, rp.useLinear, rp.seed = 1, 1, SEED
    rc = vro.RaycastParams()
    rc.samplingRate = 1.5
    _, brf, _ = vro.brick_layout(p.volume_res[:3])
    rc.brickRes[:] = brf + [0]
    ref, _, _ = vro.render_tile(data, vro.FLOAT, frontend.tff_from_stops(), cam, rp, rc, W=W, H=H)
    _same(got, ref)
