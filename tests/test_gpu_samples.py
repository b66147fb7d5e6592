"""render_samples / vrhip_render_samples: n consecutive iterations of the progressive path-traced image in a few
launch sets (a sample kernel whose work queue holds every patch once per sample, then a fold in sample order),
bit for bit what n one-sample frames leave in the frame buffer.  The reference is always the ORACLE, chained over
the same seeds and iterations with in_accum (as test_pathtrace_accumulates_like_oracle does); every comparison is
np.testing.assert_array_equal."""
import numpy as np
import pytest

from oracle import vro
from tests import common
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _setup(vr, vol, fmt, tff, view, background=(1.0, 1.0, 1.0, 1.0), ext=100.0):
    vr.loadVolumeArrays([vol], fmt)
    vr.setTransferFunction(tff)
    vr.setIllumination(1)
    vr.setLinearInterpolation(True)
    vr.setCamOrtho(False)
    vr.setUseGradient(False)
    vr.setContours(False)
    vr.setAerial(False)
    vr.setObjEss(True)
    vr.updateSamplingRate(1.5)
    vr.setAmbientOcclusion(False)
    vr.setTechnique(1)
    vr.setExtinction(ext)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.setShowESS(False)
    vr.setImgEss(False)
    vr.setEnvironmentMap(None)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = list(background)
    vr.updateView(view)
    vr.setIteration(0)


def _seeds(n):
    mt = frontend.Mt19937()
    return [mt() for _ in range(n)]


def _oracle_chain(vr, vol, fmt, tff, W, H, seeds, first=0, env=None):
    """The oracle's frames for seeds[k] at iteration first + k, each accumulating into the one before; the last
    frame and the per-sample work counters.  Leaves the renderer at iteration `first`."""
    ref, stats = None, []
    for k, seed in enumerate(seeds):
        vr.setSeed(seed)
        vr.setIteration(first + k)
        ref, st, _ = common.oracle_frame(vr, vol, fmt, tff, W, H, in_accum=ref, env=env)
        stats.append(st)
    vr.setIteration(first)
    return ref, stats


NOISE = dict(res=(40, 40, 40), seed=4)
# the default camera direction from further back: the box covers the middle of the frame (1291 of 64x48 rays hit it)
FAR = frontend.view_matrix(translation=(0.0, 0.0, 3.0))


def _noise_scene(vr, fmt=FLOAT, view="rot30", **kw):
    vol = common.noise_volume(NOISE["res"], fmt, seed=NOISE["seed"], smooth=True)
    tff = common.tffs()["default"]
    _setup(vr, vol, fmt, tff, common.views()[view] if isinstance(view, str) else view, **kw)
    return vol, tff


@pytest.mark.parametrize("stats", [False, True])
def test_eight_samples_equal_oracle_chain(vr, stats):
    """Case 1: 8 Mt19937 seeds, 40^3 FLOAT noise, rot30, 64x48 -- production kernels and the stats build, whose
    counters are the sums over the samples."""
    W, H = 64, 48
    vol, tff = _noise_scene(vr)
    seeds = _seeds(8)
    ref, rstats = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds)
    vr.setStatsEnabled(stats)
    try:
        got = vr.render_samples(W, H, seeds)
        assert vr.params()[1].iteration == 8
        info = vr.lastLaunchInfo()
        assert info["samples"] == 1 and info["technique"] == 1 and info["instrumented"] == (1 if stats else 0)
        np.testing.assert_array_equal(got, ref)
        if stats:
            g = vr.getStats()
            assert g["samples_taken"] == sum(s["samples_taken"] for s in rstats)
            assert g["rays_hit"] == sum(s["rays_hit"] for s in rstats)
            assert g["samples_taken"] > 0 and g["rays_hit"] > 0
    finally:
        vr.setStatsEnabled(False)
        vr.setIteration(0)


@pytest.mark.parametrize("stats", [False, True])
def test_continuation_and_chained_sets(vr, stats):
    """Case 2: 3 samples and then 5 more in a second call (first_iteration = 3), and samples_per_launch = 3 (sets
    of 3 + 3 + 2), both equal to the 8-fold chain; with stats the chained sets' counters add up."""
    W, H = 64, 48
    vol, tff = _noise_scene(vr)
    seeds = _seeds(8)
    ref, rstats = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds)
    vr.setStatsEnabled(stats)
    try:
        vr.render_samples(W, H, seeds[:3])
        assert vr.params()[1].iteration == 3
        got = vr.render_samples(W, H, seeds[3:])
        assert vr.params()[1].iteration == 8
        np.testing.assert_array_equal(got, ref)
        vr.setIteration(0)
        got = vr.render_samples(W, H, seeds, samples_per_launch=3)
        assert vr.lastLaunchInfo()["frames"] == 2     # the last set of 3 + 3 + 2
        np.testing.assert_array_equal(got, ref)
        if stats:
            g = vr.getStats()
            assert g["samples_taken"] == sum(s["samples_taken"] for s in rstats)
            assert g["rays_hit"] == sum(s["rays_hit"] for s in rstats)
    finally:
        vr.setStatsEnabled(False)
        vr.setIteration(0)


def test_stale_frame_buffer_does_not_leak_into_iteration_zero(vr):
    """first_iteration == 0: the first sample is written, not averaged -- whatever an earlier image left behind."""
    W, H = 64, 48
    vol, tff = _noise_scene(vr)
    seeds = _seeds(6)
    vr.render_samples(W, H, seeds[3:] + seeds[:3])     # another image in the frame buffer
    vr.setIteration(0)
    ref, _ = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds[:4])
    np.testing.assert_array_equal(vr.render_samples(W, H, seeds[:4]), ref)
    vr.setIteration(0)


def test_miss_and_hit_flip_between_samples(vr):
    """Case 3: a background whose alpha is neither 0 nor 1 and a view in which the box does not fill the frame
    (the oracle finds 60 such pixels among these 8 samples).
    On the box's silhouette the jittered ray hits in one sample (alpha 1, the sample enters the mean) and misses in
    another (the pixel is overwritten with the background, alpha 0.5, and the next sample averages from there)."""
    W, H = 64, 48
    bg = (1.0, 1.0, 1.0, 0.5)
    vol, tff = _noise_scene(vr, view=FAR, background=bg)
    seeds = _seeds(8)
    alphas = []
    for seed in seeds:                                  # every sample on its own, at iteration 0
        vr.setSeed(seed)
        vr.setIteration(0)
        one, _, _ = common.oracle_frame(vr, vol, FLOAT, tff, W, H)
        alphas.append(np.asarray(one)[..., 3])
    alphas = np.stack(alphas)
    assert set(np.unique(alphas).tolist()) == {0.5, 1.0}
    flips = ((alphas == 0.5).any(axis=0) & (alphas == 1.0).any(axis=0))
    assert flips.sum() >= 1, "the scene has no pixel that misses the box in one sample and hits it in another"
    ref, _ = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds)
    got = vr.render_samples(W, H, seeds)
    np.testing.assert_array_equal(got, ref)
    # ... and a background alpha of exactly 1, which no alpha value tells from a traced sample's w = 1
    vol, tff = _noise_scene(vr, view=FAR, background=(0.25, 0.5, 0.75, 1.0))
    ref, _ = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds)
    np.testing.assert_array_equal(vr.render_samples(W, H, seeds, samples_per_launch=4), ref)
    vr.setIteration(0)


@pytest.mark.parametrize("fmt", [UCHAR, USHORT])
def test_integer_voxels(vr, fmt):
    """Case 4: the other voxel types, 4 samples."""
    W, H = 64, 48
    vol, tff = _noise_scene(vr, fmt=fmt)
    seeds = _seeds(4)
    ref, _ = _oracle_chain(vr, vol, fmt, tff, W, H, seeds)
    np.testing.assert_array_equal(vr.render_samples(W, H, seeds), ref)
    vr.setIteration(0)


def test_environment_map(vr):
    """Case 4: an environment map stands in for the background -- a missed sample's colour depends on its jittered
    direction, so every sample's own record has to reach the fold."""
    W, H = 88, 64
    rng = np.random.default_rng(11)
    env = rng.random((48, 96, 4), dtype=np.float32) * 1.5
    env[..., 3] = 0.0                  # what the .hdr loader produces
    vol, tff = _noise_scene(vr, view="close", ext=40.0)
    vr.setEnvironmentMap(env)
    try:
        seeds = _seeds(4)
        ref, _ = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds, env=env)
        np.testing.assert_array_equal(vr.render_samples(W, H, seeds), ref)
        vr.setIteration(0)
        vr.updateView(FAR)                             # with pixels that miss the box
        ref, _ = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds, env=env)
        np.testing.assert_array_equal(vr.render_samples(W, H, seeds), ref)
    finally:
        vr.setEnvironmentMap(None)
        vr.setIteration(0)


def test_tile_subset_equals_full_frame(vr):
    """Case 5: every second 32x32 tile of a 120x70 frame, 4 samples, compact [n_tiles][tile_h][tile_w][4] -- into
    device memory and into host memory -- equals the same pixels of the full frame (which equals the oracle)."""
    import torch
    W, H, TW, TH = 120, 70, 32, 32
    vol, tff = _noise_scene(vr)
    seeds = _seeds(4)
    ref, _ = _oracle_chain(vr, vol, FLOAT, tff, W, H, seeds)
    full = vr.render_samples(W, H, seeds)
    np.testing.assert_array_equal(full, ref)
    tiles_x, tiles_y = (W + TW - 1) // TW, (H + TH - 1) // TH
    ids = np.arange(tiles_x * tiles_y, dtype=np.uint32)[::2].copy()
    out = torch.zeros((len(ids), TH, TW, 4), dtype=torch.float32, device="cuda")
    vr.setIteration(0)
    assert vr.render_samples(W, H, seeds, out_dev_ptr=out.data_ptr(), tile_w=TW, tile_h=TH, tile_ids=ids) is None
    torch.cuda.synchronize()
    vr.setIteration(0)
    host = vr.render_samples(W, H, seeds, tile_w=TW, tile_h=TH, tile_ids=ids, samples_per_launch=3)
    vr.setIteration(0)
    assert host.shape == (len(ids), TH, TW, 4)
    o = out.cpu().numpy()
    for k, t in enumerate(ids):
        tx, ty = int(t) % tiles_x, int(t) // tiles_x
        x0, y0 = tx * TW, ty * TH
        w, h = min(TW, W - x0), min(TH, H - y0)
        np.testing.assert_array_equal(o[k, :h, :w], full[y0:y0 + h, x0:x0 + w])
        np.testing.assert_array_equal(host[k, :h, :w], full[y0:y0 + h, x0:x0 + w])


def test_device_output_equals_host_output(vr):
    import torch
    W, H = 64, 48
    vol, tff = _noise_scene(vr)
    seeds = _seeds(5)
    host = vr.render_samples(W, H, seeds)
    vr.setIteration(0)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    assert vr.render_samples(W, H, seeds, out_dev_ptr=out.data_ptr()) is None
    torch.cuda.synchronize()
    vr.setIteration(0)
    np.testing.assert_array_equal(out.cpu().numpy(), host)


def test_launch_info_names_the_sample_kernel(vr):
    """Case 6: the new kernel, not a loop over the old one, produced the image."""
    W, H = 64, 48
    _noise_scene(vr)
    seeds = _seeds(8)
    vr.render_samples(W, H, seeds)
    info = vr.lastLaunchInfo()
    assert info["technique"] == 1 and info["samples"] == 1
    assert info["frames"] == 8 and info["work_items"] == 8 * ((W + 7) // 8) * ((H + 7) // 8)
    vr.setIteration(0)
    vr.render_samples(W, H, seeds, samples_per_launch=4)
    info = vr.lastLaunchInfo()
    assert info["samples"] == 1 and info["frames"] == 4
    assert vr.getLastExecTime() > 0.0
    vr.setIteration(0)
    vr.runRaycastNoGL(W, H)
    info = vr.lastLaunchInfo()
    assert info["technique"] == 1 and info["samples"] == 0 and info["frames"] == 1
    vr.setIteration(0)


def test_ray_caster_and_empty_seed_list_are_refused(vr):
    """Case 7."""
    W, H = 64, 48
    _noise_scene(vr)
    with pytest.raises(ValueError):
        vr.render_samples(W, H, [])
    assert vr.params()[1].iteration == 0
    vr.setTechnique(0)
    try:
        with pytest.raises(RuntimeError, match="vrhip_render_samples: path tracer only"):
            vr.render_samples(W, H, _seeds(2))
        assert vr.params()[1].iteration == 0
    finally:
        vr.setTechnique(1)


def test_config5_size_three_samples_equal_oracle_chain():
    """Case 8: BASELINE config 5's size and field -- 1024^3 FLOAT sphere generated in HBM, max_extinction 100 --
    a 96x80 frame, 3 samples, through the stats build and the production kernels."""
    N = 1024
    tff = common.tffs()["default"]
    W, H = 96, 80
    r = VolumeRenderCL()
    r.initialize()
    try:
        r.synthVolume("sphere", (N, N, N), FLOAT)
        vol = r.downloadVolume(0)
        assert vol.shape == (N, N, N) and vol.dtype == np.float32
        r.setTransferFunction(tff)
        r.setTechnique(1)
        r.setExtinction(100.0)
        r.updateView(common.views()["rot30"])
        seeds = _seeds(3)
        ref, rstats = _oracle_chain(r, vol, FLOAT, tff, W, H, seeds)
        for stats in (True, False):
            r.setStatsEnabled(stats)
            r.setIteration(0)
            got = r.render_samples(W, H, seeds)
            assert r.lastLaunchInfo()["samples"] == 1
            np.testing.assert_array_equal(got, ref)
            if stats:
                g = r.getStats()
                assert g["samples_taken"] == sum(s["samples_taken"] for s in rstats)
                assert g["rays_hit"] == sum(s["rays_hit"] for s in rstats)
    finally:
        r.close()
