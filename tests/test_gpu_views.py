"""Per-frame cameras in batched rendering (vrhip_render_batch_views): every frame of a batch of different views
equals the stand-alone frame of its view and seed (runRaycastNoGL) and the oracle's, bit for bit -- production and
instrumented kernels, whole frames and tile subsets, at the benchmark's size and schedule -- and the C++ host
replays recorded camera paths the same way frame by frame, in launch sets, and over tile ranks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import vro
from tests import common
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL, frontend
from volumerenderercl_amd._lib import CameraParams

pytestmark = pytest.mark.gpu

TOL = float(os.environ.get("VRHIP_TEST_TOL", "0"))
SEEDS = [3499211612, 581869302, 3890346734, 3586334585, 545404204, 4161255391, 3922919429]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")


def _views():
    v = common.views()
    return [v["default"], v["rot30"], v["close"], v["inside"],
            frontend.view_matrix(frontend.DEFAULT_ROTATION, (6.0, 0.0, 2.0)),   # misses the box
            frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 1), 140.0), (0.0, 0.2, 1.6))]


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _setup(vr, vol, fmt, tff, **kw):
    vr.loadVolumeArrays([vol], fmt)
    vr.setTransferFunction(tff)
    vr.setIllumination(kw.get("illum", 1))
    vr.setLinearInterpolation(True)
    vr.setCamOrtho(False)
    vr.setContours(kw.get("contours", False))
    vr.setObjEss(kw.get("ess", True))
    vr.updateSamplingRate(1.5)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    vr.setStatsEnabled(False)
    vr.updateView(common.views()["rot30"])
    vr.setIteration(0)


def _single(vr, view, seed, W, H):
    vr.updateView(view)
    vr.setSeed(seed)
    vr.setIteration(0)
    return vr.runRaycastNoGL(W, H)


def _batch(vr, W, H, seeds, views, **kw):
    import torch
    n = len(seeds)
    ids = kw.get("tile_ids")
    if ids is None:
        out = torch.full((n, H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    else:
        stride = kw.get("frame_stride", 0)
        T = kw["tile_w"]
        out = torch.full((n, max(stride, len(ids) * T * T), 4), -7.0, dtype=torch.float32, device="cuda")
    vr.render_batch(W, H, seeds, out.data_ptr(), views=views, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt,res,kw", [(UCHAR, (48, 48, 48), {}), (USHORT, (40, 56, 36), {"ess": False}),
                                         (FLOAT, (44, 44, 44), {"illum": 0, "contours": True})])
def test_batch_of_views_equals_singles_and_oracle(vr, fmt, res, kw):
    vol = common.noise_volume(res, fmt, seed=33, smooth=False)
    tff = common.tffs()["default"]
    W, H, T = 100, 76, 32          # (not a multiple of 8)
    _setup(vr, vol, fmt, tff, **kw)
    views = _views()
    seeds = SEEDS[:len(views)]
    singles = [_single(vr, v, s, W, H) for v, s in zip(views, seeds)]
    cam, rp, rc, pt = common.to_oracle_params(*vr.params())
    for f in range(len(views)):
        cam.viewMat[:] = views[f]
        rp.seed, rp.iteration = seeds[f], 0
        ref, _, _ = vro.render_tile(vol, fmt, tff, cam, rp, rc, pt, use_ess=kw.get("ess", True), W=W, H=H)
        assert np.abs(singles[f] - ref).max() <= TOL, "view %d" % f
    assert not np.array_equal(singles[0], singles[1]) and np.all(singles[4] == singles[4][0, 0])
    vr.updateView(common.views()["rot30"])
    for stats in (False, True):
        vr.setStatsEnabled(stats)
        got = _batch(vr, W, H, seeds, views)
        li = vr.lastLaunchInfo()
        assert li["views"] == 1 and li["frames"] == len(views) and li["instrumented"] == int(stats), li
        assert li["patch_classes"] == 0, li
        for f in range(len(views)):
            assert np.array_equal(got[f], singles[f]), "frame %d (stats %s)" % (f, stats)
    vr.setStatsEnabled(False)
    # tile subset, frames a stride apart
    tiles_x = (W + T - 1) // T
    ids = np.array([0, 2, 5, 7, 9, 11], dtype=np.uint32)
    stride = (len(ids) + 1) * T * T
    got = _batch(vr, W, H, seeds, views, tile_w=T, tile_h=T, tile_ids=ids, frame_stride=stride)
    for f in range(len(views)):
        tl = got[f, :len(ids) * T * T].reshape(len(ids), T, T, 4)
        for k, t in enumerate(ids):
            x0, y0 = (int(t) % tiles_x) * T, (int(t) // tiles_x) * T
            w, h = min(T, W - x0), min(T, H - y0)
            assert np.array_equal(tl[k, :h, :w], singles[f][y0:y0 + h, x0:x0 + w]), (f, int(t))
        assert np.all(got[f, len(ids) * T * T:] == -7.0)   # nothing written between the frames
    # views=None: every frame from the renderer's view, as before
    vr.updateView(views[2])
    got = _batch(vr, W, H, seeds[:3], None)
    assert vr.lastLaunchInfo()["views"] == 0
    for f in range(3):
        assert np.array_equal(got[f], _single(vr, views[2], seeds[f], W, H)), f
    with pytest.raises(ValueError):
        vr.render_batch(W, H, seeds[:2], 0, views=views[:3])


def test_c_abi_mixed_ortho_and_bboxes(vr):
    """vrhip_render_batch_views at the C ABI: each frame's camera struct -- view, box and ortho -- applies to that
    frame only."""
    import torch
    vol = common.noise_volume((48, 48, 48), UCHAR, seed=5, smooth=False)
    _setup(vr, vol, UCHAR, common.tffs()["default"])
    W, H = 88, 72
    views = _views()
    confs = [(views[1], False, (-1, -1, -1, 1, 1, 1)), (views[1], True, (-1, -1, -1, 1, 1, 1)),
             (views[2], False, (-0.6, -1, -0.5, 0.7, 0.4, 1)), (views[0], True, (-0.6, -1, -0.5, 0.7, 0.4, 1)),
             (views[5], False, (-1, -1, -1, 1, 1, 1))]
    singles = []
    for (v, ortho, bb), s in zip(confs, SEEDS):
        vr.setCamOrtho(ortho)
        vr.setBBox(*bb)
        singles.append(_single(vr, v, s, W, H))
    vr.setCamOrtho(False)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.setIteration(0)
    vr._push_params()
    cams = (CameraParams * len(confs))()
    for f, (v, ortho, bb) in enumerate(confs):
        cams[f].viewMat[:] = v
        cams[f].bbox_bl[:] = list(bb[:3]) + [0]
        cams[f].bbox_tr[:] = list(bb[3:]) + [0]
        cams[f].ortho = 1 if ortho else 0
    seeds = np.array(SEEDS[:len(confs)], dtype=np.uint32)
    out = torch.zeros((len(confs), H, W, 4), dtype=torch.float32, device="cuda")
    rc = vr.lib.vrhip_render_batch_views(vr.handle, W, H, 0, 0, None, 0, seeds.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.cast(cams, ctypes.c_void_p), len(confs),
                                         ctypes.c_void_p(out.data_ptr()), 0)
    assert rc == 0, vr.lib.vrhip_last_error(vr.handle)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for f in range(len(confs)):
        assert np.array_equal(got[f], singles[f]), "frame %d" % f
    # NULL cameras: exactly vrhip_render_batch
    vr.updateView(views[1])
    vr._push_params()
    rc = vr.lib.vrhip_render_batch_views(vr.handle, W, H, 0, 0, None, 0, seeds.ctypes.data_as(ctypes.c_void_p),
                                         None, 2, ctypes.c_void_p(out.data_ptr()), 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], singles[0])
    # what chains frames is refused with views as without
    vr.setAmbientOcclusion(True)
    with pytest.raises(RuntimeError):
        vr.render_batch(W, H, list(seeds[:2]), out.data_ptr(), views=views[:2])
    vr.setAmbientOcclusion(False)


def test_patch_class_cache_key_with_alternating_views(vr):
    """Batches of views run without patch classes; batches that alternate between two view sets, then an ordinary
    batch and a single frame (both with patch classes) each equal their singles: the cached classes of the
    renderer's camera are never taken for another camera or kept past a change."""
    W, H = 128, 96
    vr.synthVolume("shells", (96, 96, 96), UCHAR)
    vr.setTransferFunction(common.tffs()["default"])
    vr.setIllumination(1)
    vr.setObjEss(True)
    vr.setCamOrtho(False)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    va = [frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 0), a), (0, 0, 2.6)) for a in (0, 10, 20)]
    vb = [frontend.view_matrix(frontend.quat_from_axis_angle((1, 0, 0), a), (0.3, 0, 2.2)) for a in (35, 50, 65)]
    seeds = SEEDS[:3]
    want = {k: [_single(vr, v, s, W, H) for v, s in zip(vs, seeds)] for k, vs in (("a", va), ("b", vb))}
    own = frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30), (0, 0, 2.4))
    want_own = [_single(vr, own, s, W, H) for s in seeds]
    assert vr.lastLaunchInfo()["patch_classes"] == 1   # (the scene has class-1 patches)
    for k in ("a", "b", "a", "b"):
        got = _batch(vr, W, H, seeds, va if k == "a" else vb)
        for f in range(3):
            assert np.array_equal(got[f], want[k][f]), (k, f)
    vr.updateView(own)
    got = _batch(vr, W, H, seeds, None)
    assert vr.lastLaunchInfo()["patch_classes"] == 1
    for f in range(3):
        assert np.array_equal(got[f], want_own[f]), f
    got = _batch(vr, W, H, seeds, vb)
    for f in range(3):
        assert np.array_equal(got[f], want["b"][f]), f
    assert np.array_equal(_single(vr, own, seeds[1], W, H), want_own[1])
    assert np.array_equal(_single(vr, va[2], seeds[2], W, H), want["a"][2])


def test_256_orbit_views(vr):
    vol = common.noise_volume((40, 40, 40), UCHAR, seed=35, smooth=False)
    _setup(vr, vol, UCHAR, common.tffs()["default"])
    W, H = 72, 56
    mt = frontend.Mt19937()
    N = 256
    seeds = [mt() for _ in range(N)]
    views = frontend.orbit_views((0, 1, 0), N, frontend.quat_from_axis_angle((1, 0, 0), 25.0), (0, 0, 2.2))
    got = _batch(vr, W, H, seeds, views)
    for f in (0, 1, 31, 32, 63, 64, 127, 128, 200, 255):
        assert np.array_equal(got[f], _single(vr, views[f], seeds[f], W, H)), "frame %d" % f


def test_share_volumes_twin_renders_views(vr):
    import torch
    vol = common.noise_volume((48, 48, 48), UCHAR, seed=8, smooth=False)
    _setup(vr, vol, UCHAR, common.tffs()["default"])
    W, H = 96, 64
    views = _views()[:4]
    seeds = SEEDS[:4]
    singles = [_single(vr, v, s, W, H) for v, s in zip(views, seeds)]
    vr.updateView(common.views()["rot30"])
    twin = vr.shareVolumes()
    try:
        outs = []
        for x, vs, sd in ((vr, views[:2], seeds[:2]), (twin, views[2:], seeds[2:])):
            out = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda")
            x.render_batch(W, H, sd, out.data_ptr(), views=vs)   # both sets in flight
            outs.append(out)
        torch.cuda.synchronize()
        got = np.concatenate([o.cpu().numpy() for o in outs])
        for f in range(4):
            assert np.array_equal(got[f], singles[f]), f
    finally:
        twin.close()


def test_views_at_size_on_the_timed_schedule():
    """2048^3 UCHAR shells (generated in HBM), 1024^2, phase-1 budget 48, a 32-view orbit as one launch set: the
    12-wave phase 1 with the empty-run lookahead and per-frame cameras; frames 0, 13, 31 equal the stand-alone
    frames of their views and seeds, and a tile of one frame equals the oracle's."""
    import torch
    N, W, H = 2048, 1024, 1024
    tff = common.tffs()["default"]
    r = VolumeRenderCL()
    r.initialize()
    try:
        r.synthVolume("shells", (N, N, N), UCHAR)
        r.setTransferFunction(tff)
        r.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
        start = frontend.quat_from_axis_angle((1, 1, 0), 30.0)
        views = frontend.orbit_views((0, 1, 0), 32, start, frontend.DEFAULT_TRANSLATION)
        mt = frontend.Mt19937(91)
        seeds = [mt() for _ in range(32)]
        r.updateView(views[0])
        r.setStatsEnabled(False)
        r.setRoundBudget(48)
        r.setFrameTiming(False)
        out = torch.zeros((32, H, W, 4), dtype=torch.float32, device="cuda")
        r.render_batch(W, H, seeds, out.data_ptr(), views=views)
        torch.cuda.synchronize()
        li = r.lastLaunchInfo()
        assert li["views"] == 1 and li["frames"] == 32 and li["ray_list"] == 1 and li["prepass"] == 1, li
        assert li["phase1_waves"] == 12 and li["empty_skip"] == 1 and li["round_budget"] == 48, li
        got = {f: out[f].cpu().numpy() for f in (0, 13, 31)}
        del out
        for f in (0, 13, 31):
            assert np.array_equal(got[f], _single(r, views[f], seeds[f], W, H)), "frame %d" % f
        # one frame against the oracle, on a tile through the shells (the voxels downloaded)
        vol = r.downloadVolume(0)
        bricks = vro.generate_bricks(vol, UCHAR)
        r.updateView(views[13])
        cam, rp, rc, pt = common.to_oracle_params(*r.params())
        rp.seed, rp.iteration = seeds[13], 0
        x0, y0, T = 448, 480, 64
        ref, _, _ = vro.render_tile(vol, UCHAR, tff, cam, rp, rc, pt, W=W, H=H, tile=(x0, y0, T, T), bricks=bricks)
        assert np.abs(got[13][y0:y0 + T, x0:x0 + T].astype(np.float64) - ref).max() <= TOL
        assert ref[..., 3].max() > 0
    finally:
        r.setRoundBudget(10)
        r.close()


def _run(args, tmp_path, name, W, H):
    out = str(tmp_path / name)
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return np.fromfile(out + ".frames.rgba.f32", dtype=np.float32).reshape(-1, H, W, 4), res.stdout


def test_cli_camera_path_batched_equals_frame_by_frame(tmp_path):
    """vrhip_render --camera-path: a recorded path (recordViewConfig files) rendered one frame per entry by
    runRaycastNoGL, in launch sets of 8 views (two renderers), and over two loopback tile ranks in batches: all
    equal; and an interaction log whose transferFunction line changes the table mid-path gives, after that line,
    the frames of the same views under the new table."""
    W, H = 120, 88
    n = 19
    rng = np.random.default_rng(4)
    quats = [frontend.quat_from_axis_angle(rng.normal(size=3), float(a)) for a in rng.uniform(0, 360, n)]
    trans = [(float(x), float(y), float(z)) for x, y, z in zip(rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n),
                                                             rng.uniform(0.8, 2.6, n))]
    prefix = str(tmp_path / "path")
    with open(prefix + "_quat.txt", "w") as f:
        f.write("".join("%g %g %g %g; " % tuple(float(np.float32(v)) for v in q) for q in quats))
    with open(prefix + "_trans.txt", "w") as f:
        f.write("".join("%g %g %g; " % tuple(float(np.float32(v)) for v in t) for t in trans))
    base = ["--synth", "shells", 96, "UCHAR", "--size", W, H, "--camera-path", prefix]
    one, _ = _run(base, tmp_path, "one", W, H)
    assert one.shape[0] == n and np.isfinite(one).all()
    assert not np.array_equal(one[0], one[1])
    fpl, stdout = _run(base + ["--frames-per-launch", 8], tmp_path, "fpl", W, H)
    np.testing.assert_array_equal(fpl, one)
    ranks, _ = _run(base + ["--ranks", 2, "--loopback", "--tile", 32, "--frames-per-launch", 4], tmp_path, "ranks",
                    W, H)
    np.testing.assert_array_equal(ranks, one)
    # the same views as an interaction log with a new transfer function before entry k
    k = 7
    tff2 = frontend.haze_tff()
    lines = ["0; tffInterpolation; linear"]
    for i, (q, t) in enumerate(zip(quats, trans)):
        if i == k:
            lines.append("%d; transferFunction; %s" % (i, "".join("%d " % c for c in np.asarray(tff2).reshape(-1))))
        lines.append("%d; camera; %s, %s" % (i, " ".join("%g" % float(np.float32(v)) for v in q),
                                             " ".join("%g" % float(np.float32(v)) for v in t)))
    log = str(tmp_path / "log.txt")
    with open(log, "w") as f:
        f.write("\n".join(lines) + "\n")
    raw = str(tmp_path / "tf2.txt")
    frontend.write_raw_tff(raw, tff2)
    new_tf, _ = _run(base[:-2] + ["--camera-path", prefix, "--tf", raw], tmp_path, "newtf", W, H)
    for extra in ([], ["--frames-per-launch", 8]):
        logged, _ = _run(base[:-2] + ["--camera-path", log] + extra, tmp_path, "log", W, H)
        np.testing.assert_array_equal(logged[:k], one[:k])
        np.testing.assert_array_equal(logged[k:], new_tf[k:])
    assert not np.array_equal(new_tf[k], one[k])
