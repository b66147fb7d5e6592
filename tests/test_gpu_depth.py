"""Depth images and picking (vrhip_render_depth, vr_depth.hip) against their CPU restatement (tests/ref/depth_ref.c,
pinned by tests/test_depth_ref.py) with a difference of exactly 0 in all three outputs: every mode, voxel type and
filter with object-order ESS on and off (the skipping must not change a bit), partial patches, rectangles and picks,
camera kinds, seeds, refinement counts, non-finite voxels, a second time step, device outputs, every refusal of the
contract, the renderer's state around a depth call, the C++ class and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import common, depth_ref
from volumerenderercl_amd import (FLOAT, TECH_ISO, TECH_MIP, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT,
                                  VolumeRenderCL, _lib, frontend)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")
SEEDS = [3499211612, 581869302]
RES = (48, 40, 36)           # (tests/test_gpu_iso.py's)
W, H = 61, 43                # partial patches on both edges
BOX = ((-0.5, -0.7, -0.3), (0.6, 0.4, 0.8))
VIEWS = common.views()
MODES = {"iso": depth_ref.ISO, "max": depth_ref.MAX, "opacity": depth_ref.OPACITY}
THRESHOLD = {"iso": 0.15, "max": 0.0, "opacity": 0.3}
RECTS = [(5, 3, 13, 9), (60, 42, 1, 1), (30, 21, 1, 1)]


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _quantise(f, fmt):
    if fmt == UCHAR:
        return np.round(f * 255).astype(np.uint8)
    if fmt == USHORT:
        return np.round(f * 65535).astype(np.uint16)
    return f.astype(np.float32)


def _volume(fmt, seed=5):
    """A noisy ball in the +x half; the -x half and the corners are exactly 0: whole cells of the grid, halo included,
    hold nothing but 0 -- bound 0 for ISO and MAX, and the empty bit under _tff()."""
    f = common.noise_volume(RES, FLOAT, seed=seed, smooth=False).astype(np.float32)
    f[:, :, : RES[0] // 2] = 0
    return _quantise(f, fmt)


def _tff():
    """Opacity exactly 0 for the lower quarter of the table, a ramp above; some colour."""
    tff = np.zeros((256, 4), np.uint8)
    tff[:, 0] = np.arange(256)
    tff[:, 1] = 200
    tff[64:, 3] = np.linspace(1, 255, 192).round()
    return tff


def _load(vr, vols, fmt, tff):
    vr.loadVolumeArrays(vols if isinstance(vols, list) else [vols], fmt)
    if tff is not None:
        vr.setTransferFunction(tff)
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)


def _conf(vr, view="rot30", linear=True, ortho=False, rate=1.0, box=None, ess=True, seed=SEEDS[0]):
    vr.setLinearInterpolation(linear)
    vr.setCamOrtho(ortho)
    vr.updateSamplingRate(rate)
    bl, tr = box if box else ((-1, -1, -1), (1, 1, 1))
    vr.setBBox(*bl, *tr)
    vr.setObjEss(ess)
    vr.updateView(VIEWS[view] if isinstance(view, str) else view)
    vr.setSeed(seed)


def _ref(vr, vol, fmt, tff, mode, threshold, refine=4, w=W, h=H, rect=None):
    cam, rp, rc, _ = common.to_oracle_params(*vr.params())
    return depth_ref.render(vol, fmt, tff, cam, rp, rc, MODES[mode], threshold, refine, W=w, H=h, rect=rect)


def _equal(got, ref, what):
    names = ("xyzt", "aux", "kind")
    for name, g, r in zip(names, got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, name)
        gb, rb = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == np.float32 else (g, r)
        bad = gb != rb
        assert not bad.any(), "%s: %s differs in %d places, first at %s" % (what, name, bad.sum(), np.argwhere(bad)[0])


def _both_ess(vr, vol, fmt, tff, mode, what, threshold=None, refine=4, **conf):
    """The depth image with ESS on and off: both equal the restatement, and so each other."""
    threshold = THRESHOLD[mode] if threshold is None else threshold
    ref = None
    for ess in (True, False):
        _conf(vr, ess=ess, **conf)
        got = vr.render_depth(W, H, mode, threshold, refine)
        di = vr.lastDepthInfo()
        assert di == {"mode": MODES[mode], "work_items": ((W + 7) // 8) * ((H + 7) // 8), "empty_skip": int(ess)}, di
        if ref is None:
            ref = _ref(vr, vol, fmt, tff, mode, threshold, refine)
        _equal(got, ref, "%s, ESS %s" % (what, ess))
    return ref


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_equals_restatement(vr, mode, fmt, linear):
    """Three modes x three voxel types x two filters, object-order ESS on and off, on a 61 x 43 frame."""
    vol, tff = _volume(fmt), _tff()
    _load(vr, vol, fmt, tff)
    xyzt, aux, kind = _both_ess(vr, vol, fmt, tff, mode, "%s %d %s" % (mode, fmt, linear), linear=linear)
    hit = kind == depth_ref.HIT
    assert hit.sum() > 60 and (kind == depth_ref.MISS).any()
    if mode != "max":
        assert (kind == depth_ref.NO_HIT).any()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_rectangles_and_picks(vr, mode):
    """Each rectangle equals the same pixels cut from the whole-frame answer; pick() is its 1 x 1 case."""
    vol, tff = _volume(UCHAR), _tff()
    _load(vr, vol, UCHAR, tff)
    _conf(vr)
    thr = THRESHOLD[mode]
    whole = vr.render_depth(W, H, mode, thr)
    _equal(whole, _ref(vr, vol, UCHAR, tff, mode, thr), "whole")
    for rect in RECTS:
        x0, y0, w, h = rect
        part = vr.render_depth(W, H, mode, thr, rect=rect)
        _equal(part, tuple(np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for a in whole), "rect %s" % (rect,))
        assert vr.lastDepthInfo()["work_items"] == ((w + 7) // 8) * ((h + 7) // 8)
    hits = 0
    ys, xs = np.nonzero(whole[2] == depth_ref.HIT)
    assert ys.size
    for x, y in ((int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1])), (int(xs[ys.size // 2]), int(ys[ys.size // 2])),
                 (0, 0), (60, 42)):
        p = vr.pick(W, H, x, y, mode, thr)
        if whole[2][y, x] != depth_ref.HIT:
            assert p is None
            continue
        hits += 1
        assert np.array_equal(p["pos"].view(np.uint32), whole[0][y, x, :3].view(np.uint32))
        assert np.float32(p["t"]) == whole[0][y, x, 3] and np.float32(p["aux"]) == whole[1][y, x]
        assert np.array_equal(p["voxel"], (whole[0][y, x, :3].astype(np.float64) * 0.5 + 0.5) * np.asarray(RES, np.float64))
    assert hits >= 1


CAMERAS = {
    "orthographic": dict(view="close", ortho=True),
    "inside": dict(view="inside"),
    "clip_box": dict(view="rot30", box=BOX, rate=2.0),
    "low_rate": dict(view="rot30", rate=0.5),
}


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_cameras(vr, mode, cam):
    vol, tff = _volume(USHORT), _tff()
    _load(vr, vol, USHORT, tff)
    ref = _both_ess(vr, vol, USHORT, tff, mode, "%s %s" % (mode, cam), **CAMERAS[cam])
    assert (ref[2] == depth_ref.HIT).any()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_seeds_move_the_samples(vr, mode):
    vol, tff = _volume(UCHAR), _tff()
    _load(vr, vol, UCHAR, tff)
    t = []
    for seed in SEEDS:
        ref = _both_ess(vr, vol, UCHAR, tff, mode, "seed %d" % seed, seed=seed)
        t.append(ref[0][..., 3])
    both = np.isfinite(t[0]) & np.isfinite(t[1])
    assert both.any() and np.any(t[0][both] != t[1][both])


def test_refine_steps(vr):
    """refineSteps 0 and 16 both equal the restatement, and the refinement moves t."""
    vol, tff = _volume(FLOAT), _tff()
    _load(vr, vol, FLOAT, tff)
    t = [_both_ess(vr, vol, FLOAT, tff, "iso", "refine %d" % refine, refine=refine)[0][..., 3] for refine in (0, 16)]
    both = np.isfinite(t[0])
    assert np.array_equal(both, np.isfinite(t[1])) and np.any(t[0][both] != t[1][both])
    assert np.all(t[1][both] <= t[0][both])   # tb only moves towards ta


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_float_voxels_outside_the_unit_range_nan_and_inf(vr, mode, linear):
    f = common.noise_volume(RES, FLOAT, seed=7, smooth=False).astype(np.float32) * np.float32(1.6) - np.float32(0.3)
    f[:, :, : RES[0] // 2] = 0
    f[6:10, 8:14, 30:36] = np.nan
    f[20:24, 18:22, 38:42] = np.inf
    f[14:17, 28:31, 26:29] = -np.inf
    tff = _tff()
    _load(vr, f, FLOAT, tff)
    for thr in ((0.7, 1.2) if mode == "iso" else (THRESHOLD[mode],)):
        ref = _both_ess(vr, f, FLOAT, tff, mode, "specials %s" % thr, threshold=thr, linear=linear)
        assert (ref[2] == depth_ref.HIT).any()


def test_thresholds_at_the_edges(vr):
    """OPACITY threshold 0 hits at k = 0 whatever cell the ray starts in (nothing is skipped there); above 1 nothing
    hits and aux is the opacity the ray ran out of samples with.  ISO at 0 likewise hits at k = 0."""
    vol, tff = _volume(UCHAR), _tff()
    _load(vr, vol, UCHAR, tff)
    for mode in ("opacity", "iso"):
        for thr in (0.0, 1.5, -0.25):
            ref = _both_ess(vr, vol, UCHAR, tff, mode, "%s at %g" % (mode, thr), threshold=thr)
            entered = ref[2] != depth_ref.MISS
            assert np.all(ref[2][entered] == (depth_ref.NO_HIT if thr > 1 else depth_ref.HIT))


def test_second_time_step(vr):
    a, b, tff = _volume(UCHAR, 5), _volume(UCHAR, 11), _tff()
    _load(vr, [a, b], UCHAR, tff)
    try:
        first = _both_ess(vr, a, UCHAR, tff, "iso", "step 0")
        vr.setTimestep(1)
        for mode in sorted(MODES):
            second = _both_ess(vr, b, UCHAR, tff, mode, "step 1 %s" % mode)
        vr.setTimestep(0)
        again = _both_ess(vr, a, UCHAR, tff, "iso", "step 0 again")
        _equal(again, first, "back at step 0")
        assert not np.array_equal(first[1], _ref(vr, b, UCHAR, tff, "iso", THRESHOLD["iso"])[1])
    finally:
        vr.setTimestep(0)


def test_device_outputs_equal_host_outputs(vr):
    import torch
    vol, tff = _volume(USHORT), _tff()
    _load(vr, vol, USHORT, tff)
    _conf(vr)
    rs = torch.cuda.ExternalStream(vr.get_stream())
    for mode in sorted(MODES):
        host = vr.render_depth(W, H, mode, THRESHOLD[mode], rect=(5, 3, 40, 31))
        xyzt = torch.full((31, 40, 4), -7.0, dtype=torch.float32, device="cuda")
        aux = torch.full((31, 40), -7.0, dtype=torch.float32, device="cuda")
        kind = torch.full((31, 40), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert vr.render_depth(W, H, mode, THRESHOLD[mode], rect=(5, 3, 40, 31),
                               out_dev_ptrs=(xyzt.data_ptr(), aux.data_ptr(), kind.data_ptr())) is None
        rs.synchronize()
        _equal((xyzt.cpu().numpy(), aux.cpu().numpy(), kind.cpu().numpy()), host, "device %s" % mode)
        # any output may be left out
        only = torch.full((31, 40), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vr.render_depth(W, H, mode, THRESHOLD[mode], rect=(5, 3, 40, 31), out_dev_ptrs=(None, None, only.data_ptr()))
        rs.synchronize()
        assert np.array_equal(only.cpu().numpy(), host[2])


# ---- refusals

def _raw(vr, w, h, p, outs=(True, True, True), n=None):
    """vrhip_render_depth itself: the return code."""
    n = n if n is not None else max(1, w * h)
    xyzt, aux, kind = np.zeros(4 * n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    ptr = [a.ctypes.data_as(C.c_void_p) if on else None for a, on in zip((xyzt, aux, kind), outs)]
    return vr._lib.vrhip_render_depth(vr._h, w, h, C.byref(p) if p is not None else None, ptr[0], ptr[1], ptr[2], 0)


def _params(mode=0, threshold=0.5, refine=4, rect=(0, 0, 0, 0), reserved=0):
    p = _lib.DepthParams()
    p.mode, p.threshold, p.refineSteps, p.reserved = mode, threshold, refine, reserved
    p.x0, p.y0, p.w, p.h = rect
    return p


def test_refusals(vr):
    vol, tff = _volume(UCHAR), _tff()
    _load(vr, vol, UCHAR, tff)
    _conf(vr)
    good = vr.render_depth(W, H, "iso", 0.15)
    inf, nan = float("inf"), float("nan")
    invalid = [
        (W, H, None, (True, True, True)),
        (W, H, _params(), (False, False, False)),
        (W, H, _params(mode=3), None), (W, H, _params(reserved=1), None),
        (W, H, _params(mode=0, threshold=nan), None), (W, H, _params(mode=0, threshold=inf), None),
        (W, H, _params(mode=2, threshold=nan), None), (W, H, _params(mode=2, threshold=-inf), None),
        (W, H, _params(mode=0, refine=17), None),
        (0, H, _params(), None), (W, 0, _params(), None), (16385, H, _params(), None), (W, 16385, _params(), None),
        (W, H, _params(rect=(0, 0, 5, 0)), None), (W, H, _params(rect=(0, 0, 0, 5)), None),
        (W, H, _params(rect=(W - 4, 0, 5, 5)), None), (W, H, _params(rect=(0, H - 4, 5, 5)), None),
        (W, H, _params(rect=(W, 0, 1, 1)), None), (W, H, _params(rect=(0, 0, W + 1, H)), None),
        (W, H, _params(rect=(0xffffffff, 0, 2, 1)), None), (W, H, _params(rect=(3, 2, 0, 0)), None),
    ]
    for w, h, p, outs in invalid:
        rc = _raw(vr, w, h, p, outs or (True, True, True), n=W * H)
        assert rc == _lib.ERR_INVALID, (w, h, outs, p and (p.mode, p.threshold, p.refineSteps, p.x0, p.y0, p.w, p.h, p.reserved))
    assert vr._lib.vrhip_render_depth(None, W, H, C.byref(_params()), None, None, None, 0) == _lib.ERR_INVALID
    # what MAX does not read is not checked; refineSteps is ISO's alone
    assert _raw(vr, W, H, _params(mode=1, threshold=nan, refine=99)) == _lib.OK
    assert _raw(vr, W, H, _params(mode=2, threshold=0.5, refine=99)) == _lib.OK
    with pytest.raises(ValueError):
        vr.render_depth(W, H, "iso", nan)
    with pytest.raises(ValueError):
        vr.render_depth(W, H, "depth")
    _equal(vr.render_depth(W, H, "iso", 0.15), good, "after the refusals")

    r = VolumeRenderCL()
    r.initialize()
    try:
        di = _lib.DepthInfo()
        assert r._lib.vrhip_last_depth_info(r._h, C.byref(di)) == _lib.ERR_NODATA
        assert _raw(r, W, H, _params(mode=1)) == _lib.ERR_NODATA          # no volume
        r.loadVolumeArrays([vol], UCHAR)
        assert r._lib.vrhip_last_depth_info(r._h, C.byref(di)) == _lib.ERR_NODATA
        assert _raw(r, W, H, _params(mode=2)) == _lib.ERR_NODATA          # OPACITY without a transfer function
        with pytest.raises(RuntimeError, match="No transfer function set."):
            r.render_depth(W, H, "opacity", 0.5)
        # ISO and MAX need none, with object-order ESS on and off
        for ess in (True, False):
            _conf(r, ess=ess)
            for mode in ("iso", "max"):
                _equal(r.render_depth(W, H, mode, THRESHOLD[mode]), _ref(r, vol, UCHAR, None, mode, THRESHOLD[mode]),
                       "no TF, %s" % mode)
                assert r.lastDepthInfo()["empty_skip"] == int(ess)
        r.setTransferFunction(tff)
        _equal(r.render_depth(W, H, "opacity", 0.3), _ref(r, vol, UCHAR, tff, "opacity", 0.3), "TF set afterwards")
        rg = np.zeros((RES[2], RES[1], RES[0], 2), np.uint8)
        rg[..., 0] = vol
        r.loadVolumeArrays([rg], UCHAR, channels=2)
        r.setTransferFunction(tff)
        for mode in range(3):
            assert _raw(r, W, H, _params(mode=mode)) == _lib.ERR_UNSUPPORTED
        r.loadVolumeArrays([vol], UCHAR)
        r.setTransferFunction(tff)
        _conf(r)
        _equal(r.render_depth(W, H, "iso", 0.15), good, "the renderer still answers")
    finally:
        r.close()


# ---- state

def _sequence(vr, w, h, n, between=None):
    vr.setIteration(0)
    vr.updateOutputImg(w, h)
    frames = []
    for i in range(n):
        vr.setSeed(500 + i)
        frames.append(vr.runRaycastNoGL(w, h))
        if between is not None:
            between()
    vr.setIteration(0)
    return frames


@pytest.mark.parametrize("case", ["raycast", "pathtrace", "image_ess"])
def test_state_neutral(vr, case):
    """Progressive frames with depth calls between them -- at the frame's size and at another, every mode -- equal the
    uninterrupted sequence bit for bit; lastLaunchInfo() is what it was."""
    vol, tff = _volume(UCHAR), _tff()
    _load(vr, vol, UCHAR, tff)
    _conf(vr, rate=1.5)
    vr.setTechnique(TECH_PATHTRACE if case == "pathtrace" else TECH_RAYCAST)
    vr.setImgEss(case == "image_ess")
    vr.setIllumination(1)
    fw, fh = 72, 56
    infos = []

    def between():
        before = vr.lastLaunchInfo()
        for mode in sorted(MODES):
            vr.render_depth(fw, fh, mode, THRESHOLD[mode])
            vr.render_depth(W, H, mode, THRESHOLD[mode], rect=RECTS[0])
        vr.pick(fw, fh, 36, 28, "iso", 0.3)
        assert vr.lastLaunchInfo() == before
        infos.append(before)

    try:
        plain = _sequence(vr, fw, fh, 2)
        mixed = _sequence(vr, fw, fh, 2, between)
    finally:
        vr.setImgEss(False)
        vr.setTechnique(TECH_RAYCAST)
    for i in range(2):
        assert np.array_equal(plain[i].view(np.uint32), mixed[i].view(np.uint32)), "%s: frame %d differs" % (case, i)
    assert not np.array_equal(plain[0], plain[1]) and len(infos) == 2
    assert infos[0]["technique"] == (1 if case == "pathtrace" else 0)
    assert C.sizeof(_lib.LaunchInfo) == 128


def test_ignored_state(vr):
    """The answer does not depend on the selected technique, illumination, useAO, aerial, showEss, imgEss, the
    iteration or vrhip_iso_params."""
    vol, tff = _volume(UCHAR), _tff()
    _load(vr, vol, UCHAR, tff)
    _conf(vr)
    ref = {mode: vr.render_depth(W, H, mode, THRESHOLD[mode]) for mode in MODES}
    try:
        for tech in (TECH_PATHTRACE, TECH_MIP, TECH_ISO, 3, 5):
            vr.params()[1].technique = tech   # (3 and 5 are unassigned: a render call would refuse them, this one does not look)
            vr.setAmbientOcclusion(True)
            vr.setIteration(7)
            vr.setIllumination(3)
            vr.setImgEss(True)
            vr.params()[2].aerial = 1
            vr.params()[1].showEss = 1
            vr.setIsoValue(0.9)
            vr.setIsoRefinement(1)
            for mode in MODES:
                _equal(vr.render_depth(W, H, mode, THRESHOLD[mode]), ref[mode], "technique %d, %s" % (tech, mode))
    finally:
        vr.setTechnique(TECH_RAYCAST)
        vr.setAmbientOcclusion(False)
        vr.setIteration(0)
        vr.setIllumination(1)
        vr.setImgEss(False)
        vr.params()[2].aerial = 0
        vr.params()[1].showEss = 0
        vr.setIsoValue(0.5)
        vr.setIsoRefinement(4)


# ---- C++ class and CLI

def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_depth")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_depth.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "depth.bin")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    cw, ch = 45, 29
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, *shape):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape)), offset=at).reshape(shape)
        at += n
        return a

    a, b = take(np.float32, ch, cw, 4), take(np.float32, ch, cw, 4)
    images = []
    for w, h in ((cw, ch),) * 3 + ((13, 9),):
        images.append((take(np.float32, h, w, 4), take(np.float32, h, w), take(np.uint8, h, w)))
    pick, voxel = take(np.float32, 6), take(np.float64, 3)
    assert at == len(raw)

    tff = np.zeros((256, 4), np.uint8)
    tff[:, 0] = np.arange(256)
    tff[:, 1] = 255 - np.arange(256)
    tff[:, 2] = 40
    tff[:, 3] = np.arange(256)
    vr.synthVolume("sphere", (32, 32, 32), UCHAR)
    vr.setTransferFunction(tff)
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIllumination(1)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    view = [2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1]
    _conf(vr, view=view, rate=1.5, seed=77)
    vol = vr.downloadVolume(0)
    calls = (("iso", 0.4, 6, None), ("max", 0.0, 4, None), ("opacity", 0.6, 4, None), ("iso", 0.4, 6, (5, 3, 13, 9)))
    for got, (mode, thr, refine, rect) in zip(images, calls):
        mine = vr.render_depth(cw, ch, mode, thr, refine, rect=rect)
        _equal(mine, _ref(vr, vol, UCHAR, tff, mode, thr, refine, w=cw, h=ch, rect=rect), "python %s" % mode)
        _equal(tuple(np.array(x) for x in got), mine, "c++ %s %s" % (mode, rect))
    assert (images[0][2] == depth_ref.HIT).sum() > 50
    p = vr.pick(cw, ch, 22, 14, "iso", 0.4, 6)
    assert pick[0] == 1.0 and np.array_equal(pick[1:4].view(np.uint32), p["pos"].view(np.uint32))
    assert pick[4] == np.float32(p["t"]) and pick[5] == np.float32(p["aux"]) and np.array_equal(voxel, p["voxel"])
    # the caller's two frames: iterations 0 and 1 of an uninterrupted progressive sequence
    vr.setIteration(0)
    vr.updateOutputImg(cw, ch)
    f0 = vr.runRaycastNoGL(cw, ch)
    vr.setSeed(78)
    f1 = vr.runRaycastNoGL(cw, ch)
    vr.setIteration(0)
    assert np.array_equal(a.view(np.uint32), f0.view(np.uint32)) and np.array_equal(b.view(np.uint32), f1.view(np.uint32))
    assert not np.array_equal(f0, f1)


CLI_SCENE = ["--synth", "shells", 32, "UCHAR", "--seed", 1234]


def _cli(args, tmp_path, name):
    out = str(tmp_path / name)
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return out, json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("mode,opt,rect", [("iso", ["iso", 0.35, "--depth-refine", 3], None), ("max", ["max"], None),
                                           ("opacity", ["opacity", 0.5], (30, 22, 13, 9))])
def test_cli_files_equal_the_python_arrays(vr, tmp_path, mode, opt, rect):
    cw, ch = 72, 56
    view = VIEWS["rot30"]
    args = CLI_SCENE + ["--size", cw, ch, "--view"] + [repr(float(np.float32(v))) for v in view] + ["--depth"] + opt
    if rect:
        args += ["--depth-rect"] + list(rect)
    out, info = _cli(args, tmp_path, "d_" + mode)
    w, h = (rect[2], rect[3]) if rect else (cw, ch)
    xyzt = np.fromfile(out + ".depth.f32", np.float32).reshape(h, w, 4)
    aux = np.fromfile(out + ".depth.aux.f32", np.float32).reshape(h, w)
    kind = np.fromfile(out + ".depth.kind.u8", np.uint8).reshape(h, w)
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    tff = frontend.tff_from_stops()
    vr.setTransferFunction(tff)
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    _conf(vr, view=view, rate=1.5, seed=1234)
    thr = opt[1] if len(opt) > 1 else 0.0
    refine = 3 if mode == "iso" else 4
    mine = vr.render_depth(cw, ch, mode, thr, refine, rect=rect)
    _equal(mine, _ref(vr, vr.downloadVolume(0), UCHAR, tff, mode, thr, refine, w=cw, h=ch, rect=rect), "python")
    _equal((xyzt, aux, kind), mine, "cli")
    hit = kind == depth_ref.HIT
    assert info["mode"] == mode and info["hits"] == int(hit.sum()) and hit.any()
    assert np.float32(info["t_min"]) == xyzt[..., 3][hit].min() and np.float32(info["t_max"]) == xyzt[..., 3][hit].max()
    ppm = open(out + ".ppm", "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert ppm.startswith(head) and len(ppm) == len(head) + w * h * 3
    grey = np.frombuffer(ppm, np.uint8, offset=len(head)).reshape(h, w, 3)
    assert np.all(grey[~hit] == 0) and np.all(grey[..., 0] == grey[..., 1]) and grey[hit].max() == 255


@pytest.mark.parametrize("extra", [["--depth", "max", "--pathtrace"], ["--depth", "max", "--mip"],
                                   ["--depth", "max", "--iso", 0.4], ["--depth", "max", "--slice-axis", "Z", 0],
                                   ["--depth", "max", "--slice-value"], ["--depth", "max", "--ranks", 2],
                                   ["--depth", "max", "--frames-per-launch", 4], ["--depth", "min"],
                                   ["--depth", "max", "--orbit", 0, 1, 0, 4], ["--depth", "max", "--camera-path", "none"],
                                   ["--depth", "max", "--frames", 2], ["--depth", "max", "--rgba8"],
                                   ["--depth", "max", "--img-ess"],
                                   ["--depth", "iso", 0.4, "--depth-refine", 17],
                                   ["--depth", "max", "--depth-rect", 60, 0, 8, 8], ["--depth-refine", 3],
                                   ["--depth-rect", 0, 0, 4, 4], ["--iso-refine", 3],
                                   ["--depth", "iso", 0.4, "--iso-refine", 3]])
def test_cli_usage_errors(tmp_path, extra):
    """What does not combine with --depth ends with the usage text and status 2 before anything is loaded; --iso-refine
    still needs --iso."""
    args = ["--synth", "shells", 32, "UCHAR", "--size", 64, 48] + extra
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", str(tmp_path / "bad")], capture_output=True,
                         text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), res.stderr
    assert "--depth iso V | max | opacity A" in res.stderr
    assert not os.path.exists(str(tmp_path / "bad") + ".depth.f32")
