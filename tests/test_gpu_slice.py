"""Slice views (vrhip_render_slices, vr_slice.hip) against their CPU restatement (tests/ref/slice_ref.c, pinned by
tests/test_slice_ref.py) with a difference of exactly 0: planes and slabs of every voxel type, filter, mode and output,
several slices per launch, device and host output, the C++ class and the CLI, every rejection, the state the call
follows and the state it must leave alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common, slice_ref
from volumerenderercl_amd import (FLOAT, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT, SliceParams, VolumeRenderCL, _lib,
                                  frontend)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")
BG = [0.1, 0.9, 0.5, 0.25]
F32 = np.float32
RESOLUTIONS = [(5, 7, 9), (17, 9, 33), (16, 16, 1), (1, 1, 1), (32, 32, 32)]
VIEWPORTS = [(1, 1), (8, 8), (37, 21), (64, 64)]
SLAB_N = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256]
MODES = ["max", "min", "mean"]
OUTPUTS = ["tf", "value"]
# the nearest q outside the box whose tex = q * 0.5f + 0.5f is outside [0, 1] (tests/test_slice_ref.py, Q_BELOW / Q_ABOVE)
Q_BELOW = float(np.nextafter(F32(-1), F32(-2)))
Q_ABOVE = float(np.nextafter(np.nextafter(F32(1), F32(2)), F32(2)))
FMT_IDS = dict(ids=["uchar", "ushort", "float"])


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


def _quantise(vol01, fmt):
    if fmt == UCHAR:
        return np.round(vol01 * 255).astype(np.uint8)
    if fmt == USHORT:
        return np.round(vol01 * 65535).astype(np.uint16)
    return vol01.astype(np.float32)


def _structured(res, fmt):
    """A ramp along x + y under a ball: every plane through it is a picture; [z, y, x]."""
    x, y, z = res
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, z), np.linspace(-1, 1, y), np.linspace(-1, 1, x), indexing="ij")
    f = 0.25 + 0.2 * xx + 0.15 * yy + 0.4 * (xx * xx + yy * yy + zz * zz < 0.5)
    return _quantise(np.clip(f, 0, 1), fmt)


def _random(res, fmt, seed):
    x, y, z = res
    return _quantise(np.random.default_rng(seed).random((z, y, x), dtype=np.float32), fmt)


def _load(vr, vol, fmt, tff):
    vr.loadVolumeArrays([vol], fmt)
    if tff is not None:
        vr.setTransferFunction(tff)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = BG


def _check(vr, vol, fmt, tff, slices, W, H, linear, what, nan_is_nan=False):
    """The call's images equal the restatement's, raw bits (nan_is_nan: where the restatement has a NaN, any NaN)."""
    vr.setLinearInterpolation(linear)
    got = vr.render_slices(W, H, slices)
    ref = slice_ref.render_all(vol, fmt, tff, slices, linear, BG, W, H)
    assert got.shape == ref.shape == (len(slices), H, W, 4)
    bad = _bits(got) != _bits(ref)
    if nan_is_nan:
        bad &= ~(np.isnan(got) & np.isnan(ref))
    bad = np.any(bad, axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first at (slice, row, column) %s" % (what, bad.sum(), np.argwhere(bad)[0])
    return ref


def _is_bg(img):
    return np.all(_bits(img) == _bits(np.asarray(BG, F32)), axis=-1)


def _planes(res):
    """The planes of the issue, for a volume of `res`: (name, SliceParams)."""
    out = []
    for a, axis in enumerate("xyz"):
        n = res[a]
        for i in sorted({0, n // 2, n - 1}):
            out.append(("%s centre %d" % (axis, i), frontend.axis_slice(axis, (2.0 * (i + 0.5)) / n - 1.0, output="value")))
        out.append((axis + " face -1", frontend.axis_slice(axis, -1.0, output="value")))
        out.append((axis + " face +1", frontend.axis_slice(axis, 1.0, output="value")))
        out.append((axis + " outside -", frontend.axis_slice(axis, Q_BELOW)))
        out.append((axis + " outside +", frontend.axis_slice(axis, Q_ABOVE)))
        out.append((axis + " tf", frontend.axis_slice(axis, 0.3)))
    # obliques that cut corners: a wave mixes taken and untaken pixels
    out.append(("oblique 111", frontend.plane_slice([0.0, 0.0, 0.0], [1, 1, 1], [0, 0, 1], 1.6, 1.6)))
    out.append(("oblique corner", frontend.plane_slice([0.7, 0.6, -0.65], [1, -2, 0.5], [0, 1, 1], 1.1, 0.9, output="value")))
    out.append(("oblique skew", frontend.make_slice([0.2, -0.1, 0.3], [0.9, 0.7, -0.2], [0.3, -0.5, 1.1])))
    out.append(("u = 0", frontend.make_slice([0.1, 0.0, -0.2], [0, 0, 0], [0.2, 1.3, 0.4], output="value")))
    out.append(("u = v = 0", frontend.make_slice([0.3, 0.2, 0.1], [0, 0, 0], [0, 0, 0])))
    out.append(("wholly outside", frontend.make_slice([3.0, 0.2, 0.1], [0.5, 0, 0], [0, 0.5, 0.5])))
    return out


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], **FMT_IDS)
def test_planes_equal_restatement(vr, fmt, linear):
    tff = common.tffs()["opaque"]
    pictures = 0
    for res in RESOLUTIONS:
        named = _planes(res)
        slices = [s for _, s in named]
        for content, vol in (("structured", _structured(res, fmt)), ("random", _random(res, fmt, 7 + res[0]))):
            _load(vr, vol, fmt, tff)
            for W, H in VIEWPORTS:
                ref = _check(vr, vol, fmt, tff, slices, W, H, linear, "%r %s %dx%d" % (res, content, W, H))
                for (name, _), img in zip(named, ref):
                    if "outside" in name:
                        assert _is_bg(img).all(), name
                    elif "face" in name or "centre" in name:
                        assert not _is_bg(img).any(), name
                    elif name.startswith("oblique") and (W, H) == (64, 64) and res == (32, 32, 32) and content == "structured":
                        assert 0 < _is_bg(img).sum() < W * H, name     # taken and untaken pixels side by side
                pictures += sum(np.unique(img.reshape(-1, 4), axis=0).shape[0] > 30 for img in ref)
    assert pictures >= 20


def _slabs(through, ns=SLAB_N):
    """Slabs of every N, mode and output through `through` = (origin, u, v, w): partly outside the box."""
    o, u, v, w = through
    return [frontend.make_slice(o, u, v, w, samples=n, mode=m, output=out) for n in ns for m in MODES for out in OUTPUTS]


SLAB_GEOMETRY = {
    "axial, sticking out of the top": ([0.0, 0.0, 0.6], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]),
    "oblique, across a corner": ([0.5, 0.4, -0.5], [0.8, -0.3, 0.1], [0.1, 0.6, 0.7], [0.9, 0.8, -1.2]),
}


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], **FMT_IDS)
def test_slabs_equal_restatement(vr, fmt, linear):
    tff = common.tffs()["default"]
    for res in ((17, 9, 33), (32, 32, 32)):
        vol = _random(res, fmt, 3) if res[0] == 17 else _structured(res, fmt)
        _load(vr, vol, fmt, tff)
        for name, through in SLAB_GEOMETRY.items():
            slices = _slabs(through)
            ref = _check(vr, vol, fmt, tff, slices, 37, 21, linear, "%r %s" % (res, name))
            counts = slice_ref.render(vol, fmt, tff, slices[-1], linear, BG, 37, 21)[2]
            assert counts.max() > 0 and (counts < 256).any()   # part of the slab is outside the box
            # N = 1: the three modes give the same bits
            assert _same(ref[0], ref[2]) and _same(ref[0], ref[4]) and _same(ref[1], ref[3]) and _same(ref[1], ref[5])


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "nearest"])
@pytest.mark.parametrize("kind", ["beyond_unit", "nan", "inf"])
def test_float_volumes(vr, kind, linear):
    rng = np.random.default_rng(21)
    x, y, z = 17, 9, 33
    if kind == "beyond_unit":
        vol = rng.normal(0.3, 1.5, (z, y, x)).astype(np.float32)
        vol[: z // 2, :, : x // 2] = -np.abs(vol[: z // 2, :, : x // 2]) - 0.5
    elif kind == "nan":
        vol = rng.random((z, y, x), dtype=np.float32)
        vol[rng.random((z, y, x)) < 0.05] = np.nan
        vol[4:12, 2:6, 5:12] = np.nan
    else:
        vol = rng.random((z, y, x), dtype=np.float32)
        vol[rng.random((z, y, x)) < 0.03] = np.inf
        vol[rng.random((z, y, x)) < 0.03] = -np.inf
        vol[20:26, 3:7, 2:9] = 3.0e38
    tff = common.tffs()["opaque"]
    _load(vr, vol, FLOAT, tff)
    slices = [s for _, s in _planes((x, y, z))]
    for through in SLAB_GEOMETRY.values():
        slices += _slabs(through, ns=(1, 3, 5, 64))
    # inf - inf (a lerp between +inf and -inf, a sum of both) makes a NaN whose sign the hardware chooses: only there,
    # i.e. only in the volume that holds infinities, a NaN pixel of the restatement may be any NaN
    ref = _check(vr, vol, FLOAT, tff, slices, 37, 21, linear, kind, nan_is_nan=(kind == "inf"))
    if kind != "beyond_unit":
        assert not np.isfinite(ref).all()


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        o = rng.uniform(-0.4, 0.4, 3)
        nrm, up = rng.normal(size=3), rng.normal(size=3)
        out.append(frontend.plane_slice(o, nrm, up, rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5),
                                        thickness=rng.uniform(0.0, 1.0), samples=int(rng.choice([1, 2, 3, 5, 8, 17, 64, 256])),
                                        mode=MODES[i % 3], output=OUTPUTS[(i // 3) % 2]))
    return out


@pytest.mark.parametrize("fmt", [UCHAR, FLOAT], ids=["uchar", "float"])
def test_several_slices_per_call(vr, fmt):
    """1, 2 and 33 slices with different N, mode and output in one launch, in both orders: slice i lands at image i."""
    vol = _structured((32, 32, 32), fmt)
    tff = common.tffs()["haze"]
    _load(vr, vol, fmt, tff)
    for n in (1, 2, 33):
        slices = _mixed(n, 40 + n)
        for W, H in ((37, 21), (64, 64)):
            fwd = _check(vr, vol, fmt, tff, slices, W, H, True, "%d slices" % n)
            rev = _check(vr, vol, fmt, tff, slices[::-1], W, H, True, "%d slices, reversed" % n)
            assert _same(fwd, rev[::-1])
        assert n == 1 or not _same(fwd[0], fwd[1])


def test_device_and_host_output_give_the_same_bits(vr):
    import torch
    vol = _random((17, 9, 33), USHORT, 5)
    tff = common.tffs()["opaque"]
    _load(vr, vol, USHORT, tff)
    slices = _mixed(5, 3)
    W, H = 37, 21
    host = _check(vr, vol, USHORT, tff, slices, W, H, True, "host")
    dev = torch.full((len(slices), H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    assert vr.render_slices(W, H, slices, out_dev_ptr=dev.data_ptr()) is None
    torch.cuda.synchronize()
    rs = torch.cuda.ExternalStream(vr.get_stream())
    rs.synchronize()
    assert _same(dev.cpu().numpy(), host)
    # a single SliceParams is a call of one slice
    assert _same(vr.render_slices(W, H, slices[2]), host[2:3])


def test_cxx_class(vr, tmp_path):
    """tests/cxx/caller_slice.cpp, compiled against include/ alone: its helpers build frontend's parameter blocks, its
    images are this renderer's, and the two progressive frames around them are undisturbed."""
    exe = str(tmp_path / "caller_slice")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_slice.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "slices.bin")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    W, H, n = 37, 21, 6
    blob = open(out, "rb").read()
    theirs = [SliceParams.from_buffer_copy(blob[80 * i: 80 * (i + 1)]) for i in range(n)]
    img, a, b = np.split(np.frombuffer(blob[80 * n:], dtype=np.float32), [n * H * W * 4, (n + 1) * H * W * 4])
    img, a, b = img.reshape(n, H, W, 4), a.reshape(H, W, 4), b.reshape(H, W, 4)
    mine = [frontend.axis_slice("z", F32(0.1)), frontend.axis_slice("x", F32(-0.3), F32(0.5), 5, "mean", "value"),
            frontend.plane_slice([F32(0.1), 0.0, F32(-0.1)], [1, 1, 1], [0, 0, 1], F32(0.9), F32(0.8), F32(0.3), 4, "min")]
    mine += frontend.slice_stack(frontend.axis_slice("y", 0.0), 3, 2.0)
    for i, (s, t) in enumerate(zip(mine, theirs)):
        assert (s.samples, s.mode, s.output, s.reserved) == (t.samples, t.mode, t.output, t.reserved), i
        for name in ("origin", "u", "v", "w"):   # (double arithmetic in both, rounded to float: an ulp at the most)
            p, q = np.asarray(getattr(s, name)[:], F32), np.asarray(getattr(t, name)[:], F32)
            assert np.all(np.abs(p - q) <= np.spacing(np.maximum(np.abs(p), np.abs(q)))), (i, name, p, q)
    assert bytes(mine[0]) == bytes(theirs[0]) and bytes(mine[1]) == bytes(theirs[1]) and bytes(mine[5]) == bytes(theirs[5])
    tff = np.zeros((256, 4), np.uint8)
    tff[:, 0] = np.arange(256)
    tff[:, 1] = 255 - np.arange(256)
    tff[:, 2] = 40
    tff[:, 3] = np.arange(256)
    vr.synthVolume("sphere", (32, 32, 32), UCHAR)
    vr.setTransferFunction(tff)
    vr.setTechnique(TECH_RAYCAST)
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    vr.setLinearInterpolation(True)
    vol = vr.downloadVolume(0)
    got = vr.render_slices(W, H, theirs)
    assert _same(got, slice_ref.render_all(vol, UCHAR, tff, theirs, True, [1, 1, 1, 1], W, H))
    assert _same(img, got)
    assert np.unique(img.reshape(-1, 4), axis=0).shape[0] > 50
    # the caller's two frames: iterations 0 and 1 of an uninterrupted progressive sequence
    vr.setIllumination(1)
    vr.setObjEss(True)
    vr.setCamOrtho(False)
    vr.updateSamplingRate(1.5)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.updateView([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1])
    vr.setSeed(77)
    assert _same(a, vr.runRaycastNoGL(W, H)) and _same(b, vr.runRaycastNoGL(W, H))
    assert np.unique(a.reshape(-1, 4), axis=0).shape[0] > 20
    vr.setIteration(0)


def _cli(args, tmp_path, name, W, H):
    out = str(tmp_path / name)
    res = subprocess.run([EXE] + [str(a) for a in args] + ["--out", out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    frames = np.fromfile(out + ".frames.rgba.f32", dtype=np.float32).reshape(-1, H, W, 4)
    assert _same(np.fromfile(out + ".rgba.f32", dtype=np.float32).reshape(H, W, 4), frames[-1])
    return frames, out


def _unit_normal(u, v):
    """u x v / |u x v| with the CLI's double operations."""
    c = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    ln = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    return [x / ln for x in c]


CLI_FORMS = ["axis", "axis_value_nearest", "axis_slab", "plane", "plane_slab", "axis_stack", "plane_stack"]


@pytest.mark.parametrize("name", CLI_FORMS)
def test_cli(vr, tmp_path, name):
    """vrhip_render's slice options in each form, float and --rgba8: the frames are this renderer's for the same
    parameter blocks, the bytes vrhip_quantise_rgba8's (frontend.quantise_rgba8 states the conversion)."""
    W, H = 37, 21
    base = ["--synth", "shells", 32, "UCHAR", "--size", W, H, "--bg", 0.25, 0.5, 0.75]
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.setStatsEnabled(False)
    vr.setBackground((0.25, 0.5, 0.75))   # (as the CLI sets it: alpha 0)
    o, u, v = [0.125, -0.25, 0.0625], [0.75, 0.25, 0.0], [-0.125, 0.5, 0.625]
    nrm = _unit_normal(u, v)
    d = sum(F32(a) * b for a, b in zip(o, nrm))
    centred = [float(F32(float(F32(a)) - d * b)) for a, b in zip(o, nrm)]
    span = 2.0 * sum(abs(c) for c in nrm)
    forms = {
        "axis": (["--slice-axis", "Z", 0.3125], [frontend.axis_slice("z", 0.3125)], True),
        "axis_value_nearest": (["--slice-axis", "x", -0.5, "--slice-value", "--nearest"],
                               [frontend.axis_slice("x", -0.5, output="value")], False),
        "axis_slab": (["--slice-axis", "Y", 0.25, "--slab", 0.5, 5, "mean"],
                      [frontend.axis_slice("y", 0.25, 0.5, 5, "mean")], True),
        "plane": (["--slice"] + o + u + v, [frontend.make_slice(o, u, v)], True),
        "plane_slab": (["--slice"] + o + u + v + ["--slab", 0.375, 7, "min", "--slice-value"],
                       [frontend.make_slice(o, u, v, [0.375 * c for c in nrm], 7, "min", "value")], True),
        "axis_stack": (["--slice-axis", "Z", 0.3125, "--slice-stack", 5],
                       frontend.slice_stack(frontend.axis_slice("z", 0.0), 5, 2.0), True),
        "plane_stack": (["--slice"] + o + u + v + ["--slice-stack", 3, "--slab", 0.25, 2, "max"],
                        frontend.slice_stack(frontend.make_slice(centred, u, v, [0.25 * c for c in nrm], 2, "max"), 3, span),
                        True),
    }
    assert sorted(forms) == sorted(CLI_FORMS)
    args, slices, linear = forms[name]
    vr.setLinearInterpolation(linear)
    want = vr.render_slices(W, H, slices)
    vr.setLinearInterpolation(True)
    frames, _ = _cli(base + args, tmp_path, name, W, H)
    assert _same(frames, want)
    frames8, out = _cli(base + args + ["--rgba8"], tmp_path, name + "8", W, H)
    assert _same(frames8, want)
    q = np.fromfile(out + ".frames.rgba.u8", dtype=np.uint8).reshape(-1, H, W, 4)
    assert np.array_equal(q, frontend.quantise_rgba8(want))
    assert np.array_equal(np.fromfile(out + ".rgba.u8", dtype=np.uint8).reshape(H, W, 4), q[-1])
    assert np.unique(want.reshape(-1, 4), axis=0).shape[0] > 1


def test_cli_usage_errors():
    base = [EXE, "--synth", "sphere", "32", "UCHAR", "--out", "unused"]
    ax = ["--slice-axis", "Z", "0"]
    plane = ["--slice", "0", "0", "0", "1", "0", "0", "0", "1", "0"]
    bad = [ax + ["--mip"], ax + ["--iso", "0.5"], ax + ["--pathtrace"], ax + ["--orbit", "0", "1", "0", "4"],
           ax + ["--camera-path", "nowhere"], ax + ["--ranks", "2"], ax + plane, ["--slab", "0.1", "4", "max"],
           ["--slice-stack", "4"], ["--slice-value"], ["--slice-axis", "Q", "0"], ["--slice-axis", "Z"],
           ax + ["--slab", "0.1", "0", "max"], ax + ["--slab", "0.1", "257", "max"], ax + ["--slab", "0.1", "4", "median"],
           ax + ["--slice-stack", "0"], plane[:-1], ["--slice", "0", "0", "0", "0", "0", "0", "0", "1", "0", "--slab", "0.1", "2", "max"],
           ["--slice", "0", "0", "0", "1", "0", "0", "2", "0", "0", "--slice-stack", "3"]]
    for args in bad:
        res = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert res.returncode == 2 and "usage:" in res.stderr, args


def _raw_call(vr, W, H, slices, n=None, out=True, null_slices=False):
    """vrhip_render_slices as given: (return code, message)."""
    arr = (SliceParams * max(1, len(slices)))(*slices)
    buf = np.zeros((max(1, len(slices)), max(1, min(H, 64)), max(1, min(W, 64)), 4), np.float32)
    vr._push_params()
    rc = vr.lib.vrhip_render_slices(vr.handle, W, H, None if null_slices else C.cast(arr, C.c_void_p),
                                    len(slices) if n is None else n, buf.ctypes.data_as(C.c_void_p) if out else None, 0)
    return rc, (vr.lib.vrhip_last_error(vr.handle) or b"").decode()


def test_rejections(vr):
    vol = _structured((17, 9, 33), UCHAR)
    tff = common.tffs()["opaque"]
    _load(vr, vol, UCHAR, tff)
    good = frontend.axis_slice("z", 0.0)

    def variant(**kw):
        s = SliceParams.from_buffer_copy(bytes(good))
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(s, k)[val[0]] = val[1]
            else:
                setattr(s, k, val)
        return s

    invalid = [dict(samples=0), dict(samples=257), dict(mode=3), dict(output=2), dict(reserved=1)]
    for name in ("origin", "u", "v", "w"):
        for c in range(3):
            for x in (np.nan, np.inf, -np.inf):
                invalid.append({name: (c, x)})
    for kw in invalid:
        rc, msg = _raw_call(vr, 8, 8, [good, variant(**kw)])
        assert rc == _lib.ERR_INVALID and msg, kw
        with pytest.raises(ValueError):
            vr.render_slices(8, 8, [variant(**kw)])
    assert _raw_call(vr, 8, 8, [good], n=0)[0] == _lib.ERR_INVALID
    assert _raw_call(vr, 8, 8, [good], out=False)[0] == _lib.ERR_INVALID
    assert _raw_call(vr, 8, 8, [good], null_slices=True)[0] == _lib.ERR_INVALID
    assert vr.lib.vrhip_render_slices(None, 8, 8, None, 1, None, 0) == _lib.ERR_INVALID
    for W, H in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        rc, msg = _raw_call(vr, W, H, [good])
        assert rc == _lib.ERR_INVALID
        frame_rc = vr.lib.vrhip_render_frame(vr.handle, W, H, None, 0)
        assert frame_rc == _lib.ERR_INVALID and msg == vr.lib.vrhip_last_error(vr.handle).decode()
    # the renderer still renders: a slice and a frame
    _check(vr, vol, UCHAR, tff, [good], 37, 21, True, "after the rejections")
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)
    assert np.isfinite(vr.runRaycastNoGL(16, 16)).all()
    vr.setIteration(0)

    # RG / RGBA volumes
    for ch in (2, 4):
        vr.loadVolumeArrays([np.zeros((4, 4, 4, ch), np.uint8)], UCHAR)
        vr.setTransferFunction(tff)
        rc, msg = _raw_call(vr, 8, 8, [good])
        assert rc == _lib.ERR_UNSUPPORTED and "RG / RGBA" in msg
        with pytest.raises(RuntimeError):
            vr.render_slices(8, 8, [good])
    _load(vr, vol, UCHAR, tff)
    _check(vr, vol, UCHAR, tff, [good], 8, 8, True, "after an RGBA volume")

    # no volume; a volume but no transfer function: what vrhip_render_frame answers -- and VALUE needs no table
    fresh = VolumeRenderCL()
    fresh.initialize()
    try:
        rc, msg = _raw_call(fresh, 8, 8, [good])
        frame_rc = fresh.lib.vrhip_render_frame(fresh.handle, 8, 8, None, 0)
        assert rc == frame_rc == _lib.ERR_NODATA and msg == fresh.lib.vrhip_last_error(fresh.handle).decode()
        with pytest.raises(RuntimeError):
            fresh.render_slices(8, 8, [good])
        fresh.loadVolumeArrays([vol], UCHAR)
        fresh.params()[1].backgroundColor[:] = BG
        value = frontend.axis_slice("z", 0.0, output="value")
        rc, msg = _raw_call(fresh, 8, 8, [value, good])
        frame_rc = fresh.lib.vrhip_render_frame(fresh.handle, 8, 8, None, 0)
        assert rc == frame_rc == _lib.ERR_NODATA and msg == fresh.lib.vrhip_last_error(fresh.handle).decode()
        _check(fresh, vol, UCHAR, None, [value], 37, 21, True, "VALUE without a transfer function")
    finally:
        fresh.close()


def test_follows_volume_timestep_and_transfer_function(vr):
    a, b = _structured((17, 9, 33), USHORT), _random((17, 9, 33), USHORT, 9)
    tffs = common.tffs()
    slices = _mixed(4, 11)
    W, H = 37, 21
    vr.loadVolumeArrays([a, b], USHORT)
    vr.setTransferFunction(tffs["opaque"])
    vr.setStatsEnabled(False)
    vr.params()[1].backgroundColor[:] = BG
    vr.setTimestep(0)
    ra = _check(vr, a, USHORT, tffs["opaque"], slices, W, H, True, "time step 0")
    vr.setTimestep(1)
    rb = _check(vr, b, USHORT, tffs["opaque"], slices, W, H, True, "time step 1")
    vr.setTransferFunction(tffs["haze"])
    rh = _check(vr, b, USHORT, tffs["haze"], slices, W, H, True, "new transfer function")
    assert not _same(ra, rb) and not _same(rb, rh)
    vr.params()[1].backgroundColor[:] = [0.5, 0.25, 0.125, 1.0]
    got = vr.render_slices(W, H, slices)
    assert _same(got, slice_ref.render_all(b, USHORT, tffs["haze"], slices, True, [0.5, 0.25, 0.125, 1.0], W, H))
    vr.params()[1].backgroundColor[:] = BG
    vr.setTimestep(0)
    c = _random((5, 7, 9), FLOAT, 2)
    _load(vr, c, FLOAT, tffs["default"])
    _check(vr, c, FLOAT, tffs["default"], slices, W, H, False, "new volume")


def test_independent_of_everything_else(vr):
    """Technique (3 and 5 included), camera, illumination, ESS switches, iteration, seed: the images do not change."""
    vol = _structured((17, 9, 33), UCHAR)
    tff = common.tffs()["opaque"]
    _load(vr, vol, UCHAR, tff)
    slices = _mixed(4, 12)
    ref = _check(vr, vol, UCHAR, tff, slices, 37, 21, True, "plain")
    views = common.views()
    for tech in (0, 1, 2, 3, 4, 5):
        vr.setTechnique(tech)
        vr.updateView(views["rot30"] if tech % 2 else views["close"])
        vr.setIllumination(tech % 6)
        vr.setObjEss(tech % 2 == 0)
        vr.setImgEss(tech == 2)
        vr.setCamOrtho(tech == 3)
        vr.setSeed(1000 + tech)
        vr.setIteration(tech)
        vr.setBBox(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5)
        assert _same(vr.render_slices(37, 21, slices), ref), tech
    vr.setTechnique(TECH_RAYCAST)
    vr.setIllumination(1)
    vr.setObjEss(True)
    vr.setImgEss(False)
    vr.setCamOrtho(False)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.setIteration(0)


def _sequence(vr, W, H, n, between=None):
    vr.setIteration(0)
    vr.updateOutputImg(W, H)
    frames = []
    for i in range(n):
        vr.setSeed(500 + i)
        frames.append(vr.runRaycastNoGL(W, H))
        if between is not None:
            between()
    vr.setIteration(0)
    return frames


@pytest.mark.parametrize("case", ["raycast", "image_ess", "pathtrace"])
def test_state_neutral(vr, case):
    """Progressive frames at iterations 0, 1, 2 with slices rendered between them -- at the frame's own size and at
    another -- equal the uninterrupted sequence bit for bit; lastLaunchInfo() is what it was."""
    vol = common.noise_volume((48, 40, 36), UCHAR, seed=5)
    _load(vr, vol, UCHAR, common.tffs()["default"])
    vr.setTechnique(TECH_PATHTRACE if case == "pathtrace" else TECH_RAYCAST)
    vr.setImgEss(case == "image_ess")
    vr.setObjEss(True)
    vr.setIllumination(1)
    vr.setCamOrtho(False)
    vr.updateSamplingRate(1.5)
    vr.setBBox(-1, -1, -1, 1, 1, 1)
    vr.updateView(common.views()["rot30"])
    W, H = 72, 56
    slices = _mixed(3, 13)
    infos = []

    def between():
        before = vr.lastLaunchInfo()
        a = vr.render_slices(W, H, slices)
        vr.render_slices(37, 21, slices[:1])
        assert _same(vr.render_slices(W, H, slices), a)
        assert vr.lastLaunchInfo() == before
        infos.append(before)

    try:
        plain = _sequence(vr, W, H, 3)
        mixed = _sequence(vr, W, H, 3, between)
    finally:
        vr.setImgEss(False)
        vr.setTechnique(TECH_RAYCAST)
    for i in range(3):
        assert _same(plain[i], mixed[i]), "%s: frame %d differs" % (case, i)
    assert not _same(plain[0], plain[2]) and len(infos) == 3
    assert infos[0]["technique"] == (1 if case == "pathtrace" else 0)
