"""The CPU restatement of technique 2 (maximum intensity projection, tests/ref/mip_ref.c) pinned to what the
project already trusts, on the CPU alone: its ray set-up to the oracle's technique-0 frames (silhouettes of binary
volumes, hit and sample counts), its transfer-function stage to the oracle's tff_linear and to the stated
formula, and known answers in float64.  tests/test_gpu_mip.py then holds the HIP kernel to the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import vro
from tests import common, mip_ref
from volumerenderercl_amd import frontend

W = H = 64
SEEDS = [3499211612, 581869302, 3890346734]
BG = [0.2, 0.3, 0.4, 0.0]   # alpha 0: the oracle's hit-but-untouched pixel (alpha 0) is then the background itself


def _params(view, res, ortho=0, rate=1.5, seed=SEEDS[0], bbox=None, scale=(1.0, 1.0, 1.0), linear=0, bg=BG):
    cam = vro.CameraParams()
    cam.viewMat[:] = view
    bl, tr = bbox if bbox else ((-1, -1, -1), (1, 1, 1))
    cam.bbox_bl[:] = list(bl) + [0]
    cam.bbox_tr[:] = list(tr) + [0]
    cam.ortho = ortho
    rp = vro.RenderingParams()
    rp.backgroundColor[:] = bg
    rp.modelScale[:] = list(scale) + [0]
    rp.illumType, rp.useLinear, rp.seed = 0, linear, seed
    rc = vro.RaycastParams()
    rc.samplingRate = rate
    _, brf, _ = vro.brick_layout(res)
    rc.brickRes[:] = brf + [0]
    return cam, rp, rc


def _binary_volume(res, seed):
    """Voxels 0 or 255: random blobs plus single isolated voxels; [z, y, x]."""
    rng = np.random.default_rng(seed)
    x, y, z = res
    zz, yy, xx = np.meshgrid(np.arange(z), np.arange(y), np.arange(x), indexing="ij")
    vol = np.zeros((z, y, x), np.uint8)
    for _ in range(5):
        c = rng.uniform(0.15, 0.85, 3) * np.array([x, y, z])
        r = rng.uniform(1.5, 0.14 * min(res))
        vol[(xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2 <= r * r] = 255
    for _ in range(40):
        vol[rng.integers(z), rng.integers(y), rng.integers(x)] = 255
    return vol


def _binary_tff(n=256):
    """Entry 0 fully transparent, the last entry opaque (and not the background's colour)."""
    tff = np.zeros((n, 4), np.uint8)
    tff[1:, 3] = np.linspace(1, 255, n - 1).round()
    tff[-1] = [255, 30, 30, 255]
    return tff


V = common.views()
CASES = {
    "perspective": dict(view=V["rot30"], res=(40, 40, 40)),
    "orthographic": dict(view=V["rot30"], res=(40, 40, 40), ortho=1),
    "inside": dict(view=V["inside"], res=(40, 40, 40)),
    "clip_box": dict(view=V["close"], res=(40, 40, 40), bbox=((-0.5, -0.7, -0.3), (0.6, 0.4, 0.8))),
    "anisotropic": dict(view=V["rot30"], res=(40, 28, 20), scale=(1.0, 0.7, 0.5)),
    "rate_0.5": dict(view=V["rot30"], res=(40, 40, 40), rate=0.5),
    "rate_1.5_ortho_close": dict(view=V["close"], res=(36, 40, 33), rate=1.5, ortho=1),
}


def _is_bg(img, bg=BG):
    return np.all(img == np.asarray(bg, np.float32), axis=-1)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_ray_setup_pinned_to_oracle_silhouettes(case, seed):
    """Binary volume, nearest filter, TF[0] transparent and TF[n-1] opaque: the oracle's technique-0 pixel is the
    background exactly when no sample of the ray met a set voxel, i.e. when the restatement's m is 0 (or the ray
    took no sample at all).  Every pixel must agree.  With a fully transparent TF the oracle never terminates a ray
    early: its hit and sample counters are then those of the restatement's rays."""
    kw = dict(CASES[case])
    res = kw["res"]
    vol = _binary_volume(res, 7)
    tff = _binary_tff()
    cam, rp, rc = _params(seed=seed, linear=0, **kw)
    img, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    _, m, kind, count = mip_ref.render_tile(vol, mip_ref.UCHAR, tff, cam, rp, rc, W=W, H=H)
    assert np.all((m == 0) | (m == 1) | (kind != mip_ref.SAMPLED))
    ref_bg = (kind != mip_ref.SAMPLED) | (m == 0)
    assert np.array_equal(_is_bg(img), ref_bg), "%d pixels differ" % np.sum(_is_bg(img) != ref_bg)
    assert 0 < ref_bg.sum() < ref_bg.size or case == "inside"          # a silhouette is in the frame
    assert st["rays_hit"] == int(np.sum(kind != mip_ref.MISS))
    clear = np.zeros((4, 4), np.uint8)
    _, st0, _ = vro.render_tile(vol, vro.UCHAR, clear, cam, rp, rc, use_ess=False, W=W, H=H)
    assert st0["samples_taken"] == int(count.sum())


@pytest.mark.parametrize("case", sorted(CASES))
def test_linear_filter_one_sided(case):
    """Linear filter, TF[0] transparent and every other entry opaque: a sample above the first entry's coordinate
    0.5 / n has an opacity, which shows in the oracle's alpha channel -- so a pixel the oracle leaves as background
    has every sample, hence m, at or below that coordinate."""
    kw = dict(CASES[case])
    vol = _binary_volume(kw["res"], 11)
    n = 64
    tff = np.zeros((n, 4), np.uint8)
    tff[1:] = [255, 30, 30, 255]
    cam, rp, rc = _params(linear=1, **kw)
    img, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    _, m, kind, _ = mip_ref.render_tile(vol, mip_ref.UCHAR, tff, cam, rp, rc, W=W, H=H)
    bg = _is_bg(img)
    assert not bg.all() and (bg.any() or case == "inside")   # (from inside, every ray meets a blob's halo)
    thr = np.float32(0.5) / np.float32(n)
    assert np.all(m[bg & (kind == mip_ref.SAMPLED)] <= thr)
    assert np.all(bg[kind != mip_ref.SAMPLED])


def test_tf_stage_and_composite():
    """tff_linear(m) inside the restatement is the oracle's, bit for bit; the pixel is the stated formula in numpy
    fp32, one rounded operation per product and sum, for a few thousand m and the no-sample case."""
    rng = np.random.default_rng(3)
    special = [0.0, -0.0, 1.0, -1.0, 2.0, 0.5, 1e-30, -1e30, 1e30, 3.0e38, np.inf, -np.inf]
    m = np.concatenate([np.asarray(special, np.float32), np.linspace(-0.5, 1.5, 1500, dtype=np.float32),
                        rng.random(1500, dtype=np.float32), rng.normal(0, 4, 200).astype(np.float32)])
    for tff in (frontend.tff_from_stops(), frontend.haze_tff(), _binary_tff(37)):
        mine = mip_ref.tff_linear(tff, m)
        want = vro.math_batch("tff_linear", m.reshape(-1, 1), tff=tff).view(np.float32)
        assert np.array_equal(mine.view(np.uint32), want.view(np.uint32))
        for bg in ([0.2, 0.3, 0.4, 0.0], [1.0, 1.0, 1.0, 1.0], [0.1, 0.9, 0.5, 0.25]):
            b = np.asarray(bg, np.float32)
            c = want
            oma = np.float32(1.0) - c[:, 3]
            exp = np.empty_like(c)
            for k in range(3):
                exp[:, k] = (c[:, k] * c[:, 3]) + (b[k] * oma)
            exp[:, 3] = c[:, 3] + (b[3] * oma)
            assert exp.dtype == np.float32
            got = mip_ref.pixel(tff, m, True, b)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
            none = mip_ref.pixel(tff, m[:16], False, b)
            assert np.array_equal(none.view(np.uint32), np.tile(b, (16, 1)).view(np.uint32))


# ---- known answers: the orthographic ray of pixel (gx, gy) in float64, from the definition

def _rng3(x, y, z):
    return vro.lib().vro_parallel_rng3(int(x) & 0xffffffff, int(y) & 0xffffffff, int(z) & 0xffffffff)


def _ortho_ray(view, gx, gy, seed, res, rate):
    """(origin, direction, tnear, tfar, step, offset) of the square W x H frame's pixel, model scale 1, box
    [-1, 1]^3, in float64."""
    Vm = np.asarray(view, np.float64).reshape(4, 4)
    gs = W + (8 - W % 8)
    rnd = _rng3(gx, gy, seed) / 4294967296.0
    rnd2 = _rng3(gy, gx, 2 * seed) / 4294967296.0
    icx = 2.0 * gx / gs - 1.0 + rnd2 * 2.0 / gs
    icy = -(2.0 * gy / gs - 1.0) - rnd * 2.0 / gs
    cam = Vm[:3, 3]
    o = (cam + Vm[:3, 0] * icx + Vm[:3, 1] * icy) * np.linalg.norm(cam)
    d = -Vm[:3, 2] / np.linalg.norm(Vm[:3, 2])
    with np.errstate(divide="ignore"):
        t0, t1 = (-1.0 - o) / d, (1.0 - o) / d
    tnear, tfar = np.max(np.minimum(t0, t1)), np.min(np.maximum(t0, t1))
    if not tfar > tnear:
        return None
    sd = tfar - tnear
    r = np.asarray(res, np.float64)
    step0 = min(sd, sd / (rate * np.linalg.norm(d * sd * r)))
    step = sd / math.ceil(sd / step0)
    offset = np.linalg.norm(1.0 / r) * rnd * 2.0
    return o, d, max(0.0, tnear), tfar, step, offset


def test_known_answer_ramp_along_x():
    """FLOAT ramp f = x / (N - 1), orthographic camera looking along +x: the field grows along every ray, so m is
    the last sample's value.  The last sample lies within one step before the exit face (shifted back by the
    jitter offset), and the field's slope is N / (N - 1) per texel -- unit slope over the grid: m lies between the
    ramp at (exit - offset - step) and at (exit - offset)."""
    N, rate, seed = 33, 1.3, SEEDS[1]
    vol = np.broadcast_to(np.arange(N, dtype=np.float32) / np.float32(N - 1), (N, N, N)).copy()
    view = frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 0), -90.0), (0.0, 0.0, 2.0))
    cam, rp, rc = _params(view, (N, N, N), ortho=1, rate=rate, seed=seed, linear=1)
    _, m, kind, count = mip_ref.render_tile(vol, mip_ref.FLOAT, frontend.tff_from_stops(), cam, rp, rc, W=W, H=H)

    def ramp(xw):   # the clamp-to-edge trilinear ramp at world x, float64
        return np.clip(((xw * 0.5 + 0.5) * N - 0.5) / (N - 1), 0.0, 1.0)

    checked = 0
    for gy in range(0, H, 2):
        for gx in range(0, W, 2):
            ray = _ortho_ray(view, gx, gy, seed, (N, N, N), rate)
            if ray is None:
                assert kind[gy, gx] == mip_ref.MISS
                continue
            o, d, tnear, tfar, step, offset = ray
            assert abs(d[0] - 1.0) < 1e-6 and tnear > 0.5
            if min(1 - abs(o[1]), 1 - abs(o[2])) < 1e-3:
                continue   # grazes an edge of the box: float32 and float64 may disagree on the hit
            assert kind[gy, gx] == mip_ref.SAMPLED
            n_nominal = round((tfar - tnear) / step)
            assert count[gy, gx] in (n_nominal, n_nominal + 1)
            lo = ramp(1.0 - offset - step) - 1e-5
            hi = ramp(1.0 - offset) + 1e-5
            assert lo <= m[gy, gx] <= hi, (gx, gy, lo, m[gy, gx], hi)
            assert hi - lo <= step * N / (2.0 * (N - 1)) + 3e-5   # the sampling error: slope x step length
            checked += 1
    assert checked > 50


def test_known_answer_single_voxel_footprint():
    """One bright voxel in an empty FLOAT volume, orthographic camera along -z, linear filter: m > 0 exactly on the
    pixels whose ray passes within one texel of the voxel's centre in x and y (the trilinear tent's support), and
    there m is the product of the two tents times the best sample's tent along the ray -- at rate 2 a sample
    lies within a quarter texel of the centre plane."""
    N, rate, seed = 24, 2.0, SEEDS[2]
    vox = (9, 13, 11)   # x, y, z
    vol = np.zeros((N, N, N), np.float32)
    vol[vox[2], vox[1], vox[0]] = 1.0
    view = frontend.view_matrix(frontend.DEFAULT_ROTATION, (0.0, 0.0, 1.5))
    cam, rp, rc = _params(view, (N, N, N), ortho=1, rate=rate, seed=seed, linear=1)
    _, m, kind, _ = mip_ref.render_tile(vol, mip_ref.FLOAT, frontend.tff_from_stops(), cam, rp, rc, W=W, H=H)
    lit = 0
    for gy in range(H):
        for gx in range(W):
            ray = _ortho_ray(view, gx, gy, seed, (N, N, N), rate)
            if ray is None:
                assert kind[gy, gx] == mip_ref.MISS and m[gy, gx] == -np.inf
                continue
            o, d, _, _, step, _ = ray
            assert abs(d[2] + 1.0) < 1e-6
            u = (o[0] * 0.5 + 0.5) * N - 0.5 - vox[0]
            v = (o[1] * 0.5 + 0.5) * N - 0.5 - vox[1]
            if min(abs(abs(u) - 1), abs(abs(v) - 1), 1 - abs(o[0]), 1 - abs(o[1])) < 1e-3:
                continue   # on the rim of the footprint or of the box
            tent = max(0.0, 1 - abs(u)) * max(0.0, 1 - abs(v))
            if tent == 0.0:
                assert m[gy, gx] == 0.0, (gx, gy)
            else:
                lit += 1
                step_texels = step * N / 2.0
                assert step_texels <= 0.5 + 1e-6
                assert tent * (1 - step_texels / 2) - 1e-5 <= m[gy, gx] <= tent + 1e-5, (gx, gy)
    assert lit >= 4


def test_known_answer_empty_and_miss():
    """An empty volume and a ray that misses the box give the background exactly."""
    bg = [0.1, 0.9, 0.5, 0.25]
    tff = frontend.tff_from_stops()
    want = np.asarray(bg, np.float32).view(np.uint32)
    for fmt, dt in ((mip_ref.UCHAR, np.uint8), (mip_ref.FLOAT, np.float32)):
        vol = np.zeros((20, 24, 28), dt)
        for linear in (0, 1):
            cam, rp, rc = _params(V["rot30"], (28, 24, 20), linear=linear, bg=bg)
            img, m, kind, _ = mip_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H)
            assert (kind == mip_ref.SAMPLED).any() and np.all(m[kind == mip_ref.SAMPLED] == 0)
            assert np.all(img.view(np.uint32) == want)   # (TF(0) of the default table is fully transparent)
    vol = common.noise_volume((28, 24, 20), 2)
    away = frontend.view_matrix(frontend.DEFAULT_ROTATION, (6.0, 0.0, 2.0))
    cam, rp, rc = _params(away, (28, 24, 20), linear=1, bg=bg)
    img, m, kind, count = mip_ref.render_tile(vol, mip_ref.FLOAT, frontend.opaque_ramp_tff(), cam, rp, rc, W=W, H=H)
    assert np.all(kind == mip_ref.MISS) and np.all(count == 0) and np.all(m == -np.inf)
    assert np.all(img.view(np.uint32) == want)
    # a ray that hits sees the volume: the same scene from the front is not the background
    cam, rp, rc = _params(V["default"], (28, 24, 20), linear=1, bg=bg)
    img, _, kind, _ = mip_ref.render_tile(vol, mip_ref.FLOAT, frontend.opaque_ramp_tff(), cam, rp, rc, W=W, H=H)
    assert (kind == mip_ref.SAMPLED).any() and not np.all(img.view(np.uint32) == want)
    assert C.sizeof(vro.CameraParams) == 128
