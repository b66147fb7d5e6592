"""The CPU restatement of the depth images (tests/ref/depth_ref.c) pinned to what the project already trusts, on the
CPU alone, every check on raw bits: ISO to technique 4's restatement (kind, t_hit), MAX to technique 2's (m, kind) and
to a brute-force search for the first sample that attains m, OPACITY to the alpha channel of the oracle's technique-0
frames, the positions to cam + dir * (t - offset) recomputed from the restatement's own rays.
tests/test_gpu_depth.py then holds the HIP kernel to the restatement."""
import math

import numpy as np
import pytest

from oracle import vro
from tests import common, depth_ref, iso_ref, mip_ref
from tests.test_mip_ref import CASES, SEEDS, _params

W = H = 64   # (the frames of tests/test_iso_ref.py)
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scene(case, fmt=depth_ref.UCHAR, linear=1, seed=SEEDS[0], **over):
    kw = dict(CASES[case])
    kw.update(over)
    vol = common.noise_volume(kw["res"], fmt, 2, smooth=False)
    cam, rp, rc = _params(seed=seed, linear=linear, **kw)
    return vol, cam, rp, rc


def _float_volume_with_specials(res=(28, 24, 20)):
    """FLOAT voxels outside [0, 1], with NaN and +-inf islands."""
    vol = common.noise_volume(res, depth_ref.FLOAT, 5, smooth=False) * F32(1.6) - F32(0.3)
    vol[4:7, 5:9, 6:10] = np.nan
    vol[12:14, 10:13, 15:18] = np.inf
    vol[9:11, 16:19, 3:6] = -np.inf
    return vol


# ---- ISO: technique 4's hit and refinement, word for word

@pytest.mark.parametrize("refine", [0, 4, 16])
@pytest.mark.parametrize("case", sorted(CASES))
def test_iso_equals_technique4_restatement(case, refine):
    """kind and t equal iso_ref.render_tile's kind and t_hit; `inside` starts in the solid (hits at k = 0, unrefined)."""
    vol, cam, rp, rc = _scene(case)
    tff = common.tffs()["default"]
    iso = 0.08 if case == "inside" else 0.35
    _, kind4, k4, t4, _ = iso_ref.render_tile(vol, iso_ref.UCHAR, tff, cam, rp, rc, iso_value=iso, refine_steps=refine,
                                              W=W, H=H)
    xyzt, aux, kind = depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.ISO, iso, refine, W=W, H=H)
    assert np.array_equal(kind, kind4)
    hit = kind == depth_ref.HIT
    assert hit.any()
    if case == "inside":
        assert np.any(k4[hit] == 0)
    else:
        assert np.any(k4[hit] > 0) and (kind == depth_ref.NO_HIT).any()
    assert np.array_equal(_bits(xyzt[..., 3])[hit], _bits(t4)[hit])
    assert np.all(np.isposinf(xyzt[..., 3][~hit])) and np.all(xyzt[..., :3][~hit] == 0)
    assert np.all(aux[hit] >= F32(iso)) and np.all(aux[~hit] == 0)


@pytest.mark.parametrize("linear", [0, 1])
def test_iso_float_volume_with_nan_and_inf(linear):
    vol = _float_volume_with_specials()
    res = (vol.shape[2], vol.shape[1], vol.shape[0])
    cam, rp, rc = _params(common.views()["rot30"], res, linear=linear)
    tff = common.tffs()["default"]
    for iso, refine in ((0.7, 4), (1.2, 16), (-0.1, 0)):
        _, kind4, _, t4, _ = iso_ref.render_tile(vol, iso_ref.FLOAT, tff, cam, rp, rc, iso_value=iso,
                                                 refine_steps=refine, W=W, H=H)
        xyzt, aux, kind = depth_ref.render(vol, depth_ref.FLOAT, None, cam, rp, rc, depth_ref.ISO, iso, refine, W=W, H=H)
        hit = kind == depth_ref.HIT
        assert np.array_equal(kind, kind4) and hit.any()
        assert np.array_equal(_bits(xyzt[..., 3])[hit], _bits(t4)[hit])
        assert not np.isnan(aux).any() and np.all(aux[hit] >= F32(iso))   # a NaN never hits
        if iso == 1.2:
            assert np.isposinf(aux).any()   # (the +inf island is hit)


# ---- MAX: technique 2's maximum, and the first sample that attains it

def _nearest_samples(vol, fmt, rays, n_max):
    """s_k of the nearest filter for every ray, k < n_max, in numpy float32: [n_rays, n_max]; NaN past the ray's end."""
    d, h, w = vol.shape
    inv_max = {0: F32(1) / F32(255), 1: F32(1) / F32(65535), 2: F32(1)}[fmt]
    t = rays["tnear"].copy()
    alive = t < rays["tfar"]
    out = np.full((rays.size, n_max), np.nan, F32)
    ts = np.full((rays.size, n_max), np.nan, F32)
    for k in range(n_max):
        dist = t - rays["offset"]
        p = [(rays["cam"][:, a] + rays["dir"][:, a] * dist) * F32(0.5) + F32(0.5) for a in range(3)]
        with np.errstate(invalid="ignore"):
            f = [np.floor(p[a] * F32((w, h, d)[a])) for a in range(3)]
            ok = np.ones(rays.size, bool)
            for a in range(3):
                ok &= (f[a] >= 0) & (f[a] <= F32((w, h, d)[a] - 1))
        idx = [np.where(ok, f[a], 0).astype(np.int64) for a in range(3)]
        s = np.where(ok, vol[idx[2], idx[1], idx[0]].astype(F32) * inv_max, F32(0))
        out[alive, k] = s[alive]
        ts[alive, k] = t[alive]
        tn = t + rays["step"]
        alive = alive & (tn > t) & (tn < rays["tfar"])
        t = np.where(alive, tn, t)
        if not alive.any():
            return out[:, :k + 1], ts[:, :k + 1]
    raise AssertionError("rays longer than %d samples" % n_max)


@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_max_equals_technique2_restatement(case, linear):
    vol, cam, rp, rc = _scene(case, linear=linear)
    tff = common.tffs()["default"]
    _, m2, kind2, count2 = mip_ref.render_tile(vol, mip_ref.UCHAR, tff, cam, rp, rc, W=W, H=H)
    xyzt, aux, kind, rays = depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.MAX, W=W, H=H,
                                             with_rays=True)
    assert np.array_equal(kind, kind2)   # (MISS / NO_SAMPLE / SAMPLED are 0 / 1 / 2: no ray of this volume is all NaN)
    entered = kind != depth_ref.MISS
    hit = kind == depth_ref.HIT
    assert hit.any() and np.array_equal(_bits(aux)[entered], _bits(m2)[entered]) and np.all(aux[~entered] == 0)
    if not linear:
        # brute force: the first sample whose value equals m
        r = rays[hit]
        s, ts = _nearest_samples(vol, depth_ref.UCHAR, r, 4096)
        assert np.array_equal(np.sum(~np.isnan(ts), axis=1), count2[hit])
        with np.errstate(invalid="ignore"):
            assert np.array_equal(_bits(np.nanmax(s, axis=1)), _bits(aux[hit]))
            first = np.argmax(s == aux[hit][:, None], axis=1)
        assert np.array_equal(_bits(ts[np.arange(r.size), first]), _bits(xyzt[..., 3][hit]))
        assert np.any(first > 0)
    else:
        # the linear filter: the first sample at or above m is the first that attains it -- ISO with threshold m and no
        # refinement, a pixel at a time, on a sample of the hits
        # (NOT an independent search: it is this restatement's own ISO march, which the tests above pin to iso_ref.c;
        #  the numpy search covers the nearest filter alone, where a fetch needs no emulated fma)
        ys, xs = np.nonzero(hit)
        for i in range(0, ys.size, max(1, ys.size // 48)):
            y, x = int(ys[i]), int(xs[i])
            one = depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.ISO, float(aux[y, x]), 0, W=W, H=H,
                                   rect=(x, y, 1, 1))
            assert one[2][0, 0] == depth_ref.HIT
            assert _bits(one[0])[0, 0, 3] == _bits(xyzt)[y, x, 3] and _bits(one[1])[0, 0] == _bits(aux)[y, x]


def test_max_of_rays_that_never_replace_m_is_no_hit():
    """All NaN (the linear filter clamps to the edge: nothing but NaN) or all -inf: `s > m` never holds."""
    cam, rp, rc = _params(common.views()["rot30"], (12, 12, 12), linear=1)
    for fill in (np.nan, -np.inf):
        vol = np.full((12, 12, 12), fill, F32)
        xyzt, aux, kind = depth_ref.render(vol, depth_ref.FLOAT, None, cam, rp, rc, depth_ref.MAX, W=W, H=H)
        entered = kind != depth_ref.MISS
        assert entered.any() and np.all(kind[entered] == depth_ref.NO_HIT)
        assert np.all(np.isneginf(aux[entered])) and np.all(np.isposinf(xyzt[..., 3]))


# ---- OPACITY: technique 0's accumulated opacity

RATES = sorted({CASES[c].get("rate", 1.5) for c in CASES})


def test_powr_of_one_is_one():
    """What lets the kernel step over samples of opacity 0: opacity = 1 - powr(1, 1 / rate) = 0 exactly."""
    for rate in RATES + [0.1, 3.0, 1000.0]:
        assert vro.lib().vro_powr(1.0, float(F32(1) / F32(rate))) == 1.0


@pytest.mark.parametrize("tf", ["default", "haze", "opaque"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_opacity_equals_oracle_technique0_alpha(case, tf):
    """threshold 0.98f: the oracle's early ray termination `(double)alpha > 0.98` and the fp32 `alpha >= 0.98f` select
    the same floats (0.98f is the smallest float above 0.98), so both stop at the same sample and aux is the oracle's
    alpha channel on every pixel whose ray enters the box (object-order ESS off, no depth cue, no showEss)."""
    vol, cam, rp, rc = _scene(case)
    tff = common.tffs()[tf]
    assert float(F32(0.98)) > 0.98 > float(np.nextafter(F32(0.98), F32(0)))
    rc.aerial, rp.showEss = 0, 0
    img, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    xyzt, aux, kind = depth_ref.render(vol, depth_ref.UCHAR, tff, cam, rp, rc, depth_ref.OPACITY, float(F32(0.98)),
                                       W=W, H=H)
    entered = kind != depth_ref.MISS
    assert st["rays_hit"] == int(entered.sum()) and entered.any()
    assert np.array_equal(_bits(aux)[entered], _bits(img[..., 3])[entered])
    hit = kind == depth_ref.HIT
    assert np.array_equal(hit, entered & (img[..., 3] >= F32(0.98)))
    if tf == "opaque":
        assert hit.any()
    assert (entered & ~hit).any() or case == "inside"   # (from inside, every ray may reach the threshold)


# ---- positions and the edges of the threshold

@pytest.mark.parametrize("mode", [depth_ref.ISO, depth_ref.MAX, depth_ref.OPACITY])
@pytest.mark.parametrize("case", ["perspective", "orthographic", "clip_box", "anisotropic"])
def test_positions_are_the_rays_own(case, mode):
    vol, cam, rp, rc = _scene(case, seed=SEEDS[1])
    tff = common.tffs()["opaque"]
    xyzt, aux, kind, rays = depth_ref.render(vol, depth_ref.UCHAR, tff, cam, rp, rc, mode, 0.3, 4, W=W, H=H,
                                             with_rays=True)
    hit = kind == depth_ref.HIT
    assert hit.any()
    r, t = rays[hit], xyzt[..., 3][hit]
    dist = t - r["offset"]
    pos = r["cam"] + r["dir"] * dist[:, None]
    assert pos.dtype == np.float32
    assert np.array_equal(_bits(pos), _bits(xyzt[..., :3][hit]))
    assert np.all(t >= r["tnear"]) and np.all(t < r["tfar"])
    # in the box, up to the jitter: sample k sits at t_k - offset with 0 <= offset < 2 |voxLen|, so the first samples
    # of a ray lie up to that far before the entry face
    res = np.asarray(CASES[case]["res"], np.float64)
    slack = 2.0 * math.sqrt(np.sum(1.0 / res ** 2))
    lo, hi = (CASES[case]["bbox"] if "bbox" in CASES[case] else ((-1, -1, -1), (1, 1, 1)))
    assert np.all(xyzt[..., :3][hit] > np.asarray(lo) - slack - 1e-5) and np.all(xyzt[..., :3][hit] < np.asarray(hi) + slack + 1e-5)


@pytest.mark.parametrize("mode", [depth_ref.ISO, depth_ref.OPACITY])
def test_threshold_zero_hits_everywhere_and_above_one_nowhere(mode):
    vol, cam, rp, rc = _scene("perspective")
    tff = common.tffs()["default"]
    xyzt, aux, kind, rays = depth_ref.render(vol, depth_ref.UCHAR, tff, cam, rp, rc, mode, 0.0, 4, W=W, H=H,
                                             with_rays=True)
    entered = kind != depth_ref.MISS
    assert entered.any() and not entered.all() and np.all(kind[entered] == depth_ref.HIT)
    assert np.array_equal(_bits(xyzt[..., 3])[entered], _bits(rays["tnear"])[entered])   # k = 0
    xyzt, aux, kind = depth_ref.render(vol, depth_ref.UCHAR, tff, cam, rp, rc, mode, 1.5, 4, W=W, H=H)
    assert np.all(kind[entered] == depth_ref.NO_HIT) and np.all(kind[~entered] == depth_ref.MISS)
    assert np.all(np.isposinf(xyzt[..., 3])) and np.all(xyzt[..., :3] == 0)
    if mode == depth_ref.OPACITY:
        assert np.any(aux[entered] > 0) and np.all(aux[entered] <= 1)   # the opacity the ray ran out of samples with
    else:
        assert np.all(aux == 0)


def test_rectangles_are_cut_from_the_frame():
    vol, cam, rp, rc = _scene("perspective")
    whole = depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.MAX, W=61, H=43)
    for rect in ((5, 3, 13, 9), (60, 42, 1, 1), (0, 0, 61, 43)):
        x0, y0, w, h = rect
        part = depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.MAX, W=61, H=43, rect=rect)
        for a, b in zip(whole, part):
            assert np.array_equal(a[y0:y0 + h, x0:x0 + w].view(np.uint8), b.view(np.uint8))


def test_invalid_parameters_are_refused():
    vol, cam, rp, rc = _scene("perspective")
    tff = common.tffs()["default"]
    bad = [dict(mode=3), dict(mode=depth_ref.ISO, threshold=math.nan), dict(mode=depth_ref.OPACITY, threshold=math.inf),
           dict(mode=depth_ref.ISO, refine=17), dict(mode=depth_ref.MAX, rect=(60, 0, 5, 5)),
           dict(mode=depth_ref.MAX, rect=(0, 0, 0, 5)), dict(mode=depth_ref.MAX, rect=(0, 0, 5, 0))]
    for kw in bad:
        with pytest.raises(RuntimeError):
            depth_ref.render(vol, depth_ref.UCHAR, tff, cam, rp, rc, W=W, H=H, **kw)
    with pytest.raises(RuntimeError):   # OPACITY without a transfer function
        depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.OPACITY, 0.5, W=W, H=H)
    depth_ref.render(vol, depth_ref.UCHAR, None, cam, rp, rc, depth_ref.MAX, math.nan, 99, W=W, H=H)   # MAX reads neither
