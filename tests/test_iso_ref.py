"""The CPU restatement of technique 4 (first-hit isosurface rendering, tests/ref/iso_ref.c) pinned to what the
project already trusts, on the CPU alone: to the oracle's technique-0 frames bit for bit on the scene where the two
coincide, to the analytic crossing of a ramp, and to known answers.  tests/test_gpu_iso.py then holds the HIP
kernel to the restatement."""
import math

import numpy as np
import pytest

from oracle import vro
from tests import common, iso_ref
from tests.test_mip_ref import CASES as MIP_CASES, SEEDS, _binary_volume, _ortho_ray, _params

W = H = 64
ZERO = [0.0, 0.0, 0.0, 0.0]

# the cases of test_mip_ref.py, and the three sampling rates on one of them
CASES = dict(MIP_CASES)
for _r in (0.5, 1.0, 2.0):
    CASES["rate_%g" % _r] = dict(view=common.views()["rot30"], res=(40, 40, 40), rate=_r)


def _step_tff(n=256, colour=(200, 90, 30)):
    """One constant colour; entry 0 fully transparent, every other entry opaque."""
    tff = np.zeros((n, 4), np.uint8)
    tff[:, :3] = colour
    tff[1:, 3] = 255
    return tff


@pytest.mark.parametrize("illum", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_equals_oracle_technique0_on_binary_volume(case, seed, illum):
    """Binary UCHAR volume {0, 255}, nearest filter, isoValue 0.5, no refinement, background 0, a transfer function of
    one constant colour that is transparent in entry 0 and opaque elsewhere.  The oracle's technique-0 ray ends at
    its first opaque sample with opacity 1 - powr(0, .) = 1, and with a zero background bg - (bg - lit) * 1 is lit
    exactly: its frame IS the first-hit frame, all four components, bit for bit, with and without shading.  The
    oracle's sample counter is the restatement's count of march samples up to and including the hit."""
    kw = dict(CASES[case])
    vol = _binary_volume(kw["res"], 7)
    tff = _step_tff()
    cam, rp, rc = _params(seed=seed, linear=0, bg=ZERO, **kw)
    rp.illumType = illum
    img, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    mine, kind, k, _, count = iso_ref.render_tile(vol, iso_ref.UCHAR, tff, cam, rp, rc, iso_value=0.5, refine_steps=0,
                                                  W=W, H=H)
    hit = kind == iso_ref.HIT
    assert hit.any() and (not hit.all() or case == "inside")
    assert np.array_equal(hit, img[..., 3] == 1.0)                       # the silhouette
    assert st["samples_taken"] == int(count.sum())                       # the samples up to the hit
    assert np.array_equal(count[hit], k[hit] + 1)
    assert np.array_equal(mine.view(np.uint32), img.view(np.uint32)), \
        "%d pixels differ" % np.sum(np.any(mine != img, axis=-1))
    assert st["rays_hit"] == int(np.sum(kind != iso_ref.MISS))
    if illum:   # the shading does something: lit pixels are not all the flat colour
        flat = vro.tff_linear(tff, 0.5)[:3]
        assert np.any(mine[hit][:, :3] != flat)


# ---- refinement: the analytic crossing of a ramp

def _ramp_scene(N=33, rate=1.3, seed=SEEDS[1]):
    from volumerenderercl_amd import frontend
    vol = np.broadcast_to(np.arange(N, dtype=np.float32) / np.float32(N - 1), (N, N, N)).copy()
    view = frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 0), -90.0), (0.0, 0.0, 2.0))
    cam, rp, rc = _params(view, (N, N, N), ortho=1, rate=rate, seed=seed, linear=1)
    return vol, view, cam, rp, rc, frontend.tff_from_stops()


def test_refinement_converges_to_the_analytic_crossing():
    """FLOAT ramp v = x / (X - 1), orthographic camera along +x, linear filter: the field along a ray is
    ((x_w * 0.5 + 0.5) * N - 0.5) / (N - 1) with x_w = o_x + (t - offset), so it crosses isoValue at
    t* = offset - o_x + ((iso * (N - 1) + 0.5) / N * 2 - 1).  The march brackets t* within one step; every refinement
    round halves the bracket: |t_hit - t*| <= step / 2^refineSteps, plus a few ulps of t (t < 4: 1 ulp <= 2.4e-7; the
    fp32 ray set-up and fetch move the crossing by some ulps of the position, and each midpoint rounds once)."""
    N, rate, seed, iso = 33, 1.3, SEEDS[1], 0.37
    vol, view, cam, rp, rc, tff = _ramp_scene(N, rate, seed)
    slack = 16 * 2.4e-7
    prev_err = None
    for steps in (0, 1, 4, 16):
        _, kind, k, t_hit, _ = iso_ref.render_tile(vol, iso_ref.FLOAT, tff, cam, rp, rc, iso_value=iso,
                                                   refine_steps=steps, W=W, H=H)
        errs = []
        for gy in range(0, H, 2):
            for gx in range(0, W, 2):
                ray = _ortho_ray(view, gx, gy, seed, (N, N, N), rate)
                if ray is None:
                    assert kind[gy, gx] == iso_ref.MISS
                    continue
                o, d, tnear, tfar, step, offset = ray
                assert abs(d[0] - 1.0) < 1e-6
                if min(1 - abs(o[1]), 1 - abs(o[2])) < 1e-3:
                    continue   # grazes an edge of the box
                assert kind[gy, gx] == iso_ref.HIT and k[gy, gx] > 0
                t_star = offset - o[0] + ((iso * (N - 1) + 0.5) / N * 2.0 - 1.0)
                err = t_hit[gy, gx] - t_star
                assert -slack <= err <= step / 2.0 ** steps + slack, (steps, gx, gy, err, step)
                errs.append(abs(err))
        assert len(errs) > 50
        worst = max(errs)
        if prev_err is not None:
            assert worst <= prev_err + slack   # non-increasing in refineSteps
        prev_err = worst
    assert prev_err <= 2 * slack   # 16 rounds: the bracket is below the resolution of t


# ---- known answers

def _all(fmt, vol, iso, linear, bg, illum=0, refine=4, tff=None, view="rot30"):
    from volumerenderercl_amd import frontend
    res = (vol.shape[2], vol.shape[1], vol.shape[0])
    cam, rp, rc = _params(common.views()[view], res, linear=linear, bg=bg)
    rp.illumType = illum
    tff = frontend.tff_from_stops() if tff is None else tff
    return iso_ref.render_tile(vol, fmt, tff, cam, rp, rc, iso_value=iso, refine_steps=refine, W=W, H=H), tff


BG = [0.1, 0.9, 0.5, 0.25]


def test_iso_above_every_voxel_keeps_the_background_alpha_included():
    vol = common.noise_volume((28, 24, 20), iso_ref.UCHAR, 2)
    for linear in (0, 1):
        (img, kind, _, _, count), _ = _all(iso_ref.UCHAR, vol, 1.5, linear, BG)
        assert (kind == iso_ref.NO_HIT).any() and not (kind == iso_ref.HIT).any()
        assert np.all(img.view(np.uint32) == np.asarray(BG, np.float32).view(np.uint32))
        assert np.all(count[kind == iso_ref.NO_HIT] > 0)


@pytest.mark.parametrize("iso", [0.0, -0.25])
def test_iso_at_or_below_zero_hits_at_the_first_sample(iso):
    """Every sample -- border reads of the nearest filter (0) included -- is >= isoValue."""
    vol = common.noise_volume((28, 24, 20), iso_ref.UCHAR, 2)
    for linear in (0, 1):
        (img, kind, k, t_hit, count), tff = _all(iso_ref.UCHAR, vol, iso, linear, BG)
        sampled = kind != iso_ref.MISS
        assert sampled.any() and np.all(kind[sampled] == iso_ref.HIT)
        assert np.all(k[sampled] == 0) and np.all(count[sampled] == 1)
        c = vro.tff_linear(tff, iso)
        assert np.all(img[sampled][:, :3].view(np.uint32) == c[:3].view(np.uint32))
        assert np.all(img[sampled][:, 3] == 1.0)
        assert np.all(img[~sampled].view(np.uint32) == np.asarray(BG, np.float32).view(np.uint32))   # a miss keeps bg


def test_constant_volume_equal_to_iso_hits_at_the_first_sample():
    vol = np.full((20, 24, 28), 0.625, np.float32)
    (img, kind, k, _, _), _ = _all(iso_ref.FLOAT, vol, 0.625, 1, BG)
    sampled = kind != iso_ref.MISS
    assert sampled.any() and np.all(kind[sampled] == iso_ref.HIT) and np.all(k[sampled] == 0)
    vol8 = np.full((20, 24, 28), 51, np.uint8)   # 51 / 255 = 0.2 in fp32: 51 * fl(1 / 255)
    iso = float(np.float32(51) * (np.float32(1.0) / np.float32(255.0)))
    (img, kind, k, _, _), _ = _all(iso_ref.UCHAR, vol8, iso, 1, BG)
    assert np.all(kind[sampled] == iso_ref.HIT) and np.all(k[sampled] == 0)
    (img, kind, _, _, _), _ = _all(iso_ref.UCHAR, vol8, float(np.nextafter(np.float32(iso), np.float32(1))), 1, BG)
    assert not (kind == iso_ref.HIT).any()


def test_nan_voxels_never_hit():
    vol = np.full((20, 24, 28), np.nan, np.float32)
    for linear in (0, 1):
        (img, kind, _, _, _), _ = _all(iso_ref.FLOAT, vol, -1.0e30, linear, BG, view="default")
        # (nearest: samples before the entry face read the border's 0 >= isoValue -- only the linear fetch, which
        #  clamps to the edge, sees nothing but NaN)
        if linear:
            assert not (kind == iso_ref.HIT).any()
            assert np.all(img.view(np.uint32) == np.asarray(BG, np.float32).view(np.uint32))
    # a NaN island in a solid: the rays through it hit behind it, never in it
    vol = np.zeros((24, 24, 24), np.float32)
    vol[:, :, 16:] = 1.0
    vol[8:16, 8:16, 4:10] = np.nan
    from volumerenderercl_amd import frontend
    view = frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 0), -90.0), (0.0, 0.0, 2.0))
    cam, rp, rc = _params(view, (24, 24, 24), ortho=1, linear=1, bg=BG)
    clean = vol.copy()
    clean[np.isnan(clean)] = 0.0
    a = iso_ref.render_tile(vol, iso_ref.FLOAT, frontend.tff_from_stops(), cam, rp, rc, 0.5, 0, W=W, H=H)
    b = iso_ref.render_tile(clean, iso_ref.FLOAT, frontend.tff_from_stops(), cam, rp, rc, 0.5, 0, W=W, H=H)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and (a[1] == iso_ref.HIT).any()


def test_surface_colour_is_the_transfer_function_at_iso():
    from volumerenderercl_amd import frontend
    vol = common.noise_volume((28, 24, 20), iso_ref.USHORT, 2)
    for tff in (frontend.tff_from_stops(), frontend.haze_tff(), frontend.opaque_ramp_tff()):
        for iso in (0.3, 0.55):
            (img, kind, _, _, _), _ = _all(iso_ref.USHORT, vol, iso, 1, BG, tff=tff)
            hit = kind == iso_ref.HIT
            assert hit.any() and not hit.all()
            c = vro.tff_linear(tff, iso)
            assert np.all(img[hit][:, :3].view(np.uint32) == c[:3].view(np.uint32))
            assert np.all(img[hit][:, 3] == 1.0)
            assert np.all(img[~hit].view(np.uint32) == np.asarray(BG, np.float32).view(np.uint32))


def test_invalid_parameters_are_refused():
    vol = np.zeros((8, 8, 8), np.uint8)
    for kw in (dict(iso=math.nan), dict(iso=math.inf), dict(iso=0.5, refine=17)):
        with pytest.raises(RuntimeError):
            _all(iso_ref.UCHAR, vol, kw["iso"], 1, BG, refine=kw.get("refine", 4))
