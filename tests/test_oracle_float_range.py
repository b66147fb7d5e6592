"""FLOAT voxels are raw values (volumerendercl.cpp:274-276, :645-646 make a CL_FLOAT image of them): a CT
volume in Hounsfield units or a simulation field reaches the kernels as it is, with values outside [0, 1],
+-inf and NaN.  The oracle's TF read and brick build against float64 restatements of the reference's rules."""
import numpy as np
import pytest

from oracle import vro
from tests import scenes

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)


def _tff(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    t[0] = [3, 250, 17, 40]          # first and last entries differ from each other and their neighbours
    t[-1] = [251, 9, 130, 222]
    return t


def _tff_linear_ref(tff, x):
    """read_imagef(tffData, linearSmp, x): normalised, CLAMP_TO_EDGE, LINEAR (OpenCL 1.2 8.2) on an RGBA8
    table, in float64.  +inf reads TF[n-1]; -inf and NaN read TF[0] (the definition, DESIGN "Numerics")."""
    n = tff.shape[0]
    t = tff.astype(np.float64) / 255.0
    if np.isnan(x) or x == -np.inf:
        return t[0]
    if x == np.inf:
        return t[n - 1]
    u = np.float64(x) * n - 0.5
    i0 = np.floor(u)
    a = u - i0
    lo = t[int(np.clip(i0, 0, n - 1))]
    hi = t[int(np.clip(i0 + 1, 0, n - 1))]
    return (1.0 - a) * lo + a * hi


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_tff_read_known_answers(n):
    """The oracle's TF read (bit-equal to the kernels' tff_linear) against 8.2 across the table, its edges
    and beyond: within 1 ulp inside, exactly TF[0] / TF[n-1] outside -- including x * n past 2^31, where an
    unclamped float -> int index conversion saturates and wraps to the wrong end of the table."""
    tff = _tff(n, seed=n)
    rng = np.random.default_rng(1)
    xs = [0.0, -0.0, 0.5 / n, 1.0 / n, (n - 0.5) / n, (n - 1.0) / n, 1.0, 1.0 + 1e-7, 1.7, 2.0, 2.0000002, 1e3,
          (2.0 ** 31 + 0.5) / n, 2.0e6, 2.2e6, 5e6, 1e30, FLT_MAX, np.inf,
          -1e-45, -1e-40, 1e-40, -0.5 / n, -1.0, -1.0000001, -3.0, -5e6, -FLT_MAX, -np.inf, np.nan]
    xs += list(rng.random(200)) + list(rng.uniform(-3, 4, 100)) + list(np.arange(n + 1) / n)
    for x in xs:
        x = float(F32(x))
        got = vro.tff_linear(tff, x).astype(np.float64)
        want = _tff_linear_ref(tff, x)
        assert np.isfinite(got).all(), x
        if x <= 0.5 / n or x >= (n - 0.5) / n or not np.isfinite(x):
            np.testing.assert_array_equal(got, want.astype(F32), err_msg="x=%r" % x)   # one entry: exact
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-7, err_msg="x=%r" % x)


def _bricks_ref(vol):
    """generateBricks (volumeraycast.cl:932-961) in float64: per brick, voxels [lo, min(lo + vpc, dim - 1))
    on each axis -- the last voxel plane excluded -- with minVal = 1, maxVal = 0 to start and OpenCL's
    min / max, which keep the number against a NaN."""
    res = [vol.shape[2], vol.shape[1], vol.shape[0]]
    _, _, tex = vro.brick_layout(res)
    vpc = [int(np.ceil(F32(res[i]) / F32(tex[i]))) for i in range(3)]
    out = np.zeros((tex[2], tex[1], tex[0], 2), np.float64)
    v = vol.astype(np.float64)
    for cz in range(tex[2]):
        for cy in range(tex[1]):
            for cx in range(tex[0]):
                lo = [vpc[0] * cx, vpc[1] * cy, vpc[2] * cz]
                hi = [min(max(lo[i] + vpc[i], 0), res[i] - 1) for i in range(3)]
                box = v[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].ravel()
                box = box[~np.isnan(box)]
                out[cz, cy, cx] = (min(1.0, box.min()) if box.size else 1.0,
                                   max(0.0, box.max()) if box.size else 0.0)
    return out


@pytest.mark.parametrize("palette", scenes.FLOAT_PALETTES + ("nan_bricks",))
@pytest.mark.parametrize("res", [(37, 29, 23), (70, 9, 66)])
def test_generate_bricks_float_range(palette, res):
    """Values outside [0, 1] meet the start values min 1 / max 0 (an all-negative brick has max 0, an
    all-above-1 brick min 1); +-inf are ordinary extrema; NaN is ignored and an all-NaN brick keeps (1, 0);
    -0.0 and +0.0 compare equal."""
    if palette == "nan_bricks":
        vol = scenes.float_volume("straddle", res, seed=3)
        vol[:12, :, :] = np.nan                  # whole bricks of NaN
        vol[20, 5, 7] = -0.0
        vol[21, 5, 7] = 1e-40
    else:
        vol = scenes.float_volume(palette, res, seed=3)
    got = vro.generate_bricks(vol, vro.FLOAT)
    want = _bricks_ref(vol)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got.astype(np.float64), want)
    if palette == "negative":
        assert np.all(got[..., 1] == 0.0)
    if palette == "huge":
        assert np.all(got[..., 0] == 1.0)
