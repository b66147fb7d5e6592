"""The CPU restatement of technique 8 (pre-integrated classification, tests/ref/preint_ref.c) and the library's host
function vrhip_preint_slab, on the CPU alone: the two against each other bit for bit, both against an independent
extended-precision evaluation of the integrals, the exact zero of a transparent interval, the ray caster's read for
sf == sb, the oracle's technique-0 frame on volumes that are constant along every ray, and the point of the feature
stated as conditions on a scene whose peak technique 0 steps over.  tests/test_gpu_preint.py then holds the HIP
kernel to the restatement."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import vro
from tests import common, preint_ref
from tests.test_mip_ref import SEEDS, _params
from volumerenderercl_amd import _lib, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "r4", "preint_accuracy.json")
W, H = 40, 32
BG = [0.1, 0.9, 0.5, 0.25]
SIZES = (1, 2, 256, 4096)
INF, NAN = float("inf"), float("nan")
FMT_NAMES = {"UCHAR": preint_ref.UCHAR, "USHORT": preint_ref.USHORT, "FLOAT": preint_ref.FLOAT}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_table(rng, n, transparent=0.3):
    t = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    t[rng.random(n) < transparent, 3] = 0
    return t


def lib_slab(E, sf, sb, raw=False):
    out = (C.c_float * 4)()
    rc = _lib.load().vrhip_preint_slab(E.ctypes.data, E.shape[0], 1 if raw else 0, float(sf), float(sb), out)
    assert rc == _lib.OK, (rc, sf, sb, raw)
    return np.array(out[:], np.float32)


def _value_at(u, n):
    """The value whose table coordinate is (about) u."""
    return np.float32((u + 0.5) / n)


def _cases(rng, n):
    """(sf, sb) pairs: on knots, inside one segment, across one knot, across many, beyond both ends, reversed."""
    k = int(rng.integers(0, n))
    pairs = [(_value_at(k, n), _value_at(min(k + 1, n - 1), n)),            # knot to knot
             (_value_at(k, n), _value_at(k, n)),                            # the same knot
             (_value_at(k + 0.2, n), _value_at(k + 0.7, n)),                # inside one segment
             (_value_at(k + 0.9, n), _value_at(k + 1.1, n)),                # across one knot
             (_value_at(0.3, n), _value_at(n - 1.4, n)),                    # across (nearly) all of them
             (np.float32(-0.2), np.float32(1.3)), (np.float32(-0.4), np.float32(-0.1)),   # beyond the ends
             (np.float32(1.01), np.float32(1.5)), (np.float32(0.0), np.float32(1.0))]
    pairs += [(np.float32(a), np.float32(b)) for a, b in rng.uniform(-0.1, 1.1, (60, 2))]
    a = rng.uniform(0, 1, 20).astype(np.float32)
    pairs += [(x, np.nextafter(x, np.float32(2))) for x in a]              # one ulp apart
    return pairs + [(b, a) for a, b in pairs]                              # ... and reversed


@pytest.mark.parametrize("n", SIZES)
def test_library_slab_equals_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    for trial in range(3):
        E = preint_ref.entries(random_table(rng, n, transparent=0.3 * trial))
        for sf, sb in _cases(rng, n):
            for raw in (False, True):
                got, want = lib_slab(E, sf, sb, raw), preint_ref.slab(E, sf, sb, raw)
                assert np.array_equal(_bits(got), _bits(want)), (n, sf, sb, raw, got, want)
        # RAW values far outside the table, infinities and NaN (a NaN reads coordinate -1: entry 0)
        special = [-INF, -3e38, -2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 2.0, 5.0, 3e38, INF, NAN]
        for sf in special:
            for sb in special:
                got, want = lib_slab(E, sf, sb, True), preint_ref.slab(E, sf, sb, True)
                assert np.array_equal(_bits(got), _bits(want)), (n, sf, sb, got, want)
                assert np.all(np.isfinite(got)) and np.all(got >= 0) and got[3] <= 1
        assert np.array_equal(_bits(lib_slab(E, NAN, NAN, True)), _bits(E[0]))
        assert np.array_equal(_bits(lib_slab(E, NAN, -5.0, True)), _bits(E[0]))
        assert np.array_equal(_bits(lib_slab(E, INF, 7.0, True)), _bits(E[n - 1]))
    # the Python front end is the same call on the uint8 table
    t = random_table(rng, n)
    assert np.array_equal(_bits(frontend.preint_slab(t, 0.25, 0.75)), _bits(preint_ref.slab(preint_ref.entries(t), 0.25, 0.75)))
    # refusals: nothing is written
    out = (C.c_float * 4)(9, 9, 9, 9)
    slab = _lib.load().vrhip_preint_slab
    E = preint_ref.entries(t)
    assert slab(None, n, 0, 0.0, 1.0, out) == _lib.ERR_INVALID
    assert slab(E.ctypes.data, 0, 0, 0.0, 1.0, out) == _lib.ERR_INVALID
    assert slab(E.ctypes.data, 4097, 0, 0.0, 1.0, out) == _lib.ERR_INVALID
    assert slab(E.ctypes.data, n, 0, 0.0, 3.0, out) == _lib.ERR_INVALID     # not RAW: values in [-1, 2]
    assert slab(E.ctypes.data, n, 0, NAN, 0.5, out) == _lib.ERR_INVALID
    assert slab(E.ctypes.data, n, 0, 0.0, 1.0, None) == _lib.ERR_INVALID
    assert list(out) == [9, 9, 9, 9]


# ---- accuracy: an evaluation of the same integrals written separately, in extended precision

def _coords(x, n):
    f = np.float32
    return (x.astype(np.float32) * f(n) - f(0.5)).astype(np.float32)


def exact_slabs(E, ua, ub):
    """(Cbar.rgb, abar) for the table coordinates ua != ub (float32 arrays), in np.longdouble: per segment the
    mean-value forms -- a linear integrand's integral is h * f(mid), a quadratic one's h * (f(mid) + f'' h^2 / 24) --
    and the classical whole-segment integrals (pa + qa) / 2 and (pc pa + qc qa) / 3 + (pc qa + qc pa) / 6, cumulated."""
    L = np.longdouble
    n = E.shape[0]
    Ed = E.astype(L)
    lo, hi = np.minimum(ua, ub).astype(L), np.maximum(ua, ub).astype(L)
    jl = np.clip(np.floor(lo), -1, n - 1).astype(np.int64)
    jh = np.clip(np.floor(hi), -1, n - 1).astype(np.int64)
    p, q = Ed[:-1], Ed[1:]
    whole = np.zeros((max(n - 1, 0), 4), L)
    if n > 1:
        whole[:, 3] = (p[:, 3] + q[:, 3]) / 2
        whole[:, :3] = (p[:, :3] * p[:, 3:] + q[:, :3] * q[:, 3:]) / 3 + (p[:, :3] * q[:, 3:] + q[:, :3] * p[:, 3:]) / 6
    cum = np.concatenate([np.zeros((1, 4), L), np.cumsum(whole, axis=0)])   # cum[i] = the integral over [0, i]

    def part(j, u0, u1):
        pe, qe = Ed[np.clip(j, 0, n - 1)], Ed[np.clip(j + 1, 0, n - 1)]
        tail = (j < 0) | (j >= n - 1)
        h = (u1 - u0)[:, None]
        mid = np.where(tail, L(0), (u0 + u1) / 2 - j)[:, None]
        d = qe - pe
        a_mid = pe[:, 3:] + mid * d[:, 3:]
        c_mid = pe[:, :3] + mid * d[:, :3]
        out = np.empty((len(j), 4), L)
        out[:, 3:] = h * a_mid
        out[:, :3] = h * (c_mid * a_mid + d[:, :3] * d[:, 3:] * np.where(tail[:, None], L(0), h * h) / 12)
        return out

    same = jl == jh
    total = np.where(same[:, None], part(jl, lo, hi),
                     part(jl, lo, np.minimum(jl + 1, hi).astype(L)) + (cum[jh] - cum[np.minimum(jl + 1, n - 1)]) +
                     part(jh, np.maximum(jh, lo).astype(L), hi))
    mean = total / (hi - lo)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        colour = np.where(mean[:, 3:] > 0, total[:, :3] / total[:, 3:], L(0))
    return np.concatenate([colour, mean[:, 3:]], axis=1)


def interval_set(rng, n, count=10000):
    """Random values over and a little beyond [0, 1]; a fifth of the intervals short (a few ulps), and of those the
    ones low in the table shorter than 2^-20 of a texel."""
    sf = rng.uniform(-0.05, 1.05, count).astype(np.float32)
    sb = rng.uniform(-0.05, 1.05, count).astype(np.float32)
    k = count // 5
    sf[:k] = (rng.uniform(0.0, min(3.5, 1.9 * n), k) / n).astype(np.float32)   # table coordinates -0.5 .. 3: ulp <= 2^-22
    sb[:k] = sf[:k]
    for _ in range(3):
        step = rng.random(k) < 0.6
        sb[:k] = np.where(step, np.nextafter(sb[:k], np.float32(2)), sb[:k])
    return sf, sb


def measure_errors(n, seed=0):
    """The largest absolute error per channel (r, g, b, a) of vrhip_preint_slab against exact_slabs over
    interval_set, and how many of the intervals were shorter than 2^-20 of a texel."""
    rng = np.random.default_rng(7000 + 13 * n + seed)
    E = preint_ref.entries(random_table(rng, n))
    sf, sb = interval_set(rng, n)
    ua, ub = _coords(sf, n), _coords(sb, n)
    keep = ua != ub
    sf, sb, ua, ub = sf[keep], sb[keep], ua[keep], ub[keep]
    got = np.stack([lib_slab(E, a, b) for a, b in zip(sf, sb)])
    want = exact_slabs(E, ua, ub)
    err = np.abs(got.astype(np.longdouble) - want).max(axis=0)
    short = int(np.sum(np.abs(ub.astype(np.float64) - ua.astype(np.float64)) < 2.0 ** -20))
    return [float(e) for e in err], short, int(keep.sum())


def accuracy_limit(n):
    """4 x the error recorded in profiles/r4/preint_accuracy.json (headroom for other libm builds), at most 1e-6: the
    outputs are fp32 values of size <= 1 after three fp32 roundings, so more than that is cancellation -- a bug."""
    rec = json.load(open(ACCURACY))["max_abs_error"][str(n)]
    return [min(4.0 * e, 1e-6) for e in rec]


@pytest.mark.parametrize("n", SIZES)
def test_accuracy_against_an_independent_evaluation(n):
    err, short, count = measure_errors(n)
    print("n %d: max |error| rgba %s over %d intervals, %d shorter than 2^-20 texel" % (n, err, count, short))
    assert count >= 8000 and (n == 1 or short >= 100)
    limit = accuracy_limit(n)
    assert all(e <= l for e, l in zip(err, limit)), (err, limit)


@pytest.mark.parametrize("n", SIZES)
def test_transparent_interval_is_exactly_plus_zero(n):
    """Every entry the interval can read has alpha 0 -- whatever its colour: abar has the bits of +0.0f and Cbar is 0."""
    rng = np.random.default_rng(n)
    t = random_table(rng, n, transparent=0.0)
    t[:, 3] = np.where(t[:, 3] == 0, 1, t[:, 3])
    lo, hi = (0, n) if n <= 2 else (n // 4, n // 2)
    t[lo:hi, 3] = 0
    E = preint_ref.entries(t)
    pairs = []
    for _ in range(300):
        a, b = sorted(rng.uniform(lo, max(lo, hi - 1), 2)) if n > 2 else sorted(rng.uniform(-1.4, 1.4, 2))
        pairs.append((_value_at(a, n), _value_at(b, n)))
    if n > 2:
        pairs += [(_value_at(lo + 0.01, n), _value_at(hi - 1.01, n)), (_value_at(lo, n), _value_at(hi - 1, n))]
    checked = 0
    for sf, sb in pairs:
        ua, ub = _coords(np.array([sf, sb]), n)
        i0 = int(np.clip(np.floor(min(ua, ub)), 0, n - 1))
        i1 = int(np.clip(np.floor(max(ua, ub)) + 1, 0, n - 1))
        if t[i0:i1 + 1, 3].any():
            continue
        checked += 1
        for a, b in ((sf, sb), (sb, sf)):
            for got in (lib_slab(E, a, b), preint_ref.slab(E, a, b)):
                assert _bits(got)[3] == 0, (n, a, b, got)
                assert ua == ub or np.all(_bits(got)[:3] == 0), (n, a, b, got)
    assert checked >= 100


@pytest.mark.parametrize("n", SIZES)
def test_equal_ends_give_the_ray_casters_read(n):
    rng = np.random.default_rng(50 + n)
    E = preint_ref.entries(random_table(rng, n))
    xs = np.concatenate([rng.uniform(-0.2, 1.2, 300), [0.0, 1.0, -1.0, 2.0, 0.5]]).astype(np.float32)
    for x in xs:
        for raw in (False, True):
            want = preint_ref.tff_linear(E, x, raw)
            assert np.array_equal(_bits(lib_slab(E, x, x, raw)), _bits(want)), (n, x, raw)
            assert np.array_equal(_bits(preint_ref.slab(E, x, x, raw)), _bits(want)), (n, x, raw)
    # tff_linear itself, in numpy: fmaf(a, t1 - t0, t0) through float64 (exact product, one rounding that matters)
    ub = _coords(xs, n)
    fl = np.floor(ub)
    a = (ub - fl).astype(np.float32)[:, None]
    i = fl.astype(np.int64)
    t0, t1 = E[np.clip(i, 0, n - 1)], E[np.clip(i + 1, 0, n - 1)]
    want = (a.astype(np.float64) * (t1 - t0).astype(np.float64) + t0.astype(np.float64)).astype(np.float32)
    got = np.stack([preint_ref.tff_linear(E, x) for x in xs])
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n", SIZES)
def test_all_entries_equal_give_that_entry(n):
    rng = np.random.default_rng(n + 9)
    entry = np.array([200, 17, 99, 140], np.uint8)
    E = preint_ref.entries(np.repeat(entry[None], n, axis=0))
    limit = accuracy_limit(n)
    sf, sb = interval_set(rng, n, 2000)
    for a, b in zip(sf, sb):
        got = lib_slab(E, a, b)
        assert np.all(np.abs(got.astype(np.float64) - E[0].astype(np.float64)) <= np.array(limit)[[0, 1, 2, 3]]), (n, a, b, got)


# ---- frames

def _constant_along_rays(fmt, res, view):
    """A volume that is constant along the viewing direction of an orthographic camera looking down z: values vary
    in x and y only.  Every ray then reads one value at all of its samples (nearest filter)."""
    x, y, z = res
    rng = np.random.default_rng(3)
    plane = rng.uniform(0, 1, (1, y, x))
    f = np.broadcast_to(plane, (z, y, x))
    if fmt == preint_ref.UCHAR:
        return np.ascontiguousarray(np.round(f * 255).astype(np.uint8))
    if fmt == preint_ref.USHORT:
        return np.ascontiguousarray(np.round(f * 65535).astype(np.uint16))
    return np.ascontiguousarray((f * 1.4 - 0.2).astype(np.float32))


@pytest.mark.parametrize("illum", [0, 1])
@pytest.mark.parametrize("fmt", sorted(FMT_NAMES))
def test_constant_volume_is_the_oracles_technique_0(fmt, illum):
    """sf == sb at every slab: the frame is the oracle's technique-0 frame (ESS off) bit for bit -- the ray, the
    filter, the read, the shading and the compositing at once.  A volume of one value from two views; and a volume
    that varies across the rays but not along them (orthographic, down the z axis), on the rays whose samples the
    restatement reports as all equal."""
    f = FMT_NAMES[fmt]
    res = (24, 17, 3)
    tff = frontend.tff_from_stops()
    dt = {preint_ref.UCHAR: np.uint8, preint_ref.USHORT: np.uint16, preint_ref.FLOAT: np.float32}[f]
    value = {preint_ref.UCHAR: 140, preint_ref.USHORT: 30000, preint_ref.FLOAT: 0.37}[f]
    vol = np.full((res[2], res[1], res[0]), value, dt)
    for view, seed in zip(("rot30", "close"), SEEDS):
        # (the linear filter clamps to the edge: the value is the same wherever a sample falls)
        cam, rp, rc = _params(common.views()[view], res, seed=seed, linear=1, bg=BG)
        rp.illumType = illum
        ref, st, _ = vro.render_tile(vol, f, tff, cam, rp, rc, use_ess=False, W=W, H=H)
        img, kind, samples, visible, marginal = preint_ref.render_tile(vol, f, tff, cam, rp, rc, W=W, H=H)
        assert np.any(ref[..., 3] > 0)
        assert np.array_equal(_bits(img), _bits(ref)), int(np.sum(np.any(_bits(img) != _bits(ref), axis=-1)))
        assert st["samples_taken"] == int(samples.sum())
    vol = _constant_along_rays(f, res, None)
    cam, rp, rc = _params(common.views()["default"], res, ortho=1, seed=SEEDS[2], linear=1, bg=BG)
    rp.illumType = illum
    ref, _, _ = vro.render_tile(vol, f, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    img, _, _, _, _, values = preint_ref.render_tile(vol, f, tff, cam, rp, rc, W=W, H=H, max_values=64)
    steady = np.all((values == values[..., :1]) | np.isnan(values), axis=-1)
    assert steady.sum() > steady.size // 4
    assert np.array_equal(_bits(img)[steady], _bits(ref)[steady])


# ---- the point of the feature

def peak_scene():
    """32^3 UCHAR radial ramp, value = distance from the centre / 1.2 in box units (0.5 on the sphere of radius 0.6),
    and a 256-entry table that is opaque white in the two entries at 0.5 and transparent elsewhere."""
    g = (np.arange(32) + 0.5) / 16.0 - 1.0
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    vol = np.round(np.clip(np.sqrt(xx * xx + yy * yy + zz * zz) / 1.2, 0, 1) * 255).astype(np.uint8)
    tff = np.zeros((256, 4), np.uint8)
    tff[127:129] = 255
    return vol, tff


def crossing_rays(values, tff):
    """Rays with two consecutive samples on either side of the peak: one at or below the last transparent entry
    before it, the other at or above the first transparent entry after it (table coordinates)."""
    n = tff.shape[0]
    shown = np.flatnonzero(tff[:, 3])
    below, above = shown[0] - 1, shown[-1] + 1
    with np.errstate(invalid="ignore"):
        u = values * np.float32(n) - np.float32(0.5)
        a, b = u[..., :-1], u[..., 1:]
        cross = (np.minimum(a, b) <= below) & (np.maximum(a, b) >= above)
    return np.any(cross, axis=-1)


def peak_params(rate, seed=SEEDS[0]):
    cam, rp, rc = _params(common.views()["rot30"], (32, 32, 32), rate=rate, seed=seed, linear=1, bg=[0.0, 0.0, 0.0, 0.0])
    rp.illumType = 0
    return cam, rp, rc


def test_the_peak_between_two_samples_is_seen():
    vol, tff = peak_scene()
    fmt = preint_ref.UCHAR
    cam, rp, rc = peak_params(0.5)
    pre, _, samples, _, _, values = preint_ref.render_tile(vol, fmt, tff, cam, rp, rc, W=W, H=H, max_values=96)
    assert samples.max() <= 96
    R = crossing_rays(values, tff)
    assert R.sum() > 100
    # A: technique 8 shows the peak on every such ray
    assert np.all(pre[..., 3][R] > 0)
    # B: technique 0 at the same rate steps over it on some of them (a property of the scene)
    t0_low, _, _ = vro.render_tile(vol, fmt, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    missed = int(np.sum(t0_low[..., 3][R] == 0))
    print("rays across the peak: %d, of them technique 0 misses %d" % (R.sum(), missed))
    assert missed >= 1
    # C: against technique 0 at samplingRate 16, technique 8 at 0.5 is closer than technique 0 at 0.5
    cam, rp, rc = peak_params(16.0)
    t0_high, _, _ = vro.render_tile(vol, fmt, tff, cam, rp, rc, use_ess=False, W=W, H=H)
    d_pre = float(np.mean(np.abs(pre.astype(np.float64) - t0_high)))
    d_t0 = float(np.mean(np.abs(t0_low.astype(np.float64) - t0_high)))
    print("mean |difference| to technique 0 at rate 16: technique 8 at 0.5 %.6f, technique 0 at 0.5 %.6f" % (d_pre, d_t0))
    assert d_pre < d_t0
