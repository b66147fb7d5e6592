"""The oracle's fp32 definitions (vro.math_batch) against plain float64 restatements of the same operations.

Compared on D and N of tests/math_argsets.py, where the mathematical function is defined; E is checked for the
definitions' stated special cases only.  The bounds below are the worst errors MEASURED on these sets, rounded up
to the next half ulp (elementary functions: ulps of the correctly rounded fp32 result) or to the next power of
two (absolute errors).  The code is a fixed sequence of operations, so there is no noise margin.  The same table
is in DESIGN.md section 4.
"""
import numpy as np
import pytest

from oracle import vro
from tests import math_argsets as A

F64 = np.float64

# measured worst error -> asserted bound ("Measured accuracy of the definitions")
BOUNDS = {
    # ulps of the correctly rounded fp32 result              measured worst
    "logf": 1.0,                                           # 0.804
    "atan2f": 3.0,                                         # 2.955
    "acosf": 1.5,                                          # 1.191
    "len3": 1.5,                                           # 1.401
    # likewise, per exponent y = 1 / rate (0: the specular exponent 40); exp(y log x) carries the rounding of
    # t = y * log(x), half an ulp of a t of up to 87, into the result's relative error
    "powr": {0.5: 64.5,                                    # 64.211
             0.7: 107.5,                                   # 107.366
             1.0: 64.0,                                    # 64 exactly (pow(x, 1) == x: the error is a dyadic number)
             1.5: 85.0,                                    # 84.720
             2.0: 32.5,                                    # 32.280
             3.1: 36.0,                                    # 35.944
             0: 142.0},                                    # 141.728
    # absolute: sin / cos have zeros inside the domain, where an error in ulps of the result says nothing ...
    "sinf": 2.0 ** -23,                                    # 8.403e-08
    "cosf": 2.0 ** -23,                                    # 9.213e-08
    # ... and in ulps where |sin|, |cos| >= 1/2
    "sinf_ulp": 1.5,                                       # 1.410
    "cosf_ulp": 2.0,                                       # 1.546
    "normalize3": 2.0 ** -22,                              # 1.656e-07, per component
    "lerpf": 2.0 ** -24,                                   # 5.845e-08, p and q in [0, 1], w in [0, 1)
    # units of 2^-24 * (|a.x b.x| + |a.y b.y| + |a.z b.z|): a sum that cancels has no bound in ulps of the result
    "dot3": 3.0,                                           # 2.788
    # absolute, tables in [0, 1], per table size, <false> and <true> alike: the product x * n is exact for the
    # powers of two and rounded for the others
    "tff_linear": {1: 2.0 ** -26,                          # 1.391e-08
                   3: 2.0 ** -23,                          # 1.131e-07
                   255: 2.0 ** -17,                        # 7.281e-06
                   256: 2.0 ** -23,                        # 7.363e-08
                   257: 2.0 ** -17,                        # 7.439e-06
                   1024: 2.0 ** -23,                       # 6.779e-08
                   4096: 2.0 ** -23},                      # 6.942e-08
}


def half_ulp_up(v):
    return float(np.ceil(v * 2.0) / 2.0)


def pow2_up(v):
    return 0.0 if v == 0 else float(2.0 ** np.ceil(np.log2(v)))


def ulps(got, exact):
    """|got - exact| in ulps of the correctly rounded fp32 result"""
    with np.errstate(over="ignore"):
        ulp = np.abs(np.spacing(exact.astype(np.float32))).astype(F64)
    return np.abs(got.astype(F64) - exact) / ulp


def collect(op, tags, tables=False):
    """[(args float32/uint32 [n, n_in], result bits [n, n_out], table index)] of the op's cases with a tag in tags"""
    out = []
    for o, tag, args, ti in A.cases(ops={op}):
        if tag in tags:
            tff, prefix = A.tables()[ti] if ti is not None else (None, None)
            out.append((args, vro.math_batch(op, args, tff=tff, prefix=prefix), ti))
    return out


def joined(op, tags):
    c = collect(op, tags)
    return np.concatenate([a for a, _, _ in c]), np.concatenate([r for _, r, _ in c])


MEASURED = {}


def record(name, worst, bound, unit):
    MEASURED[name] = (worst, bound, unit)
    print("%-22s worst %.6g %s, bound %s" % (name, worst, unit, bound))
    return worst


def check(name, worst, bound, unit, roundup):
    record(name, worst, bound, unit)
    assert bound is not None, "%s: measured %.9g -> bound %.9g" % (name, worst, roundup(worst))
    assert worst <= bound


# ------------------------------------------------------------------------------------ elementary functions

def test_logf():
    a, r = joined("logf", "DN")
    x, got = a.view(np.float32)[:, 0].astype(F64), r.view(np.float32)[:, 0]
    pos = x > 0
    assert np.all(got[~pos] == -np.inf)          # log(x <= 0) == -inf (1 - u with u == 1.0 lands here)
    check("logf", ulps(got[pos], np.log(x[pos])).max(), BOUNDS["logf"], "ulp", half_ulp_up)


def test_logf_special_cases():
    a, r = joined("logf", "E")
    x, got = a.view(np.float32)[:, 0], r.view(np.float32)[:, 0]
    with np.errstate(invalid="ignore"):
        assert np.all(got[x <= 0] == -np.inf)
    assert np.all(got[np.isnan(x)] == -np.inf)   # !(x > 0)
    assert np.all(got[x == 1.0] == 0.0)


def test_powr():
    a, r = joined("powr", "DN")
    f = a.view(np.float32)
    x, y, got = f[:, 0].astype(F64), f[:, 1].astype(F64), r.view(np.float32)[:, 0].astype(F64)
    exact = np.power(x, y)
    assert np.all(got[x == 0] == 0.0) and np.all(got[x == 1] == 1.0)
    # The definition cuts exp(t) off at t < -87: results below e^-87 = 1.6e-38 are 0.  Ulps are measured where the
    # exact result is at least 2^-125 = 2.4e-38, clear of the cut-off; below, the result is 0 or as close.
    big = exact >= 2.0 ** -125
    for r_, yv in zip(A.POWR_RATES, A.POWR_Y):   # the error of y * log(x) grows with y: one bound per exponent
        m = big & (f[:, 1] == yv)
        check("powr, y = %s" % ("1/%g" % r_ if r_ else "40"), ulps(got[m], exact[m]).max(), BOUNDS["powr"][r_], "ulp",
              half_ulp_up)
    assert np.all(np.abs(got[~big] - exact[~big]) <= 2.0 ** -125)
    # the bounds the project states already, on their own domains (test_oracle_literal / test_oracle_golden)
    unit = x <= 1
    ref32 = exact.astype(np.float32).astype(F64)
    worst_abs = np.abs(got[unit] - ref32[unit]).max()
    print("powr on [0, 1], all listed y: max |powr - (float)pow| = %.3g" % worst_abs)
    assert worst_abs <= 2e-7
    for yv, tol in ((np.float32(1) / np.float32(1.5), 6e-7), (np.float32(40), 2e-5)):
        m = (f[:, 1] == yv) & (x >= 1e-4) & (x <= 1) & (exact > 1e-30)
        rel = (np.abs(got[m] - exact[m]) / exact[m]).max()
        print("powr(x, %.6g), x in [1e-4, 1]: max relative error %.3g" % (yv, rel))
        assert rel < tol


def test_powr_special_cases():
    a, r = joined("powr", "E")
    f, got = a.view(np.float32), r.view(np.float32)[:, 0]
    x = f[:, 0]
    assert np.all(got[x == 0] == 0.0)                       # powr(+-0, y > 0) == 0
    assert np.all(got[x == 1] == 1.0)
    with np.errstate(invalid="ignore"):
        assert np.all(np.isnan(got[(x < 0) | np.isnan(x)]))  # powr is defined for x >= 0


def test_sincosf():
    a, r = joined("sincosf", "DN")
    x, got = a.view(np.float32)[:, 0].astype(F64), r.view(np.float32).astype(F64)
    check("sinf", np.abs(got[:, 0] - np.sin(x)).max(), BOUNDS["sinf"], "abs", pow2_up)
    check("cosf", np.abs(got[:, 1] - np.cos(x)).max(), BOUNDS["cosf"], "abs", pow2_up)
    # away from the zeros in ulps as well
    s, c = np.sin(x), np.cos(x)
    check("sinf, |sin| >= 1/2", ulps(got[:, 0], s)[np.abs(s) >= 0.5].max(), BOUNDS["sinf_ulp"], "ulp", half_ulp_up)
    check("cosf, |cos| >= 1/2", ulps(got[:, 1], c)[np.abs(c) >= 0.5].max(), BOUNDS["cosf_ulp"], "ulp", half_ulp_up)


def test_atan2f():
    a, r = joined("atan2f", "DN")
    f = a.view(np.float32).astype(F64)
    got = r.view(np.float32)[:, 0]
    exact = np.arctan2(f[:, 0], f[:, 1])
    check("atan2f", ulps(got, exact).max(), BOUNDS["atan2f"], "ulp", half_ulp_up)
    worst_abs = np.abs(got.astype(F64) - exact).max()
    print("atan2f: max absolute error %.3g" % worst_abs)
    assert worst_abs <= 5e-7                                 # the bound test_hdr_golden states


def test_atan2f_special_cases():
    a, r = joined("atan2f", "E")
    f, got = a.view(np.float32), r.view(np.float32)[:, 0]
    zero = (f[:, 0] == 0) & (f[:, 1] == 0)
    assert zero.sum() == 4 and np.all(got[zero] == 0.0)     # atan2(+-0, +-0) == 0
    # finite arguments, not both zero: within the same absolute bound of the real function, whatever the binades
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        ratio = np.abs(f[:, 0] / f[:, 1])                    # the fp32 quotient the definition forms
    fin = np.isfinite(f).all(axis=1) & ~zero & (ratio >= 2.0 ** -126) & np.isfinite(ratio)
    exact = np.arctan2(f[fin, 0].astype(F64), f[fin, 1].astype(F64))
    assert np.abs(got[fin].astype(F64) - exact).max() <= 5e-7


def test_acosf():
    a, r = joined("acosf", "DN")
    x, got = a.view(np.float32)[:, 0].astype(F64), r.view(np.float32)[:, 0]
    m = np.abs(x) <= 1
    exact = np.arccos(x[m])
    nz = exact > 0                                           # acos(1) == 0 must be exact
    assert np.all(got[m][~nz] == 0.0)
    check("acosf", ulps(got[m][nz], exact[nz]).max(), BOUNDS["acosf"], "ulp", half_ulp_up)
    worst_abs = np.abs(got[m].astype(F64) - exact).max()
    print("acosf: max absolute error %.3g" % worst_abs)
    assert worst_abs <= 5e-7


# ------------------------------------------------------------------------------------------------ vectors

def test_vectors():
    a, r = joined("normalize3", "D")
    v, got = a.view(np.float32).astype(F64), r.view(np.float32).astype(F64)
    exact = v / np.sqrt((v * v).sum(axis=1))[:, None]
    check("normalize3", np.abs(got - exact).max(), BOUNDS["normalize3"], "abs", pow2_up)
    a, r = joined("len3", "D")
    v = a.view(np.float32).astype(F64)
    check("len3", ulps(r.view(np.float32)[:, 0], np.sqrt((v * v).sum(axis=1))).max(), BOUNDS["len3"], "ulp",
          half_ulp_up)
    a, r = joined("dot3", "D")
    v = a.view(np.float32).astype(F64)
    prod = v[:, :3] * v[:, 3:]
    err = np.abs(r.view(np.float32)[:, 0].astype(F64) - prod.sum(axis=1)) / (2.0 ** -24 * np.abs(prod).sum(axis=1))
    check("dot3", err.max(), BOUNDS["dot3"], "x 2^-24 sum|a_i b_i|", half_ulp_up)


def test_vector_special_cases():
    a, r = joined("normalize3", "N")
    v, got = a.view(np.float32), r.view(np.float32)
    zero = (v == 0).all(axis=1)
    assert zero.sum() == 8 and np.all(got[zero] == 0.0)      # the zero vector stays zero
    den = (np.abs(v) < 2.0 ** -126).all(axis=1)               # dot underflows to 0: zero as well
    assert np.all(got[den] == 0.0)
    big = (np.abs(v) >= 2.0 ** 60).all(axis=1)                # dot overflows: v * (1 / inf)
    assert big.sum() == 1024 and np.all(got[big] == 0.0)
    _, r = joined("len3", "N")
    assert np.all(r.view(np.float32)[:, 0][big] == np.inf)


def test_min_max_clamp():
    """OpenCL's min / max / clamp as the spec words them: min(x, y) = y < x ? y : x, max(x, y) = x < y ? y : x,
    clamp(x, lo, hi) = min(max(x, lo), hi).  Exact, NaNs and signed zeros included."""
    with np.errstate(invalid="ignore"):
        a, r = joined("vmin", "NE")
        x, y = a.view(np.float32).T
        np.testing.assert_array_equal(r[:, 0], np.where(y < x, a[:, 1], a[:, 0]))
        a, r = joined("vmax", "NE")
        x, y = a.view(np.float32).T
        np.testing.assert_array_equal(r[:, 0], np.where(x < y, a[:, 1], a[:, 0]))
        a, r = joined("vclamp", "NE")
        x, lo, hi = a.view(np.float32).T
        mx = np.where(x < lo, a[:, 1], a[:, 0])
        np.testing.assert_array_equal(r[:, 0], np.where(hi < mx.view(np.float32), a[:, 2], mx))


def test_lerpf():
    a, r = joined("lerpf", "D")
    p, q, w = a.view(np.float32).astype(F64).T
    check("lerpf", np.abs(r.view(np.float32)[:, 0].astype(F64) - (p + w * (q - p))).max(), BOUNDS["lerpf"], "abs",
          pow2_up)


# --------------------------------------------------------------------------------------------- exact ones

def wang(v):
    """random.cl:2-13 in uint32 arithmetic"""
    v = v.astype(np.uint32)
    v = (v ^ np.uint32(61)) ^ (v >> np.uint32(16))
    v = v * np.uint32(9)
    v = v ^ (v << np.uint32(4))
    v = v * np.uint32(0x27d4eb2d)
    return v ^ (v >> np.uint32(15))


def test_hash_and_map_uint_float_are_exact():
    a, r = joined("rng", "D")
    np.testing.assert_array_equal(r[:, 0], wang(a[:, 0]))
    a, r = joined("rng3", "DN")
    np.testing.assert_array_equal(r[:, 0], wang(a[:, 2] ^ wang(a[:, 1] ^ wang(a[:, 0]))))
    a, r = joined("map_uint_float", "D")
    np.testing.assert_array_equal(r[:, 0], A.bits(A.map_uint_float(a[:, 0])))
    assert r[a[:, 0] == 0xffffffff, 0][0] == 0x3f800000       # (float)0xffffffff / 2^32 == 1.0f


# ------------------------------------------------------------------------------------------------ TF reads

def tf_linear64(tff, x):
    """OpenCL 1.2 spec 8.2, 1-D image, normalised coordinates, CLAMP_TO_EDGE, CLK_FILTER_LINEAR, in float64:
    u = x * n, i0 = floor(u - 0.5), a = frac(u - 0.5), T = (1 - a) T[i0] + a T[i0 + 1], indices clamped."""
    n = len(tff)
    t = tff.astype(F64) / 255.0
    u = x.astype(F64) * n - 0.5
    i0 = np.floor(u)
    w = (u - i0)[:, None]
    j0 = np.clip(i0, 0, n - 1).astype(np.int64)
    j1 = np.clip(i0 + 1, 0, n - 1).astype(np.int64)
    return (1.0 - w) * t[j0] + w * t[j1]


@pytest.mark.parametrize("op", ["tff_linear", "tff_linear_raw"])
def test_tff_linear(op):
    worst = {}
    for args, res, ti in collect(op, "DN"):
        tff = A.tables()[ti][0]
        err = np.abs(res.view(np.float32).astype(F64) - tf_linear64(tff, args.view(np.float32)[:, 0])).max()
        worst[len(tff)] = max(worst.get(len(tff), 0.0), err)
    for n, w in sorted(worst.items()):
        check("%s, n = %d" % (op, n), w, BOUNDS["tff_linear"][n], "abs", pow2_up)


def test_tff_alpha_is_the_fourth_channel():
    for op4, op1 in (("tff_linear", "tff_alpha"), ("tff_linear_raw", "tff_alpha_raw")):
        for (a4, r4, _), (a1, r1, _) in zip(collect(op4, "DNE"), collect(op1, "DNE")):
            np.testing.assert_array_equal(a4, a1)
            np.testing.assert_array_equal(r4[:, 3], r1[:, 0])


def test_tff_special_cases():
    """Every x <= 0 reads TF[0] and every x >= 1 reads TF[n - 1] exactly, whatever the binade; a NaN reads TF[0]."""
    for args, res, ti in collect("tff_linear_raw", "E"):
        tff = A.tables()[ti][0]
        t = (tff.astype(np.float32) / np.float32(255)).view(np.uint32)
        x = args.view(np.float32)[:, 0]
        with np.errstate(invalid="ignore"):
            lo, hi = (x <= 0) | np.isnan(x), x >= 1
        assert np.isnan(x).sum() > 600 and np.isinf(x).sum() == 2
        np.testing.assert_array_equal(res[lo], np.broadcast_to(t[0], (lo.sum(), 4)))
        np.testing.assert_array_equal(res[hi], np.broadcast_to(t[-1], (hi.sum(), 4)))


def test_prefix_nearest():
    """read_imageui(.., nearestSmp, x): prefix[floor(x n)] inside [0, n - 1], border 0 outside, against the same in
    float64.  fp32 rounds the product x * n once; where that rounding reaches a whole number that the exact product
    does not, the index is the neighbour's -- and only there."""
    for args, res, ti in collect("prefix_nearest", "DNE"):
        prefix = A.tables()[ti][1]
        n = len(prefix)
        x = args.view(np.float32)[:, 0]
        with np.errstate(invalid="ignore", over="ignore"):
            u = x.astype(F64) * n
            i = np.floor(u)
            inside = (i >= 0) & (i <= n - 1)
            exact = np.where(inside, prefix[np.where(inside, i, 0).astype(np.int64)], 0)
            u32 = (x * np.float32(n)).astype(F64)             # the product as fp32 rounds it
        diff = res[:, 0] != exact
        assert np.all(np.floor(u32[diff]) != i[diff])         # only where the rounding crossed a whole number
        assert np.all(u32[diff] == np.round(u[diff]))
        assert diff.sum() <= len(x) // 100
        with np.errstate(invalid="ignore"):
            out = np.isnan(x) | (x < 0) | (x >= 1)
        assert np.all(res[out & ~(x == 0), 0] == 0)


def test_skip_test_is_its_parts():
    """skip = TF(max).a < 1e-6 and prefix[min] == prefix[max] (volumeraycast.cl:777-787), from the reads checked above;
    both outcomes occur on every table that has more than one entry."""
    for args, res, ti in collect("skip_test", "DNE"):
        tff, prefix = A.tables()[ti]
        alpha = vro.math_batch("tff_alpha_raw", args[:, 1], tff=tff).view(np.float32)[:, 0]
        pmin = vro.math_batch("prefix_nearest", args[:, 0], tff=tff, prefix=prefix)[:, 0]
        pmax = vro.math_batch("prefix_nearest", args[:, 1], tff=tff, prefix=prefix)[:, 0]
        expect = (alpha < np.float32(1e-6)) & (pmin == pmax)
        np.testing.assert_array_equal(res[:, 0], expect.astype(np.uint32))
        if len(tff) >= 3:
            assert 0 < expect.sum() < len(expect)


def test_batch_ignores_literal_mode():
    x = A.strided(1, A.ONE, 1000)
    ref = vro.math_batch("logf", x)
    vro.lib().vro_set_literal(1)
    try:
        got = vro.math_batch("logf", x)
        assert vro.lib().vro_get_literal() == 1
    finally:
        vro.lib().vro_set_literal(0)
    np.testing.assert_array_equal(got, ref)
