// vr_preint_math.h -- the slab classification of technique 8 (VRHIP_TECHNIQUE_PREINT, include/vrhip.h
// "technique == 8"), written once for the host (vrhip_preint_api.hip: the table build and
// vrhip_preint_slab) and for the device (vr_preint.hip).  Plain C++: no HIP header, no library call -- compiler
// builtins only -- so that a C++ compiler builds it for the stand-alone sanitizer program as well.  Both builds run
// without contraction (-ffp-contract=off): every line below is one rounded operation per operator, an fma only where
// __builtin_fmaf is written.  tests/ref/preint_ref.c restates these lines in C and is compared bit for bit.
//
// Coordinates.  u is tff_linear's table coordinate ub = tff_coord(x) * (float)n - 0.5f, so that entry i sits at u = i.
// c(u) is linear on every segment j = [j, j + 1], 0 <= j <= n - 2, between the entries j and j + 1, and constant on
// the two tails: segment -1 = (-inf, 0] reads entry 0, segment n - 1 = [n - 1, +inf) reads entry n - 1.  So segment j
// has the end entries p = E[clamp(j, 0, n - 1)] and q = E[clamp(j + 1, 0, n - 1)]: tff_linear's i0 and i1.
//
// A part [u0, u1] of one segment, local coordinates w = u - j (exact in double: u is a widened float below 2^14, j an
// integer) and v = 1 - w, on a tail w = 0 and v = 1 (the value is p itself), h = u1 - u0, wm = 0.5 * (w0 + w1):
//   a(w) = p.a * v + q.a * w,  c(w) = p.c * v + q.c * w        (convex: products of non-negative numbers)
//   A    = h * a(wm)                                            (the midpoint rule, exact for a linear integrand)
//   M_c  = (h * (1.0 / 6.0)) * ((c(w0) * a(w0) + 4.0 * (c(wm) * a(wm))) + c(w1) * a(w1))
//                                                               (Simpson's rule, exact for a quadratic integrand)
// The prefix table: P[0] = 0, P[i] = P[i - 1] + the part [i - 1, i] of segment i - 1, four doubles (A, M_r, M_g, M_b)
// per entry, i < n.
//
// A slab with ua != ub (fp32 compare of the two table coordinates), lo = min, hi = max, jl = clamp((int)floorf(lo), -1,
// n - 1), jh likewise:
//   jl == jh:  S = part(jl, lo, hi)                             -- the closed form alone, never a difference of
//                                                                  prefix values for an interval inside a segment
//   else:      S = (part(jl, lo, jl + 1) + (P[jh] - P[jl + 1])) + part(jh, jh, hi)
//   r = 1.0 / (hi - lo);  abar = (float)(S.A * r);  m_c = (float)(S.M_c * r);  Cbar_c = abar > 0 ? m_c / abar : 0
// (the last division in fp32).  ua == ub: the colour is tff_linear's, operation for operation.
//
// Exact zero.  Every term is a sum of products of non-negative numbers (entries in [0, 1], w and v in [0, 1], h >= 0),
// and P is non-decreasing.  When the entries clamp(jl, 0, n - 1) .. clamp(jh + 1, 0, n - 1) all have alpha 0, a(w) is
// 0 * v + 0 * w = +0, both parts' A are h * +0 = +0, the whole segments between them added +0 to P so that
// P[jh].A - P[jl + 1].A = x - x = +0, and abar = (float)(+0 * r) = +0 exactly; Cbar = 0 by the rule above.  The
// kernel's skipping rests on this.
#ifndef VR_PREINT_MATH_H
#define VR_PREINT_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define VR_PREINT_FN __host__ __device__ inline
#else
#define VR_PREINT_FN inline
#endif

namespace preint {

VR_PREINT_FN int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// tff_coord (vr_sampling.h): RAW values outside [-1, 2] read what -1 or 2 reads, a NaN reads -1
VR_PREINT_FN float coord(bool raw, float x)
{
    if (!raw) return x;
    const float c = x > -1.0f ? x : -1.0f;
    return c < 2.0f ? c : 2.0f;
}

// tff_linear's table coordinate
VR_PREINT_FN float table_coord(bool raw, float x, int n) { return coord(raw, x) * (float)n - 0.5f; }

// The table entries a slab between the table coordinates ua and ub can read: i0 of the smaller, i1 of the larger
// (tff_linear's index arithmetic; monotone in the coordinate).
VR_PREINT_FN void columns(float ua, float ub, int n, int *i0, int *i1)
{
    const float lo = ua < ub ? ua : ub, hi = ua < ub ? ub : ua;
    *i0 = clampi((int)__builtin_floorf(lo), 0, n - 1);
    *i1 = clampi((int)__builtin_floorf(hi) + 1, 0, n - 1);
}

// adds the part [u0, u1] of segment j to S = (A, M_r, M_g, M_b); tff: n entries of four floats
VR_PREINT_FN void add_part(const float *tff, int n, int j, double u0, double u1, double S[4])
{
    const float *p = tff + 4 * clampi(j, 0, n - 1), *q = tff + 4 * clampi(j + 1, 0, n - 1);
    const bool tail = j < 0 || j >= n - 1;
    const double h = u1 - u0;
    const double w0 = tail ? 0.0 : u0 - (double)j, w1 = tail ? 0.0 : u1 - (double)j, wm = 0.5 * (w0 + w1);
    const double v0 = 1.0 - w0, v1 = 1.0 - w1, vm = 1.0 - wm;
    const double pa = (double)p[3], qa = (double)q[3];
    const double a0 = pa * v0 + qa * w0, am = pa * vm + qa * wm, a1 = pa * v1 + qa * w1;
    const double h6 = h * (1.0 / 6.0);
    S[0] = S[0] + h * am;
    for (int ch = 0; ch < 3; ++ch) {
        const double pc = (double)p[ch], qc = (double)q[ch];
        const double c0 = pc * v0 + qc * w0, cm = pc * vm + qc * wm, c1 = pc * v1 + qc * w1;
        S[ch + 1] = S[ch + 1] + h6 * ((c0 * a0 + 4.0 * (cm * am)) + c1 * a1);
    }
}

// the prefix table P (n entries of four doubles) and nz (n + 1 words: nz[i] = the number of entries i' < i with
// alpha != 0, so that the entries i0..i1 are all transparent <=> nz[i1 + 1] == nz[i0])
VR_PREINT_FN void build_tables(const float *tff, int n, double *P, uint32_t *nz)
{
    P[0] = P[1] = P[2] = P[3] = 0.0;
    for (int i = 1; i < n; ++i) {
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        add_part(tff, n, i - 1, (double)(i - 1), (double)i, S);
        for (int c = 0; c < 4; ++c) P[4 * i + c] = P[4 * (i - 1) + c] + S[c];
    }
    nz[0] = 0u;
    for (int i = 0; i < n; ++i) nz[i + 1] = nz[i] + (tff[4 * i + 3] != 0.0f ? 1u : 0u);
}

// The slab between the table coordinates ua (front, s_{k-1}) and ub (back, s_k): out = (Cbar.rgb, abar).
VR_PREINT_FN void slab(const float *tff, const double *P, int n, float ua, float ub, float out[4])
{
    if (ua == ub) {   // tff_linear(sb), operation for operation
        const float fl = __builtin_floorf(ub);
        const float a = ub - fl;
        const int i = (int)fl;
        const float *t0 = tff + 4 * clampi(i, 0, n - 1), *t1 = tff + 4 * clampi(i + 1, 0, n - 1);
        for (int ch = 0; ch < 4; ++ch) out[ch] = __builtin_fmaf(a, t1[ch] - t0[ch], t0[ch]);
        return;
    }
    const float lof = ua < ub ? ua : ub, hif = ua < ub ? ub : ua;
    const int jl = clampi((int)__builtin_floorf(lof), -1, n - 1), jh = clampi((int)__builtin_floorf(hif), -1, n - 1);
    const double lo = (double)lof, hi = (double)hif;
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    if (jl == jh) {
        add_part(tff, n, jl, lo, hi, S);
    } else {
        add_part(tff, n, jl, lo, (double)(jl + 1), S);
        const double *Ph = P + 4 * jh, *Pl = P + 4 * (jl + 1);
        for (int c = 0; c < 4; ++c) S[c] = S[c] + (Ph[c] - Pl[c]);
        add_part(tff, n, jh, (double)jh, hi, S);
    }
    const double r = 1.0 / (hi - lo);
    const float abar = (float)(S[0] * r);
    for (int ch = 0; ch < 3; ++ch) {
        const float m = (float)(S[ch + 1] * r);
        out[ch] = abar > 0.0f ? m / abar : 0.0f;
    }
    out[3] = abar;
}

} // namespace preint

#endif
