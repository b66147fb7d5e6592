/*
 * preint_ref.c -- scalar CPU restatement of technique 8, ray casting with pre-integrated classification
 * (VRHIP_TECHNIQUE_PREINT, include/vrhip.h).
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_preint.hip and of vrhip_preint_slab.  One pixel at a time, every
 * sample fetched and every slab classified, transparent or not: no skipping, no prefix count, no vector code; the
 * prefix sums of whole segments are made by the header's recurrence, once per table.  Compiled by tests/preint_ref.py with the flags oracle/Makefile compiles the oracle with
 * (-ffp-contract=off) and linked to the oracle's library for its exported vro_powr.
 *
 * It restates -- it cannot call -- the oracle's ray set-up, image reads, central-difference taps and Blinn-Phong
 * terms, which are `static` in oracle/vr_oracle.c, with the same sequences of fp32 operations, and the non-ESS branch
 * of render_pixel's sample loop line for line.  tests/test_preint_ref.py pins it to the oracle: on a volume that is
 * constant along every ray (sf == sb at every slab) the oracle's technique-0 frame (ESS off) IS the frame.
 *
 * Definition: include/vrhip.h "technique == 8".  The loop: t = max(0, tnear); while (t < tfar) { sample at
 * cam + dir * (t - offset); sb = s; sf = the previous sample's s (the first: sb); c = slab(sf, sb); illumType 1 and
 * c.a > 0.1f: illumination(c.rgb, toLight, -normalize(G)); x = bg - c.rgb; opacity = 1 - powr(1 - c.a,
 * 1 / samplingRate); result -= (x * opacity) * (1 - alpha); alpha += opacity * (1 - alpha); if (t >= tfar) break;
 * if ((double)alpha > 0.98) break; t += stepSize (a step that leaves t unchanged ends the sequence) }.
 * Pixel (result.rgb, alpha); a ray that misses the clip box keeps backgroundColor, alpha included.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

typedef struct {
    float viewMat[16];
    float bbox_bl[4];
    float bbox_tr[4];
    uint32_t ortho;
    uint32_t pad[7];
} pre_camera_params; /* vrhip_camera_params */

typedef struct {
    float backgroundColor[4];
    float modelScale[4];
    uint32_t illumType, imgEss, showEss, useLinear, useGradient, technique, seed, iteration;
} pre_rendering_params; /* vrhip_rendering_params */

typedef struct {
    float samplingRate;
    uint32_t useAO, contours, aerial;
    float brickRes[4];
} pre_raycast_params; /* vrhip_raycast_params */

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;       /* 0 UCHAR, 1 USHORT, 2 FLOAT */
    const uint8_t *tff;   /* n RGBA8 entries */
    uint32_t n;
} pre_scene;

enum { PRE_MISS = 0, PRE_MARCHED = 1 };

typedef struct { float x, y, z; } f3;

static float vmin(float x, float y) { return y < x ? y : x; } /* OpenCL min */
static float vmax(float x, float y) { return x < y ? y : x; } /* OpenCL max */
static int iclamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
static f3 mk3(float x, float y, float z) { f3 r = {x, y, z}; return r; }
static float dot3(f3 a, f3 b) { return ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z); }
static float len3(f3 a) { return sqrtf(dot3(a, a)); }
static f3 mul3(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
static f3 scale3(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
static f3 add3(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static f3 neg3(f3 a) { return mk3(-a.x, -a.y, -a.z); }
static f3 normalize3(f3 v)
{
    float d = dot3(v, v);
    if (d == 0.0f) return mk3(0.0f, 0.0f, 0.0f);
    float inv = 1.0f / sqrtf(d);
    return scale3(v, inv);
}
static float lerpf(float p, float q, float w) { return fmaf(w, q - p, p); }

static uint32_t rng1(uint32_t x)
{
    uint32_t value = x;
    value = (value ^ 61u) ^ (value >> 16);
    value *= 9u;
    value ^= value << 4;
    value *= 0x27d4eb2du;
    value ^= value >> 15;
    return value;
}
static uint32_t rng3(uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t value = rng1(x);
    value = rng1(y ^ value);
    value = rng1(z ^ value);
    return value;
}

/* ---- image reads */

static float vox_raw(const pre_scene *s, int x, int y, int z)
{
    size_t i = ((size_t)z * s->res[1] + (size_t)y) * s->res[0] + (size_t)x;
    switch (s->format) {
    case 0: return (float)((const uint8_t *)s->voxels)[i];
    case 1: return (float)((const uint16_t *)s->voxels)[i];
    default: return ((const float *)s->voxels)[i];
    }
}

static float inv_max_of(const pre_scene *s)
{
    return s->format == 0 ? 1.0f / 255.0f : s->format == 1 ? 1.0f / 65535.0f : 1.0f;
}

/* normalised coordinates, CLAMP_TO_EDGE, LINEAR */
static float vol_linear(const pre_scene *s, float px, float py, float pz)
{
    int w = (int)s->res[0], h = (int)s->res[1], d = (int)s->res[2];
    float u = px * (float)w, vv = py * (float)h, ww = pz * (float)d;
    float ub = u - 0.5f, vb = vv - 0.5f, wb = ww - 0.5f;
    float fx = floorf(ub), fy = floorf(vb), fz = floorf(wb);
    float a = ub - fx, b = vb - fy, c = wb - fz;
    int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    int x0 = iclamp(ix, 0, w - 1), x1 = iclamp(ix + 1, 0, w - 1);
    int y0 = iclamp(iy, 0, h - 1), y1 = iclamp(iy + 1, 0, h - 1);
    int z0 = iclamp(iz, 0, d - 1), z1 = iclamp(iz + 1, 0, d - 1);
    float c00 = lerpf(vox_raw(s, x0, y0, z0), vox_raw(s, x1, y0, z0), a);
    float c10 = lerpf(vox_raw(s, x0, y1, z0), vox_raw(s, x1, y1, z0), a);
    float c01 = lerpf(vox_raw(s, x0, y0, z1), vox_raw(s, x1, y0, z1), a);
    float c11 = lerpf(vox_raw(s, x0, y1, z1), vox_raw(s, x1, y1, z1), a);
    float c0 = lerpf(c00, c10, b);
    float c1 = lerpf(c01, c11, b);
    return lerpf(c0, c1, c) * inv_max_of(s);
}

/* normalised coordinates, CLAMP (border 0), NEAREST */
static float vol_nearest(const pre_scene *s, float px, float py, float pz)
{
    int w = (int)s->res[0], h = (int)s->res[1], d = (int)s->res[2];
    float fx = floorf(px * (float)w), fy = floorf(py * (float)h), fz = floorf(pz * (float)d);
    if (!(fx >= 0.0f && fx <= (float)(w - 1) && fy >= 0.0f && fy <= (float)(h - 1) && fz >= 0.0f &&
          fz <= (float)(d - 1)))
        return 0.0f;
    return vox_raw(s, (int)fx, (int)fy, (int)fz) * inv_max_of(s);
}

float vro_powr(float x, float y); /* oracle/vr_oracle.c */

static f3 sub3(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }

/* trilinear blend with weights (a, b, c) of the texels (xi, yi, zi)[0..1] */
static float vol_tri(const pre_scene *s, const int xi[2], const int yi[2], const int zi[2], float a, float b, float c)
{
    float c00 = lerpf(vox_raw(s, xi[0], yi[0], zi[0]), vox_raw(s, xi[1], yi[0], zi[0]), a);
    float c10 = lerpf(vox_raw(s, xi[0], yi[1], zi[0]), vox_raw(s, xi[1], yi[1], zi[0]), a);
    float c01 = lerpf(vox_raw(s, xi[0], yi[0], zi[1]), vox_raw(s, xi[1], yi[0], zi[1]), a);
    float c11 = lerpf(vox_raw(s, xi[0], yi[1], zi[1]), vox_raw(s, xi[1], yi[1], zi[1]), a);
    float c0 = lerpf(c00, c10, b);
    float c1 = lerpf(c01, c11, b);
    return lerpf(c0, c1, c) * inv_max_of(s);
}

/* s2 - s1 of the central difference: six taps one texel from the centre sample, in texel space (the centre's filter
 * weights, indices shifted by -+1 and clamped to the edge) */
static f3 central_diff(const pre_scene *s, f3 pos)
{
    int w = (int)s->res[0], h = (int)s->res[1], d = (int)s->res[2];
    float ub = pos.x * (float)w - 0.5f, vb = pos.y * (float)h - 0.5f, wb = pos.z * (float)d - 0.5f;
    float fx = floorf(ub), fy = floorf(vb), fz = floorf(wb);
    float a = ub - fx, b = vb - fy, c = wb - fz;
    int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    int X[4], Y[4], Z[4];
    for (int k = 0; k < 4; ++k) {
        X[k] = iclamp(ix - 1 + k, 0, w - 1);
        Y[k] = iclamp(iy - 1 + k, 0, h - 1);
        Z[k] = iclamp(iz - 1 + k, 0, d - 1);
    }
    f3 s1, s2;
    s1.x = vol_tri(s, X + 0, Y + 1, Z + 1, a, b, c);
    s2.x = vol_tri(s, X + 2, Y + 1, Z + 1, a, b, c);
    s1.y = vol_tri(s, X + 1, Y + 0, Z + 1, a, b, c);
    s2.y = vol_tri(s, X + 1, Y + 2, Z + 1, a, b, c);
    s1.z = vol_tri(s, X + 1, Y + 1, Z + 0, a, b, c);
    s2.z = vol_tri(s, X + 1, Y + 1, Z + 2, a, b, c);
    return sub3(s2, s1);
}

/* ---- the slab classification (include/vrhip.h "technique == 8") */

static float coord(int raw, float x)
{
    if (!raw) return x;
    float c = x > -1.0f ? x : -1.0f; /* the other operand for a NaN */
    return c < 2.0f ? c : 2.0f;
}

/* the part [u0, u1] of segment j (end entries p, q; a tail reads one entry: w = 0) added to S = (A, M_r, M_g, M_b):
 * midpoint rule for alpha, Simpson's rule for colour x alpha, in the header's order */
static void part(const float *E, int n, int j, double u0, double u1, double S[4])
{
    const float *p = E + 4 * iclamp(j, 0, n - 1), *q = E + 4 * iclamp(j + 1, 0, n - 1);
    int tail = j < 0 || j >= n - 1;
    double h = u1 - u0;
    double w0 = tail ? 0.0 : u0 - (double)j;
    double w1 = tail ? 0.0 : u1 - (double)j;
    double wm = 0.5 * (w0 + w1);
    double v0 = 1.0 - w0, v1 = 1.0 - w1, vm = 1.0 - wm;
    double pa = p[3], qa = q[3];
    double a0 = pa * v0 + qa * w0;
    double am = pa * vm + qa * wm;
    double a1 = pa * v1 + qa * w1;
    double h6 = h * (1.0 / 6.0);
    S[0] = S[0] + h * am;
    for (int ch = 0; ch < 3; ++ch) {
        double pc = p[ch], qc = q[ch];
        double c0 = pc * v0 + qc * w0;
        double cm = pc * vm + qc * wm;
        double c1 = pc * v1 + qc * w1;
        S[ch + 1] = S[ch + 1] + h6 * ((c0 * a0 + 4.0 * (cm * am)) + c1 * a1);
    }
}

/* the header's prefix table: P[0] = 0, P[i] = P[i - 1] + the whole segment i - 1; n entries of four doubles */
static void prefix_table(const float *E, int n, double *P)
{
    P[0] = P[1] = P[2] = P[3] = 0.0;
    for (int i = 1; i < n; ++i) {
        double W[4] = {0.0, 0.0, 0.0, 0.0};
        part(E, n, i - 1, (double)(i - 1), (double)i, W);
        for (int c = 0; c < 4; ++c) P[4 * i + c] = P[4 * (i - 1) + c] + W[c];
    }
}

/* E: n entries of four floats, P: their prefix table */
static void slab(const float *E, const double *P, int n, int raw, float sf, float sb, float out[4])
{
    float ua = coord(raw, sf) * (float)n - 0.5f;
    float ub = coord(raw, sb) * (float)n - 0.5f;
    if (ua == ub) {
        float fl = floorf(ub);
        float a = ub - fl;
        int i = (int)fl;
        const float *t0 = E + 4 * iclamp(i, 0, n - 1), *t1 = E + 4 * iclamp(i + 1, 0, n - 1);
        for (int ch = 0; ch < 4; ++ch) out[ch] = lerpf(t0[ch], t1[ch], a);
        return;
    }
    float lof = ua < ub ? ua : ub, hif = ua < ub ? ub : ua;
    int jl = iclamp((int)floorf(lof), -1, n - 1), jh = iclamp((int)floorf(hif), -1, n - 1);
    double lo = lof, hi = hif;
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    if (jl == jh) {
        part(E, n, jl, lo, hi, S);
    } else {
        part(E, n, jl, lo, (double)(jl + 1), S);
        for (int c = 0; c < 4; ++c) S[c] = S[c] + (P[4 * jh + c] - P[4 * (jl + 1) + c]);
        part(E, n, jh, (double)jh, hi, S);
    }
    double r = 1.0 / (hi - lo);
    float abar = (float)(S[0] * r);
    for (int ch = 0; ch < 3; ++ch) {
        float m = (float)(S[ch + 1] * r);
        out[ch] = abar > 0.0f ? m / abar : 0.0f;
    }
    out[3] = abar;
}

/* the table as the renderer holds it: c / 255.0f */
static void entries_of(const uint8_t *rgba8, int n, float *E)
{
    for (int i = 0; i < 4 * n; ++i) E[i] = (float)rgba8[i] / 255.0f;
}

#define PRE_MAX_N 4096

/* one slab of a table of n float entries (what vrhip_preint_slab is compared with) */
int pre_slab(const float *E, uint32_t n, int raw, float sf, float sb, float out[4])
{
    static double P[4 * PRE_MAX_N];
    if (!E || !out || n < 1 || n > PRE_MAX_N) return 1;
    prefix_table(E, (int)n, P);
    slab(E, P, (int)n, raw, sf, sb, out);
    return 0;
}

/* the ray caster's transfer-function read of a table of n float entries (tff_linear) */
void pre_tff_linear(const float *E, uint32_t n_u, int raw, float x, float out[4])
{
    int n = (int)n_u;
    float ub = coord(raw, x) * (float)n - 0.5f;
    float fl = floorf(ub);
    float a = ub - fl;
    int i = (int)fl;
    const float *t0 = E + 4 * iclamp(i, 0, n - 1), *t1 = E + 4 * iclamp(i + 1, 0, n - 1);
    for (int ch = 0; ch < 4; ++ch) out[ch] = lerpf(t0[ch], t1[ch], a);
}

/* can the slab read an entry that is not transparent?  (for the counts only: the march never asks) */
static int slab_shows(const float *E, int n, int raw, float sf, float sb)
{
    float ua = coord(raw, sf) * (float)n - 0.5f, ub = coord(raw, sb) * (float)n - 0.5f;
    float lof = ua < ub ? ua : ub, hif = ua < ub ? ub : ua;
    int i0 = iclamp((int)floorf(lof), 0, n - 1), i1 = iclamp((int)floorf(hif) + 1, 0, n - 1);
    for (int i = i0; i <= i1; ++i)
        if (E[4 * i + 3] != 0.0f) return 1;
    return 0;
}

typedef struct {
    int kind;          /* PRE_* */
    uint32_t samples;  /* samples taken */
    uint32_t visible;  /* slabs with abar != 0 */
    uint32_t marginal; /* slabs that can read an entry which is not transparent */
    float *values;     /* optional: the first max_values sample values of the ray */
    float *positions;  /* optional: their positions, three texture coordinates in [0, 1] each */
    uint32_t max_values;
} pre_ray;

/* ---- one ray (out holds the background on entry) */
static int ray_march(const pre_scene *s, const float *E, const double *P, const pre_camera_params *cam, const pre_rendering_params *rp,
                     const pre_raycast_params *rc, uint32_t gsx_u, uint32_t gsy_u, uint32_t gx, uint32_t gy,
                     pre_ray *res, float out[4])
{
    const float *V = cam->viewMat;
    const f3 ms = mk3(rp->modelScale[0], rp->modelScale[1], rp->modelScale[2]);

    float rnd = (float)rng3(gx, gy, rp->seed) / 4294967296.0f;

    /* the camera is derived from the padded launch size */
    float gsx = (float)gsx_u, gsy = (float)gsy_u;
    float aspect = gsy / gsx;
    aspect = vmin(aspect, gsx / gsy);
    int maxImg = (int)(gsx_u > gsy_u ? gsx_u : gsy_u);
    float icx = ((float)(int)gx / (float)maxImg) * 2.f;
    float icy = ((float)(int)gy / (float)maxImg) * 2.f;
    if (gsx_u > gsy_u) { icx -= 1.0f; icy -= aspect; }
    else { icx -= aspect; icy -= 1.0f; }
    icy *= -1.f;
    float psx = 2.f / gsx, psy = 2.f / gsy;
    float rnd2 = (float)rng3(gy, gx, 2u * rp->seed) / 4294967296.0f;
    icx += rnd2 * psx;
    icy += (-rnd) * psy;

    f3 npp = mk3(icx, icy, -1.0f);
    f3 rayDir = mk3(dot3(mk3(V[0], V[1], V[2]), npp), dot3(mk3(V[4], V[5], V[6]), npp),
                    dot3(mk3(V[8], V[9], V[10]), npp));
    f3 camPos = mul3(mk3(V[3], V[7], V[11]), ms);
    if (cam->ortho) {
        camPos = mk3(V[3], V[7], V[11]);
        f3 vpx = mk3(V[0], V[4], V[8]);
        f3 vpy = mk3(V[1], V[5], V[9]);
        f3 vpz = mk3(V[2], V[6], V[10]);
        rayDir = neg3(vpz);
        npp = add3(add3(camPos, scale3(vpx, icx)), scale3(vpy, icy));
        npp = scale3(npp, len3(camPos));
        camPos = mul3(npp, ms);
    }
    rayDir = normalize3(mul3(rayDir, ms));

    /* clip box */
    float o[3] = {camPos.x, camPos.y, camPos.z}, d[3] = {rayDir.x, rayDir.y, rayDir.z};
    float tmin[3], tmax[3];
    for (int i = 0; i < 3; ++i) {
        float inv = 1.0f / d[i];
        float tbot = inv * (cam->bbox_bl[i] - o[i]);
        float ttop = inv * (cam->bbox_tr[i] - o[i]);
        tmin[i] = vmin(ttop, tbot);
        tmax[i] = vmax(ttop, tbot);
    }
    float tnear = vmax(vmax(tmin[0], tmin[1]), vmax(tmin[0], tmin[2]));
    float tfar = vmin(vmin(tmax[0], tmax[1]), vmin(tmax[0], tmax[2]));
    if (!(tfar > tnear) || tfar < 0) return PRE_MISS;
    float sampleDist = tfar - tnear;
    if (sampleDist <= 0.f) return PRE_MISS;

    /* step length, start, jitter offset */
    f3 resf = mk3((float)s->res[0], (float)s->res[1], (float)s->res[2]);
    float stepSize = vmin(sampleDist,
                          sampleDist / (rc->samplingRate * len3(mul3(scale3(rayDir, sampleDist), resf))));
    float samples = ceilf(sampleDist / stepSize);
    stepSize = sampleDist / samples;
    tnear = vmax(0.f, tnear);
    f3 voxLen = mk3(1.f / resf.x, 1.f / resf.y, 1.f / resf.z);
    float offset = (len3(voxLen) * rnd) * 2.0f;

    /* the sample loop: oracle/vr_oracle.c render_pixel, the non-ESS branch */
    const float env[3] = {rp->backgroundColor[0], rp->backgroundColor[1], rp->backgroundColor[2]};
    float result[3] = {env[0], env[1], env[2]};
    float alpha = 0.f;
    float t = tnear;
    const float refInterval = 1.f / rc->samplingRate;
    const f3 toLight = neg3(rayDir);
    const int raw = s->format == 2;
    float prev = 0.f;
    while (t < tfar) {
        res->samples++;
        f3 pos = add3(camPos, scale3(rayDir, t - offset));
        pos = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
        float density = rp->useLinear ? vol_linear(s, pos.x, pos.y, pos.z) : vol_nearest(s, pos.x, pos.y, pos.z);
        if (res->values && res->samples <= res->max_values) res->values[res->samples - 1] = density;
        if (res->positions && res->samples <= res->max_values) {
            res->positions[3 * (res->samples - 1) + 0] = pos.x;
            res->positions[3 * (res->samples - 1) + 1] = pos.y;
            res->positions[3 * (res->samples - 1) + 2] = pos.z;
        }
        const float sb = density, sf = res->samples == 1 ? density : prev;
        prev = density;
        float tfc[4];
        slab(E, P, (int)s->n, raw, sf, sb, tfc);
        if (tfc[3] != 0.f) res->visible++;
        if (slab_shows(E, (int)s->n, raw, sf, sb)) res->marginal++;
        if (tfc[3] > 0.1f && rp->illumType) {
            f3 G = central_diff(s, pos);
            f3 n = normalize3(G);
            if (dot3(G, G) == 0.0f) n = mk3(0.57735f, 0.57735f, 0.57735f);
            n = neg3(n);
            /* illumination(color, toLight, n) with specularBlinnPhong(n, l, toLight) */
            const f3 lgt = normalize3(toLight);
            f3 hv = add3(toLight, lgt);
            const int hvalid = !(dot3(hv, hv) < 1.e-6f);
            hv = normalize3(hv);
            const float ndl = vmax(0.f, dot3(n, lgt));
            const float spec = hvalid ? vro_powr(vmax(dot3(n, hv), 0.f), 40.f) * 0.15f : 0.0f;
            for (int i = 0; i < 3; ++i) tfc[i] = ((tfc[i] * 0.15f) + ((tfc[i] * ndl) * 0.7f)) + spec;
        }
        tfc[0] = env[0] - tfc[0];
        tfc[1] = env[1] - tfc[1];
        tfc[2] = env[2] - tfc[2];
        float opacity = 1.f - vro_powr(1.f - tfc[3], refInterval);
        float oma = 1.f - alpha;
        result[0] = result[0] - (tfc[0] * opacity) * oma;
        result[1] = result[1] - (tfc[1] * opacity) * oma;
        result[2] = result[2] - (tfc[2] * opacity) * oma;
        alpha = alpha + opacity * oma;
        if (t >= tfar) break;
        if ((double)alpha > 0.98) break;
        float tn = t + stepSize;
        if (!(tn > t)) break;
        t = tn;
    }
    out[0] = result[0]; out[1] = result[1]; out[2] = result[2];
    out[3] = alpha;
    return PRE_MARCHED;
}

/* Tile (x0, y0, w, h) of the W x H frame: rgba [h][w][4]; optionally per pixel the samples taken, the slabs with
 * abar != 0, the slabs that can read an entry which is not transparent, and the first max_values sample values and
 * positions (texture coordinates). */
int pre_render_tile(const pre_scene *s, const pre_camera_params *cam, const pre_rendering_params *rp,
                    const pre_raycast_params *rc, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w,
                    uint32_t h, float *rgba, uint8_t *kind_out, uint32_t *samples_out, uint32_t *visible_out,
                    uint32_t *marginal_out, float *values_out, float *positions_out, uint32_t max_values)
{
    static float E[4 * PRE_MAX_N];
    static double P[4 * PRE_MAX_N];
    if (!s || !s->voxels || !s->tff || !cam || !rp || !rc || !rgba) return 1;
    if (s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return 1;
    if (x0 + w > W || y0 + h > H) return 1;
    if (s->n < 1 || s->n > PRE_MAX_N || rp->illumType > 1) return 2;
    entries_of(s->tff, (int)s->n, E);
    prefix_table(E, (int)s->n, P);
    /* the padded launch size: a whole extra group of 8 when the size is a multiple of 8 already */
    const uint32_t gsx = W + (8u - W % 8u), gsy = H + (8u - H % 8u);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            pre_ray r = {PRE_MISS, 0u, 0u, 0u, values_out ? values_out + i * max_values : NULL,
                         positions_out ? positions_out + 3 * i * max_values : NULL, max_values};
            memcpy(rgba + 4 * i, rp->backgroundColor, 4 * sizeof(float));
            r.kind = ray_march(s, E, P, cam, rp, rc, gsx, gsy, x0 + x, y0 + y, &r, rgba + 4 * i);
            if (kind_out) kind_out[i] = (uint8_t)r.kind;
            if (samples_out) samples_out[i] = r.samples;
            if (visible_out) visible_out[i] = r.visible;
            if (marginal_out) marginal_out[i] = r.marginal;
        }
    return 0;
}
