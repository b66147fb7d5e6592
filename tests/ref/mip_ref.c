/*
 * mip_ref.c -- scalar CPU restatement of technique 2, maximum intensity projection
 * (VRHIP_TECHNIQUE_MIP, include/vrhip.h; DESIGN.md "Maximum intensity projection").
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_mip.hip.  One pixel at a time, every sample
 * fetched, no skipping, no vector code.  Compiled by tests/mip_ref.py with the flags oracle/Makefile
 * compiles the oracle with (-ffp-contract=off: every fp32 operation is rounded as written, an FMA
 * only where fmaf() is written).
 *
 * It restates -- it cannot call -- the oracle's ray set-up and image reads, which are `static` in
 * oracle/vr_oracle.c (render_pixel up to the sample loop, vol_linear, vol_nearest, tff_linear), with
 * the same sequences of fp32 operations.  tests/test_mip_ref.py pins it to the oracle: the
 * silhouettes of the oracle's technique-0 frames, the transfer-function read, known answers.
 *
 * Definition.
 *   Ray: technique 0's (view matrix, ortho, clip box, step length from samplingRate, start jitter
 *     from the seed) with object-order ESS off: t_0 = max(0, tnear), t_{k+1} = t_k + stepSize while
 *     t_k < tfar, sample k at cam + dir * (t_k - offset).  A step that leaves t unchanged ends the
 *     sequence (it would repeat one sample for ever, which cannot change a maximum).
 *   Value: m = max over the samples of the filtered, normalised channel-0 value, taken as
 *     `if (s > m) m = s` from m = -inf: a NaN sample never replaces it.
 *   Pixel: c = tff_linear(m); rgb = c.rgb * c.a + bg.rgb * (1 - c.a), a = c.a + bg.a * (1 - c.a),
 *     bg = backgroundColor (useGradient is ignored), one rounded operation per product and sum.
 *     A ray that misses the clip box or takes no sample: bg unchanged.
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
} mip_camera_params; /* vrhip_camera_params */

typedef struct {
    float backgroundColor[4];
    float modelScale[4];
    uint32_t illumType, imgEss, showEss, useLinear, useGradient, technique, seed, iteration;
} mip_rendering_params; /* vrhip_rendering_params */

typedef struct {
    float samplingRate;
    uint32_t useAO, contours, aerial;
    float brickRes[4];
} mip_raycast_params; /* vrhip_raycast_params */

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;      /* 0 UCHAR, 1 USHORT, 2 FLOAT */
    const uint8_t *tff;  /* RGBA8 table */
    uint32_t tff_n;
} mip_scene;

enum { MIP_MISS = 0, MIP_NO_SAMPLE = 1, MIP_SAMPLED = 2 };

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

static float vox_raw(const mip_scene *s, int x, int y, int z)
{
    size_t i = ((size_t)z * s->res[1] + (size_t)y) * s->res[0] + (size_t)x;
    switch (s->format) {
    case 0: return (float)((const uint8_t *)s->voxels)[i];
    case 1: return (float)((const uint16_t *)s->voxels)[i];
    default: return ((const float *)s->voxels)[i];
    }
}

static float inv_max_of(const mip_scene *s)
{
    return s->format == 0 ? 1.0f / 255.0f : s->format == 1 ? 1.0f / 65535.0f : 1.0f;
}

/* normalised coordinates, CLAMP_TO_EDGE, LINEAR */
static float vol_linear(const mip_scene *s, float px, float py, float pz)
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
static float vol_nearest(const mip_scene *s, float px, float py, float pz)
{
    int w = (int)s->res[0], h = (int)s->res[1], d = (int)s->res[2];
    float fx = floorf(px * (float)w), fy = floorf(py * (float)h), fz = floorf(pz * (float)d);
    if (!(fx >= 0.0f && fx <= (float)(w - 1) && fy >= 0.0f && fy <= (float)(h - 1) && fz >= 0.0f &&
          fz <= (float)(d - 1)))
        return 0.0f;
    return vox_raw(s, (int)fx, (int)fy, (int)fz) * inv_max_of(s);
}

/* the transfer-function read: x clamped to [-1, 2] (a NaN reads as -1), LINEAR, CLAMP_TO_EDGE */
static float tff_coord(float x)
{
    float c = x > -1.0f ? x : -1.0f;
    return c < 2.0f ? c : 2.0f;
}
void mip_tff_linear(const uint8_t *tff, uint32_t tff_n, float x, float out[4])
{
    int n = (int)tff_n;
    float ub = tff_coord(x) * (float)n - 0.5f;
    float fl = floorf(ub);
    float a = ub - fl;
    int i = (int)fl;
    int i0 = iclamp(i, 0, n - 1), i1 = iclamp(i + 1, 0, n - 1);
    for (int c = 0; c < 4; ++c) {
        float t0 = (float)tff[4 * (size_t)i0 + c] / 255.0f;
        float t1 = (float)tff[4 * (size_t)i1 + c] / 255.0f;
        out[c] = lerpf(t0, t1, a);
    }
}

/* ---- the pixel of a ray whose maximum is m */
void mip_pixel(const uint8_t *tff, uint32_t tff_n, float m, int sampled, const float bg[4], float out[4])
{
    if (!sampled) {
        memcpy(out, bg, 4 * sizeof(float));
        return;
    }
    float c[4];
    mip_tff_linear(tff, tff_n, m, c);
    float oma = 1.f - c[3];
    out[0] = (c[0] * c[3]) + (bg[0] * oma);
    out[1] = (c[1] * c[3]) + (bg[1] * oma);
    out[2] = (c[2] * c[3]) + (bg[2] * oma);
    out[3] = c[3] + (bg[3] * oma);
}

/* ---- one ray: its maximum and what became of it (MIP_*) */
static int ray_max(const mip_scene *s, const mip_camera_params *cam, const mip_rendering_params *rp,
                   const mip_raycast_params *rc, uint32_t gsx_u, uint32_t gsy_u, uint32_t gx, uint32_t gy,
                   float *m_out, uint32_t *n_out)
{
    const float *V = cam->viewMat;
    const f3 ms = mk3(rp->modelScale[0], rp->modelScale[1], rp->modelScale[2]);
    *m_out = -INFINITY;
    *n_out = 0;

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
    if (!(tfar > tnear) || tfar < 0) return MIP_MISS;
    float sampleDist = tfar - tnear;
    if (sampleDist <= 0.f) return MIP_MISS;

    /* step length, start, jitter offset */
    f3 resf = mk3((float)s->res[0], (float)s->res[1], (float)s->res[2]);
    float stepSize = vmin(sampleDist,
                          sampleDist / (rc->samplingRate * len3(mul3(scale3(rayDir, sampleDist), resf))));
    float samples = ceilf(sampleDist / stepSize);
    stepSize = sampleDist / samples;
    tnear = vmax(0.f, tnear);
    f3 voxLen = mk3(1.f / resf.x, 1.f / resf.y, 1.f / resf.z);
    float offset = (len3(voxLen) * rnd) * 2.0f;

    float m = -INFINITY;
    uint32_t n = 0;
    float t = tnear;
    while (t < tfar) {
        f3 pos = add3(camPos, scale3(rayDir, t - offset));
        pos = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
        float v = rp->useLinear ? vol_linear(s, pos.x, pos.y, pos.z) : vol_nearest(s, pos.x, pos.y, pos.z);
        if (v > m) m = v;
        ++n;
        float tn = t + stepSize;
        if (!(tn > t)) break;
        t = tn;
    }
    *m_out = m;
    *n_out = n;
    return n ? MIP_SAMPLED : MIP_NO_SAMPLE;
}

/* Tile (x0, y0, w, h) of the W x H frame: rgba [h][w][4]; optionally the maxima m [h][w], the ray classes
 * kind [h][w] (MIP_*) and the sample counts count [h][w]. */
int mip_render_tile(const mip_scene *s, const mip_camera_params *cam, const mip_rendering_params *rp,
                    const mip_raycast_params *rc, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w,
                    uint32_t h, float *rgba, float *m_out, uint8_t *kind_out, uint32_t *count_out)
{
    if (!s || !s->voxels || !s->tff || !s->tff_n || !cam || !rp || !rc || !rgba) return 1;
    if (s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return 1;
    if (x0 + w > W || y0 + h > H) return 1;
    /* the padded launch size: a whole extra group of 8 when the size is a multiple of 8 already */
    const uint32_t gsx = W + (8u - W % 8u), gsy = H + (8u - H % 8u);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            float m;
            uint32_t n;
            const int kind = ray_max(s, cam, rp, rc, gsx, gsy, x0 + x, y0 + y, &m, &n);
            const size_t i = (size_t)y * w + x;
            mip_pixel(s->tff, s->tff_n, m, kind == MIP_SAMPLED, rp->backgroundColor, rgba + 4 * i);
            if (m_out) m_out[i] = m;
            if (kind_out) kind_out[i] = (uint8_t)kind;
            if (count_out) count_out[i] = n;
        }
    return 0;
}
