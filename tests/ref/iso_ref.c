/*
 * iso_ref.c -- scalar CPU restatement of technique 4, first-hit isosurface rendering
 * (VRHIP_TECHNIQUE_ISO, include/vrhip.h; DESIGN.md "First-hit isosurface").
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_iso.hip.  One pixel at a time, every march sample
 * fetched, no skipping, no vector code.  Compiled by tests/iso_ref.py with the flags oracle/Makefile
 * compiles the oracle with (-ffp-contract=off: every fp32 operation is rounded as written, an FMA
 * only where fmaf() is written) and linked to the oracle's library for its exported vro_powr and
 * vro_tff_linear.
 *
 * It restates -- it cannot call -- the oracle's ray set-up, image reads, central-difference gradient
 * and Blinn-Phong terms, which are `static` in oracle/vr_oracle.c (render_pixel up to the sample
 * loop, vol_linear, vol_nearest, neg_gradient_central_diff, illumination), with the same sequences
 * of fp32 operations.  tests/test_iso_ref.py pins it to the oracle: on a binary volume with an
 * opaque transfer function the oracle's technique-0 frame IS the first-hit frame.
 *
 * Definition.
 *   Ray: technique 0's (view matrix, ortho, clip box, step length from samplingRate, start jitter
 *     from the seed) with object-order ESS off: t_0 = max(0, tnear), t_{k+1} = t_k + stepSize while
 *     t_k < tfar, sample k at cam + dir * (t_k - offset).  A step that leaves t unchanged ends the
 *     sequence.
 *   Hit: the first k whose filtered, normalised channel-0 value s_k satisfies s_k >= isoValue (a NaN
 *     sample never does).  k = 0 is a hit like any other: the clip box caps the solid.
 *   Refinement (skipped when k = 0 or refineSteps = 0): ta = t_{k-1}, tb = t_k; refineSteps times
 *     tm = (ta + tb) * 0.5f, s = fetch(tm), s >= isoValue ? tb = tm : ta = tm.  t_hit = tb.
 *   Pixel: c = tff_linear(isoValue); illumType 0: rgb = c.rgb; illumType 1: g = neg_gradient at the
 *     hit position, ndl = max(0, g . lgt), spec = hvalid ? powr(max(g . hv, 0), 40) * 0.15 : 0,
 *     rgb = ((c * 0.15) + ((c * ndl) * 0.7)) + spec per channel; a = 1.
 *     A ray that misses the clip box or finds no hit: backgroundColor unchanged, alpha included.
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
} iso_camera_params; /* vrhip_camera_params */

typedef struct {
    float backgroundColor[4];
    float modelScale[4];
    uint32_t illumType, imgEss, showEss, useLinear, useGradient, technique, seed, iteration;
} iso_rendering_params; /* vrhip_rendering_params */

typedef struct {
    float samplingRate;
    uint32_t useAO, contours, aerial;
    float brickRes[4];
} iso_raycast_params; /* vrhip_raycast_params */

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;      /* 0 UCHAR, 1 USHORT, 2 FLOAT */
    const uint8_t *tff;  /* RGBA8 table */
    uint32_t tff_n;
} iso_scene;

enum { ISO_MISS = 0, ISO_NO_HIT = 1, ISO_HIT = 2 };

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

static float vox_raw(const iso_scene *s, int x, int y, int z)
{
    size_t i = ((size_t)z * s->res[1] + (size_t)y) * s->res[0] + (size_t)x;
    switch (s->format) {
    case 0: return (float)((const uint8_t *)s->voxels)[i];
    case 1: return (float)((const uint16_t *)s->voxels)[i];
    default: return ((const float *)s->voxels)[i];
    }
}

static float inv_max_of(const iso_scene *s)
{
    return s->format == 0 ? 1.0f / 255.0f : s->format == 1 ? 1.0f / 65535.0f : 1.0f;
}

/* normalised coordinates, CLAMP_TO_EDGE, LINEAR */
static float vol_linear(const iso_scene *s, float px, float py, float pz)
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
static float vol_nearest(const iso_scene *s, float px, float py, float pz)
{
    int w = (int)s->res[0], h = (int)s->res[1], d = (int)s->res[2];
    float fx = floorf(px * (float)w), fy = floorf(py * (float)h), fz = floorf(pz * (float)d);
    if (!(fx >= 0.0f && fx <= (float)(w - 1) && fy >= 0.0f && fy <= (float)(h - 1) && fz >= 0.0f &&
          fz <= (float)(d - 1)))
        return 0.0f;
    return vox_raw(s, (int)fx, (int)fy, (int)fz) * inv_max_of(s);
}


float vro_powr(float x, float y);                                                  /* oracle/vr_oracle.c */
void vro_tff_linear(const uint8_t *tff_rgba, uint32_t n, float x, float out[4]);   /* oracle/vr_oracle.c */

typedef struct {
    float isoValue;
    uint32_t refineSteps;
    uint32_t reserved[2];
} iso_params; /* vrhip_iso_params */

static f3 sub3(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }

/* trilinear blend with weights (a, b, c) of the texels (xi, yi, zi)[0..1] */
static float vol_tri(const iso_scene *s, const int xi[2], const int yi[2], const int zi[2], float a, float b, float c)
{
    float c00 = lerpf(vox_raw(s, xi[0], yi[0], zi[0]), vox_raw(s, xi[1], yi[0], zi[0]), a);
    float c10 = lerpf(vox_raw(s, xi[0], yi[1], zi[0]), vox_raw(s, xi[1], yi[1], zi[0]), a);
    float c01 = lerpf(vox_raw(s, xi[0], yi[0], zi[1]), vox_raw(s, xi[1], yi[0], zi[1]), a);
    float c11 = lerpf(vox_raw(s, xi[0], yi[1], zi[1]), vox_raw(s, xi[1], yi[1], zi[1]), a);
    float c0 = lerpf(c00, c10, b);
    float c1 = lerpf(c01, c11, b);
    return lerpf(c0, c1, c) * inv_max_of(s);
}

/* the negated central-difference gradient, normalised: six taps one texel from the centre sample, in texel
 * space (the centre's filter weights, indices shifted by -+1 and clamped to the edge) */
static f3 neg_gradient(const iso_scene *s, f3 pos)
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
    f3 g = sub3(s2, s1);
    f3 n = normalize3(g);
    if (dot3(g, g) == 0.0f) n = mk3(0.57735f, 0.57735f, 0.57735f);
    return neg3(n);
}

static float fetch(const iso_scene *s, const iso_rendering_params *rp, f3 camPos, f3 rayDir, float t, float offset, f3 *pos_out)
{
    f3 pos = add3(camPos, scale3(rayDir, t - offset));
    pos = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
    if (pos_out) *pos_out = pos;
    return rp->useLinear ? vol_linear(s, pos.x, pos.y, pos.z) : vol_nearest(s, pos.x, pos.y, pos.z);
}

typedef struct {
    int kind;        /* ISO_* */
    uint32_t k;      /* hit: index of the first sample at or above isoValue */
    float t_hit;     /* hit: ray parameter after refinement */
    uint32_t count;  /* march samples fetched: k + 1 for a hit, all of them otherwise */
} iso_ray;

/* ---- one ray: march, refinement, pixel (out holds the background on entry) */
static int ray_march(const iso_scene *s, const iso_camera_params *cam, const iso_rendering_params *rp,
                     const iso_raycast_params *rc, const iso_params *ip, uint32_t gsx_u, uint32_t gsy_u,
                     uint32_t gx, uint32_t gy, iso_ray *res, float out[4])
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
    if (!(tfar > tnear) || tfar < 0) return ISO_MISS;
    float sampleDist = tfar - tnear;
    if (sampleDist <= 0.f) return ISO_MISS;

    /* step length, start, jitter offset */
    f3 resf = mk3((float)s->res[0], (float)s->res[1], (float)s->res[2]);
    float stepSize = vmin(sampleDist,
                          sampleDist / (rc->samplingRate * len3(mul3(scale3(rayDir, sampleDist), resf))));
    float samples = ceilf(sampleDist / stepSize);
    stepSize = sampleDist / samples;
    tnear = vmax(0.f, tnear);
    f3 voxLen = mk3(1.f / resf.x, 1.f / resf.y, 1.f / resf.z);
    float offset = (len3(voxLen) * rnd) * 2.0f;


    /* march: the first sample at or above isoValue */
    const float iso = ip->isoValue;
    float t = tnear, t_prev = tnear;
    uint32_t k = 0;
    int hit = 0;
    while (t < tfar) {
        float v = fetch(s, rp, camPos, rayDir, t, offset, NULL);
        res->count = k + 1;
        if (v >= iso) { hit = 1; break; }
        float tn = t + stepSize;
        if (!(tn > t)) break;
        t_prev = t;
        t = tn;
        ++k;
    }
    if (!hit) return ISO_NO_HIT;

    /* refinement */
    float tb = t;
    if (k != 0) {
        float ta = t_prev;
        for (uint32_t i = 0; i < ip->refineSteps; ++i) {
            float tm = (ta + tb) * 0.5f;
            float v = fetch(s, rp, camPos, rayDir, tm, offset, NULL);
            if (v >= iso) tb = tm; else ta = tm;
        }
    }
    res->k = k;
    res->t_hit = tb;

    /* pixel */
    float c[4];
    vro_tff_linear(s->tff, s->tff_n, iso, c);
    if (rp->illumType == 1) {
        f3 pos;
        (void)fetch(s, rp, camPos, rayDir, tb, offset, &pos);
        const f3 toLight = neg3(rayDir);
        const f3 lgt = normalize3(toLight);
        f3 hv = add3(toLight, lgt);
        const int hvalid = !(dot3(hv, hv) < 1.e-6f);
        hv = normalize3(hv);
        const f3 g = neg_gradient(s, pos);
        const float ndl = vmax(0.f, dot3(g, lgt));
        const float spec = hvalid ? vro_powr(vmax(dot3(g, hv), 0.f), 40.f) * 0.15f : 0.0f;
        for (int i = 0; i < 3; ++i) c[i] = ((c[i] * 0.15f) + ((c[i] * ndl) * 0.7f)) + spec;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    out[3] = 1.0f;
    return ISO_HIT;
}

/* ---- one ray: what became of it, and its pixel */
static iso_ray ray_pixel(const iso_scene *s, const iso_camera_params *cam, const iso_rendering_params *rp,
                         const iso_raycast_params *rc, const iso_params *ip, uint32_t gsx_u, uint32_t gsy_u,
                         uint32_t gx, uint32_t gy, float out[4])
{
    iso_ray res = {ISO_MISS, 0u, 0.f, 0u};
    memcpy(out, rp->backgroundColor, 4 * sizeof(float));
    res.kind = ray_march(s, cam, rp, rc, ip, gsx_u, gsy_u, gx, gy, &res, out);
    return res;
}

/* Tile (x0, y0, w, h) of the W x H frame: rgba [h][w][4]; optionally the ray classes kind [h][w] (ISO_*), the hit
 * indices k [h][w], the refined hit parameters t_hit [h][w] and the march sample counts count [h][w]. */
int iso_render_tile(const iso_scene *s, const iso_camera_params *cam, const iso_rendering_params *rp,
                    const iso_raycast_params *rc, const iso_params *ip, uint32_t W, uint32_t H, uint32_t x0,
                    uint32_t y0, uint32_t w, uint32_t h, float *rgba, uint8_t *kind_out, uint32_t *k_out,
                    float *t_out, uint32_t *count_out)
{
    if (!s || !s->voxels || !s->tff || !s->tff_n || !cam || !rp || !rc || !ip || !rgba) return 1;
    if (s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return 1;
    if (x0 + w > W || y0 + h > H) return 1;
    if (rp->illumType > 1 || ip->refineSteps > 16 || !isfinite(ip->isoValue)) return 2;
    /* the padded launch size: a whole extra group of 8 when the size is a multiple of 8 already */
    const uint32_t gsx = W + (8u - W % 8u), gsy = H + (8u - H % 8u);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            const iso_ray r = ray_pixel(s, cam, rp, rc, ip, gsx, gsy, x0 + x, y0 + y, rgba + 4 * i);
            if (kind_out) kind_out[i] = (uint8_t)r.kind;
            if (k_out) k_out[i] = r.k;
            if (t_out) t_out[i] = r.t_hit;
            if (count_out) count_out[i] = r.count;
        }
    return 0;
}
