/*
 * depth_ref.c -- scalar CPU restatement of the depth images (vrhip_render_depth, include/vrhip.h "depth images and
 * picking").
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_depth.hip.  One pixel at a time, every sample fetched, no skipping,
 * no vector code.  Compiled by tests/depth_ref.py with the flags oracle/Makefile compiles the oracle with
 * (-ffp-contract=off: every fp32 operation is rounded as written, an FMA only where fmaf() is written) and linked to
 * the oracle's library for its exported vro_powr and vro_tff_linear.
 *
 * The ray set-up and the image reads are those of tests/ref/iso_ref.c and tests/ref/mip_ref.c, operation for
 * operation (they restate what is `static` in oracle/vr_oracle.c); tests/test_depth_ref.py pins this file to both of
 * them and to the oracle's technique-0 alpha channel.
 *
 * Definition.
 *   Ray: technique 0's (view matrix, ortho, clip box, step length from samplingRate, start jitter from the seed) with
 *     object-order ESS off: t_0 = max(0, tnear), t_{k+1} = t_k + stepSize while t_k < tfar, sample k at
 *     cam + dir * (t_k - offset), value s_k = the filtered, normalised channel-0 value.  A step that leaves t unchanged
 *     ends the sequence.
 *   ISO: the first k with s_k >= threshold (a NaN never does); unless k = 0, refineSteps times tm = (ta + tb) * 0.5f,
 *     s = fetch(tm), s >= threshold ? tb = tm : ta = tm from ta = t_{k-1}, tb = t_k; t = tb; aux = the value of the
 *     fetch that last answered >= threshold.
 *   MAX: m = -inf; s_k > m ? (m = s_k, t = t_k); a hit when some sample replaced m; aux = m.
 *   OPACITY: c = tff_linear(s_k); opacity = 1.f - powr(1.f - c.a, 1.f / samplingRate);
 *     alpha = alpha + opacity * (1.f - alpha) from 0; the first k with alpha >= threshold after its update, t = t_k;
 *     aux = alpha where the ray stopped.
 *   xyzt: hit: d = t - offset, (cam.x + dir.x * d, cam.y + dir.y * d, cam.z + dir.z * d, t); else (0, 0, 0, +inf).
 *   aux of a MISS in any mode and of a NO_HIT in ISO: 0.
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
} depth_camera_params; /* vrhip_camera_params */

typedef struct {
    float backgroundColor[4];
    float modelScale[4];
    uint32_t illumType, imgEss, showEss, useLinear, useGradient, technique, seed, iteration;
} depth_rendering_params; /* vrhip_rendering_params */

typedef struct {
    float samplingRate;
    uint32_t useAO, contours, aerial;
    float brickRes[4];
} depth_raycast_params; /* vrhip_raycast_params */

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;      /* 0 UCHAR, 1 USHORT, 2 FLOAT */
    const uint8_t *tff;  /* RGBA8 table */
    uint32_t tff_n;
} depth_scene;

enum { DEPTH_ISO = 0, DEPTH_MAX = 1, DEPTH_OPACITY = 2 };   /* mode */
enum { DEPTH_MISS = 0, DEPTH_NO_HIT = 1, DEPTH_HIT = 2 };    /* kind */

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

static float vox_raw(const depth_scene *s, int x, int y, int z)
{
    size_t i = ((size_t)z * s->res[1] + (size_t)y) * s->res[0] + (size_t)x;
    switch (s->format) {
    case 0: return (float)((const uint8_t *)s->voxels)[i];
    case 1: return (float)((const uint16_t *)s->voxels)[i];
    default: return ((const float *)s->voxels)[i];
    }
}

static float inv_max_of(const depth_scene *s)
{
    return s->format == 0 ? 1.0f / 255.0f : s->format == 1 ? 1.0f / 65535.0f : 1.0f;
}

/* normalised coordinates, CLAMP_TO_EDGE, LINEAR */
static float vol_linear(const depth_scene *s, float px, float py, float pz)
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
static float vol_nearest(const depth_scene *s, float px, float py, float pz)
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
    uint32_t mode;
    float threshold;
    uint32_t refineSteps;
    uint32_t x0, y0, w, h;
    uint32_t reserved;
} depth_params; /* vrhip_depth_params */

static float fetch(const depth_scene *s, const depth_rendering_params *rp, f3 camPos, f3 rayDir, float t, float offset)
{
    f3 pos = add3(camPos, scale3(rayDir, t - offset));
    pos = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
    return rp->useLinear ? vol_linear(s, pos.x, pos.y, pos.z) : vol_nearest(s, pos.x, pos.y, pos.z);
}

typedef struct {
    float cam[3], dir[3];   /* of a ray that enters the box */
    float tnear, tfar, stepSize, offset;
} depth_ray; /* 40 bytes */

/* ---- one ray: kind; xyzt and aux hold the MISS answer on entry */
static int ray_depth(const depth_scene *s, const depth_camera_params *cam, const depth_rendering_params *rp,
                     const depth_raycast_params *rc, const depth_params *dp, uint32_t gsx_u, uint32_t gsy_u,
                     uint32_t gx, uint32_t gy, float xyzt[4], float *aux, depth_ray *ray)
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
    if (!(tfar > tnear) || tfar < 0) return DEPTH_MISS;
    float sampleDist = tfar - tnear;
    if (sampleDist <= 0.f) return DEPTH_MISS;

    /* step length, start, jitter offset */
    f3 resf = mk3((float)s->res[0], (float)s->res[1], (float)s->res[2]);
    float stepSize = vmin(sampleDist,
                          sampleDist / (rc->samplingRate * len3(mul3(scale3(rayDir, sampleDist), resf))));
    float samples = ceilf(sampleDist / stepSize);
    stepSize = sampleDist / samples;
    tnear = vmax(0.f, tnear);
    f3 voxLen = mk3(1.f / resf.x, 1.f / resf.y, 1.f / resf.z);
    float offset = (len3(voxLen) * rnd) * 2.0f;
    if (ray) {
        ray->cam[0] = camPos.x; ray->cam[1] = camPos.y; ray->cam[2] = camPos.z;
        ray->dir[0] = rayDir.x; ray->dir[1] = rayDir.y; ray->dir[2] = rayDir.z;
        ray->tnear = tnear; ray->tfar = tfar; ray->stepSize = stepSize; ray->offset = offset;
    }

    const float thr = dp->threshold;
    int hit = 0;
    float t_hit = 0.f;
    float t = tnear;
    if (dp->mode == DEPTH_MAX) {
        float m = -INFINITY;
        while (t < tfar) {
            float v = fetch(s, rp, camPos, rayDir, t, offset);
            if (v > m) { m = v; t_hit = t; hit = 1; }
            float tn = t + stepSize;
            if (!(tn > t)) break;
            t = tn;
        }
        *aux = m;
    } else if (dp->mode == DEPTH_ISO) {
        float t_prev = tnear, val = 0.f;
        uint32_t k = 0;
        while (t < tfar) {
            float v = fetch(s, rp, camPos, rayDir, t, offset);
            if (v >= thr) { hit = 1; val = v; break; }
            float tn = t + stepSize;
            if (!(tn > t)) break;
            t_prev = t;
            t = tn;
            ++k;
        }
        float tb = t;
        if (hit && k != 0) {
            float ta = t_prev;
            for (uint32_t i = 0; i < dp->refineSteps; ++i) {
                float tm = (ta + tb) * 0.5f;
                float v = fetch(s, rp, camPos, rayDir, tm, offset);
                if (v >= thr) { tb = tm; val = v; } else ta = tm;
            }
        }
        t_hit = tb;
        *aux = hit ? val : 0.f;
    } else {
        const float refInterval = 1.f / rc->samplingRate;
        float alpha = 0.f;
        while (t < tfar) {
            float v = fetch(s, rp, camPos, rayDir, t, offset);
            float c[4];
            vro_tff_linear(s->tff, s->tff_n, v, c);
            float opacity = 1.f - vro_powr(1.f - c[3], refInterval);
            alpha = alpha + opacity * (1.f - alpha);
            if (alpha >= thr) { hit = 1; t_hit = t; break; }
            float tn = t + stepSize;
            if (!(tn > t)) break;
            t = tn;
        }
        *aux = alpha;
    }
    if (!hit) return DEPTH_NO_HIT;
    const float dist = t_hit - offset;
    xyzt[0] = camPos.x + rayDir.x * dist;
    xyzt[1] = camPos.y + rayDir.y * dist;
    xyzt[2] = camPos.z + rayDir.z * dist;
    xyzt[3] = t_hit;
    return DEPTH_HIT;
}

/* The rectangle dp->(x0, y0, w, h) -- w == h == 0: the whole frame -- of the W x H frame: xyzt [h][w][4], aux [h][w],
 * kind [h][w]; optionally the rays [h][w] (unchanged for a MISS). */
int depth_render(const depth_scene *s, const depth_camera_params *cam, const depth_rendering_params *rp,
                 const depth_raycast_params *rc, const depth_params *dp, uint32_t W, uint32_t H, float *xyzt, float *aux,
                 uint8_t *kind, depth_ray *rays)
{
    if (!s || !s->voxels || !cam || !rp || !rc || !dp || !xyzt || !aux || !kind) return 1;
    if (s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return 1;
    if (dp->mode > DEPTH_OPACITY || dp->reserved) return 2;
    if (dp->mode != DEPTH_MAX && !isfinite(dp->threshold)) return 2;
    if (dp->mode == DEPTH_ISO && dp->refineSteps > 16) return 2;
    if (dp->mode == DEPTH_OPACITY && (!s->tff || !s->tff_n)) return 3;
    uint32_t x0 = dp->x0, y0 = dp->y0, w = dp->w, h = dp->h;
    if (w == 0 && h == 0) { w = W; h = H; if (x0 || y0) return 2; }
    if (!w || !h || x0 >= W || w > W - x0 || y0 >= H || h > H - y0) return 2;
    /* the padded launch size: a whole extra group of 8 when the size is a multiple of 8 already */
    const uint32_t gsx = W + (8u - W % 8u), gsy = H + (8u - H % 8u);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            float *o = xyzt + 4 * i;
            o[0] = o[1] = o[2] = 0.f;
            o[3] = INFINITY;
            aux[i] = 0.f;
            kind[i] = (uint8_t)ray_depth(s, cam, rp, rc, dp, gsx, gsy, x0 + x, y0 + y, o, aux + i, rays ? rays + i : NULL);
        }
    return 0;
}
