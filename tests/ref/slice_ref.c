/*
 * slice_ref.c -- scalar CPU restatement of the slice views (vrhip_render_slices, include/vrhip.h "slice views";
 * DESIGN.md 5.9).
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_slice.hip.  One pixel and one sample at a time, no vector code, no
 * unrolling.  Compiled by tests/slice_ref.py with the flags oracle/Makefile compiles the oracle with
 * (-ffp-contract=off: every fp32 operation is rounded as written, an FMA only where fmaf() is written).
 *
 * The image reads (volume fetch, transfer function) and the pixel stage are mip_ref.c's, with the same sequences of
 * fp32 operations; tests/test_slice_ref.py pins them -- the transfer-function read to the oracle's, the pixel stage
 * to mip_ref.c's, the fetch to known answers and to a float64 evaluation of OpenCL's linear filter -- before the
 * kernel is held to this file.
 *
 * Definition.  All fp32, one rounded operation each, in the order written.
 *   Pixel (gx, gy) of a W x H image, row 0 at the top:
 *     sx = (2.f * ((float)gx + 0.5f)) / (float)W - 1.f,  sy = 1.f - (2.f * ((float)gy + 0.5f)) / (float)H,
 *     p = (origin + sx * u) + sy * v per component.
 *   Samples k = 0 .. N-1: a = ((float)k + 0.5f) / (float)N - 0.5f, q = p + a * w, tex = q * 0.5f + 0.5f.  Taken when
 *     0 <= tex <= 1 on all three axes (a NaN fails).  s = linear ? vol_linear(tex) : vol_nearest(tex).
 *   Reduction over the taken samples in order of k: MAX `if (s > m) m = s` from -inf, MIN `if (s < m) m = s` from
 *     +inf, MEAN sum = sum + s from 0, then sum / (float)count.
 *   Pixel: none taken: bg.  TF: c = tff_linear(val); rgb = c.rgb * c.a + bg.rgb * (1 - c.a), a = c.a + bg.a * (1 - c.a).
 *     VALUE: (val, val, val, 1); a NaN val is written as the quiet NaN 0x7fc00000 (neither its sign nor its payload
 *     is defined by the arithmetic that produced it).
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

typedef struct {
    float origin[4], u[4], v[4], w[4];
    uint32_t samples, mode, output, reserved;
} slice_params; /* vrhip_slice_params */

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;      /* 0 UCHAR, 1 USHORT, 2 FLOAT */
    const uint8_t *tff;  /* RGBA8 table, or NULL (VALUE output only) */
    uint32_t tff_n;
} slice_scene;

enum { SLICE_MAX = 0, SLICE_MIN = 1, SLICE_MEAN = 2 };
enum { SLICE_TF = 0, SLICE_VALUE = 1 };

static int iclamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
static float lerpf(float p, float q, float w) { return fmaf(w, q - p, p); }

/* ---- image reads */

static float vox_raw(const slice_scene *s, int x, int y, int z)
{
    size_t i = ((size_t)z * s->res[1] + (size_t)y) * s->res[0] + (size_t)x;
    switch (s->format) {
    case 0: return (float)((const uint8_t *)s->voxels)[i];
    case 1: return (float)((const uint16_t *)s->voxels)[i];
    default: return ((const float *)s->voxels)[i];
    }
}

static float inv_max_of(const slice_scene *s)
{
    return s->format == 0 ? 1.0f / 255.0f : s->format == 1 ? 1.0f / 65535.0f : 1.0f;
}

/* normalised coordinates, CLAMP_TO_EDGE, LINEAR */
static float vol_linear(const slice_scene *s, float px, float py, float pz)
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
static float vol_nearest(const slice_scene *s, float px, float py, float pz)
{
    int w = (int)s->res[0], h = (int)s->res[1], d = (int)s->res[2];
    float fx = floorf(px * (float)w), fy = floorf(py * (float)h), fz = floorf(pz * (float)d);
    if (!(fx >= 0.0f && fx <= (float)(w - 1) && fy >= 0.0f && fy <= (float)(h - 1) && fz >= 0.0f &&
          fz <= (float)(d - 1)))
        return 0.0f;
    return vox_raw(s, (int)fx, (int)fy, (int)fz) * inv_max_of(s);
}

/* the fetch at texture coordinates (px, py, pz), for the tests that pin it */
float slice_fetch(const slice_scene *s, int linear, float px, float py, float pz)
{
    return linear ? vol_linear(s, px, py, pz) : vol_nearest(s, px, py, pz);
}

/* the transfer-function read: x clamped to [-1, 2] (a NaN reads as -1), LINEAR, CLAMP_TO_EDGE */
static float tff_coord(float x)
{
    float c = x > -1.0f ? x : -1.0f;
    return c < 2.0f ? c : 2.0f;
}
void slice_tff_linear(const uint8_t *tff, uint32_t tff_n, float x, float out[4])
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

/* ---- the pixel of a reduced value: taken = a sample was taken */
void slice_pixel(const uint8_t *tff, uint32_t tff_n, float val, int taken, uint32_t output, const float bg[4], float out[4])
{
    if (!taken) {
        memcpy(out, bg, 4 * sizeof(float));
        return;
    }
    if (output == SLICE_VALUE) {
        if (val != val) {
            const uint32_t qnan = 0x7fc00000u;
            memcpy(&val, &qnan, sizeof val);
        }
        out[0] = out[1] = out[2] = val;
        out[3] = 1.f;
        return;
    }
    float c[4];
    slice_tff_linear(tff, tff_n, val, c);
    float oma = 1.f - c[3];
    out[0] = (c[0] * c[3]) + (bg[0] * oma);
    out[1] = (c[1] * c[3]) + (bg[1] * oma);
    out[2] = (c[2] * c[3]) + (bg[2] * oma);
    out[3] = c[3] + (bg[3] * oma);
}

/* ---- the reduced value of the slab through p: returns the number of samples taken */
static uint32_t slab_value(const slice_scene *s, const slice_params *sp, int linear, const float p[3], float *val)
{
    const uint32_t n = sp->samples;
    float m = sp->mode == SLICE_MAX ? -INFINITY : sp->mode == SLICE_MIN ? INFINITY : 0.f;
    uint32_t count = 0;
    for (uint32_t k = 0; k < n; ++k) {
        float a = ((float)k + 0.5f) / (float)n - 0.5f;
        float tex[3];
        int taken = 1;
        for (int c = 0; c < 3; ++c) {
            float q = p[c] + a * sp->w[c];
            tex[c] = q * 0.5f + 0.5f;
            if (!(tex[c] >= 0.f && tex[c] <= 1.f)) taken = 0;
        }
        if (!taken) continue;
        float v = slice_fetch(s, linear, tex[0], tex[1], tex[2]);
        if (sp->mode == SLICE_MAX) { if (v > m) m = v; }
        else if (sp->mode == SLICE_MIN) { if (v < m) m = v; }
        else m = m + v;
        ++count;
    }
    if (sp->mode == SLICE_MEAN && count) m = m / (float)count;
    *val = m;
    return count;
}

/* Tile (x0, y0, w, h) of the W x H image of one slice: rgba [h][w][4]; optionally the reduced values val [h][w] and
 * the numbers of samples taken count [h][w]. */
int slice_render_tile(const slice_scene *s, const slice_params *sp, int linear, const float bg[4], uint32_t W, uint32_t H,
                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float *rgba, float *val_out, uint32_t *count_out)
{
    if (!s || !s->voxels || !sp || !bg || !rgba) return 1;
    if (s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return 1;
    if (!sp->samples || sp->samples > 256u || sp->mode > 2u || sp->output > 1u || sp->reserved) return 1;
    if (sp->output == SLICE_TF && (!s->tff || !s->tff_n)) return 1;
    if (!W || !H || x0 + w > W || y0 + h > H) return 1;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t gx = x0 + x, gy = y0 + y;
            float sx = (2.f * ((float)gx + 0.5f)) / (float)W - 1.f;
            float sy = 1.f - (2.f * ((float)gy + 0.5f)) / (float)H;
            float p[3];
            for (int c = 0; c < 3; ++c) p[c] = (sp->origin[c] + sx * sp->u[c]) + sy * sp->v[c];
            float val;
            const uint32_t count = slab_value(s, sp, linear, p, &val);
            const size_t i = (size_t)y * w + x;
            slice_pixel(s->tff, s->tff_n, val, count != 0, sp->output, bg, rgba + 4 * i);
            if (val_out) val_out[i] = val;
            if (count_out) count_out[i] = count;
        }
    return 0;
}
