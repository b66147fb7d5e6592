/* filter_ref.c -- scalar CPU restatement of the volume filters (vrhip_filter_volume, include/vrhip.h "volume
 * filters").  TEST INFRASTRUCTURE ONLY: compiled by tests/filter_ref.py with the oracle's CFLAGS (no fp contraction).
 * It literally runs the three full-field passes on fp32 fields of the volume's size; every operation is a statement
 * of its own, in the header's order. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_RADIUS 8
enum { FMT_UCHAR = 0, FMT_USHORT = 1, FMT_FLOAT = 2 };
enum { KIND_SEPARABLE = 0, KIND_MEDIAN3 = 1 };

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;
} filter_scene;

typedef struct {
    uint32_t kind;
    uint32_t radius[3];
    float taps[3][MAX_RADIUS + 1];
    uint32_t reserved[4];
} filter_params;

static size_t clampi(long v, long hi) { return (size_t)(v < 0 ? 0 : v > hi ? hi : v); }

static float value_of(const filter_scene *sc, size_t i)
{
    if (sc->format == FMT_UCHAR) {
        const float raw = (float)((const uint8_t *)sc->voxels)[i];
        const float inv = 1.0f / 255.0f;
        return raw * inv;
    }
    if (sc->format == FMT_USHORT) {
        const float raw = (float)((const uint16_t *)sc->voxels)[i];
        const float inv = 1.0f / 65535.0f;
        return raw * inv;
    }
    return ((const float *)sc->voxels)[i];
}

/* one full-field pass along `axis` */
static void pass(const float *in, float *out, const uint32_t res[3], int axis, uint32_t R, const float *w)
{
    const size_t stride[3] = {1, res[0], (size_t)res[0] * res[1]};
    for (uint32_t z = 0; z < res[2]; ++z)
        for (uint32_t y = 0; y < res[1]; ++y)
            for (uint32_t x = 0; x < res[0]; ++x) {
                const uint32_t p[3] = {x, y, z};
                const size_t at = ((size_t)z * res[1] + y) * res[0] + x;
                const size_t base = at - p[axis] * stride[axis];
                float acc = w[0] * in[at];
                for (uint32_t k = 1; k <= R; ++k) {
                    const float lo = in[base + clampi((long)p[axis] - (long)k, (long)res[axis] - 1) * stride[axis]];
                    const float hi = in[base + clampi((long)p[axis] + (long)k, (long)res[axis] - 1) * stride[axis]];
                    const float pair = lo + hi;
                    const float term = w[k] * pair;
                    acc = acc + term;
                }
                out[at] = acc;
            }
}

static uint32_t key_of_bits(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u;
}

static uint32_t bits_of_key(uint32_t key)
{
    uint32_t bits;
    if (key == 0xffffffffu) return 0x7fc00000u;
    bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    return bits == 0x80000000u ? 0u : bits;
}

static int cmp_u32(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

static void store_separable(const filter_scene *sc, void *dst, size_t i, float c)
{
    if (sc->format == FMT_FLOAT) {
        uint32_t bits;
        memcpy(&bits, &c, 4);
        if (c != c) bits = 0x7fc00000u;
        else if (c == 0.f) bits = 0u;
        ((uint32_t *)dst)[i] = bits;
    } else {
        const float mx = sc->format == FMT_UCHAR ? 255.f : 65535.f;
        float q = c * mx;
        q = q > 0.f ? q : 0.f;
        q = q < mx ? q : mx;
        q = rintf(q);
        if (sc->format == FMT_UCHAR) ((uint8_t *)dst)[i] = (uint8_t)(uint32_t)q;
        else ((uint16_t *)dst)[i] = (uint16_t)(uint32_t)q;
    }
}

/* dst: dense, x fastest, the scene's type.  0, or -1 for arguments the entry point refuses */
int filter_compute(const filter_scene *sc, const filter_params *p, void *dst)
{
    const uint32_t *res = sc->res;
    const size_t n = (size_t)res[0] * res[1] * res[2];
    if (!n || sc->format < FMT_UCHAR || sc->format > FMT_FLOAT) return -1;
    if (p->kind != KIND_SEPARABLE && p->kind != KIND_MEDIAN3) return -1;
    for (int a = 0; a < 3; ++a) {
        if (p->radius[a] > MAX_RADIUS || (p->kind == KIND_MEDIAN3 && p->radius[a])) return -1;
        if (p->kind == KIND_SEPARABLE)
            for (uint32_t k = 0; k <= p->radius[a]; ++k)
                if (!isfinite(p->taps[a][k])) return -1;
    }
    if (p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]) return -1;

    if (p->kind == KIND_MEDIAN3) {
        for (uint32_t z = 0; z < res[2]; ++z)
            for (uint32_t y = 0; y < res[1]; ++y)
                for (uint32_t x = 0; x < res[0]; ++x) {
                    uint32_t v[27];
                    int m = 0;
                    for (long dz = -1; dz <= 1; ++dz)
                        for (long dy = -1; dy <= 1; ++dy)
                            for (long dx = -1; dx <= 1; ++dx) {
                                const size_t i = (clampi((long)z + dz, (long)res[2] - 1) * res[1] +
                                                  clampi((long)y + dy, (long)res[1] - 1)) * res[0] +
                                                 clampi((long)x + dx, (long)res[0] - 1);
                                if (sc->format == FMT_UCHAR) v[m++] = ((const uint8_t *)sc->voxels)[i];
                                else if (sc->format == FMT_USHORT) v[m++] = ((const uint16_t *)sc->voxels)[i];
                                else v[m++] = key_of_bits(((const uint32_t *)sc->voxels)[i]);
                            }
                    qsort(v, 27, sizeof v[0], cmp_u32);
                    const size_t at = ((size_t)z * res[1] + y) * res[0] + x;
                    if (sc->format == FMT_UCHAR) ((uint8_t *)dst)[at] = (uint8_t)v[13];
                    else if (sc->format == FMT_USHORT) ((uint16_t *)dst)[at] = (uint16_t)v[13];
                    else ((uint32_t *)dst)[at] = bits_of_key(v[13]);
                }
        return 0;
    }

    float *f0 = (float *)malloc(n * sizeof(float)), *f1 = (float *)malloc(n * sizeof(float));
    if (!f0 || !f1) {
        free(f0);
        free(f1);
        return -1;
    }
    for (size_t i = 0; i < n; ++i) f0[i] = value_of(sc, i);
    pass(f0, f1, res, 0, p->radius[0], p->taps[0]); /* A */
    pass(f1, f0, res, 1, p->radius[1], p->taps[1]); /* B */
    pass(f0, f1, res, 2, p->radius[2], p->taps[2]); /* C */
    for (size_t i = 0; i < n; ++i) store_separable(sc, dst, i, f1[i]);
    free(f0);
    free(f1);
    return 0;
}

/* vrhip_filter_gaussian_taps, restated */
int filter_gaussian_taps(double sigma, uint32_t radius, float *taps)
{
    double t[MAX_RADIUS + 1], tail = 0.0, sum;
    if (!taps || !isfinite(sigma) || !(sigma > 0.0) || radius > MAX_RADIUS) return -1;
    for (uint32_t k = 0; k <= radius; ++k) t[k] = exp(-((double)k * (double)k) / (2.0 * sigma * sigma));
    for (uint32_t k = 1; k <= radius; ++k) tail = tail + t[k];
    sum = t[0] + 2.0 * tail;
    for (uint32_t k = 0; k <= MAX_RADIUS; ++k) taps[k] = k <= radius ? (float)(t[k] / sum) : 0.f;
    return 0;
}
