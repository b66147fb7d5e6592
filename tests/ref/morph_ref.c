/* morph_ref.c -- scalar CPU restatement of the volume morphology (vrhip_morph_volume, include/vrhip.h "volume
 * morphology").  TEST INFRASTRUCTURE ONLY: compiled by tests/morph_ref.py with the oracle's CFLAGS (no fp contraction).
 * Straight from the definition: per voxel a loop over the structuring element B with clamped positions (or, for the
 * test that pins the two forms against each other, over the positions that lie inside the volume); a two-sweep op
 * literally runs its two sweeps through a stored intermediate. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_RADIUS 8
#define SIDE (2 * MAX_RADIUS + 1)
enum { FMT_UCHAR = 0, FMT_USHORT = 1, FMT_FLOAT = 2 };
enum { OP_ERODE = 0, OP_DILATE, OP_OPEN, OP_CLOSE, OP_GRADIENT, OP_TOPHAT, OP_BLACKHAT };
enum { SHAPE_BOX = 0, SHAPE_BALL = 1 };

typedef struct {
    const void *voxels; /* dense, x fastest */
    uint32_t res[3];
    int32_t format;
} morph_scene;

typedef struct {
    uint32_t op, shape;
    uint32_t radius[3];
    uint32_t reserved[3];
} morph_params;

static int params_ok(const morph_params *p)
{
    if (!p || p->op > OP_BLACKHAT || p->shape > SHAPE_BALL) return 0;
    for (int a = 0; a < 3; ++a)
        if (p->radius[a] > MAX_RADIUS) return 0;
    return !(p->reserved[0] | p->reserved[1] | p->reserved[2]);
}

/* is (dx, dy, dz) an offset of B? */
static int in_element(uint32_t shape, const uint32_t R[3], int dx, int dy, int dz)
{
    if (abs(dx) > (int)R[0] || abs(dy) > (int)R[1] || abs(dz) > (int)R[2]) return 0;
    if (shape == SHAPE_BOX) return 1;
    const long rx = R[0] > 1 ? (long)R[0] : 1, ry = R[1] > 1 ? (long)R[1] : 1, rz = R[2] > 1 ? (long)R[2] : 1;
    const long lhs = (long)dx * dx * ry * ry * rz * rz + (long)dy * dy * rx * rx * rz * rz + (long)dz * dz * rx * rx * ry * ry;
    return lhs <= rx * rx * ry * ry * rz * rz;
}

/* the offsets of B as (dx, dy, dz) triples, z, then y, then x ascending; returns their number, writes at most cap */
uint32_t morph_element(const morph_params *p, int8_t *out, uint32_t cap)
{
    if (!params_ok(p)) return 0;
    uint32_t n = 0;
    for (int dz = -MAX_RADIUS; dz <= MAX_RADIUS; ++dz)
        for (int dy = -MAX_RADIUS; dy <= MAX_RADIUS; ++dy)
            for (int dx = -MAX_RADIUS; dx <= MAX_RADIUS; ++dx)
                if (in_element(p->shape, p->radius, dx, dy, dz)) {
                    if (out && n < cap) {
                        out[3 * n] = (int8_t)dx;
                        out[3 * n + 1] = (int8_t)dy;
                        out[3 * n + 2] = (int8_t)dz;
                    }
                    ++n;
                }
    return n;
}

/* the order-preserving key of a FLOAT word: every NaN the largest */
static uint32_t float_key(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u);
}
/* ... and the word stored for a key: a NaN as 0x7fc00000, -0 as +0 */
static uint32_t float_unkey(uint32_t key)
{
    if (key == 0xffffffffu) return 0x7fc00000u;
    const uint32_t bits = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    return bits == 0x80000000u ? 0u : bits;
}

static uint32_t key_at(const void *v, int format, size_t i)
{
    if (format == FMT_UCHAR) return ((const uint8_t *)v)[i];
    if (format == FMT_USHORT) return ((const uint16_t *)v)[i];
    return float_key(((const uint32_t *)v)[i]);
}

static void store_key(void *v, int format, size_t i, uint32_t key)
{
    if (format == FMT_UCHAR) ((uint8_t *)v)[i] = (uint8_t)key;
    else if (format == FMT_USHORT) ((uint16_t *)v)[i] = (uint16_t)key;
    else ((uint32_t *)v)[i] = float_unkey(key);
}

static long clampl(long v, long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

/* erosion (is_max 0) or dilation (1) of `in` into `out`, both dense volumes of `format`.  inside 0: over the clamped
 * positions clamp(p + o); 1: over the positions p + o that lie inside the volume. */
static void extreme(const void *in, void *out, const uint32_t res[3], int format, uint32_t shape, const uint32_t R[3],
                    int is_max, int inside)
{
    static uint8_t member[SIDE][SIDE][SIDE];
    for (int dz = -MAX_RADIUS; dz <= MAX_RADIUS; ++dz)
        for (int dy = -MAX_RADIUS; dy <= MAX_RADIUS; ++dy)
            for (int dx = -MAX_RADIUS; dx <= MAX_RADIUS; ++dx)
                member[dz + MAX_RADIUS][dy + MAX_RADIUS][dx + MAX_RADIUS] = (uint8_t)in_element(shape, R, dx, dy, dz);
    const long W = res[0], H = res[1], D = res[2];
    for (long z = 0; z < D; ++z)
        for (long y = 0; y < H; ++y)
            for (long x = 0; x < W; ++x) {
                uint32_t best = is_max ? 0u : 0xffffffffu;
                for (int dz = -(int)R[2]; dz <= (int)R[2]; ++dz) {
                    if (inside && (z + dz < 0 || z + dz >= D)) continue;
                    const long qz = clampl(z + dz, D - 1);
                    for (int dy = -(int)R[1]; dy <= (int)R[1]; ++dy) {
                        if (inside && (y + dy < 0 || y + dy >= H)) continue;
                        const long qy = clampl(y + dy, H - 1);
                        const uint8_t *m = member[dz + MAX_RADIUS][dy + MAX_RADIUS] + MAX_RADIUS;
                        const size_t line = ((size_t)qz * (size_t)H + (size_t)qy) * (size_t)W;
                        for (int dx = -(int)R[0]; dx <= (int)R[0]; ++dx) {
                            if (!m[dx]) continue;
                            if (inside && (x + dx < 0 || x + dx >= W)) continue;
                            const uint32_t k = key_at(in, format, line + (size_t)clampl(x + dx, W - 1));
                            if (is_max ? k > best : k < best) best = k;
                        }
                    }
                }
                store_key(out, format, ((size_t)z * (size_t)H + (size_t)y) * (size_t)W + (size_t)x, best);
            }
}

/* out = a - b by the contract's store */
static void difference(const void *a, const void *b, void *out, int format, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        if (format == FMT_UCHAR) ((uint8_t *)out)[i] = (uint8_t)(((const uint8_t *)a)[i] - ((const uint8_t *)b)[i]);
        else if (format == FMT_USHORT) ((uint16_t *)out)[i] = (uint16_t)(((const uint16_t *)a)[i] - ((const uint16_t *)b)[i]);
        else {
            float fa, fb;
            memcpy(&fa, (const uint32_t *)a + i, 4);
            memcpy(&fb, (const uint32_t *)b + i, 4);
            const float c = fa - fb;
            uint32_t bits;
            memcpy(&bits, &c, 4);
            if (c != c) bits = 0x7fc00000u;
            else if (c == 0.0f) bits = 0u;
            ((uint32_t *)out)[i] = bits;
        }
    }
}

/* the whole op into out (a dense volume like the scene's); inside: see extreme().  0, or -1 for refused arguments */
int morph_compute(const morph_scene *sc, const morph_params *p, void *out, int inside)
{
    if (!sc || !sc->voxels || !out || !params_ok(p)) return -1;
    if (sc->format < FMT_UCHAR || sc->format > FMT_FLOAT || !sc->res[0] || !sc->res[1] || !sc->res[2]) return -1;
    const size_t n = (size_t)sc->res[0] * sc->res[1] * sc->res[2];
    const size_t bytes = n * (sc->format == FMT_UCHAR ? 1u : sc->format == FMT_USHORT ? 2u : 4u);
    void *t = malloc(bytes), *u = malloc(bytes);
    if (!t || !u) {
        free(t);
        free(u);
        return -1;
    }
    const void *f = sc->voxels;
    const uint32_t *res = sc->res, *R = p->radius;
    const int fmt = sc->format;
    switch (p->op) {
    case OP_ERODE: extreme(f, out, res, fmt, p->shape, R, 0, inside); break;
    case OP_DILATE: extreme(f, out, res, fmt, p->shape, R, 1, inside); break;
    case OP_OPEN:
        extreme(f, t, res, fmt, p->shape, R, 0, inside);
        extreme(t, out, res, fmt, p->shape, R, 1, inside);
        break;
    case OP_CLOSE:
        extreme(f, t, res, fmt, p->shape, R, 1, inside);
        extreme(t, out, res, fmt, p->shape, R, 0, inside);
        break;
    case OP_GRADIENT:
        extreme(f, t, res, fmt, p->shape, R, 1, inside);
        extreme(f, u, res, fmt, p->shape, R, 0, inside);
        difference(t, u, out, fmt, n);
        break;
    case OP_TOPHAT:
        extreme(f, t, res, fmt, p->shape, R, 0, inside);
        extreme(t, u, res, fmt, p->shape, R, 1, inside);
        difference(f, u, out, fmt, n);
        break;
    default: /* OP_BLACKHAT */
        extreme(f, t, res, fmt, p->shape, R, 1, inside);
        extreme(t, u, res, fmt, p->shape, R, 0, inside);
        difference(u, f, out, fmt, n);
        break;
    }
    free(t);
    free(u);
    return 0;
}
