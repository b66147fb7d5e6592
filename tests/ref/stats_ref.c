/*
 * stats_ref.c -- scalar CPU restatement of the volume statistics (vrhip_volume_statistics, include/vrhip.h "volume
 * statistics").
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_stats.hip.  Written as the contract reads: one voxel at a time from a
 * dense x-fastest array -- no staging, no cells, no skipping, no private tables.  Compiled by tests/stats_ref.py with
 * the flags oracle/Makefile compiles the oracle with (-ffp-contract=off: every operation is rounded as written).
 *
 * Definition: the header's.  s = (float)raw * inv_max; nan / below / above / value bin i with k_v computed once;
 * the central difference with the neighbour's coordinate clamped to the volume, m = 0.5f * sqrtf((gx gx + gy gy) +
 * gz gz), a NaN m to gradient_nan, else bin j with k_g computed once; hist[j * bins_v + i] += 1.
 * Moments, in the contract's order: blocks of 8^3 voxels anchored at (0,0,0); lane x + 8 y adds its column z = 0..7
 * ascending from 0.0; v += v[lane ^ k] for k = 1, 2, 4, 8, 16, 32 over the 64 lanes; the block sums of the call's
 * block grid (x fastest) from 0.0 in ascending order within chunks of STATS_SUM_CHUNK blocks; the chunk sums from 0.0
 * in ascending order.  min / max by < and >, a zero reported as +0.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct {
    const void *voxels;    /* dense, x fastest */
    uint32_t res[3];
    int32_t format;        /* 0 UCHAR, 1 USHORT, 2 FLOAT */
} stats_scene;

typedef struct {
    uint32_t lo[3], hi[3];
    uint32_t bins_v, bins_g;
    float v_lo, v_hi, g_hi;
    uint32_t flags;
    uint32_t reserved[4];
} stats_params; /* vrhip_stats_params */

typedef struct {
    uint64_t voxels, nan, below, above, gradient_nan, binned;
    float min, max;
    double sum, sum_sq;
} volume_stats; /* vrhip_volume_stats */

#define STATS_MOMENTS 1u
#define STATS_BLOCK 8u
#define STATS_SUM_CHUNK 256u

static float value_at(const stats_scene *sc, uint32_t x, uint32_t y, uint32_t z)
{
    const size_t i = ((size_t)z * sc->res[1] + y) * sc->res[0] + x;
    if (sc->format == 0) return (float)((const uint8_t *)sc->voxels)[i] * (1.0f / 255.0f);
    if (sc->format == 1) return (float)((const uint16_t *)sc->voxels)[i] * (1.0f / 65535.0f);
    return ((const float *)sc->voxels)[i] * 1.0f;
}

static uint32_t step(uint32_t c, int d, uint32_t res)   /* c + d clamped to the volume */
{
    if (d < 0) return c == 0 ? 0 : c - 1;
    return c + 1 >= res ? res - 1 : c + 1;
}

/* 0: done; -1: the arguments are refused (the header's VRHIP_ERR_INVALID cases) */
int stats_compute(const stats_scene *sc, const stats_params *p, volume_stats *out, uint64_t *hist)
{
    if (!sc || !p || !out || !hist) return -1;
    if (p->bins_v < 1 || p->bins_v > 4096 || p->bins_g < 1 || p->bins_g > 256 || (uint64_t)p->bins_v * p->bins_g > 65536) return -1;
    if (!isfinite(p->v_lo) || !isfinite(p->v_hi) || !(p->v_hi > p->v_lo)) return -1;
    const float span = p->v_hi - p->v_lo;
    const float k_v = (float)p->bins_v / span;
    if (!isfinite(span) || !isfinite(k_v)) return -1;
    float k_g = 0.f;
    if (p->bins_g > 1) {
        if (!isfinite(p->g_hi) || !(p->g_hi > 0.f)) return -1;
        k_g = (float)p->bins_g / p->g_hi;
        if (!isfinite(k_g)) return -1;
    }
    if ((p->flags & ~STATS_MOMENTS) || p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) return -1;
    uint32_t lo[3], hi[3];
    const int whole = !(p->lo[0] | p->lo[1] | p->lo[2] | p->hi[0] | p->hi[1] | p->hi[2]);
    int voxels = 1;
    for (int a = 0; a < 3; ++a) {
        lo[a] = whole ? 0 : p->lo[a];
        hi[a] = whole ? sc->res[a] : p->hi[a];
        if (hi[a] == 0 || hi[a] > sc->res[a] || lo[a] > hi[a]) return -1;
        if (hi[a] == lo[a]) voxels = 0;
    }
    const int moments = (p->flags & STATS_MOMENTS) != 0;
    memset(out, 0, sizeof *out);
    memset(hist, 0, (size_t)p->bins_v * p->bins_g * sizeof(uint64_t));
    if (moments) {
        out->min = INFINITY;
        out->max = -INFINITY;
    }
    if (!voxels) return 0;

    uint32_t b0[3], nb[3];
    for (int a = 0; a < 3; ++a) {
        b0[a] = lo[a] / STATS_BLOCK;
        nb[a] = (hi[a] - 1u) / STATS_BLOCK - b0[a] + 1u;
    }
    double total = 0.0, total_sq = 0.0, chunk = 0.0, chunk_sq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    uint64_t in_chunk = 0;
    for (uint32_t bz = 0; bz < nb[2]; ++bz)
        for (uint32_t by = 0; by < nb[1]; ++by)
            for (uint32_t bx = 0; bx < nb[0]; ++bx) {
                double lane[64], lane_sq[64];
                for (uint32_t ly = 0; ly < 8; ++ly)
                    for (uint32_t lx = 0; lx < 8; ++lx) {
                        double sum = 0.0, sum_sq = 0.0;
                        for (uint32_t lz = 0; lz < 8; ++lz) {
                            const uint32_t x = (b0[0] + bx) * 8 + lx, y = (b0[1] + by) * 8 + ly, z = (b0[2] + bz) * 8 + lz;
                            if (x < lo[0] || x >= hi[0] || y < lo[1] || y >= hi[1] || z < lo[2] || z >= hi[2]) continue;
                            ++out->voxels;
                            const float s = value_at(sc, x, y, z);
                            if (s != s) { ++out->nan; continue; }
                            if (moments) {
                                if (s < mn) mn = s;
                                if (s > mx) mx = s;
                                const double d = (double)s;
                                sum = sum + d;
                                sum_sq = sum_sq + d * d;
                            }
                            if (s < p->v_lo) { ++out->below; continue; }
                            if (s > p->v_hi) { ++out->above; continue; }
                            const float u = (s - p->v_lo) * k_v;
                            const uint32_t i = u >= (float)p->bins_v ? p->bins_v - 1u : (uint32_t)u;
                            uint32_t j = 0;
                            if (p->bins_g > 1) {
                                const float gx = value_at(sc, step(x, 1, sc->res[0]), y, z) - value_at(sc, step(x, -1, sc->res[0]), y, z);
                                const float gy = value_at(sc, x, step(y, 1, sc->res[1]), z) - value_at(sc, x, step(y, -1, sc->res[1]), z);
                                const float gz = value_at(sc, x, y, step(z, 1, sc->res[2])) - value_at(sc, x, y, step(z, -1, sc->res[2]));
                                const float m = 0.5f * sqrtf((gx * gx + gy * gy) + gz * gz);
                                if (m != m) { ++out->gradient_nan; continue; }
                                const float w = m * k_g;
                                j = w >= (float)p->bins_g ? p->bins_g - 1u : (uint32_t)w;
                            }
                            ++hist[(size_t)j * p->bins_v + i];
                            ++out->binned;
                        }
                        lane[lx + 8 * ly] = sum;
                        lane_sq[lx + 8 * ly] = sum_sq;
                    }
                if (!moments) continue;
                for (uint32_t k = 1; k < 64; k <<= 1) {   /* v += v[lane ^ k], every lane at once */
                    double t[64], t_sq[64];
                    for (uint32_t l = 0; l < 64; ++l) {
                        t[l] = lane[l] + lane[l ^ k];
                        t_sq[l] = lane_sq[l] + lane_sq[l ^ k];
                    }
                    memcpy(lane, t, sizeof t);
                    memcpy(lane_sq, t_sq, sizeof t_sq);
                }
                chunk = chunk + lane[0];
                chunk_sq = chunk_sq + lane_sq[0];
                if (++in_chunk == STATS_SUM_CHUNK) {
                    total = total + chunk;
                    total_sq = total_sq + chunk_sq;
                    chunk = chunk_sq = 0.0;
                    in_chunk = 0;
                }
            }
    if (moments) {
        if (in_chunk) {
            total = total + chunk;
            total_sq = total_sq + chunk_sq;
        }
        out->min = mn == 0.f ? 0.f : mn;
        out->max = mx == 0.f ? 0.f : mx;
        out->sum = total;
        out->sum_sq = total_sq;
    }
    return 0;
}
