/*
 * mesh_ref.c -- scalar CPU restatement of the isosurface extraction (vrhip_isosurface_count / _extract,
 * include/vrhip.h "isosurface extraction").
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of vr_mesh.hip.  Written as the contract reads: a triple loop over blocks,
 * cubes and tetrahedra, one triangle at a time, appended to a list -- no counts, no prefix sum, no skipping, no
 * vector code.  Compiled by tests/mesh_ref.py with the flags oracle/Makefile compiles the oracle with
 * (-ffp-contract=off: every fp32 operation is rounded as written, an FMA only where fmaf() is written).
 *
 * The image reads and the gradient's taps are tests/ref/iso_ref.c's own functions (vox_raw, inv_max_of, vol_tri,
 * normalize3 ...): that file is included here, so technique 4's restatement and this one cannot drift apart.  (It
 * brings its references to the oracle's library along, so this library is linked to it like that one.)
 *
 * Definition: the header's.  Grid point value s = (float)raw * inv_max, inside when s >= isoValue; six Kuhn
 * tetrahedra per cube; triangles by the table below; edge vertex t = (iso - sP) / (sQ - sP) clamped to [0, 1] with
 * !(t >= 0) -> 0, g = (float)P + (float)(Q - P) * t, coordinate (g + 0.5f) / (float)res * 2.f - 1.f; normal: the six
 * taps of technique 4's gradient at the vertex's texture coordinate, -g / |g|, (0, 0, 0) for a zero or non-finite one.
 */
#include "iso_ref.c"

typedef struct {
    float isoValue;
    uint32_t normals;
    uint32_t lo[3], hi[3];
    uint32_t reserved[4];
} mesh_params; /* vrhip_mesh_params */

#define MESH_BLOCK 8u

/* cube corners (dx + 2 dy + 4 dz) of the vertices v0..v3 of tetrahedron k: axis orders xyz, xzy, yxz, yzx, zxy, zyx */
static const uint8_t TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
/* the tetrahedron's edges: vertex pairs (i, j), i < j */
static const uint8_t TET_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
/* triangles by inside mask, per tetrahedron: up to two, three edges each, -1 ends the list (the header's table) */
#define E01 0
#define E02 1
#define E03 2
#define E12 3
#define E13 4
#define E23 5
#define NONE {-1, -1, -1, -1, -1, -1}
#define ONE(a, b, c) {a, b, c, -1, -1, -1}
#define TET_EVEN                                                                                              \
    {NONE, ONE(E01, E02, E03), ONE(E01, E13, E12), {E02, E03, E13, E02, E13, E12}, ONE(E02, E12, E23),        \
     {E01, E23, E03, E01, E12, E23}, {E01, E13, E23, E01, E23, E02}, ONE(E03, E13, E23), ONE(E03, E23, E13),  \
     {E01, E02, E23, E01, E23, E13}, {E01, E23, E12, E01, E03, E23}, ONE(E02, E23, E12),                      \
     {E02, E12, E13, E02, E13, E03}, ONE(E01, E12, E13), ONE(E01, E03, E02), NONE}
#define TET_ODD                                                                                               \
    {NONE, ONE(E01, E03, E02), ONE(E01, E12, E13), {E02, E13, E03, E02, E12, E13}, ONE(E02, E23, E12),        \
     {E01, E03, E23, E01, E23, E12}, {E01, E23, E13, E01, E02, E23}, ONE(E03, E23, E13), ONE(E03, E13, E23),  \
     {E01, E23, E02, E01, E13, E23}, {E01, E12, E23, E01, E23, E03}, ONE(E02, E12, E23),                      \
     {E02, E13, E12, E02, E03, E13}, ONE(E01, E13, E12), ONE(E01, E02, E03), NONE}
static const int8_t TET_TRI[6][16][6] = {TET_EVEN, TET_ODD, TET_ODD, TET_EVEN, TET_EVEN, TET_ODD};

static float point_value(const iso_scene *s, uint32_t x, uint32_t y, uint32_t z)
{
    return vox_raw(s, (int)x, (int)y, (int)z) * inv_max_of(s);
}

/* technique 4's gradient at texture coordinate pos -- neg_gradient's taps (iso_ref.c) -- as the mesh writes it */
static f3 mesh_normal(const iso_scene *s, f3 pos)
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
    if (dot3(g, g) == 0.0f || !isfinite(n.x) || !isfinite(n.y) || !isfinite(n.z)) return mk3(0.0f, 0.0f, 0.0f);
    return neg3(n);
}

/* The triangle list of the region (all six of lo, hi zero: the whole volume).  positions / normals: nine floats a
 * triangle, written while the list is shorter than `capacity`; either may be NULL.  Debug outputs, per triangle, may be
 * NULL: dir = three doubles, the mean of its tetrahedron's outside vertices minus the mean of its inside vertices (voxel
 * units); cube = its cube's corner 0 (x, y, z).  Returns the length of the list, or -1 for arguments the C ABI refuses. */
int64_t mesh_extract(const iso_scene *s, const mesh_params *p, float *positions, float *normals, double *dir,
                     uint32_t *cube, uint64_t capacity)
{
    if (!s || !s->voxels || !p || s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return -1;
    if (p->normals > 1 || !isfinite(p->isoValue)) return -1;
    uint32_t lo[3], hi[3];
    const int whole = !(p->lo[0] | p->lo[1] | p->lo[2] | p->hi[0] | p->hi[1] | p->hi[2]);
    for (int i = 0; i < 3; ++i) {
        lo[i] = whole ? 0u : p->lo[i];
        hi[i] = whole ? s->res[i] : p->hi[i];
        if (hi[i] == 0 || hi[i] > s->res[i] || lo[i] > hi[i]) return -1;
    }
    const float iso = p->isoValue;
    const uint32_t W = s->res[0], H = s->res[1], D = s->res[2];
    if (W < 2 || H < 2 || D < 2) return 0;
    const uint32_t nbx = (W - 1 + MESH_BLOCK - 1) / MESH_BLOCK, nby = (H - 1 + MESH_BLOCK - 1) / MESH_BLOCK,
                   nbz = (D - 1 + MESH_BLOCK - 1) / MESH_BLOCK;
    uint64_t n = 0;
    for (uint32_t bz = 0; bz < nbz; ++bz)
    for (uint32_t by = 0; by < nby; ++by)
    for (uint32_t bx = 0; bx < nbx; ++bx)
        for (uint32_t lz = 0; lz < MESH_BLOCK; ++lz)
        for (uint32_t ly = 0; ly < MESH_BLOCK; ++ly)
        for (uint32_t lx = 0; lx < MESH_BLOCK; ++lx) {
            const uint32_t c0[3] = {bx * MESH_BLOCK + lx, by * MESH_BLOCK + ly, bz * MESH_BLOCK + lz};
            if (c0[0] + 1 >= W || c0[1] + 1 >= H || c0[2] + 1 >= D) continue;   /* not a cube of the volume */
            int in_region = 1;
            for (int i = 0; i < 3; ++i) in_region = in_region && lo[i] <= c0[i] && c0[i] + 1 <= hi[i];
            if (!in_region) continue;
            float sv[8];
            for (uint32_t j = 0; j < 8; ++j) sv[j] = point_value(s, c0[0] + (j & 1u), c0[1] + ((j >> 1) & 1u), c0[2] + (j >> 2));
            for (int k = 0; k < 6; ++k) {
                const uint8_t *tv = TET_CORNER[k];
                uint32_t m = 0;
                for (int i = 0; i < 4; ++i) m |= (sv[tv[i]] >= iso ? 1u : 0u) << i;
                const int8_t *tri = TET_TRI[k][m];
                for (int t = 0; t < 2 && tri[3 * t] >= 0; ++t) {
                    if (n < capacity) {
                        for (int v = 0; v < 3; ++v) {
                            const uint8_t *e = TET_EDGE[tri[3 * t + v]];
                            const uint32_t cp = tv[e[0]], cq = tv[e[1]];
                            const float sp = sv[cp], sq = sv[cq];
                            float tt = (iso - sp) / (sq - sp);
                            if (!(tt >= 0.f)) tt = 0.f;
                            if (tt > 1.f) tt = 1.f;
                            float pos[3];
                            for (uint32_t ax = 0; ax < 3; ++ax) {
                                const uint32_t pa = c0[ax] + ((cp >> ax) & 1u), da = ((cq >> ax) & 1u) - ((cp >> ax) & 1u);
                                const float g = (float)pa + (float)da * tt;
                                pos[ax] = (g + 0.5f) / (float)s->res[ax] * 2.f - 1.f;
                            }
                            if (positions) memcpy(positions + 9 * n + 3 * v, pos, sizeof pos);
                            if (normals) {
                                const f3 nrm = mesh_normal(s, mk3(pos[0] * 0.5f + 0.5f, pos[1] * 0.5f + 0.5f, pos[2] * 0.5f + 0.5f));
                                normals[9 * n + 3 * v] = nrm.x;
                                normals[9 * n + 3 * v + 1] = nrm.y;
                                normals[9 * n + 3 * v + 2] = nrm.z;
                            }
                        }
                        if (dir) {
                            double in[3] = {0, 0, 0}, out[3] = {0, 0, 0};
                            int n_in = 0;
                            for (int i = 0; i < 4; ++i) {
                                double *acc = ((m >> i) & 1u) ? in : out;
                                n_in += (int)((m >> i) & 1u);
                                for (int ax = 0; ax < 3; ++ax) acc[ax] += (double)((tv[i] >> ax) & 1u);
                            }
                            for (int ax = 0; ax < 3; ++ax) dir[3 * n + ax] = out[ax] / (4 - n_in) - in[ax] / n_in;
                        }
                        if (cube) memcpy(cube + 3 * n, c0, sizeof c0);
                    }
                    ++n;
                }
            }
        }
    return (int64_t)n;
}
