/*
 * mesh_indexed_ref.c -- scalar CPU restatement of the indexed isosurface extraction (vrhip_isosurface_count_indexed /
 * _extract_indexed, include/vrhip.h "indexed isosurface extraction").
 *
 * TEST INFRASTRUCTURE ONLY: the yardstick of the indexed kernels of vr_mesh.hip.  Written as the contract reads: a
 * loop over point blocks, points and edges d = 1..7 that numbers every eligible crossed edge as it meets it -- the
 * numbers kept in a dense array of eight words per grid point, which a test volume affords --, then the soup's loop
 * over blocks, cubes, tetrahedra and table entries, looking each triangle vertex's edge up in that array.  No counts,
 * no prefix sums, no rank tables, no skipping.  Compiled by tests/mesh_indexed_ref.py like tests/ref/mesh_ref.c, which
 * is included here: point values, the table, the normal and the region checks are that file's, so the two
 * restatements cannot drift apart; tests/test_mesh_indexed_ref.py pins vertices[indices] to its list bit for bit.
 */
#include "mesh_ref.c"

/* The indexed mesh of the region.  vertices / normals: three floats a vertex, written while fewer than cap_v are
 * numbered; indices: three words a triangle, while fewer than cap_t; each may be NULL.  counts[0..2]: vertices,
 * triangles, and the blocks of 8^3 grid points that own an eligible edge.  Returns 0, or -1 for arguments the C ABI
 * refuses (and for a volume too large for the dense array). */
int mesh_extract_indexed(const iso_scene *s, const mesh_params *p, float *vertices, float *normals, uint32_t *indices,
                         uint64_t cap_v, uint64_t cap_t, uint64_t *counts)
{
    if (!s || !s->voxels || !p || !counts || s->format < 0 || s->format > 2 || !s->res[0] || !s->res[1] || !s->res[2]) return -1;
    if (p->normals > 1 || !isfinite(p->isoValue)) return -1;
    uint32_t lo[3], hi[3];
    const int whole = !(p->lo[0] | p->lo[1] | p->lo[2] | p->hi[0] | p->hi[1] | p->hi[2]);
    int cubes = 1;
    for (int i = 0; i < 3; ++i) {
        lo[i] = whole ? 0u : p->lo[i];
        hi[i] = whole ? s->res[i] : p->hi[i];
        if (hi[i] == 0 || hi[i] > s->res[i] || lo[i] > hi[i]) return -1;
        if (hi[i] > s->res[i] - 1u) hi[i] = s->res[i] - 1u;   /* the effective region */
        if (hi[i] <= lo[i]) cubes = 0;
    }
    counts[0] = counts[1] = counts[2] = 0;
    if (!cubes) return 0;
    const float iso = p->isoValue;
    const uint32_t res[3] = {s->res[0], s->res[1], s->res[2]};
    const uint64_t points = (uint64_t)res[0] * res[1] * res[2];
    if (points > (1u << 24)) return -1;
    uint32_t *number = calloc((size_t)points * 8u, sizeof *number);   /* of edge (P, d), plus one; 0: no vertex */
    if (!number) return -1;

    /* the vertices: point blocks x fastest, points x fastest, d ascending */
    uint32_t npb[3];
    for (int i = 0; i < 3; ++i) npb[i] = (res[i] + MESH_BLOCK - 1) / MESH_BLOCK;
    uint64_t nv = 0, blocks = 0;
    for (uint32_t bz = 0; bz < npb[2]; ++bz)
    for (uint32_t by = 0; by < npb[1]; ++by)
    for (uint32_t bx = 0; bx < npb[0]; ++bx) {
        int owns = 0;
        for (uint32_t lz = 0; lz < MESH_BLOCK; ++lz)
        for (uint32_t ly = 0; ly < MESH_BLOCK; ++ly)
        for (uint32_t lx = 0; lx < MESH_BLOCK; ++lx) {
            const uint32_t P[3] = {bx * MESH_BLOCK + lx, by * MESH_BLOCK + ly, bz * MESH_BLOCK + lz};
            if (P[0] >= res[0] || P[1] >= res[1] || P[2] >= res[2]) continue;
            for (uint32_t d = 1; d < 8; ++d) {
                int eligible = 1;
                for (uint32_t ax = 0; ax < 3; ++ax)
                    eligible = eligible && lo[ax] <= P[ax] && (((d >> ax) & 1u) ? P[ax] < hi[ax] : P[ax] <= hi[ax]);
                if (!eligible) continue;
                owns = 1;
                const uint32_t Q[3] = {P[0] + (d & 1u), P[1] + ((d >> 1) & 1u), P[2] + (d >> 2)};
                const float sp = point_value(s, P[0], P[1], P[2]), sq = point_value(s, Q[0], Q[1], Q[2]);
                if ((sp >= iso) == (sq >= iso)) continue;   /* not crossed */
                if (nv < cap_v) {
                    float tt = (iso - sp) / (sq - sp);
                    if (!(tt >= 0.f)) tt = 0.f;
                    if (tt > 1.f) tt = 1.f;
                    float pos[3];
                    for (uint32_t ax = 0; ax < 3; ++ax) {
                        const float g = (float)P[ax] + (float)(Q[ax] - P[ax]) * tt;
                        pos[ax] = (g + 0.5f) / (float)res[ax] * 2.f - 1.f;
                    }
                    if (vertices) memcpy(vertices + 3 * nv, pos, sizeof pos);
                    if (normals) {
                        const f3 nrm = mesh_normal(s, mk3(pos[0] * 0.5f + 0.5f, pos[1] * 0.5f + 0.5f, pos[2] * 0.5f + 0.5f));
                        normals[3 * nv] = nrm.x;
                        normals[3 * nv + 1] = nrm.y;
                        normals[3 * nv + 2] = nrm.z;
                    }
                }
                number[(((uint64_t)P[2] * res[1] + P[1]) * res[0] + P[0]) * 8u + d] = (uint32_t)++nv;
            }
        }
        blocks += (uint64_t)owns;
    }

    /* the triangles: the soup's list (mesh_extract), each vertex as the number of its edge */
    const uint32_t nb[3] = {(res[0] - 1 + MESH_BLOCK - 1) / MESH_BLOCK, (res[1] - 1 + MESH_BLOCK - 1) / MESH_BLOCK,
                            (res[2] - 1 + MESH_BLOCK - 1) / MESH_BLOCK};
    uint64_t nt = 0;
    int bad = 0;
    for (uint32_t bz = 0; bz < nb[2]; ++bz)
    for (uint32_t by = 0; by < nb[1]; ++by)
    for (uint32_t bx = 0; bx < nb[0]; ++bx)
        for (uint32_t lz = 0; lz < MESH_BLOCK; ++lz)
        for (uint32_t ly = 0; ly < MESH_BLOCK; ++ly)
        for (uint32_t lx = 0; lx < MESH_BLOCK; ++lx) {
            const uint32_t c0[3] = {bx * MESH_BLOCK + lx, by * MESH_BLOCK + ly, bz * MESH_BLOCK + lz};
            if (c0[0] < lo[0] || c0[0] >= hi[0] || c0[1] < lo[1] || c0[1] >= hi[1] || c0[2] < lo[2] || c0[2] >= hi[2]) continue;
            float sv[8];
            for (uint32_t j = 0; j < 8; ++j) sv[j] = point_value(s, c0[0] + (j & 1u), c0[1] + ((j >> 1) & 1u), c0[2] + (j >> 2));
            for (int k = 0; k < 6; ++k) {
                const uint8_t *tv = TET_CORNER[k];
                uint32_t m = 0;
                for (int i = 0; i < 4; ++i) m |= (sv[tv[i]] >= iso ? 1u : 0u) << i;
                const int8_t *tri = TET_TRI[k][m];
                for (int t = 0; t < 2 && tri[3 * t] >= 0; ++t) {
                    for (int v = 0; v < 3; ++v) {
                        const uint8_t *e = TET_EDGE[tri[3 * t + v]];
                        const uint32_t cp = tv[e[0]], cq = tv[e[1]], d = cq - cp;
                        const uint32_t P[3] = {c0[0] + (cp & 1u), c0[1] + ((cp >> 1) & 1u), c0[2] + (cp >> 2)};
                        const uint32_t id = number[(((uint64_t)P[2] * res[1] + P[1]) * res[0] + P[0]) * 8u + d];
                        if (id == 0 || (cp & ~cq)) bad = 1;   /* (a triangle vertex on an edge without a vertex: a bug here) */
                        if (indices && nt < cap_t) indices[3 * nt + v] = id - 1u;
                    }
                    ++nt;
                }
            }
        }
    free(number);
    counts[0] = nv;
    counts[1] = nt;
    counts[2] = blocks;
    return bad ? -1 : 0;
}
