// vrhip_mesh_api.hip -- vrhip_isosurface_count, vrhip_isosurface_extract and vrhip_last_mesh_info (include/vrhip.h
// "isosurface extraction"): the checks, the cell grid for skipping, the launches (vr_mesh.hip) and the copy to host
// destinations.  It reads the volume of the current time step and the object-ESS switch, and writes only the buffers
// the renderer keeps for it (vr_renderer.h) and the caller's destinations.  (The cell grid it may build is derived
// state every technique builds on demand and reads as it is: vr_renderer.h "derived state".)  Every call counts anew:
// nothing but allocations is kept between calls, so nothing here can go stale.
// Behind them vrhip_isosurface_count_indexed, vrhip_isosurface_extract_indexed and vrhip_last_indexed_mesh_info
// ("indexed isosurface extraction"): the same checks (mesh_prepare) and the same pass 1 (mesh_count), then the vertex
// passes.  They share the soup calls' allocations, not their info block.
#include <cmath>

#include "vr_renderer.h"

namespace {

// the checks both calls share, and the launch they describe; *cubes = false: the region holds no cube
int mesh_prepare(vrhip_renderer *r, const vrhip_mesh_params *p, MeshLaunch *a, bool *cubes)
{
    VR_REQUIRE(r, p->normals <= VRHIP_MESH_NORMALS_GRADIENT, VRHIP_ERR_INVALID, "isosurface: unknown normals mode.");
    VR_REQUIRE(r, !(p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]), VRHIP_ERR_INVALID,
               "isosurface: reserved must be 0.");
    VR_REQUIRE(r, std::isfinite(p->isoValue), VRHIP_ERR_INVALID, "isosurface: isoValue must be finite.");
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "isosurface: RG / RGBA volumes are not supported.");
    const bool whole = !(p->lo[0] | p->lo[1] | p->lo[2] | p->hi[0] | p->hi[1] | p->hi[2]);
    std::memset(a, 0, sizeof *a);
    *cubes = true;
    for (int i = 0; i < 3; ++i) {
        uint32_t lo = 0, hi = r->res[i];
        if (!whole) {
            lo = p->lo[i];
            hi = p->hi[i];
            VR_REQUIRE(r, hi != 0 && hi <= r->res[i] && lo <= hi, VRHIP_ERR_INVALID,
                       "isosurface: the region is not a box inside the volume.");
        }
        // cubes lo <= corner 0 < hi: corner 0 + 1 <= the region's hi, and corner 0 + 1 a point of the volume
        hi = std::min(hi, r->res[i] - 1u);
        if (hi <= lo) { *cubes = false; lo = hi = 0; }
        a->lo[i] = lo;
        a->hi[i] = hi;
    }
    if (*cubes)
        for (int i = 0; i < 3; ++i) {
            a->b0[i] = a->lo[i] / VRHIP_MESH_BLOCK;
            a->nb[i] = (a->hi[i] - 1u) / VRHIP_MESH_BLOCK - a->b0[i] + 1u;
        }
    a->vol = make_vol_view(r, r->vols[r->timestep].dev);
    a->format = r->format;
    a->iso = p->isoValue;
    return VRHIP_OK;
}

// pass 1 and the scan: the totals on the host, the offsets (with_offsets) in r->mesh_offsets
int mesh_count(vrhip_renderer *r, MeshLaunch &a, bool with_offsets, uint64_t *triangles, uint64_t *skipped)
{
    int rc;
    if (mip_skips(r)) {   // object-order ESS: the coarse cells' (min, max), which need no transfer function
        if ((rc = ensure_cells(r, true, false, false))) return rc;
        a.cell_minmax = cell_minmax_of(r, false);
        VR_REQUIRE(r, a.cell_minmax, VRHIP_ERR_HIP, "isosurface: the cells' (min, max) were not built.");
        a.cell_shift = r->cells.shift;
        a.cell_cx = r->cells.cx;
        a.cell_cy = r->cells.cy;
        VR_REQUIRE(r, a.cell_shift >= 3, VRHIP_ERR_HIP, "isosurface: the cells are smaller than a block.");
    }
    const size_t n_blocks = (size_t)a.nb[0] * a.nb[1] * a.nb[2], np = vr_mesh_scan_partials(n_blocks);
    VR_REQUIRE(r, n_blocks < 0x7fffffffull, VRHIP_ERR_UNSUPPORTED, "isosurface: too many blocks for one launch.");
    if ((rc = grow(r, r->mesh_counts, n_blocks * sizeof(uint32_t)))) return rc;
    if ((rc = grow(r, r->mesh_partials, (2 * np + 2) * sizeof(unsigned long long)))) return rc;
    if (with_offsets && (rc = grow(r, r->mesh_offsets, n_blocks * sizeof(unsigned long long)))) return rc;
    if ((rc = grow_pinned(r, r->mesh_totals_host, 2 * sizeof(unsigned long long)))) return rc;
    VR_HIP(r, vr_launch_mesh_count(a, r->mesh_counts, r->stream));
    VR_HIP(r, vr_launch_mesh_scan(r->mesh_counts, n_blocks, r->mesh_partials, with_offsets ? r->mesh_offsets.p : nullptr,
                                  r->stream));
    VR_HIP(r, hipMemcpyAsync(r->mesh_totals_host.p, r->mesh_partials.p + 2 * np, 2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, r->stream));
    VR_HIP(r, hipStreamSynchronize(r->stream));
    const unsigned long long *t = (const unsigned long long *)r->mesh_totals_host.p;
    *triangles = t[0];
    *skipped = t[1];
    return VRHIP_OK;
}

void mesh_note(vrhip_renderer *r, const MeshLaunch &a, bool cubes, uint64_t triangles, uint64_t skipped)
{
    std::memset(&r->mesh_info, 0, sizeof r->mesh_info);
    r->mesh_info.triangles = triangles;
    r->mesh_info.blocks = cubes ? (uint64_t)a.nb[0] * a.nb[1] * a.nb[2] : 0u;
    r->mesh_info.blocks_skipped = skipped;
    r->mesh_info.empty_skip = a.cell_minmax ? 1u : 0u;
    r->have_mesh_info = true;
}

// ---- the indexed calls

struct IndexedCounts {
    uint64_t vertices = 0, triangles = 0, point_blocks = 0, point_blocks_skipped = 0, blocks_skipped = 0;
    uint64_t tables = 0;    // point blocks that hold a vertex
    uint64_t scratch = 0;   // bytes of the count and offset words and the scans' partial sums
};

// the soup's pass 1 and scan (mesh_count), then the vertex count over the point blocks and its two scans -- of the
// counts, and of the holds-a-vertex flags: the totals on the host, the offsets and slots (with_offsets) in
// r->imesh_voffsets and r->imesh_slots
int imesh_count(vrhip_renderer *r, MeshLaunch &a, bool with_offsets, IndexedCounts *c)
{
    int rc;
    if ((rc = mesh_count(r, a, with_offsets, &c->triangles, &c->blocks_skipped))) return rc;
    uint32_t pnb[3];
    vr_mesh_point_blocks(a, pnb);
    const size_t n_blocks = (size_t)a.nb[0] * a.nb[1] * a.nb[2];
    const size_t n_pb = (size_t)pnb[0] * pnb[1] * pnb[2], np = vr_mesh_scan_partials(n_pb), part = 2 * np + 2;
    VR_REQUIRE(r, n_pb < 0x7fffffffull, VRHIP_ERR_UNSUPPORTED, "isosurface: too many blocks for one launch.");
    if ((rc = grow(r, r->imesh_vcounts, n_pb * sizeof(uint32_t)))) return rc;
    if ((rc = grow(r, r->imesh_vflags, n_pb * sizeof(uint32_t)))) return rc;
    if ((rc = grow(r, r->imesh_partials, 2 * part * sizeof(unsigned long long)))) return rc;
    if (with_offsets && (rc = grow(r, r->imesh_voffsets, n_pb * sizeof(unsigned long long)))) return rc;
    if (with_offsets && (rc = grow(r, r->imesh_slots, n_pb * sizeof(unsigned long long)))) return rc;
    if ((rc = grow_pinned(r, r->imesh_totals_host, 4 * sizeof(unsigned long long)))) return rc;
    unsigned long long *part_v = r->imesh_partials.p, *part_f = r->imesh_partials.p + part;
    unsigned long long *t = (unsigned long long *)r->imesh_totals_host.p;
    VR_HIP(r, vr_launch_mesh_vertex_count(a, r->imesh_vcounts, r->imesh_vflags, r->stream));
    VR_HIP(r, vr_launch_mesh_scan(r->imesh_vcounts, n_pb, part_v, with_offsets ? r->imesh_voffsets.p : nullptr, r->stream));
    VR_HIP(r, vr_launch_mesh_scan(r->imesh_vflags, n_pb, part_f, with_offsets ? r->imesh_slots.p : nullptr, r->stream));
    VR_HIP(r, hipMemcpyAsync(t, part_v + 2 * np, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
    VR_HIP(r, hipMemcpyAsync(t + 2, part_f + 2 * np, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
    VR_HIP(r, hipStreamSynchronize(r->stream));
    c->vertices = t[0];
    c->point_blocks_skipped = t[1];
    c->tables = t[2];
    // (the launch's one block that owns no eligible edge, where every hi is a multiple of the block, is not counted)
    c->point_blocks = n_pb - ((a.hi[0] | a.hi[1] | a.hi[2]) % VRHIP_MESH_BLOCK == 0 ? 1u : 0u);
    c->scratch = n_blocks * sizeof(uint32_t) + (2 * vr_mesh_scan_partials(n_blocks) + 2) * sizeof(unsigned long long) +
                 2 * n_pb * sizeof(uint32_t) + 2 * part * sizeof(unsigned long long) +
                 (with_offsets ? (n_blocks + 2 * n_pb) * sizeof(unsigned long long) : 0u);
    return VRHIP_OK;
}

void imesh_note(vrhip_renderer *r, const MeshLaunch &a, bool cubes, const IndexedCounts &c, uint64_t scratch)
{
    std::memset(&r->imesh_info, 0, sizeof r->imesh_info);
    r->imesh_info.vertices = c.vertices;
    r->imesh_info.triangles = c.triangles;
    r->imesh_info.point_blocks = c.point_blocks;
    r->imesh_info.point_blocks_skipped = c.point_blocks_skipped;
    r->imesh_info.blocks = cubes ? (uint64_t)a.nb[0] * a.nb[1] * a.nb[2] : 0u;
    r->imesh_info.blocks_skipped = c.blocks_skipped;
    r->imesh_info.scratch_bytes = scratch;
    r->imesh_info.empty_skip = a.cell_minmax ? 1u : 0u;
    r->have_imesh_info = true;
}

} // namespace

extern "C" {

int vrhip_isosurface_count(vrhip_renderer *r, const vrhip_mesh_params *p, uint64_t *n_triangles)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p && n_triangles, VRHIP_ERR_INVALID, "vrhip_isosurface_count: NULL argument");
    MeshLaunch a;
    bool cubes;
    int rc;
    if ((rc = mesh_prepare(r, p, &a, &cubes))) return rc;
    uint64_t triangles = 0, skipped = 0;
    if (cubes) {
        if (set_device(r)) return VRHIP_ERR_HIP;
        r->have_mesh_info = false;
        if ((rc = mesh_count(r, a, false, &triangles, &skipped))) return rc;
    }
    mesh_note(r, a, cubes, triangles, skipped);
    *n_triangles = triangles;
    return VRHIP_OK;
}

int vrhip_isosurface_extract(vrhip_renderer *r, const vrhip_mesh_params *p, float *out_positions, float *out_normals,
                             uint64_t capacity_triangles, uint64_t *n_triangles, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p && n_triangles, VRHIP_ERR_INVALID, "vrhip_isosurface_extract: NULL argument");
    VR_REQUIRE(r, out_positions, VRHIP_ERR_INVALID, "vrhip_isosurface_extract: no destination");
    VR_REQUIRE(r, p->normals > VRHIP_MESH_NORMALS_GRADIENT || (out_normals != nullptr) == (p->normals == VRHIP_MESH_NORMALS_GRADIENT),
               VRHIP_ERR_INVALID, "vrhip_isosurface_extract: out_normals goes with normals == 1, and only with it.");
    VR_REQUIRE(r, !out_is_device || (((uintptr_t)out_positions | (uintptr_t)out_normals) & 15u) == 0, VRHIP_ERR_INVALID,
               "vrhip_isosurface_extract: device destinations must be 16-byte aligned.");
    MeshLaunch a;
    bool cubes;
    int rc;
    if ((rc = mesh_prepare(r, p, &a, &cubes))) return rc;
    uint64_t triangles = 0, skipped = 0;
    if (cubes) {
        if (set_device(r)) return VRHIP_ERR_HIP;
        r->have_mesh_info = false;
        if ((rc = mesh_count(r, a, true, &triangles, &skipped))) return rc;
    }
    mesh_note(r, a, cubes, triangles, skipped);
    *n_triangles = triangles;
    if (triangles > capacity_triangles)
        return fail(r, VRHIP_ERR_INVALID, "vrhip_isosurface_extract: the destination holds " + std::to_string(capacity_triangles) +
                                              " triangles, the surface has " + std::to_string(triangles) + ".");
    if (triangles == 0) return VRHIP_OK;

    const size_t plane = (size_t)triangles * 9u * sizeof(float);   // positions; the normals follow in the staging
    float *pos = out_positions, *nrm = out_normals;
    if (!out_is_device) {
        const size_t bytes = out_normals ? 2 * plane : plane;
        if ((rc = grow(r, r->mesh_out_dev, bytes))) return rc;
        if ((rc = grow_pinned(r, r->mesh_host, bytes))) return rc;
        pos = r->mesh_out_dev.p;
        nrm = out_normals ? r->mesh_out_dev.p + (size_t)triangles * 9u : nullptr;
    }
    VR_HIP(r, vr_launch_mesh_emit(a, r->mesh_counts, r->mesh_offsets, pos, nrm, r->stream));
    if (!out_is_device) {
        const size_t bytes = out_normals ? 2 * plane : plane;
        VR_HIP(r, hipMemcpyAsync(r->mesh_host.p, r->mesh_out_dev.p, bytes, hipMemcpyDeviceToHost, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
        std::memcpy(out_positions, r->mesh_host.p, plane);
        if (out_normals) std::memcpy(out_normals, (const uint8_t *)r->mesh_host.p + plane, plane);
    }
    return VRHIP_OK;
}

int vrhip_last_mesh_info(const vrhip_renderer *r, vrhip_mesh_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_mesh_info) return fail(r, VRHIP_ERR_NODATA, "vrhip_last_mesh_info: no isosurface has been extracted yet");
    *out = r->mesh_info;
    return VRHIP_OK;
}

int vrhip_isosurface_count_indexed(vrhip_renderer *r, const vrhip_mesh_params *p, uint64_t *n_vertices, uint64_t *n_triangles)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p && n_vertices && n_triangles, VRHIP_ERR_INVALID, "vrhip_isosurface_count_indexed: NULL argument");
    MeshLaunch a;
    bool cubes;
    int rc;
    if ((rc = mesh_prepare(r, p, &a, &cubes))) return rc;
    IndexedCounts c;
    if (cubes) {
        if (set_device(r)) return VRHIP_ERR_HIP;
        r->have_imesh_info = false;
        if ((rc = imesh_count(r, a, false, &c))) return rc;
    }
    imesh_note(r, a, cubes, c, c.scratch);
    *n_vertices = c.vertices;
    *n_triangles = c.triangles;
    return VRHIP_OK;
}

int vrhip_isosurface_extract_indexed(vrhip_renderer *r, const vrhip_mesh_params *p, float *out_vertices, float *out_normals,
                                     uint32_t *out_indices, uint64_t capacity_vertices, uint64_t capacity_triangles,
                                     uint64_t *n_vertices, uint64_t *n_triangles, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p && n_vertices && n_triangles, VRHIP_ERR_INVALID, "vrhip_isosurface_extract_indexed: NULL argument");
    VR_REQUIRE(r, out_vertices && out_indices, VRHIP_ERR_INVALID, "vrhip_isosurface_extract_indexed: no destination");
    VR_REQUIRE(r, p->normals > VRHIP_MESH_NORMALS_GRADIENT || (out_normals != nullptr) == (p->normals == VRHIP_MESH_NORMALS_GRADIENT),
               VRHIP_ERR_INVALID, "vrhip_isosurface_extract_indexed: out_normals goes with normals == 1, and only with it.");
    VR_REQUIRE(r, !out_is_device || (((uintptr_t)out_vertices | (uintptr_t)out_normals | (uintptr_t)out_indices) & 15u) == 0,
               VRHIP_ERR_INVALID, "vrhip_isosurface_extract_indexed: device destinations must be 16-byte aligned.");
    MeshLaunch a;
    bool cubes;
    int rc;
    if ((rc = mesh_prepare(r, p, &a, &cubes))) return rc;
    IndexedCounts c;
    if (cubes) {
        if (set_device(r)) return VRHIP_ERR_HIP;
        r->have_imesh_info = false;
        if ((rc = imesh_count(r, a, true, &c))) return rc;
    }
    imesh_note(r, a, cubes, c, c.scratch + c.tables * kMeshTableBytes);   // (the rank tables: grown below)
    *n_vertices = c.vertices;
    *n_triangles = c.triangles;
    if (c.vertices > 0xffffffffull)
        return fail(r, VRHIP_ERR_UNSUPPORTED, "vrhip_isosurface_extract_indexed: the surface has " + std::to_string(c.vertices) +
                                                  " vertices, more than 32-bit indices name.");
    if (c.vertices > capacity_vertices || c.triangles > capacity_triangles)
        return fail(r, VRHIP_ERR_INVALID, "vrhip_isosurface_extract_indexed: the destinations hold " +
                                              std::to_string(capacity_vertices) + " vertices and " + std::to_string(capacity_triangles) +
                                              " triangles, the surface has " + std::to_string(c.vertices) + " and " +
                                              std::to_string(c.triangles) + ".");
    if (c.triangles == 0) return VRHIP_OK;   // (and no vertex: a crossed eligible edge lies in a tetrahedron that is cut)

    if ((rc = grow(r, r->imesh_row_masks, (size_t)c.tables * kMeshTableRows * sizeof(unsigned long long)))) return rc;
    if ((rc = grow(r, r->imesh_row_bases, (size_t)c.tables * kMeshTableRows * sizeof(uint32_t)))) return rc;
    // host destinations: vertices, normals, indices, one behind the other in the staging
    const size_t vwords = (size_t)c.vertices * 3u, iwords = (size_t)c.triangles * 3u;
    const size_t bytes = ((out_normals ? 2 * vwords : vwords) + iwords) * sizeof(float);
    float *vtx = out_vertices, *nrm = out_normals;
    uint32_t *idx = out_indices;
    if (!out_is_device) {
        if ((rc = grow(r, r->mesh_out_dev, bytes))) return rc;
        if ((rc = grow_pinned(r, r->mesh_host, bytes))) return rc;
        vtx = r->mesh_out_dev.p;
        nrm = out_normals ? vtx + vwords : nullptr;
        idx = reinterpret_cast<uint32_t *>(vtx + (out_normals ? 2 * vwords : vwords));
    }
    VR_HIP(r, vr_launch_mesh_vertex_emit(a, r->imesh_vcounts, r->imesh_voffsets, r->imesh_slots, vtx, nrm, r->imesh_row_masks,
                                         r->imesh_row_bases, r->stream));
    VR_HIP(r, vr_launch_mesh_index_emit(a, r->mesh_counts, r->mesh_offsets, r->imesh_slots, r->imesh_row_masks,
                                        r->imesh_row_bases, idx, r->stream));
    if (!out_is_device) {
        VR_HIP(r, hipMemcpyAsync(r->mesh_host.p, r->mesh_out_dev.p, bytes, hipMemcpyDeviceToHost, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
        const float *h = (const float *)r->mesh_host.p;
        std::memcpy(out_vertices, h, vwords * sizeof(float));
        if (out_normals) std::memcpy(out_normals, h + vwords, vwords * sizeof(float));
        std::memcpy(out_indices, h + (out_normals ? 2 * vwords : vwords), iwords * sizeof(uint32_t));
    }
    return VRHIP_OK;
}

int vrhip_last_indexed_mesh_info(const vrhip_renderer *r, vrhip_indexed_mesh_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_imesh_info)
        return fail(r, VRHIP_ERR_NODATA, "vrhip_last_indexed_mesh_info: no indexed isosurface has been extracted yet");
    *out = r->imesh_info;
    return VRHIP_OK;
}

} // extern "C"
