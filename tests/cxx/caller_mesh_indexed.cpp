// A caller of the indexed isosurface extraction through the C++ class, compiled against include/ ALONE
// (tests/test_gpu_mesh_indexed.py): VolumeRenderCL::extractIsosurfaceIndexed with normals and on a region, and
// writePly of the mesh as it is.  Writes to argv[1], raw: the vertex and triangle counts (uint64 each), the vertices
// and the normals (float32, three a vertex each), the indices (uint32, three a triangle); then the region's counts,
// vertices and indices.  argv[2] + ".ply" receives the file of the first mesh.
#include <volumerendercl.h>

#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    try {
        VolumeRenderCL vr;
        vr.initialize(false, false);
        vr.loadSyntheticVolume("sphere", 32, DatRawReader::UCHAR);
        static_assert(sizeof(vrhip_mesh_params) == 48 && sizeof(vrhip_indexed_mesh_info) == 64, "48 and 64 bytes");
        const VolumeRenderCL::welded_mesh whole = vr.extractIsosurfaceIndexed(0.4f, true);
        VolumeRenderCL::mesh_region region;
        region.lo = {{3u, 5u, 2u}};
        region.hi = {{29u, 30u, 31u}};
        const VolumeRenderCL::welded_mesh part = vr.extractIsosurfaceIndexed(0.4f, false, region);
        if (whole.vertices.empty() || whole.normals.size() != whole.vertices.size() || !part.normals.empty()) return 5;
        // (the soup call in between and after: neither disturbs the other)
        const VolumeRenderCL::iso_mesh soup = vr.extractIsosurface(0.4f, false);
        if (soup.positions.size() != whole.indices.size() * 3) return 5;
        for (size_t i = 0; i < whole.indices.size(); ++i)
            for (size_t k = 0; k < 3; ++k)
                if (soup.positions[3 * i + k] != whole.vertices[3 * size_t(whole.indices[i]) + k]) return 6;
        if (VolumeRenderCL::writePly(std::string(argv[2]) + ".ply", whole) != whole.vertices.size() / 3) return 5;
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        auto put = [&](const void *p, size_t size, size_t n) { return std::fwrite(p, size, n, f) == n; };
        for (const VolumeRenderCL::welded_mesh *m : {&whole, &part}) {
            const unsigned long long nv = m->vertices.size() / 3, nt = m->indices.size() / 3;
            if (!put(&nv, 8, 1) || !put(&nt, 8, 1) || !put(m->vertices.data(), 4, 3 * nv) ||
                !put(m->normals.data(), 4, m->normals.size()) || !put(m->indices.data(), 4, 3 * nt))
                return 4;
        }
        std::fclose(f);
        std::printf("%zu vertices, %zu triangles\n", whole.vertices.size() / 3, whole.indices.size() / 3);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
