// A caller of the isosurface extraction through the C++ class, compiled against include/ ALONE
// (tests/test_gpu_mesh.py): VolumeRenderCL::extractIsosurface with normals and on a region, weldMesh, writeStl and
// writePly.  Writes to argv[1], raw: the triangle count (uint64), the positions and the normals (float32, nine a
// triangle each), the region's triangle count and positions, then the welded mesh: vertex count (uint64), vertices,
// normals (float32), indices (uint32).  argv[2] + ".stl" and argv[2] + ".ply" receive the files.
#include <volumerendercl.h>

#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    try {
        VolumeRenderCL vr;
        vr.initialize(false, false);
        vr.loadSyntheticVolume("sphere", 32, DatRawReader::UCHAR);
        static_assert(sizeof(vrhip_mesh_params) == 48 && sizeof(vrhip_mesh_info) == 32, "48 and 32 bytes");
        const VolumeRenderCL::iso_mesh whole = vr.extractIsosurface(0.4f, true);
        VolumeRenderCL::mesh_region region;
        region.lo = {{3u, 5u, 2u}};
        region.hi = {{29u, 30u, 31u}};
        const VolumeRenderCL::iso_mesh part = vr.extractIsosurface(0.4f, false, region);
        if (whole.positions.empty() || whole.normals.size() != whole.positions.size() || !part.normals.empty()) return 5;
        const VolumeRenderCL::welded_mesh w = VolumeRenderCL::weldMesh(whole.positions, whole.normals);
        if (w.indices.size() * 3 != whole.positions.size() || w.normals.size() != w.vertices.size()) return 5;
        VolumeRenderCL::writeStl(std::string(argv[2]) + ".stl", whole.positions);
        if (VolumeRenderCL::writePly(std::string(argv[2]) + ".ply", whole.positions, whole.normals) != w.vertices.size() / 3)
            return 5;
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        auto put = [&](const void *p, size_t size, size_t n) { return std::fwrite(p, size, n, f) == n; };
        const unsigned long long n = whole.positions.size() / 9, np = part.positions.size() / 9, nv = w.vertices.size() / 3;
        if (!put(&n, 8, 1) || !put(whole.positions.data(), 4, 9 * n) || !put(whole.normals.data(), 4, 9 * n)) return 4;
        if (!put(&np, 8, 1) || !put(part.positions.data(), 4, 9 * np)) return 4;
        if (!put(&nv, 8, 1) || !put(w.vertices.data(), 4, 3 * nv) || !put(w.normals.data(), 4, 3 * nv) ||
            !put(w.indices.data(), 4, 3 * n))
            return 4;
        std::fclose(f);
        std::printf("%llu triangles\n", n);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
