// meshio.cpp -- what VolumeRenderCL does with a triangle list once it is in host memory (include/volumerendercl.h
// "isosurface extraction"): weldMesh, writeStl, writePly.  Plain C++ with no call into libvrhip, a unit of its own so
// that it also builds into a stand-alone program (a sanitizer run of the host code needs no GPU).
#include "volumerendercl.h"

#include <cmath>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <unordered_map>

namespace {

struct VertexKey {
    uint32_t w[3];
    bool operator==(const VertexKey &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2]; }
};
struct VertexHash {
    size_t operator()(const VertexKey &k) const
    {
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (uint32_t w : k.w) h = (h ^ w) * 0x100000001b3ull;
        return size_t(h ^ (h >> 29));
    }
};

void check_list(const std::vector<float> &positions, const std::vector<float> &normals)
{
    if (positions.size() % 9 != 0) throw std::invalid_argument("a triangle list holds nine floats a triangle");
    if (!normals.empty() && normals.size() != positions.size())
        throw std::invalid_argument("normals and positions must be of one size");
}

void put_u32(std::ofstream &f, uint32_t v)   // little endian
{
    const unsigned char b[4] = {(unsigned char)(v & 0xff), (unsigned char)((v >> 8) & 0xff), (unsigned char)((v >> 16) & 0xff),
                                (unsigned char)(v >> 24)};
    f.write(reinterpret_cast<const char *>(b), 4);
}

void put_f32(std::ofstream &f, float v)
{
    uint32_t w;
    std::memcpy(&w, &v, 4);
    put_u32(f, w);
}

} // namespace

VolumeRenderCL::welded_mesh VolumeRenderCL::weldMesh(const std::vector<float> &positions, const std::vector<float> &normals)
{
    check_list(positions, normals);
    welded_mesh m;
    const size_t n = positions.size() / 3;
    if (n > 0xffffffffull) throw std::invalid_argument("weldMesh: more than 2^32 vertices");
    std::unordered_map<VertexKey, uint32_t, VertexHash> seen;
    seen.reserve(n / 4 + 16);
    m.indices.resize(n);
    for (size_t i = 0; i < n; ++i) {
        VertexKey k;
        std::memcpy(k.w, positions.data() + 3 * i, sizeof k.w);
        const auto it = seen.emplace(k, uint32_t(m.vertices.size() / 3));
        if (it.second) {
            m.vertices.insert(m.vertices.end(), positions.begin() + 3 * i, positions.begin() + 3 * i + 3);
            if (!normals.empty()) m.normals.insert(m.normals.end(), normals.begin() + 3 * i, normals.begin() + 3 * i + 3);
        }
        m.indices[i] = it.first->second;
    }
    return m;
}

void VolumeRenderCL::writeStl(const std::string &path, const std::vector<float> &positions)
{
    check_list(positions, {});
    const size_t n = positions.size() / 9;
    if (n > 0xffffffffull) throw std::invalid_argument("writeStl: more than 2^32 triangles");
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("ERROR: cannot write " + path);
    char head[80];
    std::memset(head, ' ', sizeof head);
    std::memcpy(head, "vrhip isosurface", 16);
    f.write(head, sizeof head);
    put_u32(f, uint32_t(n));
    for (size_t t = 0; t < n; ++t) {
        const float *p = positions.data() + 9 * t;
        // the right-hand normal of the winding, in double; (0, 0, 0) for a degenerate triangle
        const double a[3] = {double(p[3]) - p[0], double(p[4]) - p[1], double(p[5]) - p[2]};
        const double b[3] = {double(p[6]) - p[0], double(p[7]) - p[1], double(p[8]) - p[2]};
        double nrm[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double len = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        for (double &c : nrm) c = len > 0 ? c / len : 0.0;
        for (double c : nrm) put_f32(f, float(c));
        for (int i = 0; i < 9; ++i) put_f32(f, p[i]);
        const char attr[2] = {0, 0};
        f.write(attr, 2);
    }
    if (!f) throw std::runtime_error("ERROR: cannot write " + path);
}

size_t VolumeRenderCL::writePly(const std::string &path, const std::vector<float> &positions, const std::vector<float> &normals)
{
    return writePly(path, weldMesh(positions, normals));
}

size_t VolumeRenderCL::writePly(const std::string &path, const welded_mesh &m)
{
    if (m.vertices.size() % 3 != 0 || m.indices.size() % 3 != 0 || (!m.normals.empty() && m.normals.size() != m.vertices.size()))
        throw std::invalid_argument("an indexed mesh holds three floats a vertex and three indices a triangle");
    const size_t nv = m.vertices.size() / 3, nf = m.indices.size() / 3;
    for (uint32_t i : m.indices)
        if (i >= nv) throw std::invalid_argument("writePly: an index names no vertex");
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("ERROR: cannot write " + path);
    f << "ply\nformat binary_little_endian 1.0\ncomment vrhip isosurface\nelement vertex " << nv
      << "\nproperty float x\nproperty float y\nproperty float z\n";
    if (!m.normals.empty()) f << "property float nx\nproperty float ny\nproperty float nz\n";
    f << "element face " << nf << "\nproperty list uchar uint vertex_indices\nend_header\n";
    for (size_t v = 0; v < nv; ++v) {
        for (int i = 0; i < 3; ++i) put_f32(f, m.vertices[3 * v + i]);
        if (!m.normals.empty())
            for (int i = 0; i < 3; ++i) put_f32(f, m.normals[3 * v + i]);
    }
    for (size_t t = 0; t < nf; ++t) {
        f.put(char(3));
        for (int i = 0; i < 3; ++i) put_u32(f, m.indices[3 * t + i]);
    }
    if (!f) throw std::runtime_error("ERROR: cannot write " + path);
    return nv;
}
