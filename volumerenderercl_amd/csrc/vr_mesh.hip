// vr_mesh.hip -- isosurface extraction (vrhip_isosurface_count / vrhip_isosurface_extract, include/vrhip.h
// "isosurface extraction"): the count and emit kernels, instantiated per voxel type, the three kernels of the prefix
// sum between them, and their launch entries.  Not a technique: it writes buffers of its own and the caller's.
// Behind them the kernels of the indexed extraction (vrhip_isosurface_extract_indexed), which share the staging,
// the table and the scan: see "the indexed extraction" below.
//
// Definition (tests/ref/mesh_ref.c restates it on the CPU): the volume's cubes, each cut into the six
// Kuhn tetrahedra, each tetrahedron's zero, one or two triangles from its inside mask by the table below (the
// header's, packed), an edge vertex from its edge's two grid points alone; blocks of 8^3 cubes x fastest, cubes x
// fastest, tetrahedra 0..5, triangles in table order.
//
// Execution: one wave per block of 8^3 cubes, a workgroup of its own (64 threads), so that a skipped or empty block
// ends at once and the barrier behind the staging is a wave's.
//  * pass 1 (vr_mesh_count_kernel): the block's cell of the cell grid, when it is handed over, may prove every point
//    outside or every point inside -- then the block is not fetched and its count word is kMeshSkipped.  Else the
//    block's 9^3 normalised point values go to LDS once (2916 bytes; in the micro-brick layout a row of nine is at
//    most three runs of four), lane (x, y) classifies the eight cubes of its column, and the wave's sum is the block's
//    count word.  At most 512 * 12 triangles a block: far below bit 31.
//  * the scan (vr_mesh_scan_*): reduce-then-scan in three launches -- sums of chunks of kMeshScanChunk count words,
//    one workgroup's exclusive scan of those sums, the chunks' own exclusive scans on top -- in 64 bits.  No workgroup
//    waits for another.
//  * pass 2 (vr_mesh_emit_kernel): blocks with a count reload their points and recompute the masks; a cube's place
//    is the block's offset + the layers below + a wave-level exclusive sum over the lanes of its layer, which is the
//    contract's order (lane = x + 8 y).  Every triangle is written once, to its final place, with plain stores: no
//    atomic anywhere.
//
// The skip is exact: s = fl(raw * inv_max) is monotone in raw (inv_max > 0), so raw <= max gives s <= fl(max * inv_max)
// and raw >= min gives s >= fl(min * inv_max) -- the very comparison the classification makes.  A cell with a NaN
// voxel holds (-inf, +inf) (vr_cells.hip) and passes neither test.  The cells are 2^shift >= 8 voxels wide, a multiple
// of the block, and answer for the voxels [c << shift) - 1, ((c + 1) << shift) + 1]: the block's points 8 b .. 8 b + 8
// lie in the extent of the one cell (8 b) >> shift.
#include "vr_sampling.h"

namespace {

constexpr uint32_t kMB = VRHIP_MESH_BLOCK;         // cubes per block and axis
constexpr uint32_t kMP = kMB + 1u;                 // points per block and axis
constexpr uint32_t kMeshPoints = kMP * kMP * kMP;  // 729
static_assert(kMB == 8u, "lane = x + 8 y, eight layers");

// The triangles of a tetrahedron by its inside mask: bits 0..3 their number, then three nibbles a triangle, each an
// edge 0..5 = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of the tetrahedron's vertices.  Row 0: the tetrahedra xyz, yzx, zxy;
// row 1: their mirror images xzy, yxz, zyx (include/vrhip.h).
__constant__ uint32_t kTetTriangles[2][16] = {
    {0x0000000u, 0x0002101u, 0x0003401u, 0x3414212u, 0x0005311u, 0x5302502u, 0x1505402u, 0x0005421u, 0x0004521u,
     0x4505102u, 0x5203502u, 0x0003511u, 0x2414312u, 0x0004301u, 0x0001201u, 0x0000000u},
    {0x0000000u, 0x0001201u, 0x0004301u, 0x4312412u, 0x0003511u, 0x3505202u, 0x5104502u, 0x0004521u, 0x0005421u,
     0x5401502u, 0x2505302u, 0x0005311u, 0x4213412u, 0x0003401u, 0x0002101u, 0x0000000u}};
// ... and the number alone, a nibble per mask: 0 1 1 2 1 2 2 1 1 2 2 1 2 1 1 0
constexpr unsigned long long kTetCount = 0x0112122112212110ull;
// the cube corners (dx + 2 dy + 4 dz) of vertices v1 and v2 of tetrahedron k, a nibble each; v0 = 0, v3 = 7
constexpr uint32_t kTetV1 = 0x442211u, kTetV2 = 0x656353u;
constexpr uint32_t kTetMirror = 0x26u;             // bit k: tetrahedron k takes row 1
constexpr uint32_t kEdgeLo = 0x211000u, kEdgeHi = 0x332321u;   // the two vertices of edge e, a nibble each

// what the kernels take of a MeshLaunch
struct MeshArgs {
    float iso;
    uint32_t lo[3], hi[3];
    uint32_t b0[3], nb[3];
    int cell_shift, cell_cx, cell_cy;
};

// the block of this workgroup: its coordinates in the volume's block grid
VR_DEV void mesh_block_of(const MeshArgs &a, uint32_t &bx, uint32_t &by, uint32_t &bz)
{
    const uint32_t b = blockIdx.x, row = a.nb[0] * a.nb[1];
    const uint32_t z = b / row, rem = b - z * row, y = rem / a.nb[0];
    bx = a.b0[0] + (rem - y * a.nb[0]);
    by = a.b0[1] + y;
    bz = a.b0[2] + z;
}

// the block's 9^3 normalised point values, x fastest; points beyond the volume repeat its last plane (no cube of
// the region reads them)
template <typename VT>
VR_DEV void mesh_stage_block(const Vol<VT, 0, false> &vol, uint32_t bx, uint32_t by, uint32_t bz, float *s_val)
{
    for (uint32_t i = threadIdx.x; i < kMeshPoints; i += 64u) {
        const uint32_t lz = i / (kMP * kMP), r = i - lz * (kMP * kMP), ly = r / kMP, lx = r - ly * kMP;
        const int x = min((int)(bx * kMB + lx), vol.w1), y = min((int)(by * kMB + ly), vol.h1);
        const int z = min((int)(bz * kMB + lz), vol.d1);
        s_val[i] = vol.raw(vol.xoff(x), vol.yoff(y), vol.zoff(z), x, y, z) * vol.inv_max;
    }
    __syncthreads();
}

VR_DEV uint32_t mesh_point_offset(uint32_t corner)   // of cube corner dx + 2 dy + 4 dz from the cube's corner 0, in s_val
{
    return (corner & 1u) + kMP * ((corner >> 1) & 1u) + kMP * kMP * (corner >> 2);
}

// the inside mask of cube (lx, ly, lz) of the staged block, bit = corner; 0 for a cube outside the region
VR_DEV uint32_t mesh_cube_mask(const MeshArgs &a, const float *s_val, uint32_t bx, uint32_t by, uint32_t bz, uint32_t lx,
                               uint32_t ly, uint32_t lz)
{
    const uint32_t gx = bx * kMB + lx, gy = by * kMB + ly, gz = bz * kMB + lz;
    const bool in_region = gx >= a.lo[0] && gx < a.hi[0] && gy >= a.lo[1] && gy < a.hi[1] && gz >= a.lo[2] && gz < a.hi[2];
    if (!in_region) return 0u;
    const float *c0 = s_val + (lx + kMP * (ly + kMP * lz));
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) m |= (c0[mesh_point_offset(j)] >= a.iso ? 1u : 0u) << j;   // (false for a NaN)
    return m;
}

VR_DEV uint32_t mesh_tet_mask(uint32_t cube_mask, uint32_t k)
{
    const uint32_t v1 = (kTetV1 >> (4u * k)) & 15u, v2 = (kTetV2 >> (4u * k)) & 15u;
    return (cube_mask & 1u) | (((cube_mask >> v1) & 1u) << 1) | (((cube_mask >> v2) & 1u) << 2) | ((cube_mask >> 7) << 3);
}

VR_DEV uint32_t mesh_cube_count(uint32_t cube_mask)
{
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) n += (uint32_t)(kTetCount >> (4u * mesh_tet_mask(cube_mask, k))) & 15u;
    return n;
}

template <typename VT>
__global__ __launch_bounds__(64) void vr_mesh_count_kernel(VolView vv, MeshArgs a, const float2 *__restrict__ cell_mm,
                                                           uint32_t *__restrict__ counts)
{
    __shared__ float s_val[kMeshPoints];
    uint32_t bx, by, bz;
    mesh_block_of(a, bx, by, bz);
    if (cell_mm) {   // (uniform: one block, one cell)
        const uint32_t cx = (bx * kMB) >> a.cell_shift, cy = (by * kMB) >> a.cell_shift, cz = (bz * kMB) >> a.cell_shift;
        const float2 mm = cell_mm[((size_t)cz * (uint32_t)a.cell_cy + cy) * (uint32_t)a.cell_cx + cx];
        if (mm.y * vv.inv_max < a.iso || mm.x * vv.inv_max >= a.iso) {
            if (threadIdx.x == 0) counts[blockIdx.x] = kMeshSkipped;
            return;
        }
    }
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    mesh_stage_block(vol, bx, by, bz, s_val);
    const uint32_t lx = threadIdx.x & 7u, ly = threadIdx.x >> 3;
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t lz = 0; lz < kMB; ++lz) n += mesh_cube_count(mesh_cube_mask(a, s_val, bx, by, bz, lx, ly, lz));
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// technique 4's shading normal at texture coordinate (px, py, pz) -- Vol::neg_gradient's six taps, difference and
// normalisation (tri_at blends the same texels with the same weights in the same order) -- with (0, 0, 0) where
// that one substitutes a constant for a zero gradient, and for a non-finite one
template <typename V>
VR_DEV f3 mesh_normal(const V &vol, float px, float py, float pz)
{
    const float ub = px * vol.fw - 0.5f, vb = py * vol.fh - 0.5f, sb = pz * vol.fd - 0.5f;
    const float fx = floorf(ub), fy = floorf(vb), fz = floorf(sb);
    const float a = ub - fx, b = vb - fy, c = sb - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    f3 s1, s2;
    s1.x = vol.tri_at(ix - 1, iy, iz, a, b, c);
    s2.x = vol.tri_at(ix + 1, iy, iz, a, b, c);
    s1.y = vol.tri_at(ix, iy - 1, iz, a, b, c);
    s2.y = vol.tri_at(ix, iy + 1, iz, a, b, c);
    s1.z = vol.tri_at(ix, iy, iz - 1, a, b, c);
    s2.z = vol.tri_at(ix, iy, iz + 1, a, b, c);
    const f3 g = sub3(s2, s1);
    const f3 n = normalize3(g);
    const float kInf = __builtin_inff();
    const bool ok = dot3(g, g) != 0.0f && fabsf(n.x) < kInf && fabsf(n.y) < kInf && fabsf(n.z) < kInf;   // (false for NaN)
    return ok ? neg3(n) : mk3(0.f, 0.f, 0.f);
}

template <typename VT, bool NORMALS>
__global__ __launch_bounds__(64) void vr_mesh_emit_kernel(VolView vv, MeshArgs a, const uint32_t *__restrict__ counts,
                                                          const unsigned long long *__restrict__ offsets,
                                                          float *__restrict__ positions, float *__restrict__ normals)
{
    __shared__ float s_val[kMeshPoints];
    const uint32_t cw = counts[blockIdx.x];
    if (cw == 0u || cw == kMeshSkipped) return;   // (uniform)
    uint32_t bx, by, bz;
    mesh_block_of(a, bx, by, bz);
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    mesh_stage_block(vol, bx, by, bz, s_val);
    const uint32_t lane = threadIdx.x, lx = lane & 7u, ly = lane >> 3;
    const float res[3] = {vol.fw, vol.fh, vol.fd};
    unsigned long long layer_base = offsets[blockIdx.x];
#pragma unroll 1
    for (uint32_t lz = 0; lz < kMB; ++lz) {
        const uint32_t cm = mesh_cube_mask(a, s_val, bx, by, bz, lx, ly, lz);
        const uint32_t n = mesh_cube_count(cm);
        uint32_t incl = n;   // the layer's inclusive sum over the lanes: lane = x + 8 y is the cubes' order
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t below = __shfl_up(incl, d, 64);
            if (lane >= d) incl += below;
        }
        unsigned long long tri = layer_base + (unsigned long long)(incl - n);
        layer_base += (unsigned long long)__shfl(incl, 63, 64);
        if (n != 0u) {   // (the shuffles above are the whole wave's)
            const float *c0 = s_val + (lx + kMP * (ly + kMP * lz));
            const uint32_t corner0[3] = {bx * kMB + lx, by * kMB + ly, bz * kMB + lz};
#pragma unroll 1
            for (uint32_t k = 0; k < 6u; ++k) {
                const uint32_t w = kTetTriangles[(kTetMirror >> k) & 1u][mesh_tet_mask(cm, k)];
                // the tetrahedron's vertices as cube corners, a nibble each
                const uint32_t tc = (((kTetV1 >> (4u * k)) & 15u) << 4) | (((kTetV2 >> (4u * k)) & 15u) << 8) | (7u << 12);
                const uint32_t nv = 3u * (w & 15u);
#pragma unroll 1
                for (uint32_t v = 0; v < nv; ++v) {
                    const uint32_t e = (w >> (4u + 4u * v)) & 15u;
                    const uint32_t cp = (tc >> (4u * ((kEdgeLo >> (4u * e)) & 15u))) & 15u;
                    const uint32_t cq = (tc >> (4u * ((kEdgeHi >> (4u * e)) & 15u))) & 15u;
                    const float sp = c0[mesh_point_offset(cp)], sq = c0[mesh_point_offset(cq)];
                    float t = (a.iso - sp) / (sq - sp);
                    if (!(t >= 0.f)) t = 0.f;
                    if (t > 1.f) t = 1.f;
                    float p[3];
    #pragma unroll
                    for (uint32_t ax = 0; ax < 3u; ++ax) {
                        const uint32_t pa = corner0[ax] + ((cp >> ax) & 1u), da = ((cq >> ax) & 1u) - ((cp >> ax) & 1u);
                        const float g = (float)pa + (float)da * t;
                        p[ax] = (g + 0.5f) / res[ax] * 2.f - 1.f;
                    }
                    const size_t o = (size_t)(tri + v / 3u) * 9u + (size_t)(v % 3u) * 3u;
                    positions[o] = p[0];
                    positions[o + 1] = p[1];
                    positions[o + 2] = p[2];
                    if constexpr (NORMALS) {
                        const f3 nrm = mesh_normal(vol, p[0] * 0.5f + 0.5f, p[1] * 0.5f + 0.5f, p[2] * 0.5f + 0.5f);
                        normals[o] = nrm.x;
                        normals[o + 1] = nrm.y;
                        normals[o + 2] = nrm.z;
                    }
                }
                tri += (unsigned long long)(w & 15u);
            }
        }
    }
}

// ---- the prefix sum of the count words

constexpr uint32_t kScanThreads = 256, kScanPerThread = kMeshScanChunk / kScanThreads;   // 16 words a thread

// exclusive sum of v over the workgroup's kScanThreads threads and its total; s_w: 4 words of LDS
VR_DEV unsigned long long scan_workgroup(unsigned long long v, unsigned long long *s_w, unsigned long long &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long below = __shfl_up(incl, d, 64);
        if (lane >= d) incl += below;
    }
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    unsigned long long base = 0;
    total = 0;
    for (uint32_t k = 0; k < kScanThreads / 64u; ++k) {
        base += k < wave ? s_w[k] : 0ull;
        total += s_w[k];
    }
    __syncthreads();   // (s_w may be written again)
    return base + incl - v;
}

// partials[2 c], [2 c + 1]: the triangles and the skipped blocks of chunk c
__global__ __launch_bounds__(kScanThreads) void vr_mesh_scan_reduce_kernel(const uint32_t *__restrict__ counts, size_t n,
                                                                           unsigned long long *__restrict__ partials)
{
    __shared__ unsigned long long s_w[4];
    const size_t i0 = (size_t)blockIdx.x * kMeshScanChunk + (size_t)threadIdx.x * kScanPerThread;
    unsigned long long tris = 0, skipped = 0;
    for (uint32_t k = 0; k < kScanPerThread; ++k)
        if (i0 + k < n) {
            const uint32_t c = counts[i0 + k];
            tris += c & ~kMeshSkipped;
            skipped += c >> 31;
        }
    unsigned long long total_t, total_s;
    (void)scan_workgroup(tris, s_w, total_t);
    (void)scan_workgroup(skipped, s_w, total_s);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = total_t;
        partials[2 * (size_t)blockIdx.x + 1] = total_s;
    }
}

// one workgroup: partials[2 c] becomes the triangles before chunk c; the totals go behind the n_partials pairs
__global__ __launch_bounds__(kScanThreads) void vr_mesh_scan_partials_kernel(unsigned long long *partials, size_t n_partials)
{
    __shared__ unsigned long long s_w[4];
    unsigned long long carry_t = 0, carry_s = 0;
    for (size_t base = 0; base < n_partials; base += kScanThreads) {   // (uniform)
        const size_t c = base + threadIdx.x;
        const unsigned long long t = c < n_partials ? partials[2 * c] : 0ull, s = c < n_partials ? partials[2 * c + 1] : 0ull;
        unsigned long long total_t, total_s;
        const unsigned long long excl = scan_workgroup(t, s_w, total_t);
        (void)scan_workgroup(s, s_w, total_s);
        if (c < n_partials) partials[2 * c] = carry_t + excl;
        carry_t += total_t;
        carry_s += total_s;
    }
    if (threadIdx.x == 0) {
        partials[2 * n_partials] = carry_t;
        partials[2 * n_partials + 1] = carry_s;
    }
}

// offsets[i]: the triangles before block i
__global__ __launch_bounds__(kScanThreads) void vr_mesh_scan_apply_kernel(const uint32_t *__restrict__ counts, size_t n,
                                                                          const unsigned long long *__restrict__ partials,
                                                                          unsigned long long *__restrict__ offsets)
{
    __shared__ unsigned long long s_w[4];
    const size_t i0 = (size_t)blockIdx.x * kMeshScanChunk + (size_t)threadIdx.x * kScanPerThread;
    unsigned long long mine = 0;
    for (uint32_t k = 0; k < kScanPerThread; ++k)
        if (i0 + k < n) mine += counts[i0 + k] & ~kMeshSkipped;
    unsigned long long total;
    unsigned long long at = partials[2 * (size_t)blockIdx.x] + scan_workgroup(mine, s_w, total);
    for (uint32_t k = 0; k < kScanPerThread; ++k)
        if (i0 + k < n) {
            offsets[i0 + k] = at;
            at += counts[i0 + k] & ~kMeshSkipped;
        }
}

// ---- the indexed extraction (vrhip_isosurface_count_indexed / _extract_indexed): one vertex per
// eligible crossed lattice edge (P, d), numbered by point block, point and d, and the soup's triangles as indices.
// One wave per block of 8^3 grid points, which owns the edges that start at them; all seven reach no further than
// the 9^3 points mesh_stage_block stages.
//  * vr_mesh_vertex_count_kernel: the cell test of pass 1 (the cell answers for the very points 8 b .. 8 b + 8), then
//    lane (x, y) walks z and sums the popcounts of its points' edge masks; the block's count word and a word that
//    says whether it holds a vertex.  Both are scanned by vr_mesh_scan_*: a vertex offset and a table slot per block.
//  * vr_mesh_vertex_emit_kernel: the layer loop of pass 2 over points; every vertex (and normal) is written once.
//    A block that holds a vertex also leaves its rank table at its slot: per row of eight points (row = y + 8 z)
//    the eight 7-bit masks as the bytes of one 64-bit word and the number of the row's first vertex, 32 bits,
//    the block's offset included: kMeshTableBytes = 64 * (8 + 4) = 768 bytes a block.
//  * vr_mesh_index_emit_kernel: pass 2 once more, with its counts and offsets, so every triangle lands at the soup's
//    place; a triangle vertex on (P, d) is row base + popcount(row masks below bit 8 x + d - 1) of P's block and row.

// the eligible crossed edges that start at point (lx, ly, lz) of the staged block: bit d - 1 for edge d = dx + 2 dy + 4 dz
VR_DEV uint32_t mesh_point_edges(const MeshArgs &a, const float *s_val, uint32_t bx, uint32_t by, uint32_t bz, uint32_t lx,
                                 uint32_t ly, uint32_t lz)
{
    const uint32_t g[3] = {bx * kMB + lx, by * kMB + ly, bz * kMB + lz};
    uint32_t closed = 0, open = 0;   // per axis: lo <= P <= hi, lo <= P < hi
#pragma unroll
    for (uint32_t ax = 0; ax < 3u; ++ax) {
        closed |= (g[ax] >= a.lo[ax] && g[ax] <= a.hi[ax] ? 1u : 0u) << ax;
        open |= (g[ax] >= a.lo[ax] && g[ax] < a.hi[ax] ? 1u : 0u) << ax;
    }
    if (closed != 7u) return 0u;
    const float *c0 = s_val + (lx + kMP * (ly + kMP * lz));
    const bool in0 = c0[0] >= a.iso;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t d = 1; d < 8u; ++d)
        m |= ((d & ~open) == 0u && (c0[mesh_point_offset(d)] >= a.iso) != in0 ? 1u : 0u) << (d - 1u);
    return m;
}

template <typename VT>
__global__ __launch_bounds__(64) void vr_mesh_vertex_count_kernel(VolView vv, MeshArgs a, const float2 *__restrict__ cell_mm,
                                                                  uint32_t *__restrict__ vcounts, uint32_t *__restrict__ vflags)
{
    __shared__ float s_val[kMeshPoints];
    uint32_t bx, by, bz;
    mesh_block_of(a, bx, by, bz);
    // the one block of the launch that owns no eligible edge -- its only point of the region is (hi, hi, hi) -- is
    // not one of the contract's point blocks: no vertex, and not skipped either
    if (bx * kMB == a.hi[0] && by * kMB == a.hi[1] && bz * kMB == a.hi[2]) {   // (uniform)
        if (threadIdx.x == 0) vcounts[blockIdx.x] = vflags[blockIdx.x] = 0u;
        return;
    }
    if (cell_mm) {   // (uniform: one block, one cell)
        const uint32_t cx = (bx * kMB) >> a.cell_shift, cy = (by * kMB) >> a.cell_shift, cz = (bz * kMB) >> a.cell_shift;
        const float2 mm = cell_mm[((size_t)cz * (uint32_t)a.cell_cy + cy) * (uint32_t)a.cell_cx + cx];
        if (mm.y * vv.inv_max < a.iso || mm.x * vv.inv_max >= a.iso) {
            if (threadIdx.x == 0) {
                vcounts[blockIdx.x] = kMeshSkipped;
                vflags[blockIdx.x] = 0u;
            }
            return;
        }
    }
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    mesh_stage_block(vol, bx, by, bz, s_val);
    const uint32_t lx = threadIdx.x & 7u, ly = threadIdx.x >> 3;
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t lz = 0; lz < kMB; ++lz) n += (uint32_t)__popc(mesh_point_edges(a, s_val, bx, by, bz, lx, ly, lz));
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if (threadIdx.x == 0) {
        vcounts[blockIdx.x] = n;
        vflags[blockIdx.x] = n != 0u ? 1u : 0u;
    }
}

template <typename VT, bool NORMALS>
__global__ __launch_bounds__(64) void vr_mesh_vertex_emit_kernel(VolView vv, MeshArgs a, const uint32_t *__restrict__ vcounts,
                                                                 const unsigned long long *__restrict__ voffsets,
                                                                 const unsigned long long *__restrict__ slots,
                                                                 float *__restrict__ vertices, float *__restrict__ normals,
                                                                 unsigned long long *__restrict__ row_masks,
                                                                 uint32_t *__restrict__ row_bases)
{
    __shared__ float s_val[kMeshPoints];
    const uint32_t cw = vcounts[blockIdx.x];
    if (cw == 0u || cw == kMeshSkipped) return;   // (uniform)
    uint32_t bx, by, bz;
    mesh_block_of(a, bx, by, bz);
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    mesh_stage_block(vol, bx, by, bz, s_val);
    const uint32_t lane = threadIdx.x, lx = lane & 7u, ly = lane >> 3;
    const float res[3] = {vol.fw, vol.fh, vol.fd};
    const size_t table = (size_t)slots[blockIdx.x] * kMeshTableRows;
    uint8_t *mask_bytes = reinterpret_cast<uint8_t *>(row_masks + table);   // byte x of row y + 8 z: at 64 z + lane
    uint32_t layer_base = (uint32_t)voffsets[blockIdx.x];   // (the host refuses more than 2^32 - 1 vertices)
#pragma unroll 1
    for (uint32_t lz = 0; lz < kMB; ++lz) {
        const uint32_t m = mesh_point_edges(a, s_val, bx, by, bz, lx, ly, lz);
        const uint32_t n = (uint32_t)__popc(m);
        uint32_t incl = n;   // the layer's inclusive sum over the lanes: lane = x + 8 y is the points' order
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t below = __shfl_up(incl, d, 64);
            if (lane >= d) incl += below;
        }
        uint32_t vtx = layer_base + (incl - n);
        layer_base += __shfl(incl, 63, 64);
        mask_bytes[64u * lz + lane] = (uint8_t)m;
        if (lx == 0u) row_bases[table + ly + kMB * lz] = vtx;
        if (m != 0u) {   // (the shuffles above are the whole wave's)
            const float *c0 = s_val + (lx + kMP * (ly + kMP * lz));
            const uint32_t p0[3] = {bx * kMB + lx, by * kMB + ly, bz * kMB + lz};
            const float sp = c0[0];
#pragma unroll 1
            for (uint32_t rest = m; rest != 0u; rest &= rest - 1u, ++vtx) {
                const uint32_t d = (uint32_t)__ffs((int)rest);   // (bit d - 1)
                const float sq = c0[mesh_point_offset(d)];
                float t = (a.iso - sp) / (sq - sp);
                if (!(t >= 0.f)) t = 0.f;
                if (t > 1.f) t = 1.f;
                float p[3];
#pragma unroll
                for (uint32_t ax = 0; ax < 3u; ++ax) {
                    const float g = (float)p0[ax] + (float)((d >> ax) & 1u) * t;
                    p[ax] = (g + 0.5f) / res[ax] * 2.f - 1.f;
                }
                const size_t o = (size_t)vtx * 3u;
                vertices[o] = p[0];
                vertices[o + 1] = p[1];
                vertices[o + 2] = p[2];
                if constexpr (NORMALS) {
                    const f3 nrm = mesh_normal(vol, p[0] * 0.5f + 0.5f, p[1] * 0.5f + 0.5f, p[2] * 0.5f + 0.5f);
                    normals[o] = nrm.x;
                    normals[o + 1] = nrm.y;
                    normals[o + 2] = nrm.z;
                }
            }
        }
    }
}

// pnx, pny: the point blocks per row and column of the launch (the grid of slots)
template <typename VT>
__global__ __launch_bounds__(64) void vr_mesh_index_emit_kernel(VolView vv, MeshArgs a, uint32_t pnx, uint32_t pny,
                                                                const uint32_t *__restrict__ counts,
                                                                const unsigned long long *__restrict__ offsets,
                                                                const unsigned long long *__restrict__ slots,
                                                                const unsigned long long *__restrict__ row_masks,
                                                                const uint32_t *__restrict__ row_bases,
                                                                uint32_t *__restrict__ indices)
{
    __shared__ float s_val[kMeshPoints];
    const uint32_t cw = counts[blockIdx.x];
    if (cw == 0u || cw == kMeshSkipped) return;   // (uniform)
    uint32_t bx, by, bz;
    mesh_block_of(a, bx, by, bz);
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    mesh_stage_block(vol, bx, by, bz, s_val);
    const uint32_t lane = threadIdx.x, lx = lane & 7u, ly = lane >> 3;
    unsigned long long layer_base = offsets[blockIdx.x];
#pragma unroll 1
    for (uint32_t lz = 0; lz < kMB; ++lz) {
        const uint32_t cm = mesh_cube_mask(a, s_val, bx, by, bz, lx, ly, lz);
        const uint32_t n = mesh_cube_count(cm);
        uint32_t incl = n;   // as pass 2
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t below = __shfl_up(incl, d, 64);
            if (lane >= d) incl += below;
        }
        unsigned long long tri = layer_base + (unsigned long long)(incl - n);
        layer_base += (unsigned long long)__shfl(incl, 63, 64);
        if (n != 0u) {
            const uint32_t corner0[3] = {bx * kMB + lx, by * kMB + ly, bz * kMB + lz};
#pragma unroll 1
            for (uint32_t k = 0; k < 6u; ++k) {
                const uint32_t w = kTetTriangles[(kTetMirror >> k) & 1u][mesh_tet_mask(cm, k)];
                const uint32_t tc = (((kTetV1 >> (4u * k)) & 15u) << 4) | (((kTetV2 >> (4u * k)) & 15u) << 8) | (7u << 12);
                const uint32_t nv = 3u * (w & 15u);
#pragma unroll 1
                for (uint32_t v = 0; v < nv; ++v) {
                    const uint32_t e = (w >> (4u + 4u * v)) & 15u;
                    const uint32_t cp = (tc >> (4u * ((kEdgeLo >> (4u * e)) & 15u))) & 15u;
                    const uint32_t cq = (tc >> (4u * ((kEdgeHi >> (4u * e)) & 15u))) & 15u;
                    // the edge (P, d): P = corner 0 + cp, d = cq - cp (cp's bits are among cq's)
                    const uint32_t px = corner0[0] + (cp & 1u), py = corner0[1] + ((cp >> 1) & 1u), pz = corner0[2] + (cp >> 2);
                    const uint32_t d = cq ^ cp;
                    const size_t pb = ((size_t)(pz / kMB - a.b0[2]) * pny + (py / kMB - a.b0[1])) * pnx + (px / kMB - a.b0[0]);
                    const size_t row = (size_t)slots[pb] * kMeshTableRows + ((py & 7u) + kMB * (pz & 7u));
                    const unsigned long long before = (1ull << (8u * (px & 7u) + d - 1u)) - 1ull;
                    indices[(size_t)(tri + v / 3u) * 3u + (size_t)(v % 3u)] = row_bases[row] + (uint32_t)__popcll(row_masks[row] & before);
                }
                tri += (unsigned long long)(w & 15u);
            }
        }
    }
}

MeshArgs mesh_args(const MeshLaunch &a)
{
    MeshArgs m;
    m.iso = a.iso;
    for (int i = 0; i < 3; ++i) { m.lo[i] = a.lo[i]; m.hi[i] = a.hi[i]; m.b0[i] = a.b0[i]; m.nb[i] = a.nb[i]; }
    m.cell_shift = a.cell_shift;
    m.cell_cx = a.cell_cx;
    m.cell_cy = a.cell_cy;
    return m;
}

// the launch's blocks as a grid size; 0: none, or more than a grid holds
uint32_t mesh_grid(const MeshLaunch &a)
{
    const unsigned long long n = (unsigned long long)a.nb[0] * a.nb[1] * a.nb[2];
    return n < 0x7fffffffull ? (uint32_t)n : 0u;
}

} // namespace

hipError_t vr_launch_mesh_count(const MeshLaunch &a, uint32_t *counts, hipStream_t stream)
{
    const uint32_t grid = mesh_grid(a);
    if (grid == 0) return hipErrorInvalidValue;
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        hipLaunchKernelGGL((vr_mesh_count_kernel<VT>), dim3(grid), dim3(64), 0, stream, a.vol, mesh_args(a), a.cell_minmax,
                           counts);
        return hipGetLastError();
    });
}

hipError_t vr_launch_mesh_scan(const uint32_t *counts, size_t n_blocks, unsigned long long *partials,
                               unsigned long long *offsets, hipStream_t stream)
{
    const size_t np = vr_mesh_scan_partials(n_blocks);
    if (np == 0 || np >= 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vr_mesh_scan_reduce_kernel, dim3((uint32_t)np), dim3(kScanThreads), 0, stream, counts, n_blocks,
                       partials);
    hipLaunchKernelGGL(vr_mesh_scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, stream, partials, np);
    if (offsets)
        hipLaunchKernelGGL(vr_mesh_scan_apply_kernel, dim3((uint32_t)np), dim3(kScanThreads), 0, stream, counts, n_blocks,
                           partials, offsets);
    return hipGetLastError();
}

hipError_t vr_launch_mesh_emit(const MeshLaunch &a, const uint32_t *counts, const unsigned long long *offsets,
                               float *positions, float *normals, hipStream_t stream)
{
    const uint32_t grid = mesh_grid(a);
    if (grid == 0 || !positions) return hipErrorInvalidValue;
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        if (normals)
            hipLaunchKernelGGL((vr_mesh_emit_kernel<VT, true>), dim3(grid), dim3(64), 0, stream, a.vol, mesh_args(a), counts,
                               offsets, positions, normals);
        else
            hipLaunchKernelGGL((vr_mesh_emit_kernel<VT, false>), dim3(grid), dim3(64), 0, stream, a.vol, mesh_args(a), counts,
                               offsets, positions, normals);
        return hipGetLastError();
    });
}

// ---- the indexed extraction's launches

namespace {

// the launch over the point blocks: b0 as the cubes', one block more on an axis whose hi is a multiple of the block
MeshArgs mesh_point_args(const MeshLaunch &a, uint32_t *grid)
{
    MeshArgs m = mesh_args(a);
    vr_mesh_point_blocks(a, m.nb);
    const unsigned long long n = (unsigned long long)m.nb[0] * m.nb[1] * m.nb[2];
    *grid = n < 0x7fffffffull ? (uint32_t)n : 0u;
    return m;
}

} // namespace

hipError_t vr_launch_mesh_vertex_count(const MeshLaunch &a, uint32_t *vcounts, uint32_t *vflags, hipStream_t stream)
{
    uint32_t grid;
    const MeshArgs m = mesh_point_args(a, &grid);
    if (grid == 0) return hipErrorInvalidValue;
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        hipLaunchKernelGGL((vr_mesh_vertex_count_kernel<VT>), dim3(grid), dim3(64), 0, stream, a.vol, m, a.cell_minmax, vcounts,
                           vflags);
        return hipGetLastError();
    });
}

hipError_t vr_launch_mesh_vertex_emit(const MeshLaunch &a, const uint32_t *vcounts, const unsigned long long *voffsets,
                                      const unsigned long long *slots, float *vertices, float *normals,
                                      unsigned long long *row_masks, uint32_t *row_bases, hipStream_t stream)
{
    uint32_t grid;
    const MeshArgs m = mesh_point_args(a, &grid);
    if (grid == 0 || !vertices || !row_masks || !row_bases) return hipErrorInvalidValue;
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        if (normals)
            hipLaunchKernelGGL((vr_mesh_vertex_emit_kernel<VT, true>), dim3(grid), dim3(64), 0, stream, a.vol, m, vcounts,
                               voffsets, slots, vertices, normals, row_masks, row_bases);
        else
            hipLaunchKernelGGL((vr_mesh_vertex_emit_kernel<VT, false>), dim3(grid), dim3(64), 0, stream, a.vol, m, vcounts,
                               voffsets, slots, vertices, normals, row_masks, row_bases);
        return hipGetLastError();
    });
}

hipError_t vr_launch_mesh_index_emit(const MeshLaunch &a, const uint32_t *counts, const unsigned long long *offsets,
                                     const unsigned long long *slots, const unsigned long long *row_masks,
                                     const uint32_t *row_bases, uint32_t *indices, hipStream_t stream)
{
    const uint32_t grid = mesh_grid(a);
    if (grid == 0 || !indices) return hipErrorInvalidValue;
    uint32_t pnb[3];
    vr_mesh_point_blocks(a, pnb);
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        hipLaunchKernelGGL((vr_mesh_index_emit_kernel<VT>), dim3(grid), dim3(64), 0, stream, a.vol, mesh_args(a), pnb[0], pnb[1],
                           counts, offsets, slots, row_masks, row_bases, indices);
        return hipGetLastError();
    });
}
