// vr_filter.hip -- volume filters (vrhip_filter_volume, include/vrhip.h "volume filters"): the kernel that filters the
// blocks of 8^3 voxels of one time step into another micro-bricked volume, instantiated per voxel type and per kind
// (separable smoothing, 3x3x3 median), and its launch entry.  Not a technique: it writes a time step.
//
// Definition (tests/ref/filter_ref.c restates it on the CPU): s = fl(raw * inv_max), neighbours
// clamped to the volume; SEPARABLE: three passes x, y, z, acc = w[0] f(p), acc = acc + w[k] (f(p - k) + f(p + k)) for
// k ascending; MEDIAN3: the 14th smallest of 27 integer keys; the store of the header.
//
// Execution: a workgroup of four waves takes blocks b = blockIdx.x, + gridDim.x, ... (x fastest), one at a time:
//  * the coarse cells that cover the block dilated by the radii, when the cell grid is handed over, may prove the
//    block constant (below); then the constant is written and nothing is fetched;
//  * else the block's values with a halo of radius[a] voxels per axis, coordinates clamped to the volume, go to LDS
//    once: S, (8 + 2 Rx)(8 + 2 Ry)(8 + 2 Rz) words, x fastest.  That is the one read of the source;
//  * the x pass runs on the (8 + 2 Rz)(8 + 2 Ry) rows of S and leaves A, 8 (8 + 2 Ry)(8 + 2 Rz) words; the y pass on
//    the 8 + 2 Rz slabs of A and leaves B, 8 * 8 (8 + 2 Rz) words, where S was (S is dead by then); the z pass on B
//    gives the 512 results.  The halo shrinks per pass, no intermediate leaves LDS.  A value of A or B at a clamped
//    position is the pass's result on the clamped rows of S: the full-field passes compute the same, since the field
//    of a pass at a position clamped in y or z is the pass on the same clamped row.
//  * thread t stores results t and t + 256 in micro-brick order (vr_voxel_index): a wave writes one micro-brick, 64
//    consecutive voxels.  Voxels of an existing micro-brick beyond the volume are written as 0, as an upload does.
//  * MEDIAN3 stages keys with a halo of 1 (10^3 words) and every thread selects two medians in registers with a
//    fixed network of min / max exchanges (below).
// The radii are uniform; the taps are read from the kernel's arguments with constant indices (the tap loops are
// unrolled with a uniform exit), so they stay in scalar registers.  Divisions by the halo sizes are multiplications
// by constants of the launch (i * d < 2^32: exact).
//
// The skips are exact.  The cells are 2^shift >= 8 voxels wide and their (min, max) cover at least their own voxels
// (vr_cells.hip: a halo of one more).  The voxels a block's results read are those of the block dilated by the radii
// and clamped to the volume; where all the cells that hold one of them have the one finite min == max == c, every
// value read is c (FLOAT: a zero of either sign for c == 0).
//  * SEPARABLE, c == 0: s = +-0, every product w[k] * (+-0 + +-0) is a zero (the taps are finite), every sum of
//    zeros is a zero, and a zero is stored as +0 (UCHAR / USHORT: q = +-0 -> 0).
//  * MEDIAN3: the 14th of 27 equal raw values is that value; for FLOAT and c == 0 the keys are those of +0 or -0
//    and either is stored as +0.
//  * a cell with a NaN voxel holds (-inf, +inf): not constant.
#include "vr_sampling.h"

namespace {

constexpr uint32_t kFB = VRHIP_MESH_BLOCK;   // voxels per block and axis
static_assert(kFB == 8u, "two micro-bricks per axis, 512 results for 256 threads");
constexpr uint32_t kFilterThreads = 256;
constexpr uint32_t kMaxR = VRHIP_FILTER_MAX_RADIUS;

// what the kernel takes of a FilterLaunch
struct FilterArgs {
    uint32_t nb[3], n_blocks;       // the block grid
    uint32_t R[3], P[3];            // radii and staged values per axis, 8 + 2 R
    uint32_t magic_px, magic_py;    // floor(2^32 / P) + 1: i / P = umulhi(i, magic) for i * P < 2^32
    float taps[3][kMaxR + 1];
    int cell_shift, cell_cx, cell_cy;
};

template <typename VT> struct FilterMax;
template <> struct FilterMax<uint8_t> { static constexpr float v = 255.f; };
template <> struct FilterMax<uint16_t> { static constexpr float v = 65535.f; };

// order-preserving key of a FLOAT voxel's word; every NaN above +inf
VR_DEV uint32_t filter_key(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u;
}
// ... and the word stored for a key: a NaN as 0x7fc00000, -0 as +0
VR_DEV uint32_t filter_unkey(uint32_t key)
{
    if (key == 0xffffffffu) return 0x7fc00000u;
    const uint32_t bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    return bits == 0x80000000u ? 0u : bits;
}

// the stored voxel of a SEPARABLE result
template <typename VT>
VR_DEV VT filter_store(float c)
{
    if constexpr (sizeof(VT) == 4) {
        uint32_t bits = __float_as_uint(c);
        if (c != c) bits = 0x7fc00000u;
        else if (c == 0.f) bits = 0u;
        return __uint_as_float(bits);
    } else {
        float q = c * FilterMax<VT>::v;
        q = q > 0.f ? q : 0.f;
        q = q < FilterMax<VT>::v ? q : FilterMax<VT>::v;
        return (VT)(uint32_t)rintf(q);
    }
}

// one pass at a point: f[0] the point, `stride` words between neighbours along the pass's axis
VR_DEV float filter_pass(const float *f, int stride, uint32_t R, const float (&w)[kMaxR + 1])
{
    float acc = w[0] * f[0];
#pragma unroll
    for (uint32_t k = 1; k <= kMaxR; ++k) {
        if (k > R) break;   // (uniform)
        acc = acc + w[k] * (f[-(int)k * stride] + f[(int)k * stride]);
    }
    return acc;
}

VR_DEV void filter_cx(uint32_t &a, uint32_t &b)
{
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// The 14th smallest of 27 keys.  Of n keys the smallest has n - 1 keys at or above it: with n >= 15 it is not the
// 14th of 27, and neither is the largest.  So: 15 keys, drop their minimum and maximum, add the next key, and so on
// down to three keys, whose middle one is the median.  Stage s works on v[s .. 14]: exchanges move the minimum to
// v[s] and the maximum to v[14], then v[14] takes key 15 + s.  Fixed indices: everything stays in registers.
VR_DEV uint32_t filter_median27(uint32_t (&v)[27])
{
#pragma unroll
    for (int s = 0; s < 13; ++s) {
        const int lo = s, hi = 14, n = hi - lo + 1;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) filter_cx(v[lo + i], v[hi - i]);   // minimum in the lower half, maximum in the upper
#pragma unroll
        for (int i = 1; i <= (n - 1) / 2; ++i) filter_cx(v[lo], v[lo + i]);
#pragma unroll
        for (int i = n / 2; i < n - 1; ++i) filter_cx(v[lo + i], v[hi]);
        if (s < 12) v[hi] = v[15 + s];
    }
    return v[13];
}

// result o (0 .. 511) in micro-brick order: micro-brick (o >> 6) of the block's 2 x 2 x 2, voxel (o & 63) of it
VR_DEV void filter_result_pos(uint32_t o, uint32_t &x, uint32_t &y, uint32_t &z)
{
    const uint32_t mb = o >> 6, in = o & 63u;
    x = ((mb & 1u) << 2) + (in & 3u);
    y = (((mb >> 1) & 1u) << 2) + ((in >> 2) & 3u);
    z = ((mb >> 2) << 2) + (in >> 4);
}

template <typename VT, bool MEDIAN>
__global__ __launch_bounds__(kFilterThreads) void vr_filter_kernel(VolView vv, FilterArgs a, const float2 *__restrict__ cell_mm,
                                                                   VT *__restrict__ dst, unsigned long long *__restrict__ counters)
{
    extern __shared__ float s_lds[];   // S (then B) and behind it A
    const uint32_t PX = a.P[0], PY = a.P[1], PZ = a.P[2];
    const uint32_t n_s = PX * PY * PZ;
    float *s_S = s_lds, *s_A = s_lds + n_s, *s_B = s_lds;
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    const float kInf = __builtin_inff();
    uint32_t c_fetched = 0, c_skipped = 0;   // (uniform)
    const uint32_t row = a.nb[0] * a.nb[1];
#pragma unroll 1
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const uint32_t bz = b / row, rem = b - bz * row, by = rem / a.nb[0], bx = rem - by * a.nb[0];
        const uint32_t blk[3] = {bx, by, bz};
        const int res1[3] = {vol.w1, vol.h1, vol.d1};
        bool skip = false;
        float cst = 0.f;
        if (cell_mm) {   // (uniform) every cell that holds a voxel the block's results read
            uint32_t c0[3], c1[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const int lo = max((int)(blk[ax] * kFB) - (int)a.R[ax], 0);
                const int hi = min((int)(blk[ax] * kFB + kFB - 1u + a.R[ax]), res1[ax]);
                c0[ax] = (uint32_t)lo >> a.cell_shift;
                c1[ax] = (uint32_t)hi >> a.cell_shift;
            }
            const float2 first = cell_mm[((size_t)c0[2] * (uint32_t)a.cell_cy + c0[1]) * (uint32_t)a.cell_cx + c0[0]];
            cst = first.x;
            skip = first.x == first.y && fabsf(first.x) < kInf && (MEDIAN || first.x == 0.f);
            for (uint32_t cz = c0[2]; skip && cz <= c1[2]; ++cz)
                for (uint32_t cy = c0[1]; skip && cy <= c1[1]; ++cy)
                    for (uint32_t cx = c0[0]; skip && cx <= c1[0]; ++cx) {
                        const float2 mm = cell_mm[((size_t)cz * (uint32_t)a.cell_cy + cy) * (uint32_t)a.cell_cx + cx];
                        skip = mm.x == cst && mm.y == cst;
                    }
        }
        VT out[2];
        if (skip) {
            ++c_skipped;
            VT v;
            if constexpr (sizeof(VT) == 4) v = cst == 0.f ? 0.f : cst;   // (a zero of either sign: +0)
            else v = (VT)(uint32_t)cst;
            out[0] = out[1] = v;
        } else {
            ++c_fetched;
            __syncthreads();   // (the previous block's reads of S / B and A are done)
            // the block's values with the halo, x fastest; coordinates clamped to the volume: the neighbour rule
            for (uint32_t i = threadIdx.x; i < n_s; i += kFilterThreads) {
                const uint32_t r = __umulhi(i, a.magic_px), px = i - r * PX;
                const uint32_t pz = __umulhi(r, a.magic_py), py = r - pz * PY;
                const int x = min(max((int)(bx * kFB + px) - (int)a.R[0], 0), vol.w1);
                const int y = min(max((int)(by * kFB + py) - (int)a.R[1], 0), vol.h1);
                const int z = min(max((int)(bz * kFB + pz) - (int)a.R[2], 0), vol.d1);
                const unsigned long long at = vol.zoff(z) + (unsigned long long)(vol.yoff(y) + vol.xoff(x));
                if constexpr (MEDIAN) {
                    uint32_t key;
                    if constexpr (sizeof(VT) == 4) key = filter_key(reinterpret_cast<const uint32_t *>(vol.p)[at]);
                    else key = (uint32_t)vol.p[at];
                    reinterpret_cast<uint32_t *>(s_S)[i] = key;
                } else
                    s_S[i] = (float)vol.p[at] * vol.inv_max;
            }
            __syncthreads();
            if constexpr (MEDIAN) {
                const uint32_t *keys = reinterpret_cast<const uint32_t *>(s_S);
#pragma unroll
                for (uint32_t k = 0; k < 2u; ++k) {
                    uint32_t x, y, z;
                    filter_result_pos(threadIdx.x + k * kFilterThreads, x, y, z);
                    uint32_t v[27];
#pragma unroll
                    for (uint32_t dz = 0; dz < 3u; ++dz)
#pragma unroll
                        for (uint32_t dy = 0; dy < 3u; ++dy)
#pragma unroll
                            for (uint32_t dx = 0; dx < 3u; ++dx)
                                v[(dz * 3u + dy) * 3u + dx] = keys[((z + dz) * 10u + (y + dy)) * 10u + (x + dx)];
                    const uint32_t m = filter_median27(v);
                    if constexpr (sizeof(VT) == 4) out[k] = __uint_as_float(filter_unkey(m));
                    else out[k] = (VT)m;
                }
            } else {
                // x: A[row][x], the rows of S
                const uint32_t n_a = kFB * PY * PZ;
                for (uint32_t j = threadIdx.x; j < n_a; j += kFilterThreads) {
                    const uint32_t x = j & 7u, rw = j >> 3;
                    s_A[j] = filter_pass(s_S + rw * PX + x + a.R[0], 1, a.R[0], a.taps[0]);
                }
                __syncthreads();
                // y: B[z][y][x], the slabs of A (B lies where S was)
                const uint32_t n_b = kFB * kFB * PZ;
                for (uint32_t j = threadIdx.x; j < n_b; j += kFilterThreads) {
                    const uint32_t x = j & 7u, y = (j >> 3) & 7u, z = j >> 6;
                    s_B[j] = filter_pass(s_A + (z * PY + y + a.R[1]) * kFB + x, (int)kFB, a.R[1], a.taps[1]);
                }
                __syncthreads();
#pragma unroll
                for (uint32_t k = 0; k < 2u; ++k) {
                    uint32_t x, y, z;
                    filter_result_pos(threadIdx.x + k * kFilterThreads, x, y, z);
                    out[k] = filter_store<VT>(
                        filter_pass(s_B + ((z + a.R[2]) * kFB + y) * kFB + x, (int)(kFB * kFB), a.R[2], a.taps[2]));
                }
            }
        }
        // the results in micro-brick order; micro-bricks beyond the grid do not exist, voxels beyond the volume are 0
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            uint32_t x, y, z;
            filter_result_pos(threadIdx.x + k * kFilterThreads, x, y, z);
            const int gx = (int)(bx * kFB + x), gy = (int)(by * kFB + y), gz = (int)(bz * kFB + z);
            if ((uint32_t)(gx >> 2) < vv.nbx && (uint32_t)(gy >> 2) < vv.nby && (uint32_t)(gz >> 2) < vv.nbz) {
                const bool in = gx <= vol.w1 && gy <= vol.h1 && gz <= vol.d1;
                dst[vr_voxel_index(vv, gx, gy, gz)] = in ? out[k] : (VT)0;
            }
        }
    }
    if (threadIdx.x == 0) {
        if (c_fetched) atomicAdd(&counters[kFilterFetched], (unsigned long long)c_fetched);
        if (c_skipped) atomicAdd(&counters[kFilterSkipped], (unsigned long long)c_skipped);
    }
}

template <typename VT, bool MEDIAN>
hipError_t filter_launch(const FilterLaunch &a, const FilterArgs &fa, void *dst, unsigned long long *counters, hipStream_t stream)
{
    // S (B fits in it: 64 <= PX * PY) and A
    const size_t lds = MEDIAN ? (size_t)1000 * sizeof(uint32_t)
                              : ((size_t)fa.P[0] * fa.P[1] * fa.P[2] + (size_t)kFB * fa.P[1] * fa.P[2]) * sizeof(float);
    int per_cu = 0;
    const hipError_t e = vr_prepare_kernel(vr_filter_kernel<VT, MEDIAN>, (int)kFilterThreads, lds, &per_cu, "filter", a.num_cus);
    if (e != hipSuccess) return e;
    const unsigned long long want = (unsigned long long)per_cu * (unsigned)(a.num_cus > 0 ? a.num_cus : 256) * 4ull;
    const uint32_t grid = (uint32_t)(fa.n_blocks < want ? fa.n_blocks : want);
    hipLaunchKernelGGL((vr_filter_kernel<VT, MEDIAN>), dim3(grid), dim3(kFilterThreads), lds, stream, a.vol, fa, a.cell_minmax,
                       static_cast<VT *>(dst), counters);
    return hipGetLastError();
}

} // namespace

hipError_t vr_launch_filter(const FilterLaunch &a, void *dst, unsigned long long *counters, hipStream_t stream)
{
    const size_t n = vr_filter_blocks(a.vol);
    if (n == 0 || n >= 0x7fffffffull || !dst || !counters || dst == a.vol.data) return hipErrorInvalidValue;
    const bool median = a.kind == VRHIP_FILTER_MEDIAN3;
    if (!median && a.kind != VRHIP_FILTER_SEPARABLE) return hipErrorInvalidValue;
    if (a.cell_minmax && a.cell_shift < 3) return hipErrorInvalidValue;
    FilterArgs fa;
    fa.nb[0] = (uint32_t)(a.vol.w + 7) / kFB;
    fa.nb[1] = (uint32_t)(a.vol.h + 7) / kFB;
    fa.nb[2] = (uint32_t)(a.vol.d + 7) / kFB;
    fa.n_blocks = (uint32_t)n;
    for (int i = 0; i < 3; ++i) {
        if (a.radius[i] > kMaxR || (median && a.radius[i] != 0u)) return hipErrorInvalidValue;
        fa.R[i] = median ? 1u : a.radius[i];
        fa.P[i] = kFB + 2u * fa.R[i];
        for (uint32_t k = 0; k <= kMaxR; ++k) fa.taps[i][k] = k <= a.radius[i] ? a.taps[i][k] : 0.f;
    }
    fa.magic_px = (uint32_t)(0x100000000ull / fa.P[0]) + 1u;
    fa.magic_py = (uint32_t)(0x100000000ull / fa.P[1]) + 1u;
    fa.cell_shift = a.cell_shift;
    fa.cell_cx = a.cell_cx;
    fa.cell_cy = a.cell_cy;
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        return median ? filter_launch<VT, true>(a, fa, dst, counters, stream)
                      : filter_launch<VT, false>(a, fa, dst, counters, stream);
    });
}
