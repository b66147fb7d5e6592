// vr_morph.hip -- grey-scale morphology (vrhip_morph_volume, include/vrhip.h "volume morphology"): the kernel that
// takes one sweep -- a minimum or a maximum over the structuring element, or their difference -- over the blocks of
// 8^3 voxels of one micro-bricked volume into another, instantiated per voxel type, shape and sweep mode, and its
// launch entry.  Not a technique: it writes a time step (or the intermediate of a two-sweep op).
//
// Definition (tests/ref/morph_ref.c restates it on the CPU): keys and element of vr_morph_math.h;
// erosion / dilation at p = the smallest / largest key over clamp(p + o), o in B; the modes are min, max, max - min
// (GRADIENT, both from one staged tile), f - max(T) (TOPHAT's second sweep: T the intermediate, f the source) and
// min(T) - f (BLACKHAT's); the store of the header.
//
// Execution: the launch shape of vr_filter.hip.  A workgroup of four waves takes blocks b = blockIdx.x, + gridDim.x,
// ... (x fastest), one at a time:
//  * the coarse cells that cover the block dilated by skip * R_a voxels per axis (skip = 1, second sweep 2), when
//    the cell grid is handed over, may prove the block constant (below); then the constant or 0 is written and
//    nothing is fetched;
//  * else the block with its halo, rounded out to whole micro-bricks -- none on an axis with R = 0, one ring for
//    R <= 4, two for R <= 8: P = 8, 16 or 24 voxels per axis -- goes to LDS once, 16 bytes per lane and load: a
//    lane takes 16 / 8 / 4 consecutive voxels of a micro-brick (UCHAR: a z slice, USHORT: two x rows, FLOAT: one x
//    row) and writes their 32-bit keys as whole x rows of four (ds_write_b128).  S[(pz * PY + py) * RS + px]; RS is
//    PX + 4 words for BALL and 28 words whatever PX for BOX, whose passes then load at constant offsets.  The keys of
//    a max sweep are complemented on the way in, so that every pass below is a minimum; the result is complemented back.
//  * a block whose staged extent leaves the volume (uniform per block) fixes up afterwards: a staged position
//    outside the volume -- a micro-brick beyond the grid, a padding voxel of a border micro-brick -- takes the voxel
//    at its clamped position, one load each.  That is the contract's clamped form; no sweep reads padding as data.
//  * BOX is separable, the halo shrinking per pass, in place in S: a thread owns a row (x pass) or a column (y pass),
//    reads its keys into registers once (morph_line), forms the eight windows there and writes them over the row's /
//    column's first eight places; the z pass reads 2 R + 1 keys per result.  GRADIENT's x pass writes the minima to
//    places 0-7 and the complemented maxima to 8-15 of the row, so y and z stay minima.
//  * BALL is the straight loop over B: per row (dy, dz) of B the run dx = -h .. h (h from vr_morph_math.h, computed
//    once per launch into LDS), both of a thread's results in one loop.  2109 LDS reads per voxel at radius 8.
//  * thread t stores results t and t + 256 in micro-brick order (a wave writes one micro-brick, 64 consecutive
//    voxels); voxels of an existing micro-brick beyond the volume are written 0, as an upload does.  The two
//    difference modes read f at the voxel they write.
//
// The skips are exact.  The cells' (min, max) are the SOURCE's, and cover at least their own voxels.  Sweep 1 reads
// the block dilated by R and clamped; where every covering cell holds one finite min == max == c, every key read is
// c's (FLOAT: a zero of either sign for c == 0, stored +0 either way), so min = max = c and max - min = 0.  Sweep 2
// reads the intermediate on the block dilated by R; each of those values was made from the source on that voxel
// dilated by R again, so constant cells over the block dilated by 2 R make the intermediate c wherever sweep 2 reads
// it, and f as well: the extreme is c and both differences are c - c = +0 for a finite c.  A cell with a NaN voxel
// holds (-inf, +inf): not constant.
#include "vr_sampling.h"
#include "vr_morph_math.h"

namespace {

constexpr uint32_t kMB = VRHIP_MESH_BLOCK;   // voxels per block and axis
static_assert(kMB == 8u, "two micro-bricks per axis, 512 results for 256 threads");
constexpr uint32_t kMorphThreads = 256;
constexpr uint32_t kMaxR = VRHIP_MORPH_MAX_RADIUS;
constexpr uint32_t kHW = 2u * kMaxR + 1u;    // the half-width table's side
constexpr uint32_t kRS = kMB + 2u * kMaxR + 4u;   // BOX: words per staged row, whatever the x halo (morph_line)
constexpr uint32_t kSlackRows = 4u;          // BOX: rows behind the tile that the y pass may load and never uses

// what the kernel takes of a MorphLaunch
struct MorphArgs {
    uint32_t nb[3], n_blocks;       // the block grid
    uint32_t R[3], H[3], P[3];      // radii, staged halo (0, 4 or 8) and staged voxels per axis, 8 + 2 H
    uint32_t RS;                    // BALL: words per staged row, PX + 4
    uint32_t n_mb, magic_mx, magic_my;   // staged micro-bricks; floor(2^32 / (P / 4)) + 1 for x and y
    uint32_t skip[3];               // the dilation of the constant test
    uint32_t shape;
    int cell_shift, cell_cx, cell_cy;
};

template <uint32_t MODE> struct ModeOf {
    static constexpr bool cmpl = MODE == kMorphMax || MODE == kMorphFMinusMax;   // a maximum: complemented keys
    static constexpr bool grad = MODE == kMorphMaxMin;
    static constexpr bool sub = MODE == kMorphFMinusMax || MODE == kMorphMinMinusF;
};

template <typename VT>
VR_DEV uint32_t morph_key(VT v)
{
    if constexpr (sizeof(VT) == 4) return morph::key_of_float(__float_as_uint(v));
    else return (uint32_t)v;
}
// the voxel stored for a key
template <typename VT>
VR_DEV VT morph_voxel(uint32_t key)
{
    if constexpr (sizeof(VT) == 4) return __uint_as_float(morph::float_of_key(key));
    else return (VT)key;
}
// the voxel stored for a - b
template <typename VT>
VR_DEV VT morph_diff(VT a, VT b)
{
    if constexpr (sizeof(VT) == 4) {
        const float c = a - b;
        uint32_t bits = __float_as_uint(c);
        if (c != c) bits = 0x7fc00000u;
        else if (c == 0.f) bits = 0u;
        return __uint_as_float(bits);
    } else
        return (VT)((uint32_t)a - (uint32_t)b);
}

// A uniform value held in a vector register from here on.  The kernel's arguments and what is derived from them would
// otherwise all stay in scalar registers across the whole block loop, more than a wave has: what only lanes compute
// with lives in vector registers instead, of which the kernel uses few.
VR_DEV uint32_t morph_in_vgpr(uint32_t x)
{
    uint32_t r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
template <typename T>
VR_DEV T *morph_in_vgpr(T *p)
{
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned long long lo = morph_in_vgpr((uint32_t)v), hi = morph_in_vgpr((uint32_t)(v >> 32));
    return reinterpret_cast<T *>(lo | (hi << 32));
}

// result o (0 .. 511) in micro-brick order: micro-brick (o >> 6) of the block's 2 x 2 x 2, voxel (o & 63) of it
VR_DEV void morph_result_pos(uint32_t o, uint32_t &x, uint32_t &y, uint32_t &z)
{
    const uint32_t mb = o >> 6, in = o & 63u;
    x = ((mb & 1u) << 2) + (in & 3u);
    y = (((mb >> 1) & 1u) << 2) + ((in >> 2) & 3u);
    z = ((mb >> 2) << 2) + (in >> 4);
}

// The eight windows of 2 R + 1 keys of a line whose first key is p[0], STRIDE words apart: the minima to
// q[0 .. 7 * STRIDE]; GRAD: the complemented maxima to q[(8 + x) ...] as well (rows only, STRIDE 1).  H is the line's
// halo class, H - 3 <= R <= H.  8 + 2 H keys are loaded at constant offsets from p -- no per-key scalar is kept --, up
// to H - R <= 3 of them past the line's end: those lie in the row's pad or in the next rows (BOX tiles have kRS-word
// rows and kSlackRows rows of slack behind them for this), and no window uses them.  Everything is read before anything is
// written.  Static indices only: the line stays in registers.
template <bool GRAD, uint32_t H, uint32_t STRIDE>
VR_DEV void morph_line(const uint32_t *p, uint32_t *q, uint32_t R)
{
    constexpr uint32_t NL = kMB + 2u * H;
    uint32_t r[NL];
#pragma unroll
    for (uint32_t j = 0; j < NL; ++j) r[j] = p[j * STRIDE];
    uint32_t mn[kMB], mx[kMB];
#pragma unroll
    for (uint32_t x = 0; x < kMB; ++x) mn[x] = mx[x] = r[x];
    if constexpr (H > 0u) {
#pragma unroll
        for (uint32_t d = 1; d <= 2u * H; ++d) {
            if (d > 2u * R) break;   // (uniform)
#pragma unroll
            for (uint32_t x = 0; x < kMB; ++x) {
                mn[x] = min(mn[x], r[x + d]);
                if constexpr (GRAD) mx[x] = max(mx[x], r[x + d]);
            }
        }
    }
#pragma unroll
    for (uint32_t x = 0; x < kMB; ++x) {
        q[x * STRIDE] = mn[x];
        if constexpr (GRAD) q[(kMB + x) * STRIDE] = ~mx[x];
    }
}
// ... by the halo class (uniform)
template <bool GRAD, uint32_t STRIDE>
VR_DEV void morph_line_of(uint32_t H, const uint32_t *p, uint32_t *q, uint32_t R)
{
    if (H == 8u) morph_line<GRAD, 8u, STRIDE>(p, q, R);
    else if (H == 4u) morph_line<GRAD, 4u, STRIDE>(p, q, R);
    else if constexpr (GRAD) morph_line<true, 0u, STRIDE>(p, q, 0u);
}

template <typename VT, bool BALL, uint32_t MODE>
__global__ __launch_bounds__(kMorphThreads) void vr_morph_kernel(VolView vv, MorphArgs a, const float2 *__restrict__ cell_mm,
                                                                 const VT *f_src, VT *dst, unsigned long long *counters)
{
    using M = ModeOf<MODE>;
    constexpr uint32_t VPL = 16u / sizeof(VT);   // voxels per lane and load
    constexpr uint32_t LPM = 64u / VPL;          // lanes per micro-brick
    extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];   // S, and behind it the half-widths (BALL)
    const uint32_t PX = morph_in_vgpr(a.P[0]), PY = morph_in_vgpr(a.P[1]), PZ = morph_in_vgpr(a.P[2]);   // (lanes' address arithmetic)
    const uint32_t RS = BALL ? morph_in_vgpr(a.RS) : kRS;
    uint32_t *s_S = s_lds;
    int8_t *s_h = reinterpret_cast<int8_t *>(s_lds + a.RS * a.P[1] * a.P[2]);
    const VT *src = morph_in_vgpr(static_cast<const VT *>(vv.data));
    f_src = morph_in_vgpr(f_src);
    dst = morph_in_vgpr(dst);
    counters = morph_in_vgpr(counters);
    VolView lv = vv;   // the lanes' copy of the layout
    lv.nbx = morph_in_vgpr(vv.nbx), lv.nby = morph_in_vgpr(vv.nby), lv.nbz = morph_in_vgpr(vv.nbz);
    lv.ystride = morph_in_vgpr(vv.ystride);
    lv.zstride = (unsigned long long)morph_in_vgpr((uint32_t)vv.zstride) | ((unsigned long long)morph_in_vgpr((uint32_t)(vv.zstride >> 32)) << 32);
    const uint32_t n_items = morph_in_vgpr(a.n_mb * LPM), magic_mx = morph_in_vgpr(a.magic_mx), magic_my = morph_in_vgpr(a.magic_my);
    const int w1v = (int)morph_in_vgpr((uint32_t)(vv.w - 1)), h1v = (int)morph_in_vgpr((uint32_t)(vv.h - 1)), d1v = (int)morph_in_vgpr((uint32_t)(vv.d - 1));
    const uint32_t cm = M::cmpl ? 0xffffffffu : 0u;
    const float kInf = __builtin_inff();
    const int w1 = vv.w - 1, h1 = vv.h - 1, d1 = vv.d - 1;
    if constexpr (BALL) {
        for (uint32_t i = threadIdx.x; i < kHW * kHW; i += kMorphThreads)
            s_h[i] = (int8_t)morph::half_width(a.shape, a.R, (int)(i % kHW) - (int)kMaxR, (int)(i / kHW) - (int)kMaxR);
    }
    uint32_t c_fetched = 0, c_skipped = 0;   // (uniform)
    // the constant test's parameters wait in vector registers and are read back where the test runs
    const uint32_t v_skip[3] = {morph_in_vgpr(a.skip[0]), morph_in_vgpr(a.skip[1]), morph_in_vgpr(a.skip[2])};
    const uint32_t v_shift = morph_in_vgpr((uint32_t)a.cell_shift), v_cx = morph_in_vgpr((uint32_t)a.cell_cx), v_cy = morph_in_vgpr((uint32_t)a.cell_cy);
    const uint32_t row = a.nb[0] * a.nb[1];
#pragma unroll 1
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const uint32_t bz = b / row, rem = b - bz * row, by = rem / a.nb[0], bx = rem - by * a.nb[0];
        const uint32_t blk[3] = {bx, by, bz};
        const int res1[3] = {w1, h1, d1};
        bool skip = false;
        float cst = 0.f;
        if (cell_mm) {   // (uniform) every cell that holds a voxel the block's results depend on
            uint32_t c0[3], c1[3];
            const uint32_t shift = __builtin_amdgcn_readfirstlane(v_shift), ccx = __builtin_amdgcn_readfirstlane(v_cx),
                           ccy = __builtin_amdgcn_readfirstlane(v_cy);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const uint32_t margin = __builtin_amdgcn_readfirstlane(v_skip[ax]);
                const int lo = max((int)(blk[ax] * kMB) - (int)margin, 0);
                const int hi = min((int)(blk[ax] * kMB + kMB - 1u + margin), res1[ax]);
                c0[ax] = (uint32_t)lo >> shift;
                c1[ax] = (uint32_t)hi >> shift;
            }
            const float2 first = cell_mm[((size_t)c0[2] * ccy + c0[1]) * ccx + c0[0]];
            cst = first.x;
            skip = first.x == first.y && fabsf(first.x) < kInf;
            for (uint32_t cz = c0[2]; skip && cz <= c1[2]; ++cz)
                for (uint32_t cy = c0[1]; skip && cy <= c1[1]; ++cy)
                    for (uint32_t cx = c0[0]; skip && cx <= c1[0]; ++cx) {
                        const float2 mm = cell_mm[((size_t)cz * ccy + cy) * ccx + cx];
                        skip = mm.x == cst && mm.y == cst;
                    }
        }
        VT ext[2], ext2[2];   // the extreme as stored; GRADIENT: the maximum and the minimum
        if (skip) {
            ++c_skipped;
            VT v;
            if constexpr (sizeof(VT) == 4) v = cst == 0.f ? 0.f : cst;   // (a zero of either sign: +0)
            else v = (VT)(uint32_t)cst;
            ext[0] = ext[1] = ext2[0] = ext2[1] = v;
        } else {
            ++c_fetched;
            __syncthreads();   // (the previous block's reads of S are done; the half-widths are written)
            // the block's micro-bricks with the rings around them, 16 bytes per lane
            const int m0[3] = {(int)(bx * 2u) - (int)(a.H[0] >> 2), (int)(by * 2u) - (int)(a.H[1] >> 2),
                               (int)(bz * 2u) - (int)(a.H[2] >> 2)};
            bool border = false;   // (uniform) does the staged extent leave the volume?
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
                border = border || m0[ax] < 0 || (m0[ax] << 2) + (int)a.P[ax] - 1 > res1[ax];
            for (uint32_t i = threadIdx.x; i < n_items; i += kMorphThreads) {
                const uint32_t mb = i / LPM, v0 = (i % LPM) * VPL;
                const uint32_t t = __umulhi(mb, magic_mx), mx = mb - t * (PX >> 2);
                const uint32_t mz = __umulhi(t, magic_my), my = t - mz * (PY >> 2);
                const int gmx = m0[0] + (int)mx, gmy = m0[1] + (int)my, gmz = m0[2] + (int)mz;
                const bool in_grid = gmx >= 0 && gmy >= 0 && gmz >= 0 && (uint32_t)gmx < lv.nbx && (uint32_t)gmy < lv.nby &&
                                     (uint32_t)gmz < lv.nbz;
                uint4 q = make_uint4(0u, 0u, 0u, 0u);
                if (in_grid) {
                    const unsigned long long at = (unsigned long long)(uint32_t)gmz * lv.zstride +
                                                  (unsigned long long)(uint32_t)gmy * lv.ystride +
                                                  (unsigned long long)(((uint32_t)gmx << 6) + v0);
                    q = *reinterpret_cast<const uint4 *>(src + at);
                }
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
                uint32_t keys[VPL];
#pragma unroll
                for (uint32_t j = 0; j < VPL; ++j) {
                    VT raw;
                    if constexpr (sizeof(VT) == 1) raw = (VT)((w[j >> 2] >> ((j & 3u) * 8u)) & 0xffu);
                    else if constexpr (sizeof(VT) == 2) raw = (VT)((w[j >> 1] >> ((j & 1u) * 16u)) & 0xffffu);
                    else raw = __uint_as_float(w[j]);
                    if (border) {   // (uniform) a position outside the volume takes the voxel at its clamped position
                        const uint32_t v = v0 + j;
                        const int gx = (gmx << 2) + (int)(v & 3u), gy = (gmy << 2) + (int)((v >> 2) & 3u),
                                  gz = (gmz << 2) + (int)(v >> 4);
                        if (!in_grid || gx > w1v || gy > h1v || gz > d1v)
                            raw = src[vr_voxel_index(lv, min(max(gx, 0), w1v), min(max(gy, 0), h1v), min(max(gz, 0), d1v))];
                    }
                    keys[j] = morph_key<VT>(raw) ^ cm;
                }
#pragma unroll
                for (uint32_t rr = 0; rr < VPL / 4u; ++rr) {
                    const uint32_t v = v0 + rr * 4u;
                    const uint32_t py = (my << 2) + ((v >> 2) & 3u), pz = (mz << 2) + (v >> 4);
                    *reinterpret_cast<uint4 *>(s_S + (pz * PY + py) * RS + (mx << 2)) =
                        make_uint4(keys[rr * 4u], keys[rr * 4u + 1u], keys[rr * 4u + 2u], keys[rr * 4u + 3u]);
                }
            }
            __syncthreads();
            uint32_t k_lo[2], k_hi[2];   // the minimum of the staged keys; GRADIENT: the maximum as well
            if constexpr (BALL) {
                uint32_t x[2], y[2], z[2];
                const uint32_t *c[2];
#pragma unroll
                for (uint32_t k = 0; k < 2u; ++k) {
                    morph_result_pos(threadIdx.x + k * kMorphThreads, x[k], y[k], z[k]);
                    c[k] = s_S + ((z[k] + a.H[2]) * PY + (y[k] + a.H[1])) * RS + x[k] + a.H[0];
                    k_lo[k] = 0xffffffffu;
                    k_hi[k] = 0u;
                }
                const int Ry = (int)a.R[1], Rz = (int)a.R[2];
                for (int dz = -Rz; dz <= Rz; ++dz)
                    for (int dy = -Ry; dy <= Ry; ++dy) {
                        const int h = s_h[(uint32_t)(dz + (int)kMaxR) * kHW + (uint32_t)(dy + (int)kMaxR)];   // (uniform)
                        const int at = (dz * (int)PY + dy) * (int)RS;
                        for (int dx = -h; dx <= h; ++dx) {
#pragma unroll
                            for (uint32_t k = 0; k < 2u; ++k) {
                                const uint32_t v = c[k][at + dx];
                                k_lo[k] = min(k_lo[k], v);
                                if constexpr (M::grad) k_hi[k] = max(k_hi[k], v);
                            }
                        }
                    }
            } else {
                if (M::grad || a.R[0]) {   // (uniform) x: a thread per row of S
                    for (uint32_t j = threadIdx.x; j < PY * PZ; j += kMorphThreads)
                        morph_line_of<M::grad, 1u>(a.H[0], s_S + j * kRS + (a.H[0] - a.R[0]), s_S + j * kRS, a.R[0]);
                    __syncthreads();
                }
                if (a.R[1]) {   // (uniform) y: a thread per column of a slab, the minima's and the maxima's alike
                    constexpr uint32_t NC = M::grad ? 2u * kMB : kMB;
                    for (uint32_t j = threadIdx.x; j < NC * PZ; j += kMorphThreads) {
                        uint32_t *col = s_S + (j / NC) * PY * RS + (j % NC);
                        morph_line_of<false, kRS>(a.H[1], col + (a.H[1] - a.R[1]) * kRS, col, a.R[1]);
                    }
                    __syncthreads();
                }
                const uint32_t zs = PY * RS;
#pragma unroll
                for (uint32_t k = 0; k < 2u; ++k) {
                    uint32_t x, y, z;
                    morph_result_pos(threadIdx.x + k * kMorphThreads, x, y, z);
                    const uint32_t *p = s_S + ((z + a.H[2] - a.R[2]) * PY + y) * RS + x;
                    uint32_t m = p[0], m2 = M::grad ? p[kMB] : 0u;
                    for (uint32_t d = 1; d <= 2u * a.R[2]; ++d) {
                        m = min(m, p[d * zs]);
                        if constexpr (M::grad) m2 = min(m2, p[d * zs + kMB]);
                    }
                    k_lo[k] = m;
                    k_hi[k] = ~m2;
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 2u; ++k) {
                if constexpr (M::grad) {
                    ext[k] = morph_voxel<VT>(k_hi[k]);
                    ext2[k] = morph_voxel<VT>(k_lo[k]);
                } else
                    ext[k] = ext2[k] = morph_voxel<VT>(k_lo[k] ^ cm);
            }
        }
        // the results in micro-brick order; micro-bricks beyond the grid do not exist, voxels beyond the volume are 0
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            uint32_t x, y, z;
            morph_result_pos(threadIdx.x + k * kMorphThreads, x, y, z);
            const int gx = (int)(bx * kMB + x), gy = (int)(by * kMB + y), gz = (int)(bz * kMB + z);
            if ((uint32_t)(gx >> 2) < lv.nbx && (uint32_t)(gy >> 2) < lv.nby && (uint32_t)(gz >> 2) < lv.nbz) {
                const bool in = gx <= w1v && gy <= h1v && gz <= d1v;
                const unsigned long long at = vr_voxel_index(lv, gx, gy, gz);
                VT out = (VT)0;
                if (in) {
                    if constexpr (M::grad) out = skip ? (VT)0 : morph_diff<VT>(ext[k], ext2[k]);
                    else if constexpr (MODE == kMorphFMinusMax) out = skip ? (VT)0 : morph_diff<VT>(f_src[at], ext[k]);
                    else if constexpr (MODE == kMorphMinMinusF) out = skip ? (VT)0 : morph_diff<VT>(ext[k], f_src[at]);
                    else out = ext[k];
                }
                dst[at] = out;
            }
        }
    }
    if (threadIdx.x == 0) {
        if (c_fetched) atomicAdd(&counters[kMorphFetched], (unsigned long long)c_fetched);
        if (c_skipped) atomicAdd(&counters[kMorphSkipped], (unsigned long long)c_skipped);
    }
}

template <typename VT, bool BALL, uint32_t MODE>
hipError_t morph_launch(const MorphLaunch &a, const MorphArgs &ma, void *dst, unsigned long long *counters, hipStream_t stream)
{
    const size_t lds = BALL ? (size_t)ma.RS * ma.P[1] * ma.P[2] * sizeof(uint32_t) + ((kHW * kHW + 15u) & ~15u)
                            : (size_t)kRS * (ma.P[1] * ma.P[2] + kSlackRows) * sizeof(uint32_t);
    int per_cu = 0;
    const hipError_t e = vr_prepare_kernel(vr_morph_kernel<VT, BALL, MODE>, (int)kMorphThreads, lds, &per_cu, "morph", a.num_cus);
    if (e != hipSuccess) return e;
    const unsigned long long want = (unsigned long long)per_cu * (unsigned)(a.num_cus > 0 ? a.num_cus : 256) * 4ull;
    const uint32_t grid = (uint32_t)(ma.n_blocks < want ? ma.n_blocks : want);
    hipLaunchKernelGGL((vr_morph_kernel<VT, BALL, MODE>), dim3(grid), dim3(kMorphThreads), lds, stream, a.vol, ma, a.cell_minmax,
                       static_cast<const VT *>(a.f), static_cast<VT *>(dst), counters);
    return hipGetLastError();
}

template <typename VT, bool BALL>
hipError_t morph_launch_mode(const MorphLaunch &a, const MorphArgs &ma, void *dst, unsigned long long *counters, hipStream_t stream)
{
    switch (a.mode) {
    case kMorphMin: return morph_launch<VT, BALL, kMorphMin>(a, ma, dst, counters, stream);
    case kMorphMax: return morph_launch<VT, BALL, kMorphMax>(a, ma, dst, counters, stream);
    case kMorphMaxMin: return morph_launch<VT, BALL, kMorphMaxMin>(a, ma, dst, counters, stream);
    case kMorphFMinusMax: return morph_launch<VT, BALL, kMorphFMinusMax>(a, ma, dst, counters, stream);
    case kMorphMinMinusF: return morph_launch<VT, BALL, kMorphMinMinusF>(a, ma, dst, counters, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

hipError_t vr_launch_morph(const MorphLaunch &a, void *dst, unsigned long long *counters, hipStream_t stream)
{
    const size_t n = vr_filter_blocks(a.vol);
    if (n == 0 || n >= 0x7fffffffull || !dst || !counters || dst == a.vol.data) return hipErrorInvalidValue;
    if (a.shape != VRHIP_MORPH_BOX && a.shape != VRHIP_MORPH_BALL) return hipErrorInvalidValue;
    const bool sub = a.mode == kMorphFMinusMax || a.mode == kMorphMinMinusF;
    if (sub != (a.f != nullptr) || a.f == a.vol.data) return hipErrorInvalidValue;
    if (a.skip_scale < 1u || a.skip_scale > 2u) return hipErrorInvalidValue;
    if (a.cell_minmax && a.cell_shift < 3) return hipErrorInvalidValue;
    MorphArgs ma;
    ma.nb[0] = (uint32_t)(a.vol.w + 7) / kMB;
    ma.nb[1] = (uint32_t)(a.vol.h + 7) / kMB;
    ma.nb[2] = (uint32_t)(a.vol.d + 7) / kMB;
    ma.n_blocks = (uint32_t)n;
    for (int i = 0; i < 3; ++i) {
        if (a.radius[i] > kMaxR) return hipErrorInvalidValue;
        ma.R[i] = a.radius[i];
        ma.H[i] = a.radius[i] == 0u ? 0u : (a.radius[i] <= 4u ? 4u : 8u);
        ma.P[i] = kMB + 2u * ma.H[i];
        ma.skip[i] = a.skip_scale * a.radius[i];
    }
    ma.RS = ma.P[0] + 4u;
    ma.n_mb = (ma.P[0] >> 2) * (ma.P[1] >> 2) * (ma.P[2] >> 2);
    ma.magic_mx = (uint32_t)(0x100000000ull / (ma.P[0] >> 2)) + 1u;
    ma.magic_my = (uint32_t)(0x100000000ull / (ma.P[1] >> 2)) + 1u;
    ma.shape = a.shape;
    ma.cell_shift = a.cell_shift;
    ma.cell_cx = a.cell_cx;
    ma.cell_cy = a.cell_cy;
    const bool ball = a.shape == VRHIP_MORPH_BALL;
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        return ball ? morph_launch_mode<VT, true>(a, ma, dst, counters, stream)
                    : morph_launch_mode<VT, false>(a, ma, dst, counters, stream);
    });
}
