// vr_mip.hip -- technique 2, maximum intensity projection (VRHIP_TECHNIQUE_MIP, include/vrhip.h): the kernel, its
// instantiations for the three voxel types and the launch entry vr_launch_mip.
//
// Definition (DESIGN.md "Maximum intensity projection"; tests/ref/mip_ref.c restates it on the CPU):
//  * the ray is technique 0's -- make_ray, setup_ray_head / setup_ray_tail without object-order ESS: t_0 = max(0, tnear),
//    t_{k+1} = t_k + stepSize while t_k < tfar, sample k at cam + dir * (t_k - offset);
//  * m = the maximum over those samples of the filtered, normalised channel-0 value (Vol::linear / Vol::nearest),
//    taken as `s > m ? s : m` from m = -inf: a NaN sample never replaces it;
//  * the pixel is TF(m) over the background, one rounded fp32 operation per product and sum (mip_pixel below); a ray
//    that misses the box or takes no sample keeps the background.
//
// Execution: one wave per 8x8 patch, one lane per ray, the running maximum in a register; the grid is the work
// list itself (patches x frames of the launch set, FrameView::queue read by position): no queue head, no pre-pass,
// no second phase, no LDS.  The transfer function is read once per pixel, from global memory.
//
// Skipping (object-order ESS on): the maximum does not depend on the order or on samples that cannot raise it, so
// a sample whose value is known to be <= m is left out -- only its t is stepped, with the same fp32 add.  The
// bound comes from the cell grid (CellView, vr_cells.hip): per cell of 2^shift voxels the (min, max) of the RAW
// voxels [(c << shift) - 1, ((c + 1) << shift) + 1] per axis.  Two things make `max * inv_max <= m` a proof:
//
//  (1) The bound covers the filter's footprint.  The cell is looked up from the ray's cell line (vr_sampling.h, "the
//      cell of a point on a line": floor(u') is the trilinear fetch's low-corner texel or the next one -- also with the
//      linearisation's error over kMipLook steps -- the halo covers the voxels it reads, positions outside the volume
//      clamp to the border cell).  The nearest fetch reads voxel floor(u) = x' (or a neighbour, with that error); it
//      answers 0 outside the volume (border colour), so its bound is max(cell bound, 0).  (The reference's ESS bricks
//      hold the voxels of the brick alone, no halo: a fetch at a brick face reads a voxel they do not cover.)
//  (2) The fp32 interpolation stays within [min, max] of its corners.  lerpf(p, q, w) = fmaf(w, d, p) with
//      d = fl(q - p) = (q - p)(1 + e), |e| <= 2^-24 (exact when the difference is subnormal).  The weights are
//      w = fl(ub - floor(ub)):
//        - ub >= 0: the fraction of a float is exact and < 1, so w <= 1 - 2^-24 and w (1 + e) <= (1 - 2^-24)
//          (1 + 2^-24) < 1: the exact value p + w d lies between p and q, both floats, and the fma's single rounding
//          is monotone -- the result lies in [min(p, q), max(p, q)], no ulp above;
//        - ub < 0 (where the subtraction may round w up to 1.0): both taps are clamped to texel 0, p == q, d = 0 and
//          the result is p exactly.
//      The second and third level blend values that lie in the corners' range already, and `* inv_max` is monotone, so
//      s <= fl(max * inv_max).  All of this needs q - p not to overflow and no NaN: a cell with |min| or |max| above
//      FLT_MAX / 2, or with a NaN voxel (which the grid records as (-inf, +inf)), is never skipped -- the test
//      vr_cell_bounds_kernel applies for the same reason.
//  So `bound <= m` (not only `bound < m`) implies s <= m, and `s > m` is false: the register would not change.
#include "vr_raycast_kernels.h"

namespace {

constexpr int kMipLook = 16;   // samples a lane looks ahead per round (bits of the need mask)

// Bit k set: sample k of the run t0, t0 + stepSize, ... may exceed m and has to be fetched.  (`grid`: the cell grid
// in the e* fields of a CellView, mm its (min, max) pairs.)
template <typename V>
VR_DEV uint32_t mip_need_mask(const CellView &grid, const float2 *mm, const V &vol, const RayCtx &c, float t0, float m,
                              bool linear)
{
    const CellLine line = cell_line_ray(add3(c.cam, scale3(c.dir, t0 - c.offset)), c.dir, c.stepSize, vol, grid.eshift,
                                        grid.ecx, grid.ecy, grid.ecz);
    constexpr float kHalfMax = 0x1.fffffep126f;   // FLT_MAX / 2
    uint32_t need = 0;
#pragma unroll
    for (int k = 0; k < kMipLook; ++k) {
        const float2 b = mm[cell_index_of(cell_at(line, (float)k), grid.ecx, grid.ecy)];
        float bound = b.y * vol.inv_max;
        if (!linear) bound = vmax(bound, 0.f);
        const bool known = b.x <= b.y && fabsf(b.x) <= kHalfMax && fabsf(b.y) <= kHalfMax && bound <= m;
        need |= known ? 0u : (1u << k);
    }
    return need;
}

// The pixel of a ray whose maximum is m: c = TF(m), rgb = c.rgb * c.a + bg.rgb * (1 - c.a), a = c.a + bg.a * (1 - c.a)
template <bool RAW>
VR_DEV float4 mip_pixel(const float4 *tff, int n, float m, const float (&bg)[4])
{
    const float4 c = tff_linear<RAW>(tff, n, m);
    const float oma = 1.f - c.w;
    float4 o;
    o.x = (c.x * c.w) + (bg[0] * oma);
    o.y = (c.y * c.w) + (bg[1] * oma);
    o.z = (c.z * c.w) + (bg[2] * oma);
    o.w = c.w + (bg[3] * oma);
    return o;
}

template <typename VT, bool VIEWS>
__global__ __launch_bounds__(kBlockDim) void vr_mip_kernel(VolView vv, TfView tf, CellView grid, const float2 *cell_mm,
                                                           FrameView fr, vrhip_camera_params cam,
                                                           vrhip_rendering_params rp, vrhip_raycast_params rc)
{
    VR_ZERO_NEXT_CTRL(fr);   // (the control words are the ray caster's; the sets of launches alternate whatever the technique)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (kBlockDim / 64) + (threadIdx.x >> 6);
    if (q >= fr.n_wave_tiles) return;   // (uniform per wave)
    const WaveTile wt = fr.queue[q];
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t gx = wt_col(wt) * 8u + lx, gy = wt_row(wt) * 8u + ly;
    const uint32_t frame_idx = wt_frame(wt);
    const uint32_t seed = fr.seeds ? fr.seeds[frame_idx] : rp.seed;
    const bool inside = gx < fr.W && gy < fr.H;

    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    const f3 resf = mk3(vol.fw, vol.fh, vol.fd);
    const f3 voxLen = mk3(1.f / vol.fw, 1.f / vol.fh, 1.f / vol.fd);
    Grid no_bricks;   // (setup_ray_tail<false> reads none of it)
    no_bricks.bw = no_bricks.bh = no_bricks.bd = 0;
    no_bricks.bl0 = no_bricks.bl1 = no_bricks.bl2 = no_bricks.brickDia = 0.f;
    no_bricks.oob_word = 0;
    rp.useGradient = 0;   // ignored by this technique: the background is backgroundColor itself
    fr.env = nullptr;     // (rejected by the host; never sampled here)

    RayCtx c;
    RayDyn d;
    float rnd;
    if constexpr (VIEWS) {
        const vrhip_camera_params fc = load_frame_cam<true>(fr.cams, frame_idx);
        setup_ray_head<false>(gx, gy, inside, fr, fc, rp, c, d, seed, rnd);
    } else {
        setup_ray_head<false>(gx, gy, inside, fr, cam, rp, c, d, seed, rnd);
    }
    setup_ray_tail<false>(rc, resf, voxLen, no_bricks, c, d, rnd);

    const bool linear = rp.useLinear != 0;
    const bool skip = cell_mm != nullptr;
    float t = d.t;
    float m = -__builtin_inff();
    const bool has_sample = c.valid && t < c.tfar;
    for (;;) {
        const bool act = c.valid && t < c.tfar;
        if (!__ballot(act)) break;
        uint32_t need = act ? 0xffffffffu : 0u;
        if (skip && act) need = mip_need_mask(grid, cell_mm, vol, c, t, m, linear);
#pragma unroll 1
        for (int k = 0; k < kMipLook; ++k) {
            const bool v = c.valid && t < c.tfar;
            const bool fetch = v && ((need >> k) & 1u);
            if (__ballot(fetch)) {
                if (fetch) {
                    const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
                    const float px = pos.x * 0.5f + 0.5f, py = pos.y * 0.5f + 0.5f, pz = pos.z * 0.5f + 0.5f;
                    const float s = linear ? vol.linear(px, py, pz) : vol.nearest(px, py, pz);
                    m = s > m ? s : m;
                }
            }
            // t += stepSize; a step that no longer moves t would repeat one sample for ever, which cannot change a
            // maximum: the sequence ends there
            const float tn = t + c.stepSize;
            t = v ? (tn > t ? tn : __builtin_inff()) : t;
        }
    }

    if (!inside) return;
    const float bg[4] = {c.env0, c.env1, c.env2, c.env3};
    float4 o = make_float4(bg[0], bg[1], bg[2], bg[3]);
    if (has_sample) o = mip_pixel<kRawDensity<VT>>(tf.tff, (int)tf.tff_n, m, bg);
    fr.fb[(size_t)gy * fr.W + gx] = o;
    if (fr.out) fr.out[(size_t)wt.out_base + (size_t)ly * fr.out_stride + lx] = o;
}

template <typename VT, bool VIEWS>
hipError_t launch_mip(const RaycastLaunch &a, hipStream_t stream)
{
    const uint32_t waves = kBlockDim / 64;
    const dim3 grid((a.frame.n_wave_tiles + waves - 1u) / waves), block(kBlockDim);
    if (grid.x == 0) return hipSuccess;
    // the cell grid the (min, max) pairs live on, in the e* fields: the fine grid, or the only one (ensure_cells)
    CellView g = a.cells;
    if (a.cell_minmax && !a.cell_minmax_fine) { g.ecx = g.cx; g.ecy = g.cy; g.ecz = g.cz; g.eshift = g.shift; }
    return vr_launch_bound(
        a, stream, false,
        [&](hipEvent_t start, hipEvent_t stop) {
            vr_launch_kernel(vr_mip_kernel<VT, VIEWS>, grid, block, 0, stream, start, stop, a.vol, a.tf, g, a.cell_minmax,
                             a.frame, a.cam, a.render, a.raycast);
        },
        [](hipEvent_t) {});
}

template <typename VT>
hipError_t launch_mip_typed(const RaycastLaunch &a, hipStream_t stream)
{
    return a.frame.cams ? launch_mip<VT, true>(a, stream) : launch_mip<VT, false>(a, stream);
}

} // namespace

hipError_t vr_launch_mip(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.info) {
        a.info->technique = 2;
        a.info->work_items = a.frame.n_wave_tiles;
        a.info->empty_skip = a.cell_minmax ? 1u : 0u;
    }
    return vr_for_format(a.format, [&](auto vt) { return launch_mip_typed<typename decltype(vt)::type>(a, stream); });
}
