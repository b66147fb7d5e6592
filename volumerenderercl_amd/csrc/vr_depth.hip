// vr_depth.hip -- depth images and picking (vrhip_render_depth, include/vrhip.h "depth images and picking"): the
// kernel, its nine instantiations (three voxel types x three modes) and the launch entry vr_launch_depth.  Not a
// technique: it writes three buffers of the caller's and nothing else.
//
// Definition (tests/ref/depth_ref.c restates it on the CPU):
//  * the ray is technique 0's -- make_ray, setup_ray_head / setup_ray_tail without object-order ESS: t_0 = max(0, tnear),
//    t_{k+1} = t_k + stepSize while t_k < tfar, sample k at cam + dir * (t_k - offset), its value s_k the filtered,
//    normalised channel-0 value (Vol::linear / Vol::nearest);
//  * ISO: vr_iso.hip's hit and refinement with isoValue = threshold -- the first k with s_k >= isoValue, then (not for
//    k = 0) refineSteps bisections of [t_{k-1}, t_k]; t = tb, aux = the value of the fetch that last answered >=;
//  * MAX: vr_mip.hip's maximum, `s > m` from m = -inf, and the t_k of the last replacement; a ray that never replaces
//    m has no hit; aux = m;
//  * OPACITY: c = TF(s_k), opacity = 1 - powr(1 - c.a, 1 / samplingRate), alpha = alpha + opacity * (1 - alpha) from 0
//    -- eval_batch's opacity correction and the ray caster's compositing of alpha, no depth cue; the hit is the first
//    k with alpha >= threshold after its update, t = t_k; aux = alpha where the ray stopped;
//  * out_xyzt = (cam + dir * (t - offset), t) for a hit, else (0, 0, 0, +inf); out_kind = MISS / NO_HIT / HIT.
//
// Execution: vr_mip_kernel's launch shape -- one wave per 8x8 patch, one lane per ray, no LDS.  The patches are laid
// over the rectangle from (x0, y0) and addressed straight from the block index: no work queue, no control words.
// Lanes outside the rectangle set up no ray (they are invalid, as a lane outside the frame is for techniques 2 and 4)
// and are masked at the stores.  ISO keeps vr_iso.hip's stages: the march, then ONE refinement stage the wave enters
// once for all its hits.
//
// Skipping (object-order ESS on: cell_mm, or grid.empty in OPACITY mode, is handed over): only t is stepped, with the
// same fp32 add, over a sample whose outcome is known.
//  * ISO: vr_iso.hip's test, unchanged -- the cell's bound `< isoValue`.
//  * MAX: vr_mip.hip's test against the running maximum -- `bound <= m`.  Replacement needs s > m, so a skipped sample
//    could have moved neither m nor the t of the last replacement.
//    Both bounds: vr_mip.hip's header, (1) and (2); cells with a NaN voxel or a bound beyond FLT_MAX / 2 are never
//    skipped.
//  * OPACITY: samples in cells whose EMPTY bit is set (CellView::empty, vr_cells.hip: every fetch there maps to
//    opacity exactly 0; cells with a NaN voxel or a bound beyond FLT_MAX / 2 never get the bit).  Such a sample has
//    c.a == 0, so opacity = 1 - powr(1, y).  vr_powr(1.f, y) == 1.f EXACTLY for every finite y
//    (vr_device_math.h:105-125: vr_logf_pos(1) takes m = 0.5 -> 1, f = 0, every term of the chain a product with f, z
//    or fe = 0, so log = 0; t = y * 0 = 0, n = floor(0.5) = 0, r = fma(q, 0, 0) + 1 = 1, scaled by 2^0) -- the fact
//    the ray caster's lookahead relies on ("opacity 0 gives op = 1 - powr(1, y) = 0 exactly", eval_batch).  Then
//    opacity = 0, 0 * (1 - alpha) = 0 and alpha + 0 = alpha: alpha keeps its bits.  What is left is the hit test
//    itself: a searching lane holds alpha < threshold from the sample before -- or alpha = 0 before sample 0, which
//    is below the threshold only when threshold > 0.  So with threshold <= 0 (every ray hits at k = 0, whatever cell
//    it starts in) nothing is skipped, and above 0 an unchanged alpha cannot be a hit.
#include "vr_raycast_kernels.h"

namespace {

constexpr int kDepthLook = 16;   // samples a lane looks ahead per round (bits of the need mask)

// Bit k set: sample k of the run t0, t0 + stepSize, ... has to be fetched.  MAX: it may exceed m (vr_mip.hip's
// mip_need_mask); ISO: it may reach iso (vr_iso.hip's iso_need_mask).  (`grid`: the cell grid in the e* fields.)
template <bool MAX, typename V>
VR_DEV uint32_t depth_need_mask(const CellView &grid, const float2 *mm, const V &vol, const RayCtx &c, float t0, float ref,
                                bool linear)
{
    const CellLine line = cell_line_ray(add3(c.cam, scale3(c.dir, t0 - c.offset)), c.dir, c.stepSize, vol, grid.eshift,
                                        grid.ecx, grid.ecy, grid.ecz);
    constexpr float kHalfMax = 0x1.fffffep126f;   // FLT_MAX / 2
    uint32_t need = 0;
#pragma unroll
    for (int k = 0; k < kDepthLook; ++k) {
        const float2 b = mm[cell_index_of(cell_at(line, (float)k), grid.ecx, grid.ecy)];
        float bound = b.y * vol.inv_max;
        if (!linear) bound = vmax(bound, 0.f);
        const bool below = MAX ? bound <= ref : bound < ref;
        const bool known = b.x <= b.y && fabsf(b.x) <= kHalfMax && fabsf(b.y) <= kHalfMax && below;
        need |= known ? 0u : (1u << k);
    }
    return need;
}

// the filtered, normalised channel-0 value at ray parameter t (vr_iso.hip's iso_fetch)
template <typename V>
VR_DEV float depth_fetch(const V &vol, const RayCtx &c, float t, bool linear)
{
    const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
    const float px = pos.x * 0.5f + 0.5f, py = pos.y * 0.5f + 0.5f, pz = pos.z * 0.5f + 0.5f;
    return linear ? vol.linear(px, py, pz) : vol.nearest(px, py, pz);
}

// Registers: six waves per SIMD, the occupancy MIP and ISO march at (at most 80 VGPRs); the compiler's resource
// report for the nine instantiations is in DESIGN.md 5.10 -- no scratch, no LDS.
#define VR_DEPTH_OCC __attribute__((amdgpu_waves_per_eu(6, 6)))

template <typename VT, uint32_t MODE>
__global__ __launch_bounds__(kBlockDim) VR_DEPTH_OCC void vr_depth_kernel(VolView vv, TfView tf, CellView grid,
                                                                          const float2 *cell_mm, FrameView fr,
                                                                          vrhip_camera_params cam, vrhip_rendering_params rp,
                                                                          vrhip_raycast_params rc, vrhip_depth_params dp,
                                                                          uint32_t patches_x, uint32_t n_patches,
                                                                          float4 *__restrict__ out_xyzt,
                                                                          float *__restrict__ out_aux,
                                                                          uint8_t *__restrict__ out_kind)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (kBlockDim / 64) + (threadIdx.x >> 6);
    if (q >= n_patches) return;   // (uniform per wave)
    const uint32_t prow = q / patches_x, pcol = q - prow * patches_x;
    const uint32_t rx = pcol * 8u + (lane & 7u), ry = prow * 8u + (lane >> 3);   // in the rectangle
    const uint32_t gx = dp.x0 + rx, gy = dp.y0 + ry;                             // in the frame
    const bool inside = rx < dp.w && ry < dp.h;   // (the rectangle lies inside the frame: the host has checked)

    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    const f3 resf = mk3(vol.fw, vol.fh, vol.fd);
    const f3 voxLen = mk3(1.f / vol.fw, 1.f / vol.fh, 1.f / vol.fd);
    Grid no_bricks;   // (setup_ray_tail<false> reads none of it)
    no_bricks.bw = no_bricks.bh = no_bricks.bd = 0;
    no_bricks.bl0 = no_bricks.bl1 = no_bricks.bl2 = no_bricks.brickDia = 0.f;
    no_bricks.oob_word = 0;
    rp.useGradient = 0;   // (the background is not read here)
    fr.env = nullptr;

    RayCtx c;
    RayDyn d;
    float rnd;
    setup_ray_head<false>(gx, gy, inside, fr, cam, rp, c, d, rp.seed, rnd);
    setup_ray_tail<false>(rc, resf, voxLen, no_bricks, c, d, rnd);

    const bool linear = rp.useLinear != 0;
    const float thr = dp.threshold;
    bool hit = false;
    float t_hit = 0.f, aux = 0.f;

    if constexpr (MODE == VRHIP_DEPTH_MAX) {
        // ---- vr_mip.hip's march, with the t of the last replacement
        const bool skip = cell_mm != nullptr;
        float t = d.t;
        float m = -__builtin_inff();
        for (;;) {
            const bool act = c.valid && t < c.tfar;
            if (!__ballot(act)) break;
            uint32_t need = act ? 0xffffffffu : 0u;
            if (skip && act) need = depth_need_mask<true>(grid, cell_mm, vol, c, t, m, linear);
#pragma unroll 1
            for (int k = 0; k < kDepthLook; ++k) {
                const bool v = c.valid && t < c.tfar;
                const bool fetch = v && ((need >> k) & 1u);
                if (__ballot(fetch)) {
                    if (fetch) {
                        const float s = depth_fetch(vol, c, t, linear);
                        const bool up = s > m;   // (false for a NaN sample)
                        m = up ? s : m;
                        t_hit = up ? t : t_hit;
                    }
                }
                const float tn = t + c.stepSize;   // a step that no longer moves t ends the sequence
                t = v ? (tn > t ? tn : __builtin_inff()) : t;
            }
        }
        hit = c.valid && m > -__builtin_inff();   // <=> some sample replaced m
        aux = m;
    } else {
        // ---- vr_iso.hip's march: t is sample k's parameter, t_prev sample k - 1's; a lane leaves the search with a hit
        // (t, t_prev stay) or at the end of its sequence.  OPACITY carries alpha through the same loop.
        const bool skip = MODE == VRHIP_DEPTH_ISO ? cell_mm != nullptr : (grid.empty != nullptr && thr > 0.f);
        const float refInterval = 1.f / rc.samplingRate;
        float t = d.t, t_prev = d.t;
        float alpha = 0.f, val = 0.f;
        bool searching = c.valid && t < c.tfar;
        for (;;) {
            if (!__ballot(searching)) break;
            uint32_t need = 0xffffffffu;
            if (skip && searching) {
                if constexpr (MODE == VRHIP_DEPTH_ISO) need = depth_need_mask<false>(grid, cell_mm, vol, c, t, thr, linear);
                else need = ~empty_mask<VT, 0, kDepthLook>(grid, vol, c, t);
            }
#pragma unroll 1
            for (int k = 0; k < kDepthLook; ++k) {
                const bool fetch = searching && ((need >> k) & 1u);
                if (__ballot(fetch)) {
                    if (fetch) {
                        const float s = depth_fetch(vol, c, t, linear);
                        if constexpr (MODE == VRHIP_DEPTH_ISO) {
                            hit = s >= thr;   // (false for a NaN sample)
                            val = hit ? s : val;
                        } else {
                            const float4 col = tff_linear<kRawDensity<VT>>(tf.tff, (int)tf.tff_n, s);
                            const float opacity = 1.f - vr_powr(1.f - col.w, refInterval);   // eval_batch's correction
                            alpha = alpha + opacity * (1.f - alpha);
                            hit = alpha >= thr;
                        }
                    }
                }
                // the next sample: t += stepSize while t < tfar; a step that no longer moves t ends the sequence
                const float tn = t + c.stepSize;
                const bool go = searching && !hit;
                searching = go && tn > t && tn < c.tfar;
                t_prev = go ? t : t_prev;
                t = go ? tn : t;
            }
        }
        t_hit = t;
        aux = alpha;
        if constexpr (MODE == VRHIP_DEPTH_ISO) {
            // ---- refinement: refineSteps uniform rounds over the lanes that hit at k > 0 (k = 0 <=> t is still t_0)
            const bool refine = hit && t != d.t;
            float ta = t_prev, tb = t;
            if (__ballot(refine)) {
#pragma unroll 1
                for (uint32_t i = 0; i < dp.refineSteps; ++i) {
                    const float tm = (ta + tb) * 0.5f;
                    if (refine) {
                        const float s = depth_fetch(vol, c, tm, linear);
                        const bool ge = s >= thr;
                        tb = ge ? tm : tb;
                        ta = ge ? ta : tm;
                        val = ge ? s : val;
                    }
                }
            }
            t_hit = tb;
            aux = hit ? val : 0.f;
        }
    }

    if (!inside) return;
    const size_t i = (size_t)ry * dp.w + rx;
    if (out_xyzt) {
        float4 o = make_float4(0.f, 0.f, 0.f, __builtin_inff());
        if (hit) {
            const f3 pos = add3(c.cam, scale3(c.dir, t_hit - c.offset));   // (depth_fetch's position, before * 0.5 + 0.5)
            o = make_float4(pos.x, pos.y, pos.z, t_hit);
        }
        out_xyzt[i] = o;
    }
    if (out_aux) out_aux[i] = c.valid ? aux : 0.f;
    if (out_kind) out_kind[i] = (uint8_t)(!c.valid ? VRHIP_DEPTH_MISS : hit ? VRHIP_DEPTH_HIT : VRHIP_DEPTH_NO_HIT);
}

template <typename VT, uint32_t MODE>
hipError_t launch_depth(const DepthLaunch &a, hipStream_t stream)
{
    const uint32_t waves = kBlockDim / 64;
    const uint32_t patches_x = (a.params.w + 7u) / 8u, n_patches = patches_x * ((a.params.h + 7u) / 8u);
    const dim3 grid((n_patches + waves - 1u) / waves), block(kBlockDim);
    if (grid.x == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((vr_depth_kernel<VT, MODE>), grid, block, 0, stream, a.vol, a.tf, a.cells, a.cell_minmax, a.frame,
                       a.cam, a.render, a.raycast, a.params, patches_x, n_patches, a.out_xyzt, a.out_aux, a.out_kind);
    return hipGetLastError();
}

} // namespace

hipError_t vr_launch_depth(const DepthLaunch &a, hipStream_t stream)
{
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        switch (a.params.mode) {
        case VRHIP_DEPTH_ISO: return launch_depth<VT, VRHIP_DEPTH_ISO>(a, stream);
        case VRHIP_DEPTH_MAX: return launch_depth<VT, VRHIP_DEPTH_MAX>(a, stream);
        case VRHIP_DEPTH_OPACITY: return launch_depth<VT, VRHIP_DEPTH_OPACITY>(a, stream);
        default: return hipErrorInvalidValue;
        }
    });
}
