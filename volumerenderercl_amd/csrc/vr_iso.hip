// vr_iso.hip -- technique 4, first-hit isosurface rendering (VRHIP_TECHNIQUE_ISO, include/vrhip.h): the kernel, its
// instantiations for the three voxel types and the launch entry vr_launch_iso.
//
// Definition (DESIGN.md "First-hit isosurface"; tests/ref/iso_ref.c restates it on the CPU):
//  * the ray is technique 0's -- make_ray, setup_ray_head / setup_ray_tail without object-order ESS: t_0 = max(0, tnear),
//    t_{k+1} = t_k + stepSize while t_k < tfar, sample k at cam + dir * (t_k - offset);
//  * the hit is the first k whose filtered, normalised channel-0 value (Vol::linear / Vol::nearest) is >= isoValue: a
//    NaN sample never hits, k = 0 hits like any other sample;
//  * refinement (not for k = 0): refineSteps bisections of [t_{k-1}, t_k], tm = (ta + tb) * 0.5f, one fetch each,
//    s >= isoValue ? tb = tm : ta = tm; t_hit = tb;
//  * the pixel is TF(isoValue).rgb, for illumType 1 through technique 0's Blinn-Phong terms (eval_batch) with
//    Vol::neg_gradient at the hit, alpha 1; a ray that misses the box or finds no hit keeps backgroundColor.
//
// Execution: vr_mip_kernel's launch shape -- one wave per 8x8 patch, one lane per ray, the grid is the work list
// (patches x frames of the launch set, FrameView::queue read by position), no LDS.  Three stages, each entered by
// the whole wave ONCE: a lane that has hit waits with (t_{k-1}, t_k) in two registers until no lane of the wave is
// still searching, then all hits are refined in refineSteps uniform rounds, then one gradient evaluation shades them
// all.  (Refining or shading inside the march would run those fetches -- 8 voxels a round, 32 for the gradient --
// once per lane that hits, with its 63 neighbours masked off.)
//
// Skipping (object-order ESS on): a sample whose value is known to be < isoValue cannot be the hit and is left out --
// only its t is stepped, with the same fp32 add.  The bound is the cell grid's (min, max) exactly as technique 2 uses
// it: vr_mip.hip's header proves (1) that the cell found on the ray's cell line covers the filter's footprint and (2)
// that the fp32 interpolation stays within its corners, s <= fl(max * inv_max) (nearest: max(.., 0) for the border
// colour), for every cell without a NaN voxel and with bounds within FLT_MAX / 2 -- other cells are never skipped.
// Here the bound meets a fixed threshold instead of a running maximum, and the one new line is the comparison:
// `bound < isoValue`, NOT `<=` -- a sample EQUAL to isoValue hits (s >= isoValue), so a cell whose bound equals
// isoValue may hold the hit.  Refinement and shading fetch unconditionally.
#include "vr_raycast_kernels.h"

namespace {

constexpr int kIsoLook = 16;   // samples a lane looks ahead per round (bits of the need mask)

// Bit k set: sample k of the run t0, t0 + stepSize, ... may reach isoValue and has to be fetched.  (`grid`: the cell
// grid in the e* fields of a CellView, mm its (min, max) pairs.)
template <typename V>
VR_DEV uint32_t iso_need_mask(const CellView &grid, const float2 *mm, const V &vol, const RayCtx &c, float t0, float iso,
                              bool linear)
{
    const CellLine line = cell_line_ray(add3(c.cam, scale3(c.dir, t0 - c.offset)), c.dir, c.stepSize, vol, grid.eshift,
                                        grid.ecx, grid.ecy, grid.ecz);
    constexpr float kHalfMax = 0x1.fffffep126f;   // FLT_MAX / 2
    uint32_t need = 0;
#pragma unroll
    for (int k = 0; k < kIsoLook; ++k) {
        const float2 b = mm[cell_index_of(cell_at(line, (float)k), grid.ecx, grid.ecy)];
        float bound = b.y * vol.inv_max;
        if (!linear) bound = vmax(bound, 0.f);
        const bool known = b.x <= b.y && fabsf(b.x) <= kHalfMax && fabsf(b.y) <= kHalfMax && bound < iso;
        need |= known ? 0u : (1u << k);
    }
    return need;
}

// the filtered, normalised channel-0 value at ray parameter t
template <typename V>
VR_DEV float iso_fetch(const V &vol, const RayCtx &c, float t, bool linear)
{
    const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
    const float px = pos.x * 0.5f + 0.5f, py = pos.y * 0.5f + 0.5f, pz = pos.z * 0.5f + 0.5f;
    return linear ? vol.linear(px, py, pz) : vol.nearest(px, py, pz);
}

// Registers: left alone, the gradient's 4x4x4 neighbourhood takes the USHORT and FLOAT kernels to 82 and 88 VGPRs --
// past the step at 80, five waves per SIMD instead of the six MIP's march runs at -- for a stage every ray enters at
// most once.  Asked for six waves the allocator fits all three voxel types in 72 / 76 / 78 VGPRs without scratch
// (the compiler's resource report), so the march keeps MIP's occupancy.
#define VR_ISO_OCC __attribute__((amdgpu_waves_per_eu(6, 6)))

template <typename VT, bool VIEWS>
__global__ __launch_bounds__(kBlockDim) VR_ISO_OCC void vr_iso_kernel(VolView vv, TfView tf, CellView grid,
                                                                      const float2 *cell_mm, FrameView fr,
                                                                      vrhip_camera_params cam, vrhip_rendering_params rp,
                                                                      vrhip_raycast_params rc, vrhip_iso_params ip)
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
    // (the illumination invariants are made in the shading stage, from c.dir: the march does not carry them)
    if constexpr (VIEWS) {
        const vrhip_camera_params fc = load_frame_cam<true>(fr.cams, frame_idx);
        setup_ray_head<false>(gx, gy, inside, fr, fc, rp, c, d, seed, rnd);
    } else {
        setup_ray_head<false>(gx, gy, inside, fr, cam, rp, c, d, seed, rnd);
    }
    setup_ray_tail<false>(rc, resf, voxLen, no_bricks, c, d, rnd);

    const bool linear = rp.useLinear != 0;
    const bool skip = cell_mm != nullptr;
    const float iso = ip.isoValue;

    // ---- march: t is sample k's parameter, t_prev sample k - 1's (k = 0: t itself, never read); a lane leaves the
    // search with a hit (t, t_prev stay) or at the end of its sequence.  t_prev lives across the lookahead rounds, so
    // a hit at position 0 of a round finds sample k - 1 of the round before in it.
    float t = d.t, t_prev = d.t;
    bool searching = c.valid && t < c.tfar;
    bool hit = false;
    for (;;) {
        if (!__ballot(searching)) break;
        uint32_t need = 0xffffffffu;
        if (skip && searching) need = iso_need_mask(grid, cell_mm, vol, c, t, iso, linear);
#pragma unroll 1
        for (int k = 0; k < kIsoLook; ++k) {
            const bool fetch = searching && ((need >> k) & 1u);
            if (__ballot(fetch)) {
                if (fetch) hit = iso_fetch(vol, c, t, linear) >= iso;   // (false for a NaN sample)
            }
            // the next sample: t += stepSize while t < tfar; a step that no longer moves t ends the sequence
            const float tn = t + c.stepSize;
            const bool go = searching && !hit;
            searching = go && tn > t && tn < c.tfar;
            t_prev = go ? t : t_prev;
            t = go ? tn : t;
        }
    }
    // (a lane that ran out of samples holds some t >= tfar or a stalled t: neither is read again)

    // ---- refinement: refineSteps uniform rounds over the lanes that hit at k > 0 (k = 0 <=> t is still t_0: every
    // later t is strictly greater)
    const bool refine = hit && t != d.t;
    float ta = t_prev, tb = t;
    if (__ballot(refine)) {
#pragma unroll 1
        for (uint32_t i = 0; i < ip.refineSteps; ++i) {
            const float tm = (ta + tb) * 0.5f;
            if (refine) {
                const bool ge = iso_fetch(vol, c, tm, linear) >= iso;
                tb = ge ? tm : tb;
                ta = ge ? ta : tm;
            }
        }
    }

    // ---- shading: one gradient evaluation for all lanes that hit; eval_batch's Blinn-Phong terms and operation order
    float4 o = make_float4(c.env0, c.env1, c.env2, c.env3);
    if (__ballot(hit)) {
        const float4 col = tff_linear<true>(tf.tff, (int)tf.tff_n, iso);   // (the same entries in every lane)
        if (hit) {
            o = make_float4(col.x, col.y, col.z, 1.f);
            if (rp.illumType == 1) {
                const f3 pos = add3(c.cam, scale3(c.dir, tb - c.offset));
                const f3 g = vol.neg_gradient(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
                // the illumination invariants of setup_ray_head<true> (:280-303)
                const f3 toLight = neg3(c.dir);
                const f3 lgt = normalize3(toLight);
                f3 hv = add3(toLight, lgt);
                const bool hvalid = !(dot3(hv, hv) < 1.e-6f);
                hv = normalize3(hv);
                const float ndl = vmax(0.f, dot3(g, lgt));
                float sp = hvalid ? vr_powr(vmax(dot3(g, hv), 0.f), 40.f) : 0.0f;
                sp = sp * 0.15f;
                o.x = ((col.x * 0.15f) + ((col.x * ndl) * 0.7f)) + sp;
                o.y = ((col.y * 0.15f) + ((col.y * ndl) * 0.7f)) + sp;
                o.z = ((col.z * 0.15f) + ((col.z * ndl) * 0.7f)) + sp;
            }
        }
    }

    if (!inside) return;
    fr.fb[(size_t)gy * fr.W + gx] = o;
    if (fr.out) fr.out[(size_t)wt.out_base + (size_t)ly * fr.out_stride + lx] = o;
}

template <typename VT, bool VIEWS>
hipError_t launch_iso(const RaycastLaunch &a, hipStream_t stream)
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
            vr_launch_kernel(vr_iso_kernel<VT, VIEWS>, grid, block, 0, stream, start, stop, a.vol, a.tf, g, a.cell_minmax,
                             a.frame, a.cam, a.render, a.raycast, a.iso);
        },
        [](hipEvent_t) {});
}

template <typename VT>
hipError_t launch_iso_typed(const RaycastLaunch &a, hipStream_t stream)
{
    return a.frame.cams ? launch_iso<VT, true>(a, stream) : launch_iso<VT, false>(a, stream);
}

} // namespace

hipError_t vr_launch_iso(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.info) {
        a.info->technique = VRHIP_TECHNIQUE_ISO;
        a.info->work_items = a.frame.n_wave_tiles;
        a.info->empty_skip = a.cell_minmax ? 1u : 0u;
    }
    return vr_for_format(a.format, [&](auto vt) { return launch_iso_typed<typename decltype(vt)::type>(a, stream); });
}
