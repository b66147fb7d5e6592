// vr_tf2d.hip -- technique 6, ray casting through a two-dimensional transfer function TF2(value, gradient magnitude)
// (VRHIP_TECHNIQUE_TF2D, include/vrhip.h): the kernel, its instantiations for the three voxel types and the launch
// entry vr_launch_tf2d.
//
// Definition (include/vrhip.h "technique == 6"; tests/ref/tf2d_ref.c restates it on the CPU):
//  * the ray is technique 0's -- make_ray, setup_ray_head / setup_ray_tail without object-order ESS: t_0 = max(0, tnear),
//    sample k at cam + dir * (t_k - offset), and the reference's loop (volumeraycast.cl:790-880): composite sample k,
//    stop when alpha >= 0.98f (<=> (double)alpha > 0.98), t_{k+1} = t_k + stepSize, go on while t_{k+1} < tfar; a step
//    that no longer moves t ends the sequence;
//  * per sample: s = the filtered, normalised channel-0 value (Vol::linear / Vol::nearest); G = s2 - s1, the six taps
//    of Vol::neg_gradient before it normalises them; m = 0.5f * len3(G); c = the bilinear read of the table at (s, m)
//    (tf2d_lookup); illumType 1 and c.a > 0.1f: eval_batch's Blinn-Phong terms with the normal -normalize(G) of the same
//    taps; then eval_batch's opacity correction and the ray caster's compositing from (backgroundColor, alpha 0).
//
// Execution: vr_mip_kernel's launch shape -- one wave per 8x8 patch, one lane per ray, the grid is the work list, no
// LDS.  The gradient costs 32 voxels per sample against 8 for the value, and most samples of a classified volume are
// transparent, so a round has two stages, as vr_iso.hip has three:
//  * search: every lane steps over its transparent samples -- fetch s, look at the two table COLUMNS the value axis
//    would read; when both are transparent in every row (Tf2dView::nz) the sample composites to nothing and the lane
//    goes on, up to kTf2dLook samples a round.  A lane that finds a sample that is not waits with (t, s);
//  * evaluate: the whole wave enters the gradient, the lookup and the compositing ONCE for all waiting lanes.
// A ray's samples are composited in its own order: a lane never looks past a sample it has not composited.
//
// Why leaving out a transparent sample changes no bit.  Columns i0, i1 transparent in every row: the four alphas read
// are +0, r0 = r1 = fma(a, 0 - 0, 0) = +0 (a finite), c.a = +0, no shading (c.a > 0.1f fails).  opacity =
// 1 - vr_powr(1 - 0, y) = 1 - 1 = 0 exactly for every finite y (vr_depth.hip's header walks through vr_powr(1, y); the
// ray caster's empty-run skipping rests on the same fact: DESIGN.md 5.1 "Empty-run skipping", eval_batch "opacity 0
// gives op = 1 - powr(1, y) = 0 exactly").  alpha + 0 * (1 - alpha) = alpha.  result - (x * 0) * oma with x = bg - c
// finite (bg finite, c in [0, 1.15]) and oma in [0.02, 1]: the subtrahend is +-0, and r - (+-0) == r bit for bit for
// every r but r = -0 with a subtrahend of -0, which gives +0.  result starts as bg, and x - y is -0 only for x = -0,
// y = +0 -- so a component of result is -0 only while it is still an untouched bg component of -0, and then
// x = -0 - c is -0 or negative, the subtrahend of the FIRST sample of the ray (transparent or not) is -0 or negative
// and the component becomes +0 or positive there, for good.  So: a ray that takes a sample starts from bg + 0.0f (-0
// becomes +0, every other value keeps its bits), and from then on no transparent sample can change a bit.  (DESIGN's
// proof for the ray caster does not mention -0; its march with the switch on is not held to its march with it off.)
// The early-termination test after a transparent sample reads an alpha that has not changed since it last failed.
//
// Skipping (object-order ESS on): a sample whose cell proves both columns transparent is not fetched -- only its t is
// stepped, with the same fp32 add.  The cell grid's (min, max) exactly as techniques 2 and 4 use it; vr_mip.hip's header
// proves (1) that the cell found on the ray's cell line covers the filter's footprint and (2) that every level of the
// fp32 interpolation stays within [min(p, q), max(p, q)] of its operands -- the argument there is two-sided: the exact
// value p + w d lies between the floats p and q and the fma's single rounding is monotone, so the result is neither an
// ulp above the larger nor an ulp BELOW the smaller; `* inv_max` is monotone.  Hence fl(min * inv_max) <= s <=
// fl(max * inv_max), no slack needed (nearest: the border colour 0 joins the range on both sides).  Needs, as there,
// a cell without a NaN voxel and with bounds within FLT_MAX / 2.  The value axis' indices are monotone in s:
// tff_coord's clamp, the rounded product with n_v, the rounded subtraction of 0.5, floor, the conversion and the index
// clamp are each monotone (rounding to nearest is), so i0(lo) <= i0(s) and i1(s) <= i1(hi) for lo <= s <= hi, and the
// two columns a sample reads lie in [i0(lo), i1(hi)].  All of those transparent <=> nz[i1(hi) + 1] == nz[i0(lo)].
//
// Registers (the compiler's resource report, hipcc -Rpass-analysis=kernel-resource-usage): see
// VR_TF2D_OCC below.
#include "vr_raycast_kernels.h"

namespace {

constexpr int kTf2dLook = 16;   // samples a lane looks ahead per round (bits of the need mask)
#ifndef VR_TF2D_MASK_UNROLL
#define VR_TF2D_MASK_UNROLL 4
#endif

// tff_linear's index arithmetic on an axis of n entries
template <bool RAW>
VR_DEV void tf2d_axis(float x, int n, int &i0, int &i1, float &w)
{
    const float ub = tff_coord<RAW>(x) * (float)n - 0.5f;
    const float fl = floorf(ub);
    w = ub - fl;
    const int i = (int)fl;
    i0 = iclamp(i, 0, n - 1);
    i1 = iclamp(i + 1, 0, n - 1);
}

// Can a sample of value s be anything but transparent?  (the two columns its value axis reads)
template <bool RAW>
VR_DEV bool tf2d_may_show(const Tf2dView &tf, float s)
{
    int i0, i1;
    float a;
    tf2d_axis<RAW>(s, (int)tf.n_v, i0, i1, a);
    return tf.nz[i1 + 1] != tf.nz[i0];
}

// include/vrhip.h's lookup: value axis by s (RAW: a FLOAT volume's raw value), gradient axis by m * inv_ghi
template <bool RAW>
VR_DEV float4 tf2d_lookup(const Tf2dView &tf, float s, float m)
{
    int i0, i1, j0, j1;
    float a, b;
    tf2d_axis<RAW>(s, (int)tf.n_v, i0, i1, a);
    tf2d_axis<true>(m * tf.inv_ghi, (int)tf.n_g, j0, j1, b);
    const float4 *row0 = tf.table + (uint32_t)j0 * tf.n_v, *row1 = tf.table + (uint32_t)j1 * tf.n_v;
    const float4 e00 = row0[i0], e01 = row0[i1], e10 = row1[i0], e11 = row1[i1];
    float4 c;
    c.x = lerpf(lerpf(e00.x, e01.x, a), lerpf(e10.x, e11.x, a), b);
    c.y = lerpf(lerpf(e00.y, e01.y, a), lerpf(e10.y, e11.y, a), b);
    c.z = lerpf(lerpf(e00.z, e01.z, a), lerpf(e10.z, e11.z, a), b);
    c.w = lerpf(lerpf(e00.w, e01.w, a), lerpf(e10.w, e11.w, a), b);
    return c;
}

// s2 - s1 of gradientCentralDiff: Vol::neg_gradient's taps, blends and difference (vr_sampling.h -- the 4x4x4
// neighbourhood loaded once, 32 voxels), before the normalisation: technique 6 needs the length as well.  A COPY of
// those lines: the two must stay the same operation for operation -- with every row of the table equal a technique-6
// frame is technique 0's bit for bit (tests/test_tf2d_ref.py pins the restatement to that, tests/test_gpu_tf2d.py
// this kernel to the restatement).  Change neither without the other.
template <typename V>
VR_DEV f3 tf2d_central_diff(const V &vol, float px, float py, float pz)
{
    const float ub = px * vol.fw - 0.5f, vb = py * vol.fh - 0.5f, sb = pz * vol.fd - 0.5f;
    const float fx = floorf(ub), fy = floorf(vb), fz = floorf(sb);
    const float a = ub - fx, b = vb - fy, c = sb - fz;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    int X[4], Y[4], Z[4];
    uint32_t xo[4], yo[4];
    unsigned long long zo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        X[k] = iclamp(ix - 1 + k, 0, vol.w1);
        Y[k] = iclamp(iy - 1 + k, 0, vol.h1);
        Z[k] = iclamp(iz - 1 + k, 0, vol.d1);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xo[k] = vol.xoff(X[k]);
        yo[k] = vol.yoff(Y[k]);
        zo[k] = vol.zoff(Z[k]);
    }
#define VR_L(xi, yi, zi) vol.raw(xo[xi], yo[yi], zo[zi], X[xi], Y[yi], Z[zi])
#define VR_R(yi, zi) lerpf(VR_L(1, yi, zi), VR_L(2, yi, zi), a)   /* texels (x0, x1)   */
#define VR_M(yi, zi) lerpf(VR_L(0, yi, zi), VR_L(1, yi, zi), a)   /* texels (x0-1, x0) */
#define VR_P(yi, zi) lerpf(VR_L(2, yi, zi), VR_L(3, yi, zi), a)   /* texels (x1, x1+1) */
    const float r01 = VR_R(0, 1), r11 = VR_R(1, 1), r21 = VR_R(2, 1), r31 = VR_R(3, 1);
    const float r02 = VR_R(0, 2), r12 = VR_R(1, 2), r22 = VR_R(2, 2), r32 = VR_R(3, 2);
    const float r10 = VR_R(1, 0), r20 = VR_R(2, 0), r13 = VR_R(1, 3), r23 = VR_R(2, 3);
    f3 s1, s2;
    s1.x = lerpf(lerpf(VR_M(1, 1), VR_M(2, 1), b), lerpf(VR_M(1, 2), VR_M(2, 2), b), c) * vol.inv_max;
    s2.x = lerpf(lerpf(VR_P(1, 1), VR_P(2, 1), b), lerpf(VR_P(1, 2), VR_P(2, 2), b), c) * vol.inv_max;
    s1.y = lerpf(lerpf(r01, r11, b), lerpf(r02, r12, b), c) * vol.inv_max;
    s2.y = lerpf(lerpf(r21, r31, b), lerpf(r22, r32, b), c) * vol.inv_max;
    s1.z = lerpf(lerpf(r10, r20, b), lerpf(r11, r21, b), c) * vol.inv_max;
    s2.z = lerpf(lerpf(r12, r22, b), lerpf(r13, r23, b), c) * vol.inv_max;
#undef VR_L
#undef VR_R
#undef VR_M
#undef VR_P
    return sub3(s2, s1);
}

// Bit k set: sample k of the run t0, t0 + stepSize, ... may read a column that is not transparent and has to be
// fetched.  (`grid`: the cell grid in the e* fields of a CellView, mm its (min, max) pairs.)
template <bool RAW, typename V>
VR_DEV uint32_t tf2d_need_mask(const CellView &grid, const float2 *mm, const V &vol, const RayCtx &c, float t0,
                               const Tf2dView &tf, bool linear)
{
    const CellLine line = cell_line_ray(add3(c.cam, scale3(c.dir, t0 - c.offset)), c.dir, c.stepSize, vol, grid.eshift,
                                        grid.ecx, grid.ecy, grid.ecz);
    constexpr float kHalfMax = 0x1.fffffep126f;   // FLT_MAX / 2
    uint32_t need = 0;
#pragma unroll VR_TF2D_MASK_UNROLL
    for (int k = 0; k < kTf2dLook; ++k) {
        const float2 b = mm[cell_index_of(cell_at(line, (float)k), grid.ecx, grid.ecy)];
        float lo = b.x * vol.inv_max, hi = b.y * vol.inv_max;
        if (!linear) { lo = vmin(lo, 0.f); hi = vmax(hi, 0.f); }   // (the border colour)
        int i0, i1, unused;
        float w;
        tf2d_axis<RAW>(lo, (int)tf.n_v, i0, unused, w);
        tf2d_axis<RAW>(hi, (int)tf.n_v, unused, i1, w);
        const bool known = b.x <= b.y && fabsf(b.x) <= kHalfMax && fabsf(b.y) <= kHalfMax && tf.nz[i1 + 1] == tf.nz[i0];
        need |= known ? 0u : (1u << k);
    }
    return need;
}

// Registers (the compiler's resource report for the twelve instantiations).  ISO's question -- does
// the gradient fit under 80 VGPRs at six waves per SIMD -- has another answer here: ISO's gradient stage runs after
// its march and keeps two ray parameters alive; this one sits INSIDE the march, with the ray, the background, the
// running colour and alpha, the waiting value and the lookahead mask alive across its 32 loads.  Asked for six waves
// (80 VGPRs) every instantiation spills, 44-88 bytes a lane; for five (96) all but UCHAR's uncounted pair still do
// (24-44 bytes).  Four waves: 112 / 114 / 116 VGPRs (UCHAR / USHORT / FLOAT), the counted instantiations 118 / 120 /
// 122, no scratch, no LDS.  So four waves per SIMD, occupancy 4, against the six of MIP and ISO.  (The mask loop is
// unrolled by four, not whole: whole, the counted FLOAT kernel spills 8 bytes at four waves.)
#ifndef VR_TF2D_WAVES
#define VR_TF2D_WAVES 4
#endif
#define VR_TF2D_OCC __attribute__((amdgpu_waves_per_eu(VR_TF2D_WAVES, VR_TF2D_WAVES)))

// STATS: the counted instantiation (vrhip_set_stats_enabled) -- three counters a lane and their reduction; the
// uncounted one carries none of it.
template <typename VT, bool VIEWS, bool STATS>
__global__ __launch_bounds__(kBlockDim) VR_TF2D_OCC void vr_tf2d_kernel(VolView vv, Tf2dView tf, CellView grid,
                                                                        const float2 *cell_mm, FrameView fr,
                                                                        vrhip_camera_params cam, vrhip_rendering_params rp,
                                                                        vrhip_raycast_params rc, DevStats *stats)
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
    // (the illumination invariants are made in the evaluation stage, from c.dir: the search does not carry them)
    if constexpr (VIEWS) {
        const vrhip_camera_params fc = load_frame_cam<true>(fr.cams, frame_idx);
        setup_ray_head<false>(gx, gy, inside, fr, fc, rp, c, d, seed, rnd);
    } else {
        setup_ray_head<false>(gx, gy, inside, fr, cam, rp, c, d, seed, rnd);
    }
    setup_ray_tail<false>(rc, resf, voxLen, no_bricks, c, d, rnd);

    constexpr bool RAW = kRawDensity<VT>;
    const bool linear = rp.useLinear != 0;
    const bool skip = cell_mm != nullptr;
    const bool shade = rp.illumType == 1;
    const float refInterval = 1.f / rc.samplingRate;

    float t = d.t;
    bool alive = c.valid && t < c.tfar;
    // a ray that takes a sample: -0 components of the background become +0 (header); every other value keeps its bits
    float r0 = alive ? c.env0 + 0.f : c.env0, r1 = alive ? c.env1 + 0.f : c.env1, r2 = alive ? c.env2 + 0.f : c.env2;
    float alpha = 0.f;
    uint32_t need = 0, left = 0;   // the lookahead: bit 0 of need is the sample at t, `left` bits are valid
    uint32_t n_taken = 0, n_shaded = 0, n_skipped = 0;

    for (;;) {
        if (!__ballot(alive)) break;
        if (skip && alive && left == 0) {
            need = tf2d_need_mask<RAW>(grid, cell_mm, vol, c, t, tf, linear);
            left = kTf2dLook;
        }
        // ---- search: step over transparent samples; a lane that finds another one waits with (t, s)
        bool waiting = false;
        float s = 0.f;
#pragma unroll 1
        for (int k = 0; k < kTf2dLook; ++k) {
            const bool search = alive && !waiting && (!skip || left != 0);
            if (!__ballot(search)) break;
            const bool fetch = search && (!skip || (need & 1u));
            if (__ballot(fetch)) {
                if (fetch) {
                    const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
                    const float px = pos.x * 0.5f + 0.5f, py = pos.y * 0.5f + 0.5f, pz = pos.z * 0.5f + 0.5f;
                    s = linear ? vol.linear(px, py, pz) : vol.nearest(px, py, pz);
                    waiting = tf2d_may_show<RAW>(tf, s);
                }
            }
            if constexpr (STATS) {
                n_taken += fetch ? 1u : 0u;
                n_skipped += (search && !fetch) ? 1u : 0u;
            }
            need = search ? need >> 1 : need;
            left = (search && skip) ? left - 1u : left;
            // the next sample of a lane that has stepped over this one (alpha unchanged: no termination test)
            const bool step = search && !waiting;
            const float tn = t + c.stepSize;
            alive = step ? (tn > t && tn < c.tfar) : alive;
            t = step ? tn : t;
        }
        // ---- evaluate: gradient, lookup, shading and compositing, once for all waiting lanes
        if (__ballot(waiting)) {
            if (waiting) {
                const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
                const f3 g = tf2d_central_diff(vol, pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
                const float m = 0.5f * len3(g);
                float4 col = tf2d_lookup<RAW>(tf, s, m);
                if constexpr (STATS) ++n_shaded;
                if (shade && col.w > 0.1f) {
                    f3 n = normalize3(g);
                    if (dot3(g, g) == 0.0f) n = mk3(0.57735f, 0.57735f, 0.57735f);
                    n = neg3(n);
                    // the illumination invariants of setup_ray_head<true> and eval_batch's Blinn-Phong terms
                    const f3 toLight = neg3(c.dir);
                    const f3 lgt = normalize3(toLight);
                    f3 hv = add3(toLight, lgt);
                    const bool hvalid = !(dot3(hv, hv) < 1.e-6f);
                    hv = normalize3(hv);
                    const float ndl = vmax(0.f, dot3(n, lgt));
                    float sp = hvalid ? vr_powr(vmax(dot3(n, hv), 0.f), 40.f) : 0.0f;
                    sp = sp * 0.15f;
                    col.x = ((col.x * 0.15f) + ((col.x * ndl) * 0.7f)) + sp;
                    col.y = ((col.y * 0.15f) + ((col.y * ndl) * 0.7f)) + sp;
                    col.z = ((col.z * 0.15f) + ((col.z * ndl) * 0.7f)) + sp;
                }
                const float opacity = 1.f - vr_powr(1.f - col.w, refInterval);   // opacity correction (:864)
                const float oma = 1.f - alpha;
                r0 = r0 - ((c.env0 - col.x) * opacity) * oma;
                r1 = r1 - ((c.env1 - col.y) * opacity) * oma;
                r2 = r2 - ((c.env2 - col.z) * opacity) * oma;
                alpha = alpha + opacity * oma;
                // (double)alpha > 0.98 <=> alpha >= 0.98f (ERT_THRESHOLD, :28); then t += stepSize while t < tfar
                const float tn = t + c.stepSize;
                alive = !(alpha >= 0.98f) && tn > t && tn < c.tfar;
                t = tn;
            }
        }
    }

    if constexpr (STATS) {
        const unsigned long long cnt[6] = {n_taken, 0ull, n_shaded, 0ull, n_skipped, (c.valid && alpha > 0.f) ? 1ull : 0ull};
        flush_counters(stats, lane, cnt);
    }
    if (!inside) return;
    // (a ray that misses the box keeps the background's alpha; one that enters it reports what it accumulated, :898)
    const float4 o = make_float4(r0, r1, r2, c.valid ? alpha : c.env3);
    fr.fb[(size_t)gy * fr.W + gx] = o;
    if (fr.out) fr.out[(size_t)wt.out_base + (size_t)ly * fr.out_stride + lx] = o;
}

template <typename VT, bool VIEWS, bool STATS>
hipError_t launch_tf2d(const RaycastLaunch &a, hipStream_t stream)
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
            vr_launch_kernel(vr_tf2d_kernel<VT, VIEWS, STATS>, grid, block, 0, stream, start, stop, a.vol, a.tf2d, g,
                             a.cell_minmax, a.frame, a.cam, a.render, a.raycast, a.stats);
        },
        [](hipEvent_t) {});
}

template <typename VT>
hipError_t launch_tf2d_typed(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.instr) return a.frame.cams ? launch_tf2d<VT, true, true>(a, stream) : launch_tf2d<VT, false, true>(a, stream);
    return a.frame.cams ? launch_tf2d<VT, true, false>(a, stream) : launch_tf2d<VT, false, false>(a, stream);
}

} // namespace

hipError_t vr_launch_tf2d(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.info) {
        a.info->technique = VRHIP_TECHNIQUE_TF2D;
        a.info->work_items = a.frame.n_wave_tiles;
        a.info->empty_skip = a.cell_minmax ? 1u : 0u;
        a.info->instrumented = a.instr ? 1u : 0u;
    }
    return vr_for_format(a.format, [&](auto vt) { return launch_tf2d_typed<typename decltype(vt)::type>(a, stream); });
}
