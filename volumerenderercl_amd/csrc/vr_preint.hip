// vr_preint.hip -- technique 8, ray casting with pre-integrated classification (VRHIP_TECHNIQUE_PREINT,
// include/vrhip.h): the kernel, its instantiations for the three voxel types and the launch entry vr_launch_preint.
//
// Definition (include/vrhip.h "technique == 8"; tests/ref/preint_ref.c restates it on the CPU):
//  * the ray is technique 0's -- make_ray, setup_ray_head / setup_ray_tail without object-order ESS -- and the loop
//    technique 6's (vr_tf2d.hip): composite slab k, stop when alpha >= 0.98f, t_{k+1} = t_k + stepSize while
//    t_{k+1} < tfar; a step that no longer moves t ends the sequence;
//  * slab k lies between the samples k - 1 and k (the first: k and k): u = tff_linear's table coordinate of the
//    filtered value, (Cbar, abar) = the transfer function's opacity-weighted mean colour and mean opacity over
//    [min(u_{k-1}, u_k), max(..)], vr_preint_math.h's preint::slab -- the text the host's vrhip_preint_slab compiles;
//    u_{k-1} == u_k: tff_linear's read;
//  * illumType 1 and abar > 0.1f: eval_batch's Blinn-Phong terms with Vol::neg_gradient at sample k; then eval_batch's
//    opacity correction and the ray caster's compositing from (backgroundColor, alpha 0).
//
// Execution: vr_tf2d_kernel's launch shape -- one wave per 8x8 patch, one lane per ray, the grid is the work list, no
// LDS -- and its two stages per round:
//  * search: a lane fetches s_k and steps on while slab k is transparent: the entries i0(min(u_{k-1}, u_k)) ..
//    i1(max(..)) hold no alpha != 0, one difference of the prefix count nz.  It carries u_k on as the next u_{k-1}.  A
//    lane that finds a slab that is not transparent waits with (t, u_{k-1}, u_k);
//  * evaluate: the whole wave enters the classification (two table entries and one prefix entry per slab end, a few
//    dozen fp64 operations), the gradient and the compositing ONCE for all waiting lanes.
// A lane never looks past a slab it has not composited.
//
// Why leaving out a transparent slab changes no bit.  The entries a slab can read are those of tff_linear at its two
// ends and every one between (the index arithmetic is monotone in u: vr_tf2d.hip's header).  All of them transparent:
// abar = +0 EXACTLY (vr_preint_math.h "Exact zero": sums of products of non-negative numbers, a difference x - x of
// prefix values) and Cbar = 0 by definition, or -- u_{k-1} == u_k -- tff_linear's alpha fma(a, 0 - 0, 0) = +0 with a
// finite colour.  No shading (abar > 0.1f fails); opacity = 1 - vr_powr(1, y) = 0 exactly; alpha and, after the ray's
// first slab, every component of result keep their bits: vr_tf2d.hip's header has the argument, its -0 background
// case included, and it carries over word for word with "sample" read as "slab" -- a ray that takes a sample starts
// from bg + 0.0f.
//
// Skipping (object-order ESS on).  The cell found on the ray's cell line for sample k (as tf2d_need_mask finds it)
// bounds s_k: fl(min * inv_max) <= s_k <= fl(max * inv_max) when the cell has no NaN voxel and bounds within
// FLT_MAX / 2 (vr_mip.hip's header, both sides; nearest: the border colour 0 joins the range), and u is monotone in s.
// Slab k is PROVABLY TRANSPARENT, T_k, when the cells of samples k - 1 and k both have such bounds and the entries
// i0(min(lo_{k-1}, lo_k)) .. i1(max(hi_{k-1}, hi_k)) are all transparent: u_{k-1} and u_k both lie in that hull, so
// the slab's own entries i0(min(u_{k-1}, u_k)) .. i1(max(..)) are among them.  The HULL, not each cell alone: two
// transparent ranges on either side of a peak bound a slab that crosses the peak.  (i0 and i1 are monotone, so the
// hull's entries are min(i0_{k-1}, i0_k) .. max(i1_{k-1}, i1_k).  For the ray's first slab the hull is its one cell.)
// A value is read by slab k (as its back) and by slab k + 1 (as its front) and by nothing else -- the gradient is
// taken only for a slab that is classified.  So sample k is NOT FETCHED when T_k and T_{k+1}; every other sample is.
// Then: a slab with T_k is stepped over whatever was fetched (changes no bit, above); a slab without T_k has both its
// ends fetched (sample k - 1 because T_k fails, sample k likewise) and goes through the search stage's test on the
// real values.  The sample that ends a skipped run is fetched: it is the next slab's front.  The ray's last sample
// may or may not be fetched when its slab is provably transparent: T of the slab after it comes from a cell looked up
// past tfar (the border cell); nobody reads that value either way.
// EVERY SLAB'S T IS DECIDED ONCE.  The lookahead covers 16 samples and looks up 17 cells: the 17th, with the 16th,
// decides T_16, the slab that ends at the NEXT window's first sample, and with it whether sample 15 is fetched.  The
// next window looks that sample's cell up again, from a line with another origin, and may find another cell (both
// bound the sample; they need not agree on what they prove).  It must not decide the slab again: had the first
// decision been "transparent" and sample 15 left out, a second decision "not proved" would send the slab to the test
// on real values with a front that was never fetched.  So the bit T_16 is carried into the next window and IS its
// T_0; only T_1 .. T_16 are made from that window's own cells (each from two cells of one line, each a true bound of
// its sample).  With that, "a slab without T_k has both ends fetched" holds across windows: need_{k-1} and need_k
// both read the one bit T_k.  And a step over a sample that was not fetched leaves u_{k-1} alone rather than writing
// a made-up coordinate: a stale front is only ever met by a slab with T_k, which does not read it.
//
// Registers (the compiler's resource report, hipcc -Rpass-analysis=kernel-resource-usage): see
// VR_PREINT_OCC below.
#include "vr_raycast_kernels.h"
#include "vr_preint_math.h"

namespace {

constexpr int kPreintLook = 16;   // samples a lane looks ahead per round (bits of the masks)
#ifndef VR_PREINT_MASK_UNROLL
#define VR_PREINT_MASK_UNROLL 1
#endif

// A sample's cell, as the table entries its value range can read.  i0 < 0: no usable bounds.
struct PreintCell {
    int i0, i1;
};
constexpr int kPreintFirst = -1;   // `carry` of a ray's first window: its first slab's hull is its one cell

// are the entries i0..i1 all transparent?
VR_DEV bool preint_transparent(const PreintView &tf, int i0, int i1) { return tf.nz[i1 + 1] == tf.nz[i0]; }

// Low 16 bits: bit k set when sample k of the run t0, t0 + stepSize, ... has to be fetched (not both T_k and T_{k+1}).
// High 16 bits: bit 16 + k set when slab k is provably transparent (T_k).  carry: on entry T of the slab that ends at
// sample 0 as the window before decided it (0 / 1; kPreintFirst: the ray's first slab, decided here from its one
// cell); on return T_16, the next window's.  (`grid`: the cell grid in the e* fields of a CellView, mm its pairs.)
template <bool RAW, typename V>
VR_DEV uint32_t preint_masks(const CellView &grid, const float2 *mm, const V &vol, const RayCtx &c, float t0,
                             const PreintView &tf, bool linear, int &carry)
{
    const CellLine line = cell_line_ray(add3(c.cam, scale3(c.dir, t0 - c.offset)), c.dir, c.stepSize, vol, grid.eshift,
                                        grid.ecx, grid.ecy, grid.ecz);
    constexpr float kHalfMax = 0x1.fffffep126f;   // FLT_MAX / 2
    const int n = (int)tf.n;
    uint32_t T = 0;
    PreintCell p;
    p.i0 = p.i1 = 0;
#pragma unroll VR_PREINT_MASK_UNROLL
    for (int k = 0; k <= kPreintLook; ++k) {
        const float2 b = mm[cell_index_of(cell_at(line, (float)k), grid.ecx, grid.ecy)];
        float lo = b.x * vol.inv_max, hi = b.y * vol.inv_max;
        if (!linear) { lo = vmin(lo, 0.f); hi = vmax(hi, 0.f); }   // (the border colour)
        const bool known = b.x <= b.y && fabsf(b.x) <= kHalfMax && fabsf(b.y) <= kHalfMax;
        PreintCell q;
        preint::columns(preint::table_coord(RAW, lo, n), preint::table_coord(RAW, hi, n), n, &q.i0, &q.i1);
        q.i0 = known ? q.i0 : -1;
        if (k == 0) p = q;   // (the hull of the ray's first slab is its one cell; any other slab 0 is the carried bit)
        const int h0 = p.i0 < q.i0 ? p.i0 : q.i0, h1 = p.i1 > q.i1 ? p.i1 : q.i1;   // the hull's entries
        bool t = p.i0 >= 0 && q.i0 >= 0 && preint_transparent(tf, h0 < 0 ? 0 : h0, h1);   // (the index: in bounds always)
        if (k == 0 && carry != kPreintFirst) t = carry != 0;
        T |= t ? (1u << k) : 0u;
        p = q;
    }
    carry = (int)((T >> kPreintLook) & 1u);
    const uint32_t need = ~(T & (T >> 1)) & 0xffffu;
    return need | (T << 16);
}

// Registers (the compiler's resource report for the twelve instantiations).  The supposition that this
// kernel is lighter than technique 6's did not hold: the classification keeps four fp64 sums, two coordinates and
// the reciprocal alive (two VGPRs each) next to the ray, and the 32-voxel gradient still follows it.  Left alone (three
// waves) the kernels take about 140 VGPRs, the counted ones 144.  Asked for five waves (96 VGPRs) every instantiation
// spills, 32-80 bytes a lane.  Four waves (128): the uncounted kernels fit -- 116 / 119 / 124 VGPRs (UCHAR / USHORT /
// FLOAT), no scratch; the counted ones reach 128 and the FLOAT pair spills 16-20 bytes.  So the uncounted
// instantiations run at four waves per SIMD, technique 6's occupancy, and the counted ones (vrhip_set_stats_enabled,
// a diagnostic mode) at three, 144 VGPRs, no scratch.  No LDS.
#ifndef VR_PREINT_WAVES
#define VR_PREINT_WAVES 4
#endif
#ifndef VR_PREINT_WAVES_COUNTED
#define VR_PREINT_WAVES_COUNTED 3
#endif
#define VR_PREINT_OCC                                                                                                 \
    __attribute__((amdgpu_waves_per_eu(STATS ? VR_PREINT_WAVES_COUNTED : VR_PREINT_WAVES,                            \
                                       STATS ? VR_PREINT_WAVES_COUNTED : VR_PREINT_WAVES)))

// STATS: the counted instantiation (vrhip_set_stats_enabled) -- three counters a lane and their reduction; the
// uncounted one carries none of it.
template <typename VT, bool VIEWS, bool STATS>
__global__ __launch_bounds__(kBlockDim) VR_PREINT_OCC void vr_preint_kernel(VolView vv, PreintView tf, CellView grid,
                                                                            const float2 *cell_mm, FrameView fr,
                                                                            vrhip_camera_params cam,
                                                                            vrhip_rendering_params rp,
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
    const int n = (int)tf.n;
    const float *tff = (const float *)tf.tff;
    bool first = true;       // no slab of this ray has been passed yet: the next one's front is its own back
    float uprev = 0.f;       // u_{k-1}; stale after a sample that was not fetched -- then T of the next slab holds
    int carry = kPreintFirst;   // T of the slab that ends at the next window's first sample (skip; header)
    // the lookahead: bit 0 of need / bit 16 of it (T) belong to the sample at t and the slab it ends; `left` are valid
    uint32_t look = 0, left = 0;
    uint32_t n_taken = 0, n_shaded = 0, n_skipped = 0;

    for (;;) {
        if (!__ballot(alive)) break;
        if (skip && alive && left == 0) {
            look = preint_masks<RAW>(grid, cell_mm, vol, c, t, tf, linear, carry);
            left = kPreintLook;
        }
        // ---- search: step over transparent slabs; a lane that finds another one waits with (t, uprev, u)
        bool waiting = false;
        float u = 0.f;
#pragma unroll 1
        for (int k = 0; k < kPreintLook; ++k) {
            const bool search = alive && !waiting && (!skip || left != 0);
            if (!__ballot(search)) break;
            const bool fetch = search && (!skip || (look & 1u));
            if (__ballot(fetch)) {
                if (fetch) {
                    const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
                    const float px = pos.x * 0.5f + 0.5f, py = pos.y * 0.5f + 0.5f, pz = pos.z * 0.5f + 0.5f;
                    const float s = linear ? vol.linear(px, py, pz) : vol.nearest(px, py, pz);
                    u = preint::table_coord(RAW, s, n);
                    int i0, i1;
                    preint::columns(first ? u : uprev, u, n, &i0, &i1);
                    waiting = !(skip && (look & 0x10000u)) && !preint_transparent(tf, i0, i1);
                }
            }
            if constexpr (STATS) {
                n_taken += fetch ? 1u : 0u;
                n_skipped += (search && !fetch) ? 1u : 0u;
            }
            look = search ? ((look >> 1) & 0x7fff7fffu) : look;
            left = (search && skip) ? left - 1u : left;
            // the next sample of a lane that has stepped over this slab (alpha unchanged: no termination test)
            const bool step = search && !waiting;
            const float tn = t + c.stepSize;
            alive = step ? (tn > t && tn < c.tfar) : alive;
            t = step ? tn : t;
            uprev = (step && fetch) ? u : uprev;
            first = step ? false : first;
        }
        // ---- evaluate: classification, shading and compositing, once for all waiting lanes
        if (__ballot(waiting)) {
            if (waiting) {
                float col[4];
                preint::slab(tff, tf.prefix, n, first ? u : uprev, u, col);
                if constexpr (STATS) ++n_shaded;
                if (shade && col[3] > 0.1f) {
                    const f3 pos = add3(c.cam, scale3(c.dir, t - c.offset));
                    const f3 nrm = vol.neg_gradient(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
                    // the illumination invariants of setup_ray_head<true> and eval_batch's Blinn-Phong terms
                    const f3 toLight = neg3(c.dir);
                    const f3 lgt = normalize3(toLight);
                    f3 hv = add3(toLight, lgt);
                    const bool hvalid = !(dot3(hv, hv) < 1.e-6f);
                    hv = normalize3(hv);
                    const float ndl = vmax(0.f, dot3(nrm, lgt));
                    float sp = hvalid ? vr_powr(vmax(dot3(nrm, hv), 0.f), 40.f) : 0.0f;
                    sp = sp * 0.15f;
                    col[0] = ((col[0] * 0.15f) + ((col[0] * ndl) * 0.7f)) + sp;
                    col[1] = ((col[1] * 0.15f) + ((col[1] * ndl) * 0.7f)) + sp;
                    col[2] = ((col[2] * 0.15f) + ((col[2] * ndl) * 0.7f)) + sp;
                }
                const float opacity = 1.f - vr_powr(1.f - col[3], refInterval);   // opacity correction (:864)
                const float oma = 1.f - alpha;
                r0 = r0 - ((c.env0 - col[0]) * opacity) * oma;
                r1 = r1 - ((c.env1 - col[1]) * opacity) * oma;
                r2 = r2 - ((c.env2 - col[2]) * opacity) * oma;
                alpha = alpha + opacity * oma;
                // (double)alpha > 0.98 <=> alpha >= 0.98f (ERT_THRESHOLD, :28); then t += stepSize while t < tfar
                const float tn = t + c.stepSize;
                alive = !(alpha >= 0.98f) && tn > t && tn < c.tfar;
                t = tn;
                uprev = u;
                first = false;
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
hipError_t launch_preint(const RaycastLaunch &a, hipStream_t stream)
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
            vr_launch_kernel(vr_preint_kernel<VT, VIEWS, STATS>, grid, block, 0, stream, start, stop, a.vol, a.preint, g,
                             a.cell_minmax, a.frame, a.cam, a.render, a.raycast, a.stats);
        },
        [](hipEvent_t) {});
}

template <typename VT>
hipError_t launch_preint_typed(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.instr) return a.frame.cams ? launch_preint<VT, true, true>(a, stream) : launch_preint<VT, false, true>(a, stream);
    return a.frame.cams ? launch_preint<VT, true, false>(a, stream) : launch_preint<VT, false, false>(a, stream);
}

} // namespace

hipError_t vr_launch_preint(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.info) {
        a.info->technique = VRHIP_TECHNIQUE_PREINT;
        a.info->work_items = a.frame.n_wave_tiles;
        a.info->empty_skip = a.cell_minmax ? 1u : 0u;
        a.info->instrumented = a.instr ? 1u : 0u;
    }
    return vr_for_format(a.format, [&](auto vt) { return launch_preint_typed<typename decltype(vt)::type>(a, stream); });
}
