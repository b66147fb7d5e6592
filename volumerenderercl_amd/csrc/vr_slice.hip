// vr_slice.hip -- slice views (vrhip_render_slices, include/vrhip.h "Slice views"): the kernel, its instantiations
// for the three voxel types and the launch entry vr_launch_slices.  Not a technique: no ray, no camera, no march.
//
// Definition (tests/ref/slice_ref.c restates it on the CPU).  All fp32, one rounded operation each:
//  * pixel (gx, gy) of a W x H image, row 0 at the top: sx = (2 (gx + 0.5)) / W - 1, sy = 1 - (2 (gy + 0.5)) / H,
//    p = (origin + sx * u) + sy * v per component, in box space (the volume is [-1, 1]^3);
//  * samples k = 0 .. N - 1: a_k = (k + 0.5) / N - 0.5, q_k = p + a_k * w, tex = q_k * 0.5 + 0.5; a sample is TAKEN
//    when 0 <= tex <= 1 on all three axes (a NaN fails); its value is Vol::linear / Vol::nearest at tex;
//  * reduction over the taken samples in order of k: MAX `s > m ? s : m` from -inf, MIN `s < m ? s : m` from +inf
//    (a NaN never replaces either), MEAN sum = sum + s from 0, then sum / (float)count;
//  * pixel: nothing taken -> backgroundColor; TF output -> technique 2's pixel (TF(val) over the background);
//    VALUE output -> (val, val, val, 1), a NaN val as the quiet NaN 0x7fc00000: fp32 arithmetic defines neither the
//    sign nor the payload of a NaN it hands on (here `q - p` negates p through a source modifier, sign of a NaN
//    included; an x86 subtraction does not), so the readout fixes them.
//
// Execution: one wave per 8x8 pixel patch, one lane per pixel -- the 64 fetches of a patch fall into few 4x4x4
// micro-bricks whatever the plane's orientation; the grid is patches x slices.  A wave reads its own slice's
// parameters from the device array: the index is the same for every lane, so the loads are scalar.  The slab loop
// takes kSliceUnroll samples per trip, their loads independent of each other (the reduction follows the fetches, in
// order of k), and ends with a tail of single samples for N not a multiple of it.  A sample that is not taken is
// fetched at the volume's centre instead -- never an address outside the volume, no branch around the loads -- and its
// value is left out of the reduction.  Only the plain micro-bricked volume is read: no footprint volume, no LDS.
#include "vr_sampling.h"

namespace {

constexpr int kSliceUnroll = 4;   // samples of a slab whose loads are in flight together

struct SliceAcc {
    float m;          // running maximum / minimum / sum
    uint32_t count;   // samples taken
};

// sample k of the slab through p: whether it is taken, and its value (unspecified when it is not)
template <typename VT, bool LINEAR>
VR_DEV bool slice_sample(const Vol<VT, 0, false> &vol, f3 p, f3 w, uint32_t k, float fn, float *s)
{
    const float a = ((float)k + 0.5f) / fn - 0.5f;
    const float tx = (p.x + a * w.x) * 0.5f + 0.5f;
    const float ty = (p.y + a * w.y) * 0.5f + 0.5f;
    const float tz = (p.z + a * w.z) * 0.5f + 0.5f;
    const bool taken = tx >= 0.f && tx <= 1.f && ty >= 0.f && ty <= 1.f && tz >= 0.f && tz <= 1.f;
    // (untaken: fetched at the centre of the volume and left out of the reduction -- the loads need no branch around
    // them and stay inside the volume whatever the coordinates were)
    const float cx = taken ? tx : 0.5f, cy = taken ? ty : 0.5f, cz = taken ? tz : 0.5f;
    *s = LINEAR ? vol.linear(cx, cy, cz) : vol.nearest(cx, cy, cz);
    return taken;
}

VR_DEV void slice_reduce(SliceAcc &acc, uint32_t mode, bool taken, float s)
{
    if (!taken) return;
    if (mode == VRHIP_SLICE_MAX) acc.m = s > acc.m ? s : acc.m;
    else if (mode == VRHIP_SLICE_MIN) acc.m = s < acc.m ? s : acc.m;
    else acc.m = acc.m + s;
    ++acc.count;
}

// the reduction of the n samples of the slab through p.  The filter is a template parameter so that the unrolled
// fetches below are straight-line code: the loads of kSliceUnroll samples are issued before the first is waited for.
template <typename VT, bool LINEAR>
VR_DEV SliceAcc slice_slab(const Vol<VT, 0, false> &vol, f3 p, f3 w, uint32_t n, uint32_t mode)
{
    const float fn = (float)n;
    SliceAcc acc;
    acc.m = mode == VRHIP_SLICE_MAX ? -__builtin_inff() : mode == VRHIP_SLICE_MIN ? __builtin_inff() : 0.f;
    acc.count = 0;
    uint32_t k = 0;
#pragma unroll 1
    for (; k + kSliceUnroll <= n; k += kSliceUnroll) {
        float s[kSliceUnroll];
        bool t[kSliceUnroll];
#pragma unroll
        for (int j = 0; j < kSliceUnroll; ++j) t[j] = slice_sample<VT, LINEAR>(vol, p, w, k + (uint32_t)j, fn, &s[j]);
#pragma unroll
        for (int j = 0; j < kSliceUnroll; ++j) slice_reduce(acc, mode, t[j], s[j]);
    }
#pragma unroll 1
    for (; k < n; ++k) {   // the tail: N not a multiple of kSliceUnroll
        float s;
        const bool t = slice_sample<VT, LINEAR>(vol, p, w, k, fn, &s);
        slice_reduce(acc, mode, t, s);
    }
    return acc;
}

// technique 2's pixel (vr_mip.hip mip_pixel): c = TF(val), rgb = c.rgb * c.a + bg.rgb * (1 - c.a), a = c.a + bg.a * (1 - c.a)
template <bool RAW>
VR_DEV float4 slice_tf_pixel(const float4 *tff, int n, float val, const float (&bg)[4])
{
    const float4 c = tff_linear<RAW>(tff, n, val);
    const float oma = 1.f - c.w;
    float4 o;
    o.x = (c.x * c.w) + (bg[0] * oma);
    o.y = (c.y * c.w) + (bg[1] * oma);
    o.z = (c.z * c.w) + (bg[2] * oma);
    o.w = c.w + (bg[3] * oma);
    return o;
}

template <typename VT>
__global__ __launch_bounds__(kBlockDim) void vr_slice_kernel(VolView vv, TfView tf, const vrhip_slice_params *__restrict__ slices,
                                                             uint32_t W, uint32_t H, uint32_t patches_x, uint32_t patches,
                                                             uint32_t n_waves, uint32_t use_linear, float bg0, float bg1,
                                                             float bg2, float bg3, float4 *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    // (the wave's number, made uniform for the compiler: the slice's parameters are then scalar loads)
    const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlockDim / 64) + (threadIdx.x >> 6));
    if (q >= n_waves) return;
    const uint32_t slice = q / patches, patch = q - slice * patches;
    const uint32_t prow = patch / patches_x, pcol = patch - prow * patches_x;
    const uint32_t gx = pcol * 8u + (lane & 7u), gy = prow * 8u + (lane >> 3);
    if (gx >= W || gy >= H) return;   // (no wave-wide operation below)

    const vrhip_slice_params &sp = slices[slice];
    const uint32_t n = sp.samples, mode = sp.mode;
    const bool linear = use_linear != 0;
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);

    const float sx = (2.f * ((float)gx + 0.5f)) / (float)W - 1.f;
    const float sy = 1.f - (2.f * ((float)gy + 0.5f)) / (float)H;
    const f3 p = mk3((sp.origin[0] + sx * sp.u[0]) + sy * sp.v[0], (sp.origin[1] + sx * sp.u[1]) + sy * sp.v[1],
                     (sp.origin[2] + sx * sp.u[2]) + sy * sp.v[2]);
    const f3 w = mk3(sp.w[0], sp.w[1], sp.w[2]);
    const SliceAcc acc = linear ? slice_slab<VT, true>(vol, p, w, n, mode) : slice_slab<VT, false>(vol, p, w, n, mode);

    const float bg[4] = {bg0, bg1, bg2, bg3};
    float4 o = make_float4(bg0, bg1, bg2, bg3);
    if (acc.count) {
        const float val = mode == VRHIP_SLICE_MEAN ? acc.m / (float)acc.count : acc.m;
        const float readout = val != val ? __uint_as_float(0x7fc00000u) : val;   // (one NaN, whatever arithmetic made of it)
        o = sp.output == VRHIP_SLICE_VALUE ? make_float4(readout, readout, readout, 1.f)
                                           : slice_tf_pixel<kRawDensity<VT>>(tf.tff, (int)tf.tff_n, val, bg);
    }
    out[((size_t)slice * H + gy) * W + gx] = o;
}

} // namespace

hipError_t vr_launch_slices(const VolView &vol, int format, const TfView &tf, const vrhip_slice_params *slices_dev,
                            uint32_t n_slices, uint32_t W, uint32_t H, uint32_t use_linear, const float bg[4],
                            float4 *out_dev, hipStream_t stream)
{
    const uint32_t patches_x = (W + 7u) / 8u, patches = patches_x * ((H + 7u) / 8u);
    const unsigned long long n_waves = (unsigned long long)patches * n_slices;
    const uint32_t waves = kBlockDim / 64;
    if (n_waves == 0 || n_waves > 0xffffffffull) return hipErrorInvalidValue;   // (the kernel counts waves in 32 bits)
    const dim3 grid((uint32_t)((n_waves + waves - 1u) / waves)), block(kBlockDim);
    return vr_for_format(format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        hipLaunchKernelGGL(vr_slice_kernel<VT>, grid, block, 0, stream, vol, tf, slices_dev, W, H, patches_x, patches,
                           (uint32_t)n_waves, use_linear, bg[0], bg[1], bg[2], bg[3], out_dev);
        return hipGetLastError();
    });
}
