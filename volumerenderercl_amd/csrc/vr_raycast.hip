// vr_raycast.hip -- the ray caster's launch entry (vr_launch_raycast: the format switch over the units
// vr_raycast_int.hip and vr_raycast_f32.hip, whose kernels live in vr_raycast_kernels.h) and the kernels that do
// not depend on the voxel type: patch classes, the pixel-major index, the phase-2 counting sort, the image-order ESS resolve, the skip
// bitmaps.
#include "vr_raycast_kernels.h"

namespace {

// Patch classes: one wave per 8x8 patch, ONCE per camera / parameters / skip bitmap / tile set -- the frames of
// a set, and the frames after it while nothing changes, differ only in the jitter seed, which moves every
// ray by less than a pixel on a square frame, by up to max(gsx, gsy) / gs pixels along an axis in general
// (:625-628).  The wave sets up 64 rays WITHOUT jitter on a regular grid over the patch's pixel positions grown
// by that jitter range on the + side and by two pixels on every side ([8 tx - 2, 8 tx + 10] x [8 ty - 2,
// 8 ty + 10] on a square frame): the jittered rays of the patch's pixels, in any frame, lie inside the hull
// of these.  Class 1 when
//  * all 64 hull rays hit the box SHRUNK by a thousandth of its size (rays through a convex box from one
//    eye point -- or parallel rays -- form a convex set, so every ray inside the hull hits the shrunk box,
//    and the real box by a margin far above the slab test's rounding): c.valid holds for every ray;
//  * patch_is_clear holds for the hull rays (its tube bounds |cam - cam_r| + t |dir - dir_r| by the maximum
//    over the 64 rays: the hull's corners, one pixel outside anything a jittered ray can reach) -- no ray of
//    the patch can visit a brick that is not skipped;
//  * the patch lies inside the frame, and the background is one colour (no gradient, no environment map:
//    checked by the host, with iteration 0, no showEss, no image-order ESS).
// Then every pixel of the patch ends as (backgroundColor.rgb, alpha 0) -- setup_ray_head's start values through
// write_pixel -- in every frame: the pre-pass writes that and returns, ~30 instructions instead of ~800.
__global__ __launch_bounds__(kBlockDim) void vr_patch_class_kernel(SkipView skip, FrameView fr, vrhip_camera_params cam,
                                                                   vrhip_rendering_params rp, Grid grid,
                                                                   uint32_t n_patches, uint32_t set_frames, uint8_t *cls)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pi = blockIdx.x * (kBlockDim / 64) + (threadIdx.x >> 6);
    if (pi >= n_patches) return;
    const WaveTile wt = fr.queue[(size_t)pi * set_frames];
    // make_ray's geometry (:614-650) at a fractional pixel position, no jitter
    const float *V = cam.viewMat;
    const f3 ms = mk3(rp.modelScale[0], rp.modelScale[1], rp.modelScale[2]);
    const int maxImg = (int)(fr.gsx > fr.gsy ? fr.gsx : fr.gsy);
    // The jitter moves a ray by rnd * 2 / gsx and rnd * 2 / gsy in NDC (:625-628) while a pixel is 2 / maxImg wide:
    // by up to maxImg / gsx pixels in +x and maxImg / gsy in +y -- one pixel on a square frame, `aspect` pixels
    // along the short axis of any other.  The hull is the patch's pixel positions [8 t, 8 t + 7] grown by that
    // (rounded up) on the + side and by two pixels of margin on both: [8 t - 2, 8 t + 9 + ceil(maxImg / gs)].
    const float spanx = (float)(11u + ((uint32_t)maxImg + fr.gsx - 1u) / fr.gsx);
    const float spany = (float)(11u + ((uint32_t)maxImg + fr.gsy - 1u) / fr.gsy);
    const float fx = (float)(wt_col(wt) * 8u) - 2.f + (float)(lane & 7u) * (spanx / 7.f);
    const float fy = (float)(wt_row(wt) * 8u) - 2.f + (float)(lane >> 3) * (spany / 7.f);
    float icx = (fx / (float)maxImg) * 2.f, icy = (fy / (float)maxImg) * 2.f;
    if (fr.gsx > fr.gsy) { icx -= 1.0f; icy -= fr.ray_aspect; }
    else { icx -= fr.ray_aspect; icy -= 1.0f; }
    icy *= -1.f;
    f3 npp = mk3(icx, icy, -1.0f);
    f3 rayDir = mk3(dot3(mk3(V[0], V[1], V[2]), npp), dot3(mk3(V[4], V[5], V[6]), npp), dot3(mk3(V[8], V[9], V[10]), npp));
    f3 camPos = mul3(mk3(V[3], V[7], V[11]), ms);
    if (cam.ortho) {
        camPos = mk3(V[3], V[7], V[11]);
        rayDir = neg3(mk3(V[2], V[6], V[10]));
        npp = add3(add3(camPos, scale3(mk3(V[0], V[4], V[8]), icx)), scale3(mk3(V[1], V[5], V[9]), icy));
        npp = scale3(npp, len3(camPos));
        camPos = mul3(npp, ms);
    }
    rayDir = normalize3(mul3(rayDir, ms));
    const float o[3] = {camPos.x, camPos.y, camPos.z}, dv[3] = {rayDir.x, rayDir.y, rayDir.z};
    float tn = -3.0e38f, tf = 3.0e38f, tns = -3.0e38f, tfs = 3.0e38f;
    for (int i = 0; i < 3; ++i) {
        const float inv = 1.0f / dv[i];
        const float m = 1.0e-3f * (cam.bbox_tr[i] - cam.bbox_bl[i]);
        const float tb = inv * (cam.bbox_bl[i] - o[i]), tt = inv * (cam.bbox_tr[i] - o[i]);
        const float tbs = inv * (cam.bbox_bl[i] + m - o[i]), tts = inv * (cam.bbox_tr[i] - m - o[i]);
        tn = vmax(tn, vmin(tt, tb)); tf = vmin(tf, vmax(tt, tb));
        tns = vmax(tns, vmin(tts, tbs)); tfs = vmin(tfs, vmax(tts, tbs));
    }
    const bool hit_shrunk = (tfs > tns) && !(tfs < 0.f) && (tfs - tns) > 0.f;
    RayCtx c;
    c.cam = camPos;
    c.dir = rayDir;
    c.valid = (tf > tn) && !(tf < 0.f);
    c.tnear = vmax(0.f, tn);
    c.tfar = tf;
    const bool inside = wt_col(wt) * 8u + 8u <= fr.W && wt_row(wt) * 8u + 8u <= fr.H;   // (uniform)
    const bool all_hit = __ballot(hit_shrunk) == ~0ull;
    bool clear = false;
    if (inside && all_hit && skip.near_bits) clear = patch_is_clear(skip, grid, c, lane);
    if (lane == 0) cls[pi] = clear ? 1 : 0;
}

// ------------------------------------------------------------------ pixel-major ray order

// The index of a launch set's rays in pixel-major order (vr_internal.h "pixel-major ray order"): one wave per patch of
// the set, behind the pre-pass.  The patch's set_frames notes (live ballot, first record) become one run of index
// entries -- pixel 0 in frames 0 .. set_frames - 1, pixel 1, ... -- appended as a whole to index list (patch %
// kLiveLists) and padded with kPmNone to a multiple of `group` (a power of two that divides 64).  A patch that is
// dead in every frame leaves at once.  The (pixel, frame) pairs are walked 64 at a time, so the writes are contiguous.
__global__ __launch_bounds__(kBlockDim) void vr_regroup_kernel(FrameView fr, uint32_t group)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = fr.n_wave_tiles, sf = fr.set_frames;
    const uint32_t p = blockIdx.x * (kBlockDim / 64) + (threadIdx.x >> 6);
    if (p >= n / sf) return;
    const uint32_t *notes = fr.pm + 2u * (size_t)p * sf;
    const uint32_t *first = fr.pm + 2u * (size_t)n + (size_t)p * sf;
    uint32_t total = 0;
    for (uint32_t f0 = 0; f0 < sf; f0 += 64u) {
        const uint32_t f = f0 + lane;
        const uint32_t c = f < sf ? (uint32_t)(__builtin_popcount(notes[2u * f]) + __builtin_popcount(notes[2u * f + 1u])) : 0u;
        total += (uint32_t)wave_sum((unsigned long long)c);
    }
    total = __builtin_amdgcn_readfirstlane(total);
    if (!total) return;
    const uint32_t padded = (total + group - 1u) & ~(group - 1u);   // <= 64 sf: within pm_list_cap for every patch of the list
    const uint32_t list = p % kLiveLists;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(fr.live_list_count + (kPmBase - kLiveBase) + list * kLiveStride, padded);
    base = __builtin_amdgcn_readfirstlane(base);
    uint32_t *out = fr.pm + 3u * (size_t)n + (size_t)list * pm_list_cap(n, sf) + base;
    // pair i = pixel * sf + frame, i = 64 step + lane: both advance by 64 per step without a division in the loop
    const uint32_t dq = 64u / sf, dr = 64u % sf;
    uint32_t px = lane / sf, f = lane % sf, pos = 0;
    for (uint32_t step = 0; step < sf; ++step) {
        const unsigned long long m = (unsigned long long)notes[2u * f] | ((unsigned long long)notes[2u * f + 1u] << 32);
        const bool live = (m >> px) & 1ull;
        const unsigned long long b = __ballot(live);
        if (live) out[pos + VR_LANE_RANK(b)] = first[f] + (uint32_t)__builtin_popcountll(m & ((1ull << px) - 1ull));
        pos += (uint32_t)__builtin_popcountll(b);
        px += dq;
        f += dr;
        if (f >= sf) { f -= sf; ++px; }
    }
    for (uint32_t i = total + lane; i < padded; i += 64u) out[i] = kPmNone;
}

// ------------------------------------------------------------------ phase-2 ordering

// Counting sort of the suspended rays by their key (ContRec::pad = rounds needed last frame,
// clamped to kSortBins - 1), longest first.  Two small launches between the phases.
__global__ __launch_bounds__(kBlockDim) void vr_cont_hist_kernel(const ContRec *cont,
                                                                 const uint32_t *count,
                                                                 uint32_t *bins)
{
    __shared__ uint32_t s_bins[kSortBins];
    for (uint32_t i = threadIdx.x; i < kSortBins; i += kBlockDim) s_bins[i] = 0;
    __syncthreads();
    const uint32_t n = *count;
    for (uint32_t i = blockIdx.x * kBlockDim + threadIdx.x; i < n; i += gridDim.x * kBlockDim) {
        const uint32_t k = cont[i].pad < kSortBins ? cont[i].pad : kSortBins - 1u;
        atomicAdd(&s_bins[k], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kSortBins; i += kBlockDim)
        if (s_bins[i]) atomicAdd(&bins[i], s_bins[i]);
}

__global__ __launch_bounds__(kBlockDim) void vr_cont_scatter_kernel(const ContRec *cont,
                                                                    const uint32_t *count,
                                                                    const uint32_t *bins,
                                                                    uint32_t *cursors,
                                                                    uint32_t *order)
{
    __shared__ uint32_t s_off[kSortBins], s_cnt[kSortBins], s_base[kSortBins];
    // descending keys: bin k starts after all bins above it
    for (uint32_t k = threadIdx.x; k < kSortBins; k += kBlockDim) s_cnt[k] = bins[k];
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kSortBins; k += kBlockDim) {
        uint32_t o = 0;
        for (uint32_t j = k + 1; j < kSortBins; ++j) o += s_cnt[j];
        s_off[k] = o;
    }
    const uint32_t n = *count;
    const uint32_t chunk = kBlockDim * 4u;
    for (uint32_t c0 = blockIdx.x * chunk; c0 < n; c0 += gridDim.x * chunk) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < kSortBins; k += kBlockDim) s_cnt[k] = 0;
        __syncthreads();
        uint32_t key[4], rank[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = c0 + (uint32_t)j * kBlockDim + threadIdx.x;
            key[j] = kSortBins;
            rank[j] = 0;
            if (i < n) {
                key[j] = cont[i].pad < kSortBins ? cont[i].pad : kSortBins - 1u;
                rank[j] = atomicAdd(&s_cnt[key[j]], 1u);
            }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < kSortBins; k += kBlockDim)
            s_base[k] = s_cnt[k] ? atomicAdd(&cursors[k], s_cnt[k]) : 0u;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = c0 + (uint32_t)j * kBlockDim + threadIdx.x;
            if (i < n) order[s_off[key[j]] + s_base[key[j]] + rank[j]] = i;
        }
    }
}

// Image-order ESS, end of the frame (:918-924): the hit texel of every group of this launch.
// A skipped group and a group whose first work-item missed the box leave 0; otherwise the first
// work-item reports whether any work-item that reached the end changed its pixel.
__global__ __launch_bounds__(kBlockDim) void vr_hit_resolve_kernel(FrameView fr, uint8_t *hit_out)
{
    const uint32_t i = blockIdx.x * kBlockDim + threadIdx.x;
    if (i >= fr.n_wave_tiles) return;
    const WaveTile wt = fr.queue[i];
    const size_t g = (size_t)wt_row(wt) * fr.hit_w + wt_col(wt);
    hit_out[g] = fr.hit_status[g] == HIT_FIRST_ENDS ? fr.hit_any[g] : (uint8_t)0;
}

} // namespace

hipError_t vr_launch_cont_sort(const FrameView &frame, hipStream_t stream)
{
    hipLaunchKernelGGL(vr_cont_hist_kernel, dim3(128), dim3(kBlockDim), 0, stream, frame.cont, frame.cont_count,
                       frame.sort_ws);
    hipLaunchKernelGGL(vr_cont_scatter_kernel, dim3(128), dim3(kBlockDim), 0, stream, frame.cont, frame.cont_count,
                       frame.sort_ws, frame.sort_ws + kSortBins, frame.order);
    return hipGetLastError();
}

#if defined(VR_MARCH_STATS) || defined(VR_STAMPS)
// diagnostic array `which` summed over the units' copies into out[0, n)
static int debug_total(int which, unsigned long long *out, size_t n, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::fill(out, out + n, 0ull);
    if (vr_raycast_debug_int(which, out, n, reset) != 0) return -1;
    return vr_raycast_debug_f32(which, out, n, reset);
}
#endif

#ifdef VR_MARCH_STATS
// diagnostic builds only: read (and optionally clear) the round statistics of phase 1 and the pre-pass
extern "C" int vrhip_debug_march_stats(unsigned long long out[32], int reset)
{
    return debug_total(VR_DEBUG_MARCH_STATS, out, 32, reset);
}
#endif

#ifdef VR_STAMPS
// diagnostic builds only: start/end clock of every wave of the last launches (read and cleared)
extern "C" int vrhip_debug_wave_spans(unsigned long long *out /* [2][2][8192] */)
{
    return debug_total(VR_DEBUG_WAVE_SPAN, out, 2 * 2 * 8192, 1);
}
// diagnostic builds only: read (and optionally clear) the per-phase cycle totals
extern "C" int vrhip_debug_stamps(unsigned long long out[32], int reset)
{
    return debug_total(VR_DEBUG_STAMPS, out, 32, reset);
}
#endif

hipError_t vr_launch_raycast(const RaycastLaunch &a, hipStream_t stream)
{
    hipError_t e;
    switch (a.format) {
    case VRHIP_UCHAR: e = vr_launch_raycast_u8(a, stream); break;
    case VRHIP_USHORT: e = vr_launch_raycast_u16(a, stream); break;
    case VRHIP_FLOAT: e = vr_launch_raycast_f32(a, stream); break;
    default: return hipErrorInvalidValue;
    }
    if (e == hipSuccess && a.render.imgEss && a.hit_out && a.frame.n_wave_tiles) {
        const bool bind_stop = a.bind_events && a.stop_event && a.stop_bound;
        vr_launch_kernel(vr_hit_resolve_kernel, dim3((a.frame.n_wave_tiles + kBlockDim - 1) / kBlockDim),
                         dim3(kBlockDim), 0, stream, nullptr, bind_stop ? a.stop_event : nullptr, a.frame, a.hit_out);
        e = hipGetLastError();
        if (e == hipSuccess && bind_stop) *a.stop_bound = true;
    }
    return e;
}

namespace {

// SkipView::near_bits: bytes "brick is not skipped", dilated by `radius` bricks along one axis per
// launch, then packed to bits (same bit order as the skip bitmap)
__global__ __launch_bounds__(kBlockDim) void vr_skip_live_kernel(const uint32_t *bits, size_t n, uint8_t *live)
{
    const size_t i = (size_t)blockIdx.x * kBlockDim + threadIdx.x;
    if (i < n) live[i] = ((bits[i >> 5] >> (i & 31u)) & 1u) ? 0 : 1;
}
__global__ __launch_bounds__(kBlockDim) void vr_skip_dilate_kernel(const uint8_t *in, uint8_t *out, int bw, int bh,
                                                                   int bd, int axis, int radius)
{
    const size_t n = (size_t)bw * bh * bd;
    const size_t i = (size_t)blockIdx.x * kBlockDim + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % (size_t)bw), y = (int)((i / (size_t)bw) % (size_t)bh), z = (int)(i / ((size_t)bw * bh));
    const int pos = axis == 0 ? x : axis == 1 ? y : z, len = axis == 0 ? bw : axis == 1 ? bh : bd;
    const size_t stride = axis == 0 ? 1 : axis == 1 ? (size_t)bw : (size_t)bw * bh;
    uint8_t v = 0;
    for (int k = max(pos - radius, 0); k <= min(pos + radius, len - 1); ++k) v |= in[i + (size_t)(k - pos) * stride];
    out[i] = v;
}
__global__ __launch_bounds__(kBlockDim) void vr_skip_pack_kernel(const uint8_t *live, size_t n, uint32_t *bits,
                                                                 uint32_t n_words)
{
    const size_t i = (size_t)blockIdx.x * kBlockDim + threadIdx.x;
    const unsigned long long m = __ballot(i < n && live[i] != 0);
    if ((threadIdx.x & 63) == 0) {
        const size_t w = (i >> 6) * 2;
        if (w < n_words) bits[w] = (uint32_t)m;
        if (w + 1 < n_words) bits[w + 1] = (uint32_t)(m >> 32);
    }
}

} // namespace

hipError_t vr_launch_skip_near(const BrickView &bricks, const uint32_t *bits, uint32_t n_words, uint32_t radius,
                               uint8_t *scratch, uint32_t *near_bits, hipStream_t stream)
{
    const size_t n = (size_t)bricks.bw * bricks.bh * bricks.bd;
    dim3 grid((unsigned)((n + kBlockDim - 1) / kBlockDim)), block(kBlockDim);
    uint8_t *a = scratch, *b = scratch + n;
    hipLaunchKernelGGL(vr_skip_live_kernel, grid, block, 0, stream, bits, n, a);
    for (int axis = 0; axis < 3; ++axis) {
        hipLaunchKernelGGL(vr_skip_dilate_kernel, grid, block, 0, stream, (const uint8_t *)a, b, bricks.bw, bricks.bh,
                           bricks.bd, axis, (int)radius);
        uint8_t *t = a; a = b; b = t;
    }
    hipLaunchKernelGGL(vr_skip_pack_kernel, grid, block, 0, stream, (const uint8_t *)a, n, near_bits, n_words);
    return hipGetLastError();
}

hipError_t vr_launch_skipmap(const BrickView &bricks, int format, float inv_max, const TfView &tf,
                             uint32_t *bits, uint32_t n_words, hipStream_t stream)
{
    const size_t n = (size_t)bricks.bw * bricks.bh * bricks.bd;
    dim3 grid((unsigned)((n + kBlockDim - 1) / kBlockDim)), block(kBlockDim);
    switch (format) {
    case VRHIP_UCHAR:
        hipLaunchKernelGGL(vr_skipmap_kernel<uint8_t>, grid, block, 0, stream, bricks, inv_max, tf,
                           bits, n_words);
        break;
    case VRHIP_USHORT:
        hipLaunchKernelGGL(vr_skipmap_kernel<uint16_t>, grid, block, 0, stream, bricks, inv_max, tf,
                           bits, n_words);
        break;
    case VRHIP_FLOAT:
        hipLaunchKernelGGL(vr_skipmap_kernel<float>, grid, block, 0, stream, bricks, inv_max, tf,
                           bits, n_words);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t vr_launch_regroup(const FrameView &frame, uint32_t group, hipStream_t stream)
{
    if (!frame.pm || !frame.set_frames || (group != 1u && group != 32u && group != 64u)) return hipErrorInvalidValue;
    const uint32_t n_patches = frame.n_wave_tiles / frame.set_frames;
    if (!n_patches) return hipSuccess;
    hipLaunchKernelGGL(vr_regroup_kernel, dim3((n_patches + kBlockDim / 64 - 1u) / (kBlockDim / 64)), dim3(kBlockDim), 0, stream, frame, group);
    return hipGetLastError();
}

hipError_t vr_launch_patch_classes(const RaycastLaunch &a, uint32_t n_patches, uint32_t set_frames, uint8_t *cls,
                                   hipStream_t stream)
{
    if (!n_patches) return hipSuccess;
    const Grid hg = make_grid_host(a);
    hipLaunchKernelGGL(vr_patch_class_kernel, dim3((n_patches + 3u) / 4u), dim3(kBlockDim), 0, stream, a.skip, a.frame,
                       a.cam, a.render, hg, n_patches, set_frames, cls);
    return hipGetLastError();
}
