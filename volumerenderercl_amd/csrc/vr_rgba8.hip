// vr_rgba8.hip -- 8-bit RGBA frames (include/vrhip.h "8-bit frames"): the quantiser of float pixels, and the
// 8-bit twins of the tile gather's pack and assembly kernels (vrhip_gather.hip).  Kernels of their own: nothing
// here touches the march, the pre-pass or the path tracer; they read the float pixels those have written.
//
// The conversion, per channel: q(f) = 0 for a NaN, else (uint8) rint(clamp(f * 255.0f, 0, 255)) -- one rounded
// fp32 multiply (the build has -ffp-contract=off), a clamp, round-half-to-even: OpenCL's
// convert_uchar_sat_rte(f * 255.0f), what write_imagef does on the reference's CL_UNORM_INT8 output image
// (volumerendercl.cpp:468-478).  A pixel is the word r | g << 8 | b << 16 | a << 24 (bytes R, G, B, A in memory).
#include <algorithm>

#include "vr_renderer.h"

namespace {

__device__ __forceinline__ uint32_t quantise_channel(float f)
{
    // (the NaN becomes 0 before the clamp: the conversion to an integer never sees one)
    const float v = fminf(fmaxf(f != f ? 0.0f : f * 255.0f, 0.0f), 255.0f);
    return (uint32_t)rintf(v);
}

__device__ __forceinline__ uint32_t quantise_pixel(float4 p)
{
    return quantise_channel(p.x) | quantise_channel(p.y) << 8 | quantise_channel(p.z) << 16 | quantise_channel(p.w) << 24;
}

// `rows` blocks of `row_pixels` float4 pixels, `src_stride` pixels apart in src, dense in dst: a frame (one row),
// a batch with a frame stride, a tile layout.  One pixel per lane: a 16-byte load (a wave reads 1 KiB in a piece)
// and a dword store (256 contiguous bytes per wave), so neither a row's length nor its stride has to be a
// multiple of anything and there is no tail to treat apart.  20 bytes per pixel, no reuse: a streaming kernel.
// blockIdx.y walks the rows (a grid has at most 65535 of them in y: the loop takes the rest).
__global__ __launch_bounds__(256) void vr_quantise_rgba8_kernel(const float4 *__restrict__ src, uint32_t rows,
                                                                uint32_t row_pixels, uint32_t src_stride,
                                                                uint32_t *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= row_pixels) return;
    for (uint32_t row = blockIdx.y; row < rows; row += gridDim.y)
        dst[(size_t)row * row_pixels + i] = quantise_pixel(src[(size_t)row * src_stride + i]);
}

// ---- the sparse gather message in 8-bit pixels (vrhip_pack_tiles_rgba8):
// [spad slot numbers of the whole tiles | one word per slot | the whole tiles, P words each], spad = n_slots rounded
// up to 4: the head is the float message's (vrhip_gather.hip), so vrhip_message_positions reads both.  The words
// behind the head are only 4-byte aligned (n_slots need not be a multiple of 4): dword accesses throughout.

// one workgroup per slot: is any QUANTISED pixel of the tile different from its first?  Also the slot's word.
__global__ __launch_bounds__(256) void vr_pack8_flags_kernel(const float4 *tiles, uint32_t P, int32_t *flags, uint32_t *uni)
{
    const uint32_t s = blockIdx.x;
    const float4 *t = tiles + (size_t)s * P;
    const uint32_t first = quantise_pixel(t[0]);
    bool diff = false;
    for (uint32_t i = threadIdx.x; i < P; i += 256u) diff = diff || quantise_pixel(t[i]) != first;
    __shared__ uint32_t any;
    if (threadIdx.x == 0) any = 0u;
    __syncthreads();
    if (__ballot(diff) && (threadIdx.x & 63u) == 0u) atomicOr(&any, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        flags[s] = any ? 1 : 0;
        uni[s] = first;
    }
}

// one workgroup per slot: a whole tile, quantised, to its place in the message
__global__ __launch_bounds__(256) void vr_pack8_copy_kernel(const float4 *tiles, uint32_t P, const int32_t *pos, uint32_t *out)
{
    const int32_t p = pos[blockIdx.x];
    if (p < 0) return;
    const float4 *t = tiles + (size_t)blockIdx.x * P;
    uint32_t *o = out + (size_t)p * P;
    for (uint32_t i = threadIdx.x; i < P; i += 256u) o[i] = quantise_pixel(t[i]);
}

// rank 0: the frames of a batch from the ranks' 8-bit messages -- vr_assemble_batch_kernel (vrhip_gather.hip) with
// a word per pixel: one workgroup per (tile, frame)
constexpr uint32_t kMaxGatherRanks8 = 64;
struct GatherMsgs8 { const uint32_t *p[kMaxGatherRanks8]; };

__global__ __launch_bounds__(256) void vr_assemble_batch_rgba8_kernel(GatherMsgs8 msgs, const int32_t *pos, const uint32_t *rank_slot,
                                                                      uint32_t S, uint32_t cap, uint32_t maxc, uint32_t W, uint32_t H,
                                                                      uint32_t tw, uint32_t th, uint32_t tiles_x, uint32_t *frames)
{
    const uint32_t t = blockIdx.x, f = blockIdx.y;
    const uint32_t rs = rank_slot[t];
    const uint32_t rank = rs >> 16, row = f * cap + (rs & 0xffffu);
    const uint32_t *m = msgs.p[rank];
    const int32_t p = pos[(size_t)rank * S + row];
    const uint32_t x0 = (t % tiles_x) * tw, y0 = (t / tiles_x) * th;
    uint32_t *dst = frames + ((size_t)f * H + y0) * W + x0;
    const uint32_t w = min(tw, W - x0), h = min(th, H - y0);   // (ragged right / bottom tiles)
    const uint32_t uni = m[maxc + row];
    const uint32_t *src = p < 0 ? nullptr : m + maxc + (size_t)S + (size_t)p * th * tw;
    for (uint32_t i = threadIdx.x; i < tw * th; i += 256u) {
        const uint32_t ly = i / tw, lx = i - ly * tw;
        if (lx < w && ly < h) dst[(size_t)ly * W + lx] = src ? src[i] : uni;
    }
}

int launch_quantise(vrhip_renderer *r, hipStream_t st, const float *src_dev, uint32_t rows, uint32_t row_pixels,
                    uint32_t src_stride, uint32_t *dst_dev)
{
    hipLaunchKernelGGL(vr_quantise_rgba8_kernel, dim3((uint32_t)(((uint64_t)row_pixels + 255u) / 256u), std::min(rows, 65535u)), dim3(256), 0, st,
                       (const float4 *)src_dev, rows, row_pixels, src_stride, dst_dev);
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

} // namespace

extern "C" {

int vrhip_quantise_rgba8(vrhip_renderer *r, void *hip_stream, const float *src_dev, uint32_t rows, uint32_t row_pixels,
                         uint32_t src_stride, uint8_t *dst, int dst_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, src_dev && dst, VRHIP_ERR_INVALID, "vrhip_quantise_rgba8: NULL argument");
    VR_REQUIRE(r, ((uintptr_t)src_dev & 15u) == 0 && (!dst_is_device || ((uintptr_t)dst & 3u) == 0), VRHIP_ERR_INVALID,
               "vrhip_quantise_rgba8: the source must be 16-byte aligned, a device destination 4-byte aligned");
    VR_REQUIRE(r, src_stride >= row_pixels, VRHIP_ERR_INVALID, "vrhip_quantise_rgba8: source stride smaller than a row");
    VR_REQUIRE(r, (unsigned long long)rows * row_pixels <= 0xffffffffull, VRHIP_ERR_INVALID,
               "vrhip_quantise_rgba8: rows x row_pixels must be below 2^32 pixels");
    if (set_device(r)) return VRHIP_ERR_HIP;
    if (rows == 0 || row_pixels == 0) return VRHIP_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    if (dst_is_device) return launch_quantise(r, st, src_dev, rows, row_pixels, src_stride, (uint32_t *)dst);
    // host destination: device words -> the renderer's pinned block -> the caller's memory, complete on return
    const size_t bytes = (size_t)rows * row_pixels * 4u;
    int rc = grow(r, r->rgba8_dev, bytes);
    if (rc) return rc;
    if ((rc = grow_pinned(r, r->rgba8_host, bytes))) return rc;
    if ((rc = launch_quantise(r, st, src_dev, rows, row_pixels, src_stride, r->rgba8_dev))) return rc;
    VR_HIP(r, hipMemcpyAsync(r->rgba8_host.p, r->rgba8_dev, bytes, hipMemcpyDeviceToHost, st));
    VR_HIP(r, hipStreamSynchronize(st));
    std::memcpy(dst, r->rgba8_host.p, bytes);
    return VRHIP_OK;
}

int vrhip_frame_rgba8(vrhip_renderer *r, uint32_t width, uint32_t height, uint8_t *out_rgba8, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, out_rgba8, VRHIP_ERR_INVALID, "vrhip_frame_rgba8: NULL output");
    VR_REQUIRE(r, r->fb && width && height && r->fb_w == width && r->fb_h == height, VRHIP_ERR_NODATA,
               "vrhip_frame_rgba8: the frame buffer holds no frame of this size");
    return vrhip_quantise_rgba8(r, r->stream, (const float *)(const float4 *)r->fb, 1, width * height, width * height,
                                out_rgba8, out_is_device);
}

int vrhip_render_frame_rgba8(vrhip_renderer *r, uint32_t width, uint32_t height, uint8_t *out_rgba8, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, out_rgba8, VRHIP_ERR_INVALID, "vrhip_render_frame_rgba8: NULL output");
    const int rc = vrhip_render_frame(r, width, height, nullptr, 0);   // the float frame stays in the frame buffer
    if (rc) return rc;
    return vrhip_frame_rgba8(r, width, height, out_rgba8, out_is_device);
}

int vrhip_pack_tiles_rgba8(vrhip_renderer *r, void *hip_stream, const float *tiles_dev, uint32_t n_slots, uint32_t tile_pixels,
                           int32_t *scratch_dev, uint32_t *msg_dev, uint32_t *count_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, tiles_dev && scratch_dev && msg_dev && count_dev && n_slots && tile_pixels &&
                      ((uintptr_t)tiles_dev & 15u) == 0 && ((uintptr_t)msg_dev & 15u) == 0,
               VRHIP_ERR_INVALID, "vrhip_pack_tiles_rgba8: invalid argument (buffers must be 16-byte aligned)");
    if (set_device(r)) return VRHIP_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    const uint32_t spad = (n_slots + 3u) / 4u * 4u;
    hipLaunchKernelGGL(vr_pack8_flags_kernel, dim3(n_slots), dim3(256), 0, st, (const float4 *)tiles_dev, tile_pixels,
                       scratch_dev, msg_dev + spad);
    launch_pack_scan(st, scratch_dev, n_slots, (int32_t *)msg_dev, count_dev);   // (the float message's: the same head)
    hipLaunchKernelGGL(vr_pack8_copy_kernel, dim3(n_slots), dim3(256), 0, st, (const float4 *)tiles_dev, tile_pixels,
                       (const int32_t *)scratch_dev, msg_dev + spad + (size_t)n_slots);
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

int vrhip_assemble_batch_rgba8(vrhip_renderer *r, void *hip_stream, const uint32_t *const *msgs_dev, uint32_t world,
                               uint32_t n_frames, uint32_t cap, uint32_t maxc, const int32_t *pos_dev,
                               const uint32_t *rank_slot_of_tile_dev, uint32_t width, uint32_t height, uint32_t tile_w,
                               uint32_t tile_h, uint8_t *frames_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, msgs_dev && pos_dev && rank_slot_of_tile_dev && frames_dev && world >= 1 && world <= kMaxGatherRanks8 &&
                      n_frames && cap && cap <= 65536u && width && height && tile_w && tile_h && n_frames <= 65535u,
               VRHIP_ERR_INVALID, "vrhip_assemble_batch_rgba8: invalid argument");
    if (set_device(r)) return VRHIP_ERR_HIP;
    GatherMsgs8 g;
    for (uint32_t i = 0; i < kMaxGatherRanks8; ++i) g.p[i] = i < world ? msgs_dev[i] : nullptr;
    for (uint32_t i = 0; i < world; ++i)
        VR_REQUIRE(r, g.p[i] && ((uintptr_t)g.p[i] & 15u) == 0 && maxc % 4u == 0 && ((uintptr_t)frames_dev & 3u) == 0,
                   VRHIP_ERR_INVALID,
                   "vrhip_assemble_batch_rgba8: messages must be 16-byte aligned, maxc a multiple of 4, the frames 4-byte aligned");
    const uint32_t tiles_x = (width + tile_w - 1) / tile_w;
    const uint32_t tiles_y = (height + tile_h - 1) / tile_h;
    hipLaunchKernelGGL(vr_assemble_batch_rgba8_kernel, dim3(tiles_x * tiles_y, n_frames), dim3(256), 0,
                       (hipStream_t)hip_stream, g, pos_dev, rank_slot_of_tile_dev, n_frames * cap, cap, maxc, width,
                       height, tile_w, tile_h, tiles_x, (uint32_t *)frames_dev);
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

} // extern "C"
