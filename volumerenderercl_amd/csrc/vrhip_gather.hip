// vrhip_gather.hip -- the tile gather of the multi-GPU drivers: packing a rank's tiles into its sparse message,
// and assembling frames from the ranks' messages on rank 0 (include/vrhip.h).
#include <algorithm>

#include "vr_renderer.h"

namespace {

__global__ __launch_bounds__(256) void vr_assemble_kernel(const float4 *staging, const uint32_t *slot_of_tile,
                                                          uint32_t W, uint32_t H, uint32_t tw, uint32_t th,
                                                          uint32_t tiles_x, float4 *frame)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const uint32_t slot = slot_of_tile[(y / th) * tiles_x + x / tw];
    frame[(size_t)y * W + x] = staging[((size_t)slot * th + (y % th)) * tw + (x % tw)];
}

// Multi-GPU, rank 0: the frames of a batch straight from the ranks' (sparse) gather messages, one thread per
// pixel -- tiles of one colour from their single pixel, the others from the message's whole tiles
// (TileDriver, tiles.py: message = [maxc slot numbers | S pixels | maxc whole tiles], S = frames x cap).
constexpr uint32_t kMaxGatherRanks = 64;
struct GatherMsgs { const float *p[kMaxGatherRanks]; };

__global__ __launch_bounds__(256) void vr_assemble_batch_kernel(GatherMsgs msgs, const int32_t *pos, const uint32_t *rank_slot,
                                                                uint32_t S, uint32_t cap, uint32_t maxc, uint32_t W, uint32_t H,
                                                                uint32_t tw, uint32_t th, uint32_t tiles_x, float4 *frames)
{
    // one workgroup per (tile, frame): the tile's rank, slot and position are looked up once, and a thread's
    // column inside the tile is fixed where the tile's width divides the workgroup (16 .. 256 pixels)
    const uint32_t t = blockIdx.x, f = blockIdx.y;
    const uint32_t rs = rank_slot[t];
    const uint32_t rank = rs >> 16, row = f * cap + (rs & 0xffffu);
    const float *m = msgs.p[rank];
    const int32_t p = pos[(size_t)rank * S + row];
    const uint32_t x0 = (t % tiles_x) * tw, y0 = (t / tiles_x) * th;
    float4 *dst = frames + ((size_t)f * H + y0) * W + x0;
    const uint32_t w = min(tw, W - x0), h = min(th, H - y0);   // (ragged right / bottom tiles)
    if (p < 0) {
        const float4 v = reinterpret_cast<const float4 *>(m + maxc)[row];
        if (256u % tw == 0u) {
            const uint32_t lx = threadIdx.x % tw;
            if (lx < w)
                for (uint32_t ly = threadIdx.x / tw; ly < h; ly += 256u / tw) dst[(size_t)ly * W + lx] = v;
        } else {
            for (uint32_t i = threadIdx.x; i < tw * th; i += 256u) {
                const uint32_t ly = i / tw, lx = i - ly * tw;
                if (lx < w && ly < h) dst[(size_t)ly * W + lx] = v;
            }
        }
        return;
    }
    const float4 *src = reinterpret_cast<const float4 *>(m + maxc + 4u * (size_t)S) + (size_t)p * th * tw;
    if (256u % tw == 0u) {
        const uint32_t lx = threadIdx.x % tw;
        if (lx < w)
            for (uint32_t ly = threadIdx.x / tw; ly < h; ly += 256u / tw) dst[(size_t)ly * W + lx] = src[ly * tw + lx];
    } else {
        for (uint32_t i = threadIdx.x; i < tw * th; i += 256u) {
            const uint32_t ly = i / tw, lx = i - ly * tw;
            if (lx < w && ly < h) dst[(size_t)ly * W + lx] = src[i];
        }
    }
}

// ---- the sparse gather message of a batch, packed on the GPU (vrhip_pack_tiles; the C++ host's TileGather):
// [spad slot numbers | one pixel per slot | the whole tiles], spad = n_slots rounded up to 4 -- the format
// vr_assemble_batch_kernel reads with maxc = spad (tiles.py packs the same with torch ops and maxc = the ranks'
// largest count).

// one workgroup per slot: is any pixel of the tile different (bit for bit) from its first?  Also the slot's pixel.
__global__ __launch_bounds__(256) void vr_pack_flags_kernel(const uint4 *tiles, uint32_t P, int32_t *flags, uint4 *uni)
{
    const uint32_t s = blockIdx.x;
    const uint4 *t = tiles + (size_t)s * P;
    const uint4 first = t[0];
    bool diff = false;
    for (uint32_t i = threadIdx.x; i < P; i += 256u) {
        const uint4 v = t[i];
        diff = diff || v.x != first.x || v.y != first.y || v.z != first.z || v.w != first.w;
    }
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

// one workgroup: flags -> position among the whole tiles (or -1), the slot list and the count
__global__ __launch_bounds__(1024) void vr_pack_scan_kernel(int32_t *flags_pos, uint32_t S, int32_t *slots, uint32_t *count)
{
    __shared__ uint32_t wave_sums[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < S; base += 1024u) {
        const uint32_t s = base + threadIdx.x;
        const bool f = s < S && flags_pos[s] != 0;
        const unsigned long long m = __ballot(f);
        const uint32_t below = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sums[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t off = carry;
        for (uint32_t w = 0; w < wave; ++w) off += wave_sums[w];
        if (s < S) {
            flags_pos[s] = f ? (int32_t)(off + below) : -1;
            if (f) slots[off + below] = (int32_t)s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < 16u; ++w) t += wave_sums[w];
            carry += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

// one workgroup per slot: a whole tile to its place in the message
__global__ __launch_bounds__(256) void vr_pack_copy_kernel(const uint4 *tiles, uint32_t P, const int32_t *pos, uint4 *out)
{
    const int32_t p = pos[blockIdx.x];
    if (p < 0) return;
    const uint4 *t = tiles + (size_t)blockIdx.x * P;
    uint4 *o = out + (size_t)p * P;
    for (uint32_t i = threadIdx.x; i < P; i += 256u) o[i] = t[i];
}

// root: pos[rank][row] = -1, then the position of every listed slot
__global__ __launch_bounds__(256) void vr_msg_pos_fill_kernel(int32_t *pos, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) pos[i] = -1;
}
struct GatherCounts { uint32_t c[kMaxGatherRanks]; };
__global__ __launch_bounds__(256) void vr_msg_pos_scatter_kernel(GatherMsgs msgs, GatherCounts counts, uint32_t S, int32_t *pos)
{
    const uint32_t rank = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= counts.c[rank]) return;
    const uint32_t slot = (uint32_t)reinterpret_cast<const int32_t *>(msgs.p[rank])[i];
    if (slot < S) pos[(size_t)rank * S + slot] = (int32_t)i;
}

} // namespace

void launch_pack_scan(hipStream_t st, int32_t *flags_pos, uint32_t n_slots, int32_t *slots, uint32_t *count)
{
    hipLaunchKernelGGL(vr_pack_scan_kernel, dim3(1), dim3(1024), 0, st, flags_pos, n_slots, slots, count);
}

extern "C" {

int vrhip_pack_tiles(vrhip_renderer *r, void *hip_stream, const float *tiles_dev, uint32_t n_slots, uint32_t tile_pixels,
                     int32_t *scratch_dev, float *msg_dev, uint32_t *count_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, tiles_dev && scratch_dev && msg_dev && count_dev && n_slots && tile_pixels &&
                      ((uintptr_t)tiles_dev & 15u) == 0 && ((uintptr_t)msg_dev & 15u) == 0,
               VRHIP_ERR_INVALID, "vrhip_pack_tiles: invalid argument (buffers must be 16-byte aligned)");
    if (set_device(r)) return VRHIP_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    const uint32_t spad = (n_slots + 3u) / 4u * 4u;
    hipLaunchKernelGGL(vr_pack_flags_kernel, dim3(n_slots), dim3(256), 0, st, (const uint4 *)tiles_dev, tile_pixels,
                       scratch_dev, (uint4 *)(msg_dev + spad));
    launch_pack_scan(st, scratch_dev, n_slots, (int32_t *)msg_dev, count_dev);
    hipLaunchKernelGGL(vr_pack_copy_kernel, dim3(n_slots), dim3(256), 0, st, (const uint4 *)tiles_dev, tile_pixels,
                       (const int32_t *)scratch_dev, (uint4 *)(msg_dev + spad + 4u * (size_t)n_slots));
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

int vrhip_message_positions(vrhip_renderer *r, void *hip_stream, const float *const *msgs_dev, const uint32_t *counts_host,
                            uint32_t world, uint32_t n_slots, int32_t *pos_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, msgs_dev && counts_host && pos_dev && world >= 1 && world <= kMaxGatherRanks && n_slots,
               VRHIP_ERR_INVALID, "vrhip_message_positions: invalid argument");
    if (set_device(r)) return VRHIP_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    GatherMsgs g;
    GatherCounts c;
    uint32_t maxc = 0;
    for (uint32_t i = 0; i < kMaxGatherRanks; ++i) {
        g.p[i] = i < world ? msgs_dev[i] : nullptr;
        c.c[i] = i < world ? counts_host[i] : 0u;
        VR_REQUIRE(r, c.c[i] <= n_slots && (i >= world || g.p[i]), VRHIP_ERR_INVALID,
                   "vrhip_message_positions: a count exceeds the number of slots, or a message is NULL");
        maxc = std::max(maxc, c.c[i]);
    }
    const uint32_t n = world * n_slots;
    hipLaunchKernelGGL(vr_msg_pos_fill_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, pos_dev, n);
    if (maxc)
        hipLaunchKernelGGL(vr_msg_pos_scatter_kernel, dim3((maxc + 255u) / 256u, world), dim3(256), 0, st, g, c, n_slots, pos_dev);
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

int vrhip_assemble_frame(vrhip_renderer *r, const float *staging_dev, const uint32_t *slot_of_tile_dev,
                         uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h,
                         float *frame_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, staging_dev && slot_of_tile_dev && frame_dev && width && height && tile_w && tile_h,
               VRHIP_ERR_INVALID, "vrhip_assemble_frame: invalid argument");
    if (set_device(r)) return VRHIP_ERR_HIP;
    const uint32_t tiles_x = (width + tile_w - 1) / tile_w;
    hipLaunchKernelGGL(vr_assemble_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, r->stream,
                       (const float4 *)staging_dev, slot_of_tile_dev, width, height, tile_w, tile_h, tiles_x,
                       (float4 *)frame_dev);
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

int vrhip_assemble_batch(vrhip_renderer *r, void *hip_stream, const float *const *msgs_dev, uint32_t world,
                         uint32_t n_frames, uint32_t cap, uint32_t maxc, const int32_t *pos_dev,
                         const uint32_t *rank_slot_of_tile_dev, uint32_t width, uint32_t height, uint32_t tile_w,
                         uint32_t tile_h, float *frames_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, msgs_dev && pos_dev && rank_slot_of_tile_dev && frames_dev && world >= 1 && world <= kMaxGatherRanks &&
                      n_frames && cap && cap <= 65536u && width && height && tile_w && tile_h && n_frames <= 65535u,
               VRHIP_ERR_INVALID, "vrhip_assemble_batch: invalid argument");
    if (set_device(r)) return VRHIP_ERR_HIP;
    GatherMsgs g;
    for (uint32_t i = 0; i < kMaxGatherRanks; ++i) g.p[i] = i < world ? msgs_dev[i] : nullptr;
    for (uint32_t i = 0; i < world; ++i)
        VR_REQUIRE(r, g.p[i] && ((uintptr_t)g.p[i] & 15u) == 0 && maxc % 4u == 0, VRHIP_ERR_INVALID,
                   "vrhip_assemble_batch: messages must be 16-byte aligned, maxc a multiple of 4");
    const uint32_t tiles_x = (width + tile_w - 1) / tile_w;
    const uint32_t tiles_y = (height + tile_h - 1) / tile_h;
    hipLaunchKernelGGL(vr_assemble_batch_kernel, dim3(tiles_x * tiles_y, n_frames), dim3(256), 0,
                       (hipStream_t)hip_stream, g, pos_dev, rank_slot_of_tile_dev, n_frames * cap, cap, maxc, width,
                       height, tile_w, tile_h, tiles_x, (float4 *)frames_dev);
    VR_HIP(r, hipGetLastError());
    return VRHIP_OK;
}

} // extern "C"
