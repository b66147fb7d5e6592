// vr_ingest.hip -- the per-voxel work of the host loader (DatRawReader::read_raw, host/datrawreader.cpp)
// on the device: the maximum of a time step, the USHORT stretch / FLOAT normalisation in place over the
// micro-bricked slot, and the 256-bin histogram.  Everything the loader does per voxel is an
// order-independent reduction, one exact fp32 operation (a correctly rounded divide, or a multiply and a
// round) or an integer count, so the results are the loader's bit for bit (tests/test_gpu_ingest.py).
// All three kernels stream their input once with 16-byte loads per lane; the convert kernel is bound by
// HBM like vr_build_bricks_kernel, as long as its LDS histogram keeps up.
#include <algorithm>

#include "vr_ingest.h"

namespace {

constexpr int kMaxThreads = 256;       // max / de-interleave kernels
constexpr int kHistThreads = 512;      // convert kernel: 8 waves, one sub-histogram each
constexpr int kHistWaves = kHistThreads / 64;

__device__ inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
__device__ inline uint16_t bswap16(uint16_t v) { return (uint16_t)((v << 8) | (v >> 8)); }

// ---- maximum ------------------------------------------------------------------------------------------
// The loader starts from FLT_MIN and takes std::max(maximum, f) = (maximum < f) ? f : maximum per word:
// only a word above FLT_MIN can win, NaN never does.  The candidates are positive floats, whose order is
// that of their bit patterns, so the reduction runs on uint32 (exact, and order-independent):
//   FLOAT   key = bits(f) if f > FLT_MIN, else 0          (running word starts at bits(FLT_MIN))
//   USHORT  key = the word, UNSWAPPED whatever the file's endianness (the reference's quirk); 0 = none yet
template <typename VT> __device__ inline uint32_t max_key(VT v, int swap);
template <> __device__ inline uint32_t max_key<uint16_t>(uint16_t v, int) { return v; }
template <> __device__ inline uint32_t max_key<float>(float v, int swap)
{
    uint32_t b = __float_as_uint(v);
    if (swap) b = bswap32(b);
    return __uint_as_float(b) > 1.17549435e-38f ? b : 0u;   // FLT_MIN; false for NaN
}

template <typename VT>
__global__ __launch_bounds__(kMaxThreads) void vr_ingest_max_kernel(const uint4 *__restrict__ words, size_t n,
                                                                    int swap, uint32_t *max_word)
{
    constexpr int E = 16 / (int)sizeof(VT);   // words per 16-byte load
    __shared__ uint32_t s_max[kMaxThreads / 64];
    const size_t n16 = (n + E - 1) / E;
    uint32_t m = 0u;
    for (size_t i = (size_t)blockIdx.x * kMaxThreads + threadIdx.x; i < n16; i += (size_t)gridDim.x * kMaxThreads) {
        const uint4 q = words[i];
        VT v[E];
        __builtin_memcpy(v, &q, sizeof q);
#pragma unroll
        for (int j = 0; j < E; ++j)
            if (i * E + j < n) m = max(m, max_key<VT>(v[j], swap));   // (only the last load can be cut)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kMaxThreads / 64; ++w) m = max(m, s_max[w]);
        if (m) atomicMax(max_word, m);   // device scope; one per block
    }
}

// ---- conversion + histogram ---------------------------------------------------------------------------
// One voxel with the loader's arithmetic (datrawreader.cpp, FLOAT / UCHAR / USHORT branches): the value to
// store and its bin.  CONVERT = false: the binning alone, applied to a stored value.
template <typename VT, bool CONVERT> struct Voxel;
template <bool CONVERT> struct Voxel<uint8_t, CONVERT> {
    static __device__ inline uint8_t apply(uint8_t v, const IngestParams &, uint32_t *bin)
    {
        *bin = v;
        return v;
    }
};
template <bool CONVERT> struct Voxel<uint16_t, CONVERT> {
    static __device__ inline uint16_t apply(uint16_t v, const IngestParams &p, uint32_t *bin)
    {
        uint16_t s = v;
        if (CONVERT) {
            // round half away from zero; 0 stays 0 (all-zero step: the loader's 0 * inf is undefined there)
            s = v ? (uint16_t)roundf((float)v * p.stretch) : (uint16_t)0;
        }
        *bin = s >> 8;   // = (size_t)clamp(s / 256.f, 0, 255): s / 256.f is exact and below 256
        return CONVERT && p.big_endian ? bswap16(s) : s;
    }
};
template <bool CONVERT> struct Voxel<float, CONVERT> {
    static __device__ inline float apply(float v, const IngestParams &p, uint32_t *bin)
    {
        float s = v;
        if (CONVERT) {
            if (p.big_endian) s = __uint_as_float(bswap32(__float_as_uint(v)));
            s = s / p.max_value;   // IEEE, correctly rounded, denormal results kept (Makefile flags)
        }
        // round((double)(s * 255.f)): the product is a float, so rounding it half away from zero in fp32
        // gives the same integer; outside [0, 255], NaN included, the loader's size_t cast lands in 255
        const float rb = roundf(s * 255.f);
        *bin = (rb >= 0.f && rb <= 255.f) ? (uint32_t)rb : 255u;
        return s;
    }
};

// One count into the wave's sub-histogram per lane with `valid`.  Empty space is long runs of one value:
// when every counting lane of the wave has the same bin (a ballot tells), one lane adds their number.
__device__ inline void hist_count(uint32_t *wave_hist, bool valid, uint32_t bin)
{
    const unsigned long long act = __ballot(valid);
    if (!act) return;
    const int first = __ffsll((long long)act) - 1;
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
    if (__ballot(valid && bin == b0) == act) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&wave_hist[b0], (uint32_t)__popcll(act));
    } else if (valid) {
        atomicAdd(&wave_hist[bin], 1u);
    }
}

// LINEAR = false: the micro-bricked array vol.data.  A workgroup takes whole brick rows (nbx bricks of 64
// voxels, contiguous), a lane one 16-byte chunk of a brick at a time: 16 / 8 / 4 voxels of one z slice of
// the brick.  Padding voxels of edge bricks (x >= w, y >= h, z >= d) hold 0, stay 0 and are not counted.
// LINEAR = true: n words of a flat array in "rows" of row_chunks chunks; nothing is stored.
// The histogram: one 256-bin uint32 sub-histogram per wave in LDS, summed and flushed with one 64-bit global
// atomic per non-empty bin at the end of the workgroup.  The 32-bit LDS counters cannot wrap: the launcher
// sizes the grid so that a workgroup counts fewer than 2^32 voxels before its one flush.
template <typename VT, bool CONVERT, bool STORE, bool LINEAR>
__global__ __launch_bounds__(kHistThreads) void vr_ingest_convert_kernel(VolView vol, uint4 *__restrict__ data,
                                                                         size_t n, uint32_t n_rows,
                                                                         uint32_t row_chunks, IngestParams p,
                                                                         unsigned long long *hist)
{
    constexpr int E = 16 / (int)sizeof(VT);     // voxels per chunk
    constexpr int CPB = 64 / E;                 // chunks per micro-brick
    __shared__ uint32_t s_hist[kHistWaves * 256];
    for (int i = threadIdx.x; i < kHistWaves * 256; i += kHistThreads) s_hist[i] = 0u;
    __syncthreads();
    uint32_t *wave_hist = s_hist + (threadIdx.x >> 6) * 256;

    for (uint32_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        uint4 *rp = data + (size_t)row * row_chunks;
        // extent of this row's bricks inside the volume, per axis (block-uniform)
        int ylim = 4, zlim = 4;
        if (!LINEAR) {
            const int my = (int)(row % vol.nby), mz = (int)(row / vol.nby);
            ylim = vol.h - 4 * my;
            zlim = vol.d - 4 * mz;
        }
        for (uint32_t c0 = 0; c0 < row_chunks; c0 += kHistThreads) {   // uniform trip count: wave-wide votes inside
            const uint32_t c = c0 + threadIdx.x;
            const size_t e0 = ((size_t)row * row_chunks + c) * E;   // LINEAR: the chunk's first word
            const bool in = c < row_chunks && (!LINEAR || e0 < n);   // (the array ends inside its last row)
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (in) q = rp[c];
            VT v[E];
            __builtin_memcpy(v, &q, sizeof q);
            const int sub = (int)(c % CPB);
            const int xlim = LINEAR ? 4 : vol.w - 4 * (int)(c / CPB);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int e = sub * E + j;   // voxel of the brick: dx + 4 dy + 16 dz
                const bool valid = in && (LINEAR ? e0 + j < n : ((e & 3) < xlim && ((e >> 2) & 3) < ylim && (e >> 4) < zlim));
                uint32_t bin;
                const VT s = Voxel<VT, CONVERT>::apply(v[j], p, &bin);
                if (STORE && valid) v[j] = s;
                hist_count(wave_hist, valid, bin);
            }
            if (STORE && in) {
                __builtin_memcpy(&q, v, sizeof q);
                rp[c] = q;
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 256; b += kHistThreads) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (int w = 0; w < kHistWaves; ++w) sum += s_hist[w * 256 + b];
        if (sum) atomicAdd(&hist[b], sum);
    }
}

// ---- de-interleave ------------------------------------------------------------------------------------
// A thread takes K = 16 / sizeof(VT) consecutive texels: C 16-byte loads of interleaved values, one 16-byte
// store per channel plane.  The last n_texels % K texels go value by value.
template <typename VT, int C>
__global__ __launch_bounds__(kMaxThreads) void vr_deinterleave_kernel(const uint4 *__restrict__ in, VT *__restrict__ out,
                                                                      size_t plane_stride, size_t n_texels)
{
    constexpr int K = 16 / (int)sizeof(VT);
    const size_t groups = n_texels / K;
    const size_t tid = (size_t)blockIdx.x * kMaxThreads + threadIdx.x, step = (size_t)gridDim.x * kMaxThreads;
    for (size_t g = tid; g < groups; g += step) {
        uint4 q[C];
#pragma unroll
        for (int i = 0; i < C; ++i) q[i] = in[g * C + i];
        VT v[K * C];
        __builtin_memcpy(v, q, sizeof q);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            VT o[K];
#pragma unroll
            for (int k = 0; k < K; ++k) o[k] = v[k * C + c];
            uint4 w;
            __builtin_memcpy(&w, o, sizeof w);
            *reinterpret_cast<uint4 *>(out + (size_t)c * plane_stride + g * K) = w;
        }
    }
    const VT *src = reinterpret_cast<const VT *>(in);
    for (size_t t = groups * K + tid; t < n_texels; t += step)
#pragma unroll
        for (int c = 0; c < C; ++c) out[(size_t)c * plane_stride + t] = src[t * C + c];
}

unsigned stream_grid(size_t items, int threads, int num_cus)
{
    const size_t want = (items + (size_t)threads - 1) / (size_t)threads;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(want, (size_t)std::max(num_cus, 1) * 8));
}

template <typename VT, bool CONVERT, bool STORE, bool LINEAR>
hipError_t launch_convert(const VolView &vol, void *data, size_t n, uint32_t n_rows, uint32_t row_chunks,
                          size_t voxels_per_row, const IngestParams &p, unsigned long long *hist, int num_cus,
                          hipStream_t stream)
{
    if (!n_rows || !row_chunks) return hipSuccess;
    // 16 waves per SIMD-quad keep enough 16-byte loads in flight; more workgroups where one would count
    // 2^32 voxels or more before its flush (the LDS counters are 32 bits wide)
    size_t grid = std::min<size_t>(n_rows, (size_t)std::max(num_cus, 1) * 4);
    const size_t cap_rows = std::max<size_t>(1, (((size_t)1 << 32) - 1) / std::max<size_t>(voxels_per_row, 1));
    grid = std::max(grid, (n_rows + cap_rows - 1) / cap_rows);
    hipLaunchKernelGGL((vr_ingest_convert_kernel<VT, CONVERT, STORE, LINEAR>), dim3((unsigned)grid), dim3(kHistThreads), 0,
                       stream, vol, (uint4 *)data, n, n_rows, row_chunks, p, hist);
    return hipGetLastError();
}

template <typename VT>
hipError_t convert_typed(const VolView &vol, const IngestParams &p, int convert, unsigned long long *hist, int num_cus,
                         hipStream_t stream)
{
    const uint32_t n_rows = vol.nby * vol.nbz, row_chunks = vol.nbx * (uint32_t)(4 * sizeof(VT));
    const size_t vpr = (size_t)vol.nbx * 64;
    void *d = const_cast<void *>(vol.data);
    if (!convert) return launch_convert<VT, false, false, false>(vol, d, 0, n_rows, row_chunks, vpr, p, hist, num_cus, stream);
    if constexpr (sizeof(VT) == 1) return launch_convert<VT, true, false, false>(vol, d, 0, n_rows, row_chunks, vpr, p, hist, num_cus, stream);
    else return launch_convert<VT, true, true, false>(vol, d, 0, n_rows, row_chunks, vpr, p, hist, num_cus, stream);
}

template <typename VT>
hipError_t count_typed(const void *words, size_t n, const IngestParams &p, unsigned long long *hist, int num_cus,
                       hipStream_t stream)
{
    constexpr uint32_t kRowChunks = 4096;
    constexpr size_t E = 16 / sizeof(VT);
    const size_t chunks = (n + E - 1) / E;
    const size_t rows = (chunks + kRowChunks - 1) / kRowChunks;
    if (rows > 0xffffffffull) return hipErrorInvalidValue;
    VolView none = {};
    return launch_convert<VT, true, false, true>(none, const_cast<void *>(words), n, (uint32_t)rows, kRowChunks,
                                                 (size_t)kRowChunks * E, p, hist, num_cus, stream);
}

template <typename VT>
hipError_t deinterleave_typed(const void *in, void *out, size_t plane_stride, size_t n, int channels, hipStream_t stream)
{
    constexpr size_t K = 16 / sizeof(VT);
    dim3 grid(stream_grid(n / K + 1, kMaxThreads, 256)), block(kMaxThreads);
    if (channels == 2)
        hipLaunchKernelGGL((vr_deinterleave_kernel<VT, 2>), grid, block, 0, stream, (const uint4 *)in, (VT *)out, plane_stride, n);
    else if (channels == 4)
        hipLaunchKernelGGL((vr_deinterleave_kernel<VT, 4>), grid, block, 0, stream, (const uint4 *)in, (VT *)out, plane_stride, n);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace

hipError_t vr_launch_ingest_max(const void *words, size_t n, int format, int big_endian, uint32_t *max_word,
                                int num_cus, hipStream_t stream)
{
    if (!n || format == VRHIP_UCHAR) return hipSuccess;
    const size_t E = format == VRHIP_USHORT ? 8 : 4;
    dim3 grid(stream_grid((n + E - 1) / E, kMaxThreads, num_cus)), block(kMaxThreads);
    if (format == VRHIP_USHORT)
        hipLaunchKernelGGL(vr_ingest_max_kernel<uint16_t>, grid, block, 0, stream, (const uint4 *)words, n, 0, max_word);
    else if (format == VRHIP_FLOAT)
        hipLaunchKernelGGL(vr_ingest_max_kernel<float>, grid, block, 0, stream, (const uint4 *)words, n, big_endian, max_word);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t vr_launch_ingest_convert(const VolView &vol, int format, const IngestParams &p, int convert,
                                    unsigned long long *hist, int num_cus, hipStream_t stream)
{
    switch (format) {
    case VRHIP_UCHAR: return convert_typed<uint8_t>(vol, p, convert, hist, num_cus, stream);
    case VRHIP_USHORT: return convert_typed<uint16_t>(vol, p, convert, hist, num_cus, stream);
    case VRHIP_FLOAT: return convert_typed<float>(vol, p, convert, hist, num_cus, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t vr_launch_ingest_count(const void *words, size_t n, int format, const IngestParams &p,
                                  unsigned long long *hist, int num_cus, hipStream_t stream)
{
    if (!n) return hipSuccess;
    switch (format) {
    case VRHIP_UCHAR: return count_typed<uint8_t>(words, n, p, hist, num_cus, stream);
    case VRHIP_USHORT: return count_typed<uint16_t>(words, n, p, hist, num_cus, stream);
    case VRHIP_FLOAT: return count_typed<float>(words, n, p, hist, num_cus, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t vr_launch_deinterleave(const void *interleaved, void *planar, size_t plane_stride, size_t n_texels,
                                  int format, int channels, hipStream_t stream)
{
    if (!n_texels) return hipSuccess;
    switch (format) {
    case VRHIP_UCHAR: return deinterleave_typed<uint8_t>(interleaved, planar, plane_stride, n_texels, channels, stream);
    case VRHIP_USHORT: return deinterleave_typed<uint16_t>(interleaved, planar, plane_stride, n_texels, channels, stream);
    case VRHIP_FLOAT: return deinterleave_typed<float>(interleaved, planar, plane_stride, n_texels, channels, stream);
    default: return hipErrorInvalidValue;
    }
}
