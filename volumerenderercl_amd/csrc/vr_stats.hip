// vr_stats.hip -- volume statistics (vrhip_volume_statistics, include/vrhip.h "volume statistics"): the kernel that
// classifies the voxels of a region into the value x gradient-magnitude table, the counters and the moments,
// instantiated per voxel type and for bins_g == 1 / > 1, the kernel that adds the chunks' moments, and their launch
// entries.  Not a technique: it writes buffers of its own and the caller's table.
//
// Definition (tests/ref/stats_ref.c restates it on the CPU): s = fl(raw * inv_max) per voxel, the
// classification nan / below / above / value bin, the central difference with the neighbour clamped to the volume,
// hist[j * bins_v + i] += 1; the moments in the header's order.
//
// Execution: a workgroup of four waves takes one chunk of kStatsChunk consecutive blocks of 8^3 voxels (the call's
// block grid, x fastest), wave w the blocks w, w + 4, ... of it, one block at a time:
//  * the block's cell of the cell grid, when it is handed over, may prove the outcome (below); then the block's
//    voxels of the region go to one bin (the wave's pending pair, below) or counter and the block is not fetched;
//  * else the block's values -- 10^3 with the rim of one voxel, clamped to the volume, or 8^3 when bins_g == 1 -- go
//    to the wave's part of LDS once, lane (x, y) classifies the eight voxels of its column from there;
//  * counts go to the workgroup's table in LDS (32 bits: a workgroup sees at most 256 * 512 voxels) with LDS atomics,
//    and the table's non-zero bins to the global one at the end with 64-bit integer atomics -- or, for a table
//    beyond kStatsLdsBins, straight to the global one.  Integer sums do not depend on their order: exact.  A layer
//    of 64 voxels that share one bin (flat regions) is one pending (bin, count) pair of the wave, added when the bin
//    changes and at the end: without it a sparse volume's background is 2^33 adds to a single word.
//  * the moments: a lane's column from 0.0, the xor butterfly over the wave, the block's record to LDS; thread 0 adds
//    the chunk's records in ascending order and writes the chunk's record; vr_stats_total_kernel adds those in
//    ascending order.  No floating-point atomic; the order is the header's and does not depend on which wave or
//    workgroup ran what.
// The waves of a workgroup go through different numbers of fetched blocks, so inside the block loop a wave orders
// its own LDS traffic (wave_sync) and the workgroup meets only before and after the loop.
//
// The skips are exact.  s = fl(raw * inv_max) is monotone in raw (inv_max > 0), so raw <= max gives
// s <= fl(max * inv_max) and raw >= min gives s >= fl(min * inv_max).  The cells are 2^shift >= 8 voxels wide, a
// multiple of the block, and answer for the voxels [(c << shift) - 1, ((c + 1) << shift) + 1] clamped to the volume:
// the block's voxels 8 b .. 8 b + 7 AND the neighbours 8 b - 1 .. 8 b + 8 their central differences read (clamped the
// same way) lie in the extent of the one cell (8 b) >> shift.
//  * out of window: fl(max * inv_max) < v_lo puts every voxel below, fl(min * inv_max) > v_hi above -- the very
//    comparisons the classification makes.  Taken without moments only (the values are not known).
//  * constant: min == max, finite: every voxel and every neighbour has the one raw value, so s is the one
//    c = fl(min * inv_max), every difference is c - c = +0, m = 0.5 * sqrt(0) = 0, w = 0 * k_g = 0 (k_g is finite)
//    and j = 0.  With moments only for min == max == 0: a lane's column is 0.0 + (+-0.0) ... = +0.0, so are the
//    butterfly's sums and the squares, and min and max are a zero, which the total reports as +0 -- the record
//    (+0.0, +0.0, 0, 0) the skip writes.  (n * c is exact in double for n <= 512, n * c * c is not in general.)
//  * a cell with a NaN voxel holds (-inf, +inf) (vr_cells.hip): not constant, and neither window test passes.
#include "vr_sampling.h"

namespace {

constexpr uint32_t kSB = VRHIP_MESH_BLOCK;   // voxels per block and axis
static_assert(kSB == 8u, "lane = x + 8 y, eight layers");
constexpr uint32_t kStatsWaves = 4, kStatsThreads = 64 * kStatsWaves;
static_assert(kStatsChunk % kStatsWaves == 0, "every wave the same number of slots");
constexpr uint32_t kNoBin = 0xffffffffu;     // a voxel without a bin (bins are below 65536)

// what the kernel takes of a StatsLaunch
struct StatsArgs {
    uint32_t lo[3], hi[3];
    uint32_t b0[3], nb[3];
    uint32_t n_blocks;
    uint32_t bins_v, bins_g;
    float v_lo, v_hi, k_v, k_g;
    uint32_t moments, lds_hist;
    int cell_shift, cell_cx, cell_cy;
};

// a wave's LDS writes are visible to its own later reads, and its earlier reads are done before its later writes
VR_DEV void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (one wave: LDS operations execute in order)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

VR_DEV uint32_t wave_sum(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // (lane 0's)
}

// the value bin of a value inside the window
VR_DEV uint32_t stats_value_bin(const StatsArgs &a, float s)
{
    const float u = (s - a.v_lo) * a.k_v;
    return u >= (float)a.bins_v ? a.bins_v - 1u : (uint32_t)u;
}

// n counts into bin `bin`
VR_DEV void stats_count(const StatsArgs &a, uint32_t *s_hist, unsigned long long *hist, uint32_t bin, uint32_t n)
{
    if (a.lds_hist) atomicAdd(&s_hist[bin], n);
    else atomicAdd(&hist[bin], (unsigned long long)n);
}

template <typename VT, bool GRAD>
__global__ __launch_bounds__(kStatsThreads) void vr_stats_kernel(VolView vv, StatsArgs a, const float2 *__restrict__ cell_mm,
                                                                 unsigned long long *__restrict__ hist,
                                                                 unsigned long long *__restrict__ counters,
                                                                 StatsRec *__restrict__ chunk_recs)
{
    constexpr uint32_t kP = GRAD ? kSB + 2u : kSB, kOff = GRAD ? 1u : 0u;   // staged values per axis, the rim
    constexpr uint32_t kVals = kP * kP * kP;
    extern __shared__ uint32_t s_hist[];   // lds_hist: bins_g * bins_v words
    __shared__ float s_val[kStatsWaves][kVals];
    __shared__ StatsRec s_rec[kStatsChunk];
    __shared__ uint32_t s_cnt[kStatsWaves][kStatsCounters];

    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3;
    const uint32_t n_bins = a.bins_v * a.bins_g;
    if (a.lds_hist) {   // (uniform)
        for (uint32_t i = threadIdx.x; i < n_bins; i += kStatsThreads) s_hist[i] = 0u;
        __syncthreads();
    }
    const Vol<VT, 0, false> vol = make_vol<VT, 0, false>(vv, nullptr);
    float *sv = s_val[wave];
    const float kInf = __builtin_inff();
    // per lane: at most 64 blocks * 8 voxels; the skips' counts (up to 64 * 512) on lane 0: 32 bits hold them
    uint32_t c_nan = 0, c_below = 0, c_above = 0, c_gnan = 0, c_binned = 0, c_fetched = 0, c_const = 0, c_window = 0;
    uint32_t pend_bin = kNoBin, pend_n = 0;   // (uniform) counts of one bin not yet added: at most 64 * 512
    const uint32_t chunk0 = blockIdx.x * kStatsChunk, row = a.nb[0] * a.nb[1];
#pragma unroll 1
    for (uint32_t slot = wave; slot < kStatsChunk; slot += kStatsWaves) {
        const uint32_t b = chunk0 + slot;
        if (b >= a.n_blocks) break;   // (uniform over the wave, as everything about the block is)
        const uint32_t z = b / row, rem = b - z * row, y = rem / a.nb[0];
        const uint32_t blk[3] = {a.b0[0] + (rem - y * a.nb[0]), a.b0[1] + y, a.b0[2] + z};
        uint32_t n_in = 1;   // the block's voxels of the region
#pragma unroll
        for (uint32_t ax = 0; ax < 3u; ++ax)
            n_in *= min(a.hi[ax], blk[ax] * kSB + kSB) - max(a.lo[ax], blk[ax] * kSB);
        if (cell_mm) {   // (one block, one cell)
            const uint32_t cx = (blk[0] * kSB) >> a.cell_shift, cy = (blk[1] * kSB) >> a.cell_shift;
            const uint32_t cz = (blk[2] * kSB) >> a.cell_shift;
            const float2 mm = cell_mm[((size_t)cz * (uint32_t)a.cell_cy + cy) * (uint32_t)a.cell_cx + cx];
            const float s_min = mm.x * vv.inv_max, s_max = mm.y * vv.inv_max;
            if (!a.moments && (s_max < a.v_lo || s_min > a.v_hi)) {
                if (lane == 0) {
                    if (s_max < a.v_lo) c_below += n_in;
                    else c_above += n_in;
                    ++c_window;
                }
                continue;
            }
            if (mm.x == mm.y && fabsf(mm.x) < kInf && (!a.moments || mm.x == 0.f)) {
                if (!(s_min < a.v_lo) && !(s_min > a.v_hi)) {   // (uniform) gradient bin 0: the pending pair, as a layer
                    const uint32_t bin = stats_value_bin(a, s_min);
                    if (bin == pend_bin) pend_n += n_in;
                    else {
                        if (pend_n != 0u && lane == 0) stats_count(a, s_hist, hist, pend_bin, pend_n);
                        pend_bin = bin;
                        pend_n = n_in;
                    }
                }
                if (lane == 0) {
                    if (s_min < a.v_lo) c_below += n_in;
                    else if (s_min > a.v_hi) c_above += n_in;
                    else c_binned += n_in;
                    ++c_const;
                    if (a.moments) {
                        StatsRec rec;
                        rec.sum = rec.sum_sq = 0.0;
                        rec.mn = rec.mx = 0.f;
                        s_rec[slot] = rec;
                    }
                }
                continue;
            }
        }
        if (lane == 0) ++c_fetched;
        // the block's values, x fastest, with the rim (GRAD); coordinates are clamped to the volume, which is the
        // neighbour rule of the gradient (values beyond the volume repeat its last plane: no voxel of the region
        // reads them as its own)
        wave_sync();   // (the previous block's reads are done)
        for (uint32_t i = lane; i < kVals; i += 64u) {
            const uint32_t pz = i / (kP * kP), r = i - pz * (kP * kP), py = r / kP, px = r - py * kP;
            const int x = min(max((int)(blk[0] * kSB + px) - (int)kOff, 0), vol.w1);
            const int yy = min(max((int)(blk[1] * kSB + py) - (int)kOff, 0), vol.h1);
            const int zz = min(max((int)(blk[2] * kSB + pz) - (int)kOff, 0), vol.d1);
            sv[i] = vol.raw(vol.xoff(x), vol.yoff(yy), vol.zoff(zz), x, yy, zz) * vol.inv_max;
        }
        wave_sync();
        const uint32_t gx = blk[0] * kSB + lx, gy = blk[1] * kSB + ly;
        const bool in_xy = gx >= a.lo[0] && gx < a.hi[0] && gy >= a.lo[1] && gy < a.hi[1];
        double sum = 0.0, sum_sq = 0.0;
        float mn = kInf, mx = -kInf;
#pragma unroll 1
        for (uint32_t lz = 0; lz < kSB; ++lz) {
            const uint32_t gz = blk[2] * kSB + lz;
            uint32_t bin = kNoBin;
            if (in_xy && gz >= a.lo[2] && gz < a.hi[2]) {
                const float *c = sv + ((lx + kOff) + kP * ((ly + kOff) + kP * (lz + kOff)));
                const float s = c[0];
                if (s != s) ++c_nan;
                else {
                    if (a.moments) {
                        mn = s < mn ? s : mn;
                        mx = s > mx ? s : mx;
                        const double d = (double)s;
                        sum = sum + d;
                        sum_sq = sum_sq + d * d;
                    }
                    if (s < a.v_lo) ++c_below;
                    else if (s > a.v_hi) ++c_above;
                    else {
                        bin = stats_value_bin(a, s);
                        if constexpr (GRAD) {
                            const float dx = c[1] - c[-1], dy = c[(int)kP] - c[-(int)kP];
                            const float dz = c[(int)(kP * kP)] - c[-(int)(kP * kP)];
                            const float m = 0.5f * sqrtf((dx * dx + dy * dy) + dz * dz);
                            if (m != m) {
                                ++c_gnan;
                                bin = kNoBin;
                            } else {
                                const float w = m * a.k_g;
                                bin += (w >= (float)a.bins_g ? a.bins_g - 1u : (uint32_t)w) * a.bins_v;
                            }
                        }
                        if (bin != kNoBin) ++c_binned;
                    }
                }
            }
            // the layer's counts.  Where all of its voxels share a bin (flat regions: most of a sparse volume) the
            // wave keeps one pending (bin, count) pair instead of sixty-four adds to one address
            const unsigned long long have = __ballot(bin != kNoBin);
            if (have != 0ull) {   // (uniform)
                const uint32_t lead = __shfl(bin, __ffsll((long long)have) - 1, 64);
                if (__ballot(bin == lead) == have) {
                    const uint32_t n = (uint32_t)__popcll(have);
                    if (lead == pend_bin) pend_n += n;
                    else {
                        if (pend_n != 0u && lane == 0) stats_count(a, s_hist, hist, pend_bin, pend_n);
                        pend_bin = lead;
                        pend_n = n;
                    }
                } else if (bin != kNoBin)
                    stats_count(a, s_hist, hist, bin, 1u);
            }
        }
        if (a.moments) {   // (uniform)
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                sum = sum + __shfl_xor(sum, k, 64);
                sum_sq = sum_sq + __shfl_xor(sum_sq, k, 64);
                const float on = __shfl_xor(mn, k, 64), ox = __shfl_xor(mx, k, 64);
                mn = on < mn ? on : mn;
                mx = ox > mx ? ox : mx;
            }
            if (lane == 0) {
                StatsRec rec;
                rec.sum = sum;
                rec.sum_sq = sum_sq;
                rec.mn = mn;
                rec.mx = mx;
                s_rec[slot] = rec;
            }
        }
    }
    if (pend_n != 0u && lane == 0) stats_count(a, s_hist, hist, pend_bin, pend_n);
    {
        const uint32_t c[kStatsCounters] = {c_nan, c_below, c_above, c_gnan, c_binned, c_fetched, c_const, c_window};
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kStatsCounters; ++k) {
            const uint32_t t = wave_sum(c[k]);
            if (lane == 0) s_cnt[wave][k] = t;
        }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kStatsCounters) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kStatsWaves; ++w) t += s_cnt[w][threadIdx.x];
        if (t != 0ull) atomicAdd(&counters[threadIdx.x], t);
    }
    if (a.lds_hist)
        for (uint32_t i = threadIdx.x; i < n_bins; i += kStatsThreads) {
            const uint32_t n = s_hist[i];
            if (n != 0u) atomicAdd(&hist[i], (unsigned long long)n);
        }
    if (a.moments && threadIdx.x == 0) {   // the chunk's blocks in ascending order
        const uint32_t n = min(kStatsChunk, a.n_blocks - chunk0);
        StatsRec t;
        t.sum = t.sum_sq = 0.0;
        t.mn = kInf;
        t.mx = -kInf;
        for (uint32_t k = 0; k < n; ++k) {
            const StatsRec rec = s_rec[k];
            t.sum = t.sum + rec.sum;
            t.sum_sq = t.sum_sq + rec.sum_sq;
            t.mn = rec.mn < t.mn ? rec.mn : t.mn;
            t.mx = rec.mx > t.mx ? rec.mx : t.mx;
        }
        chunk_recs[blockIdx.x] = t;
    }
}

// one wave: the chunk records in ascending order, 64 at a time through LDS; a zero minimum or maximum leaves as +0
__global__ __launch_bounds__(64) void vr_stats_total_kernel(const StatsRec *__restrict__ chunk_recs, size_t n_chunks,
                                                            StatsRec *__restrict__ total)
{
    __shared__ StatsRec s_rec[64];
    const float kInf = __builtin_inff();
    StatsRec t;
    t.sum = t.sum_sq = 0.0;
    t.mn = kInf;
    t.mx = -kInf;
    for (size_t base = 0; base < n_chunks; base += 64u) {   // (uniform)
        __syncthreads();
        if (base + threadIdx.x < n_chunks) s_rec[threadIdx.x] = chunk_recs[base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t n = (uint32_t)(n_chunks - base < 64u ? n_chunks - base : 64u);
            for (uint32_t k = 0; k < n; ++k) {
                const StatsRec rec = s_rec[k];
                t.sum = t.sum + rec.sum;
                t.sum_sq = t.sum_sq + rec.sum_sq;
                t.mn = rec.mn < t.mn ? rec.mn : t.mn;
                t.mx = rec.mx > t.mx ? rec.mx : t.mx;
            }
        }
    }
    if (threadIdx.x == 0) {
        if (t.mn == 0.f) t.mn = 0.f;
        if (t.mx == 0.f) t.mx = 0.f;
        *total = t;
    }
}

StatsArgs stats_args(const StatsLaunch &a)
{
    StatsArgs s;
    for (int i = 0; i < 3; ++i) { s.lo[i] = a.lo[i]; s.hi[i] = a.hi[i]; s.b0[i] = a.b0[i]; s.nb[i] = a.nb[i]; }
    s.n_blocks = a.nb[0] * a.nb[1] * a.nb[2];
    s.bins_v = a.bins_v;
    s.bins_g = a.bins_g;
    s.v_lo = a.v_lo;
    s.v_hi = a.v_hi;
    s.k_v = a.k_v;
    s.k_g = a.k_g;
    s.moments = a.moments ? 1u : 0u;
    s.lds_hist = a.lds_hist ? 1u : 0u;
    s.cell_shift = a.cell_shift;
    s.cell_cx = a.cell_cx;
    s.cell_cy = a.cell_cy;
    return s;
}

template <typename VT, bool GRAD>
hipError_t stats_launch(const StatsLaunch &a, uint32_t grid, unsigned long long *hist, unsigned long long *counters,
                        StatsRec *chunk_recs, hipStream_t stream)
{
    const size_t lds = a.lds_hist ? (size_t)a.bins_v * a.bins_g * sizeof(uint32_t) : 0u;
    int per_cu = 0;
    const hipError_t e = vr_prepare_kernel(vr_stats_kernel<VT, GRAD>, (int)kStatsThreads, lds, &per_cu, "stats", a.num_cus);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((vr_stats_kernel<VT, GRAD>), dim3(grid), dim3(kStatsThreads), lds, stream, a.vol, stats_args(a),
                       a.cell_minmax, hist, counters, chunk_recs);
    return hipGetLastError();
}

} // namespace

hipError_t vr_launch_stats(const StatsLaunch &a, unsigned long long *hist, unsigned long long *counters,
                           StatsRec *chunk_recs, hipStream_t stream)
{
    const unsigned long long n = (unsigned long long)a.nb[0] * a.nb[1] * a.nb[2];
    const unsigned long long bins = (unsigned long long)a.bins_v * a.bins_g;
    if (n == 0 || n >= 0x7fffffffull || !hist || !counters || (a.moments && !chunk_recs)) return hipErrorInvalidValue;
    if (bins == 0 || bins > VRHIP_STATS_MAX_BINS || (a.lds_hist && bins > kStatsLdsBins)) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)vr_stats_chunks((size_t)n);
    return vr_for_format(a.format, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        return a.bins_g > 1u ? stats_launch<VT, true>(a, grid, hist, counters, chunk_recs, stream)
                             : stats_launch<VT, false>(a, grid, hist, counters, chunk_recs, stream);
    });
}

hipError_t vr_launch_stats_total(const StatsRec *chunk_recs, size_t n_chunks, StatsRec *total, hipStream_t stream)
{
    if (!chunk_recs || !total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vr_stats_total_kernel, dim3(1), dim3(64), 0, stream, chunk_recs, n_chunks, total);
    return hipGetLastError();
}
