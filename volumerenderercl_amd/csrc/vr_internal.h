// vr_internal.h -- descriptors shared by the kernels and the C-ABI implementation.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>

#include "../../include/vrhip.h"

// Scalar field in HBM (DESIGN.md "Data layout"): 4x4x4-voxel MICRO-BRICKS of 64 contiguous
// voxels (x fastest inside a brick) -- one 64-byte line for UCHAR -- stored x-fastest over the
// brick grid.  Every line a ray bundle pulls in is a compact 3-D neighbourhood, whatever the
// view direction.  Element index of voxel (x, y, z):
//   (((z>>2)*nby + (y>>2))*nbx + (x>>2))*64 + (z&3)*16 + (y&3)*4 + (x&3)
struct VolView {
    const void *data;
    int w, h, d;
    float fw, fh, fd;
    float inv_max;              // UNORM scale: 1/255, 1/65535, 1
    uint32_t nbx, nby, nbz;     // micro-brick grid = ceil(res / 4)
    uint32_t ystride;           // elements per brick row:   nbx * 64
    unsigned long long zstride; // elements per brick slice: nbx * nby * 64
    // CL_RG / CL_RGBA volumes (volumerendercl.cpp:697-705): one planar micro-bricked array per
    // channel.  `data` is channel 0 -- the .x every single-channel reader of the kernel looks at
    // (bricks, gradients, path tracer); chan[0..2] are channels 1..3.
    const void *chan[3];
    int channels;               // 1, 2 or 4
    // Footprint volume (optional, nullptr = absent): entry (ex, ey, ez), ex in [0, w] etc., holds
    // the 8 voxels a trilinear fetch with low-corner texel ix = ex - 1 reads, edge clamping
    // applied: value j = dx + 2 dy + 4 dz is voxel (clamp(ix + dx), clamp(iy + dy), clamp(iz + dz)).
    // One 8 / 16 / 32-byte load per fetch instead of eight voxel loads; 8x the volume's bytes, laid
    // out in 4x4x4 micro-bricks of entries like the volume itself.
    const void *fp;
    uint32_t fp_nbx, fp_nby;    // micro-brick grid of the (w+1) x (h+1) x (d+1) entries
};

__host__ __device__ inline unsigned long long vr_fp_index(const VolView &v, int ex, int ey, int ez)
{
    return ((unsigned long long)(ez >> 2) * v.fp_nby + (unsigned long long)(ey >> 2)) * v.fp_nbx * 64ull +
           (unsigned long long)(((ex >> 2) << 6) + ((ez & 3) << 4) + ((ey & 3) << 2) + (ex & 3));
}

__host__ __device__ inline unsigned long long vr_voxel_index(const VolView &v, int x, int y, int z)
{
    return (unsigned long long)(z >> 2) * v.zstride + (unsigned long long)(y >> 2) * v.ystride +
           (unsigned long long)(((x >> 2) << 6) + ((z & 3) << 4) + ((y & 3) << 2) + (x & 3));
}

// min/max brick grid (generateBricks): (min,max) pairs in the volume's type, x fastest.
struct BrickView {
    const void *data;
    int bw, bh, bd;
};

struct TfView {
    const float4 *tff;     // RGBA8 table converted with c / 255.0f
    uint32_t tff_n;
    const uint32_t *prefix;
    uint32_t prefix_n;
};

// The 2-D transfer function of technique 6 (vrhip_set_transfer_function_2d), all of it made on the host at set time.
struct Tf2dView {
    const float4 *table;     // n_g rows of n_v entries, value fastest, c / 255.0f
    // Marginal opacity, as its prefix sum: nz[i] = the number of columns i' < i with max_j table[j][i'].a != 0
    // (n_v + 1 words).  Column i is transparent in every row <=> nz[i + 1] == nz[i]; columns i0..i1 all are
    // <=> nz[i1 + 1] == nz[i0].
    const uint32_t *nz;
    uint32_t n_v, n_g;
    float inv_ghi;           // 1.0f / g_hi, computed once
};

// Technique 8 (pre-integrated classification): the 1-D table and what vrhip_preint_tables makes of it on the host.
struct PreintView {
    const float4 *tff;       // the ray caster's table (TfView::tff), n entries
    const double *prefix;    // n entries of four doubles: the integrals of alpha and of r, g, b x alpha over [0, i]
    const uint32_t *nz;      // n + 1 words: nz[i] = the number of entries i' < i with alpha != 0
    uint32_t n;
};

// ESS decision per brick, precomputed from (bricks, TF, prefix sum): bit = 1 when the
// reference's test `TF(max).a < 1e-6 && prefix[min] == prefix[max]` (volumeraycast.cl:
// 777-787) holds.  x-fastest bit index; word n_words holds the decision for the (0,0) value
// defined for out-of-range cells.
struct SkipView {
    const uint32_t *bits;
    uint32_t n_words;
    uint32_t in_lds;       // bitmap is staged in LDS by every workgroup
    // Patch culling in the DDA pre-pass: bit = 1 when some brick within `near_r` bricks (Chebyshev,
    // per axis) of this one is NOT skipped.  An 8x8 patch whose rays stay -- by a conservative
    // bound -- inside bricks with bit 0 cannot meet a brick to sample: its rays are finished without
    // the walk.  nullptr / 0: off.
    const uint32_t *near_bits;
    uint32_t near_r;
};

// One 8x8-pixel patch (= one wave64) of the work queue.
struct WaveTile {
    uint16_t tx8, ty8;     // patch origin / 8 in the frame, bits 0..10; bits 11..15 of ty8 and of tx8: frame of the batch
    uint32_t out_base;     // index of its first pixel in FrameView::out
};
// Several independent frames (jitter seeds) in one set of launches: the work queue holds every
// patch once per frame, the frame index rides in the upper bits of WaveTile::ty8 (low five bits) and
// WaveTile::tx8 (high five bits) -- patch rows and columns need 11 bits up to 16384 pixels -- and of
// ContRec::state, FrameView::seeds gives each frame its seed.  32 whole frames fill a GPU; a rank's tile
// share of an 8-rank split needs 256 frames per set for the same work per launch.
constexpr uint32_t kFrameShift = 11, kMaxBatchFrames = 256;
constexpr uint32_t kPatchMask = (1u << kFrameShift) - 1u, kFrameLowBits = 16u - kFrameShift;
__host__ __device__ inline uint32_t wt_row(const WaveTile &w) { return w.ty8 & kPatchMask; }
__host__ __device__ inline uint32_t wt_col(const WaveTile &w) { return w.tx8 & kPatchMask; }
__host__ __device__ inline uint32_t wt_frame(const WaveTile &w)
{
    return (uint32_t)(w.ty8 >> kFrameShift) | ((uint32_t)(w.tx8 >> kFrameShift) << kFrameLowBits);
}
__host__ __device__ inline void wt_set_frame(WaveTile &w, uint32_t f)
{
    w.ty8 = (uint16_t)((w.ty8 & kPatchMask) | ((f & ((1u << kFrameLowBits) - 1u)) << kFrameShift));
    w.tx8 = (uint16_t)((w.tx8 & kPatchMask) | ((f >> kFrameLowBits) << kFrameShift));
}

// A patch with at least one ray that reaches a non-skipped brick (DDA pre-pass), and which rays.
struct LiveTile {
    WaveTile wt;
    uint32_t mask_lo, mask_hi;   // bit = lane (8 * row + column) of the patch
};

// Dynamic state of a suspended ray (two-phase march): everything else is recomputed from the
// pixel.  64 bytes.
struct ContRec {
    uint32_t pix;          // gx | gy << 16
    uint32_t out_index;    // pixel index in FrameView::out
    int32_t state;
    float t, t_exit, alpha, r0, r1, r2;
    int32_t cx, cy, cz;
    float tv0, tv1, tv2;
    uint32_t pad;
};

// What a record says about its ray without the kernels' locals (VR_PACK_RAY / VR_UNPACK_RAY, vr_raycast_kernels.h, are
// the code that packs and unpacks whole records): pixel and frame of the batch.  Host side, vrhip_download_ray_order.
inline uint32_t rec_gx(const ContRec &c) { return c.pix & 0xffffu; }
inline uint32_t rec_gy(const ContRec &c) { return c.pix >> 16; }
inline uint32_t rec_frame(const ContRec &c) { return (uint32_t)c.state >> 8; }

struct FrameView {
    uint32_t W, H;         // frame size in pixels
    uint32_t gsx, gsy;     // padded launch size the reference derives the camera from
    // what make_ray derives from it for every pixel alike (:614-627), computed once on the host with
    // the same IEEE operations: min(gsy / gsx, gsx / gsy), 2 / gsx, 2 / gsy
    float ray_aspect, ray_psx, ray_psy;
    const WaveTile *queue; // n_wave_tiles entries, processed in order (centre first)
    uint32_t n_wave_tiles;
    uint32_t out_stride;   // pixels per row of `out`
    uint32_t *queue_head;  // zeroed before each launch
    // the control words (kControlWords from queue_head on) of the NEXT set of launches: the renderer
    // alternates between two blocks, and the first kernel of a set zeroes the other block -- nothing else
    // touches it until the next set starts -- instead of a memset launch per frame.  nullptr: nothing to zero
    uint32_t *next_ctrl;
    // Patch classes (vr_patch_class_kernel, once per camera / transfer function / tile set, not per frame):
    // class 1 = whatever the jitter, every ray of the patch hits the box and none can meet a brick that is
    // not skipped, and the background is one colour -- the pre-pass writes 64 times (background, alpha 0)
    // for it without setting up a single ray.  patch_class[q / set_frames] for work item q; nullptr: off
    const uint8_t *patch_class;
    uint32_t set_frames;
    float4 *fb;            // W*H frame / accumulate buffer (always written)
    float4 *out;           // optional second destination (device), frame or tile layout
    // Two-phase march: rays still alive after `round_budget` sample rounds of phase 1 (0 =
    // unlimited) are appended to `cont` and resumed by the split kernel, 16 lanes per ray.
    ContRec *cont;
    uint32_t *cont_count;  // zeroed before each launch
    uint32_t *cont_head;   // zeroed before each launch
    uint32_t round_budget;
    const uint32_t *seeds; // per frame of a batch (WaveTile frame index), or nullptr: rendering_params.seed
    // per frame of a batch, like `seeds` (vrhip_render_batch_views): view matrix, box and ortho of frame f, or
    // nullptr: the launch's camera for every frame.  Read only by the kernels instantiated with VIEWS = true.
    const vrhip_camera_params *cams;
    uint32_t refill_min;   // phase 2: idle ray slots of a wave before they take new rays (0 = all 16)
    // DDA pre-pass (ESS, un-instrumented): a light, high-occupancy kernel walks every ray to its
    // first non-skipped brick; rays that never reach one get their (background) pixel there and
    // phase 1 only visits the patches listed in `live`.  nullptr: phase 1 walks the whole queue.
    LiveTile *live;
    uint32_t *live_count;  // zeroed before each launch (the list of live PATCHES, FrameView::live)
    uint32_t *live_list_count;   // kLiveLists counters, kLiveStride words apart (the lists of live RAYS, live_rays)
    uint32_t *draw_count;        // kDrawCounters counters, kLiveStride words apart (the persistent kernels' draws)
    // Default kernels: the pre-pass lists the live RAYS instead (with the DDA state they have
    // reached; live_count counts them) and phase 1 runs on that list, one lane per ray, lanes
    // refilled as rays end (vr_raycast_rays_kernel).  nullptr: the patch list above.
    ContRec *live_rays;
    // Unused: FrameView and CellView are kernel arguments, and these words keep the offsets of the arguments behind
    // them where they were.  The phase-1 kernel at three waves per SIMD, register-bound, is sensitive to them: with
    // the arguments moved it spilled differently and the benchmark took 0.5 % longer.
    // (The first two of the four now hold the mark plane of a set of samples, read only by the kernels instantiated
    // with SAMPLES = true -- vr_pathtrace.hip: one byte per record of `out`, 1 = traced sample, 0 = the ray missed
    // the box.  Same size, same offsets.)
    uint8_t *sample_mark;
    // (The other two hold the pixel-major block of a launch set of one camera, or nullptr: the pre-pass's ray order.
    // See "pixel-major ray order" below.  Same size, same offsets.)
    uint32_t *pm;
    // Phase-2 scheduling: `cost` keeps, per pixel, the phase-2 rounds the pixel's ray needed in the
    // previous frame.  Suspended rays are sorted by it, longest first (counting sort into
    // `order`), so that the longest chains start first and the 16 rays of a group are alike.
    // Purely a schedule: the image does not depend on it.
    uint16_t *cost;        // W*H, or nullptr
    uint32_t *order;       // permutation of the suspended rays, or nullptr (append order)
    uint32_t *sort_ws;     // kSortBins counts + kSortBins cursors, zeroed before each launch
    // Image-order ESS (rendering_params.imgEss, volumeraycast.cl:659-670, :912-925): one texel per
    // 8x8 work-group, (W/8 + 1) x (H/8 + 1) of them (volumerendercl.cpp:482-488).
    const uint8_t *hit_in; // last frame's hit image
    uint8_t *hit_status;   // this frame: what each group's work-items did (HIT_*, vr_raycast.hip)
    uint8_t *hit_any;      // this frame: 1 = a work-item that reached the end changed its pixel;
                           // zeroed before each launch
    uint32_t hit_w, hit_h;
    // Environment map (createEnvironmentMap, volumerendercl.cpp:1121-1150): float RGBA texels,
    // nullptr when none is set (the reference's 1x1 white map is never sampled, :655)
    const float4 *env;
    uint32_t env_w, env_h;
};
constexpr uint32_t kSortBins = 256;
// The pre-pass's ray list is kLiveLists lists, work item q appending to list q % kLiveLists through a counter of its
// own, each counter in a cache line of its own (kLiveStride words apart): waves that run side by side walk neighbouring
// work items, so their appends meet at kLiveLists addresses instead of one (one counter: 193 us of a 20-frame set's
// 580 us of pre-pass).  Phase 1 reads the lists interleaved, 64 rays from each in turn (vr_raycast_rays_kernel), which
// keeps the queue's order: all lists grow at the same pace.  List k sits at live_rays + k * live_list_cap(items).
constexpr uint32_t kLiveLists = 8, kLiveStride = 32;
constexpr uint32_t kLiveBase = 4 + 2 * kSortBins;        // first list counter, in control words
// ... and the persistent kernels draw their work through kDrawCounters counters instead of one (FrameView::draw_count, a
// cache line each): counter k hands out the work units G + kDrawCounters j + k behind the G units the waves own by
// position; a wave starts at counter (its number mod kDrawCounters) and moves on when one has run out.
constexpr uint32_t kDrawCounters = 8;
constexpr uint32_t kDrawBase = kLiveBase + kLiveLists * kLiveStride;
// Pixel-major ray order (FrameView::pm; launch sets of >= 2 frames with one camera).  The frames of such a set differ in
// the jitter seed only: the rays of one pixel in the set's frames cross the same cells, leave their empty runs and end
// within a round of each other.  Phase 1 therefore draws the set's rays pixel by pixel -- the live rays of a pixel in
// frames 0 .. set_frames - 1, then the next pixel of the same patch, patches in the queue's order -- through an INDEX
// into the pre-pass's ray lists.  The pre-pass appends its records as ever and notes, per work item q, the ballot of
// its live rays and the position of its first record; vr_regroup_kernel (one wave per patch, vr_raycast.hip) turns the
// set_frames notes of a patch into index entries, appended to list (patch % kLiveLists) through kLiveLists counters
// of their own in the control words.  A patch's entries are padded to a multiple of the group size with kPmNone, so
// that the 64 rays a wave draws at once come from one patch.  The block, in words:
//   [0, 2 n)   live ballots of the n work items       [2 n, 3 n)   position of the item's first record in live_rays
//   [3 n, ..)  kLiveLists index lists of pm_list_cap(n, set_frames) entries each
constexpr uint32_t kPmBase = kDrawBase + kDrawCounters * kLiveStride;          // first index-list counter, in control words
constexpr uint32_t kControlWords = kPmBase + kLiveLists * kLiveStride;   // queue head, cont count, cont head, live-tile count, sort_ws, list counters, draw counters, index-list counters
constexpr uint32_t kPmNone = 0xffffffffu;
__host__ __device__ inline uint32_t live_list_cap(uint32_t n_items) { return ((n_items + kLiveLists - 1u) / kLiveLists) * 64u; }
// entries per index list: ceil(patches / kLiveLists) patches of at most 64 set_frames entries (a multiple of every
// group size) -- bounded without a division by (n_items + 7 set_frames) 8 <= 8 n_items + 64 set_frames
__host__ __device__ inline uint32_t pm_list_cap(uint32_t n_items, uint32_t set_frames) { return 8u * n_items + 64u * set_frames; }
// the whole block, in 64 bits: the host uses the order only where this fits 32 bits (the kernels index with 32 bits,
// and pm_list_cap itself would wrap beyond)
inline unsigned long long pm_block_words(uint32_t n_items, uint32_t set_frames)
{
    return 3ull * n_items + (unsigned long long)kLiveLists * (8ull * n_items + 64ull * set_frames);
}
// first kernel of a set of launches, first workgroup: the control words of the next set (FrameView::next_ctrl)
#define VR_ZERO_NEXT_CTRL(fr)                                                                              \
    do {                                                                                                   \
        if (blockIdx.x == 0 && (fr).next_ctrl)                                                             \
            for (uint32_t i_ = threadIdx.x; i_ < kControlWords; i_ += blockDim.x) (fr).next_ctrl[i_] = 0u; \
    } while (0)

// Cell grid: the volume cut into cells of 2^shift voxels per axis.  For every cell the renderer
// keeps (min, max) of the voxels a trilinear fetch whose low-corner texel lies in the cell -- or
// within one texel of it -- can read: voxels [(c << shift) - 1, ((c + 1) << shift) + 1] per axis.
// Combined with the transfer function this gives, per cell (vr_cells.hip):
//  * bound: an upper bound of the opacity any such fetch can map to.  Path tracer: a tracking
//    step whose bound is below the walk's acceptance threshold cannot be accepted, so its voxel
//    loads are skipped.
//  * empty: 1 bit, set when that opacity is exactly 0.  Ray caster: such a sample composites to
//    exactly nothing (volumeraycast.cl:864-879 with alpha == 0), so runs of them are stepped over
//    with the reference's own t sequence and without touching the volume.
// Neither changes any pixel: both only skip work whose result is known.
// The two live on grids of their own: the bounds on cells of 2^shift voxels (8 up to 2048^3: the path
// tracer's table stays cache-sized), the empty bits on cells of 2^eshift voxels (4 up to 2048^3:
// fewer fetches at the rims of a structure that can only return opacity 0).  A coarse cell's extent
// is the union of the extents of the fine cells inside it, so the coarse (min, max) are reduced
// from the fine ones where both exist.
struct CellView {
    const float *bound;     // cx * cy * cz floats, x fastest; nullptr = feature off
    const uint32_t *empty;  // 1 bit per cell of the ecx * ecy * ecz grid, x fastest; nullptr = feature off
    int cx, cy, cz;
    int shift;
    int ecx, ecy, ecz;
    int eshift;
    const void *arg_pad0;   // unused (see FrameView::arg_pad)
    int arg_pad1[3];
    // The bounds once more, per macro cell of 4 x 4 x 4 cells (kLeapShift): the maximum of its cells' bounds -- what
    // lets a tracking walk leap over all its steps inside a macro cell at once (vr_pathtrace.hip).  ccx * ccy * ccz
    // floats, x fastest; nullptr = no leaps.
    const float *cbound;
    int ccx, ccy, ccz;
    // ... and how far the macro cells around one are free as well, for kLeapLevels thresholds tau_j = j / 8, j = 1..7:
    // cdist[(j - 1) * ccx * ccy * ccz + C] = 0 when macro cell C has a bound >= tau_j, else 1 + the largest R <= kLeapRadius
    // such that every macro cell of the grid within Chebyshev distance R of C has a bound < tau_j.  A walk with
    // threshold thr reads level j = floor(8 thr) (tau_j <= thr) and may leap through that whole cube.  nullptr: leaps
    // stay inside one macro cell.
    const uint8_t *cdist;
};

struct DevStats {
    unsigned long long v[6]; // order of vrhip_stats
};

struct RaycastLaunch {
    VolView vol;
    BrickView bricks;
    TfView tf;
    SkipView skip;
    FrameView frame;
    vrhip_camera_params cam;
    vrhip_rendering_params render;
    vrhip_raycast_params raycast;
    vrhip_pathtrace_params pathtrace;
    vrhip_iso_params iso;
    CellView cells;
    int format;            // vrhip_format
    int use_ess;
    int instr;             // 0 none, 1 stats, 2 stats + touched bitmap
    int occ3;              // phase 1 on the ray list at three waves per SIMD (vr_raycast_kernels.h kWavesWide): a schedule, not a result
    int occ3_split;        // the same for phase 2
    uint32_t pm_group;     // pixel-major order (frame.pm): a patch's index entries are padded to a multiple of this (1, 32 or 64)
    DevStats *stats;
    uint32_t *touched;
    int num_cus;
    hipEvent_t mid_event;  // optional: the end of phase 1
    // optional: the end of the frame's last launch.  Both events are BOUND to a kernel's own completion signal
    // (hipExtLaunchKernelGGL's stopEvent) rather than recorded behind it: a recorded event is a marker packet of its
    // own between two launches (~6 us of GPU time each).  *stop_bound tells the caller that the launchers have done
    // so (false: nothing was launched, or bind_events is off -- the caller records the event itself).
    hipEvent_t stop_event;
    bool *stop_bound;
    // optional, likewise: the start of the frame's first launch (hipExtLaunchKernelGGL's startEvent)
    hipEvent_t start_event;
    bool *start_bound;
    int bind_events;       // 0: record events behind the launches instead (VRHIP_EVENT_BIND=0, A/B)
    uint8_t *hit_out;      // imgEss: this frame's hit image (resolved after the march), or nullptr
    vrhip_launch_info *info;   // optional: the launchers record what they launched (vrhip_last_launch_info)
    // technique 1, vrhip_render_samples: the set's frames are consecutive samples of one progressive image, sample k
    // at iteration render.iteration + k.  frame.out / frame.sample_mark are the scratch planes (sample_plane records
    // each), fold_out the caller's own destination for the accumulated pixels (or nullptr).
    int samples;
    uint32_t sample_plane;
    float4 *fold_out;
    int keep_stats;            // launch_timed: the counters go on from the set before (chained sets of samples)
    // technique 2 or 4 with object-order ESS: the (min, max) pairs of the cell grid of the current time step -- the fine grid
    // (cells.ecx.., cells.eshift) when cell_minmax_fine is set, else the coarse one (cells.cx.., cells.shift) -- or
    // nullptr: every sample is fetched
    const float2 *cell_minmax;
    int cell_minmax_fine;
    Tf2dView tf2d;             // technique 6: its table (cell_minmax as for techniques 2 and 4)
    PreintView preint;         // technique 8: the 1-D table and its integrals (cell_minmax likewise)
};

// hipLaunchKernelGGL, or -- with an event -- the launch whose completion the event is bound to
template <typename F, typename... Args>
inline void vr_launch_kernel(F k, dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t start,
                             hipEvent_t stop, Args... args)
{
    if (start || stop)
        hipExtLaunchKernelGGL(k, grid, block, (uint32_t)lds, stream, start, stop, 0u, args...);
    else
        hipLaunchKernelGGL(k, grid, block, lds, stream, args...);
}

// A technique that is one launch plus an optional last launch (MIP, the isosurface; the path tracer and its fold): first(start, stop)
// and last(stop) launch with the events to bind, or nullptr.  The frame's start rides on the first launch and its end
// on the last one there is; the event between the two (RaycastLaunch::mid_event) is recorded.
template <typename First, typename Last>
inline hipError_t vr_launch_bound(const RaycastLaunch &a, hipStream_t stream, bool has_last, First first, Last last)
{
    const bool bind_stop = a.bind_events && a.stop_event && a.stop_bound;
    const bool bind_start = a.bind_events && a.start_event && a.start_bound;
    first(bind_start ? a.start_event : nullptr, bind_stop && !has_last ? a.stop_event : nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && bind_start) *a.start_bound = true;
    if (e == hipSuccess && a.mid_event) e = hipEventRecord(a.mid_event, stream);
    if (has_last && e == hipSuccess) {
        last(bind_stop ? a.stop_event : nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess && bind_stop) *a.stop_bound = true;
    return e;
}

// f(VoxelType<VT>()) for the voxel type of a vrhip_format; an unknown format is an error
template <typename VT>
struct VoxelType {
    using type = VT;
};
template <typename F>
inline hipError_t vr_for_format(int format, F f)
{
    switch (format) {
    case VRHIP_UCHAR: return f(VoxelType<uint8_t>());
    case VRHIP_USHORT: return f(VoxelType<uint16_t>());
    case VRHIP_FLOAT: return f(VoxelType<float>());
    default: return hipErrorInvalidValue;
    }
}

hipError_t vr_launch_raycast(const RaycastLaunch &a, hipStream_t stream);
// FrameView::patch_class for the n_patches patches of a set of set_frames frames (work item p * set_frames = patch
// p of frame 0); the launch's camera, parameters, skip bitmaps and queue must be those of the frames to come
hipError_t vr_launch_patch_classes(const RaycastLaunch &a, uint32_t n_patches, uint32_t set_frames, uint8_t *cls,
                                   hipStream_t stream);
// fills the footprint volume vol.fp of `vol`: (w+1)(h+1)(d+1) entries rounded up to
// whole micro-bricks, 8 values of the volume's type each; vr_bricks.hip
hipError_t vr_launch_build_footprint(const VolView &vol, int format, hipStream_t stream);
// technique 1 (Woodcock-tracking path tracer), one sample per pixel; vr_pathtrace.hip
hipError_t vr_launch_pathtrace(const RaycastLaunch &a, hipStream_t stream);
// cell grid (vr_cells.hip): per-cell (min,max) of the raw voxel values incl. halo; then opacity
// bound + empty bit from (min,max) and the transfer function.  sparse_scratch: 13 * 4096 floats.
// records: d * cy * cx float2 of scratch for the separable streaming build (cells of <= 16 voxels,
// micro-brick rows of <= 2048 bricks: the x classes of a row live in LDS), or nullptr: the
// one-wave-per-cell kernel
// records: scratch of vr_cell_record_bytes(format) * grid.cx * grid.cy * vol.d bytes for the separable
// streaming build (nullptr, or cells of more than 16 voxels: the one-wave-per-cell kernel)
inline size_t vr_cell_record_bytes(int format) { return format == VRHIP_UCHAR ? 2 : format == VRHIP_USHORT ? 4 : 8; }
hipError_t vr_launch_cell_minmax(const VolView &vol, int format, const CellView &grid,
                                 float2 *minmax, hipStream_t stream, void *records = nullptr);
hipError_t vr_launch_cell_bounds(const float2 *minmax, const CellView &grid, float inv_max,
                                 const TfView &tf, float *sparse_scratch, float *bound,
                                 uint32_t *empty_bits, hipStream_t stream);
// (min, max) of the coarse grid `grid` (cx.., shift) from those of the fine one (ecx.., eshift < shift)
hipError_t vr_launch_cell_reduce(const float2 *fine, const CellView &grid, float2 *coarse, hipStream_t stream);
// CellView::cbound from CellView::bound (grid.cx/cy/cz, grid.ccx/ccy/ccz set)
#ifndef VR_LEAP_SHIFT
#define VR_LEAP_SHIFT 2
#endif
constexpr int kLeapShift = VR_LEAP_SHIFT;
hipError_t vr_launch_cell_coarse_bounds(const CellView &grid, float *cbound, hipStream_t stream);
constexpr int kLeapLevels = 7, kLeapRadius = 15;
// CellView::cdist from `cbound`: `dist` holds 2 x kLeapLevels x ccx*ccy*ccz bytes (two buffers the erosion passes
// alternate between); returns in *result the buffer that holds the table at the end
hipError_t vr_launch_cell_leap_radius(const CellView &grid, const float *cbound, uint8_t *dist, const uint8_t **result,
                                      hipStream_t stream);
// technique 2 (maximum intensity projection): one launch, one wave per 8x8 patch of every frame; vr_mip.hip
hipError_t vr_launch_mip(const RaycastLaunch &a, hipStream_t stream);
// technique 4 (first-hit isosurface): one launch of the same shape; vr_iso.hip
hipError_t vr_launch_iso(const RaycastLaunch &a, hipStream_t stream);
// technique 6 (two-dimensional transfer function): one launch of the same shape; vr_tf2d.hip
hipError_t vr_launch_tf2d(const RaycastLaunch &a, hipStream_t stream);
// technique 8 (pre-integrated classification): one launch of the same shape; vr_preint.hip
hipError_t vr_launch_preint(const RaycastLaunch &a, hipStream_t stream);
// slice views (vrhip_render_slices): n_slices images of W x H pixels, one wave per 8x8 patch of every slice, into
// out_dev[n_slices][H][W]; slices_dev: the n_slices parameter blocks in device memory; vr_slice.hip
hipError_t vr_launch_slices(const VolView &vol, int format, const TfView &tf, const vrhip_slice_params *slices_dev,
                            uint32_t n_slices, uint32_t W, uint32_t H, uint32_t use_linear, const float bg[4],
                            float4 *out_dev, hipStream_t stream);
// depth images (vrhip_render_depth): one wave per 8x8 patch of the rectangle params.(x0, y0, w, h) -- w, h resolved,
// never 0 -- of the frame.W x frame.H frame; the outputs are dense over the rectangle, any of them nullptr.
// frame: W, H, gsx, gsy and the ray_* fields only (nothing else of it is read).  Skipping: cell_minmax (ISO, MAX; its
// grid in cells' e* fields, as for vr_launch_mip) or cells.empty (OPACITY), nullptr: every sample is fetched; vr_depth.hip
struct DepthLaunch {
    VolView vol;
    TfView tf;
    CellView cells;
    const float2 *cell_minmax;
    FrameView frame;
    vrhip_camera_params cam;
    vrhip_rendering_params render;
    vrhip_raycast_params raycast;
    vrhip_depth_params params;
    int format;            // vrhip_format
    float4 *out_xyzt;
    float *out_aux;
    uint8_t *out_kind;
};
hipError_t vr_launch_depth(const DepthLaunch &a, hipStream_t stream);
// isosurface extraction (vrhip_isosurface_count / _extract): the blocks of 8^3 cubes b0 + (0 .. nb - 1) per axis,
// x fastest, of which the cubes lo <= corner 0 < hi are classified (lo < hi <= res - 1, every block holds one).
// cell_minmax: the (min, max) pairs of the cell grid of 2^cell_shift >= 8 voxels, cell_cx x cell_cy x .. cells, or
// nullptr: every block is fetched.  vr_mesh.hip
struct MeshLaunch {
    VolView vol;
    int format;            // vrhip_format
    float iso;
    uint32_t lo[3], hi[3];
    uint32_t b0[3], nb[3];
    const float2 *cell_minmax;
    int cell_shift, cell_cx, cell_cy;
};
constexpr uint32_t kMeshSkipped = 0x80000000u;   // a block's count word: skipped by the cell grid (its count is 0)
constexpr uint32_t kMeshScanChunk = 4096;        // block counts per workgroup of the scan
inline size_t vr_mesh_scan_partials(size_t n_blocks) { return (n_blocks + kMeshScanChunk - 1) / kMeshScanChunk; }
// pass 1: counts[n_blocks], one word per block (its triangles, or kMeshSkipped)
hipError_t vr_launch_mesh_count(const MeshLaunch &a, uint32_t *counts, hipStream_t stream);
// the exclusive 64-bit prefix sum of the counts, reduce-then-scan in separate launches: partials holds
// 2 * vr_mesh_scan_partials(n_blocks) + 2 words and ends with the totals (triangles, skipped blocks); offsets
// (n_blocks words) may be nullptr: the totals alone
hipError_t vr_launch_mesh_scan(const uint32_t *counts, size_t n_blocks, unsigned long long *partials,
                               unsigned long long *offsets, hipStream_t stream);
// pass 2: every triangle to its place, nine floats each; normals may be nullptr
hipError_t vr_launch_mesh_emit(const MeshLaunch &a, const uint32_t *counts, const unsigned long long *offsets,
                               float *positions, float *normals, hipStream_t stream);
// the indexed extraction (vrhip_isosurface_count_indexed / _extract_indexed): the blocks of 8^3 grid points
// b0 + (0 .. pnb - 1) per axis, x fastest, that own a point lo <= P <= hi of the launch
inline void vr_mesh_point_blocks(const MeshLaunch &a, uint32_t pnb[3])
{
    for (int i = 0; i < 3; ++i) pnb[i] = a.hi[i] / VRHIP_MESH_BLOCK - a.b0[i] + 1u;
}
// the rank table of a point block that holds a vertex: per row of eight points (row = y + 8 z) the points' 7-bit
// edge masks as the bytes of a 64-bit word, x ascending, and the number of the row's first vertex
constexpr uint32_t kMeshTableRows = 64;
constexpr size_t kMeshTableBytes = kMeshTableRows * (sizeof(unsigned long long) + sizeof(uint32_t));   // 768
// vcounts[n_point_blocks]: a block's vertices, or kMeshSkipped; vflags: 1 where it holds a vertex, else 0
hipError_t vr_launch_mesh_vertex_count(const MeshLaunch &a, uint32_t *vcounts, uint32_t *vflags, hipStream_t stream);
// every vertex to its place (voffsets: the scan of vcounts), three floats each, normals may be nullptr; the table
// of a block that holds a vertex to its slot (slots: the scan of vflags) in row_masks / row_bases
hipError_t vr_launch_mesh_vertex_emit(const MeshLaunch &a, const uint32_t *vcounts, const unsigned long long *voffsets,
                                      const unsigned long long *slots, float *vertices, float *normals,
                                      unsigned long long *row_masks, uint32_t *row_bases, hipStream_t stream);
// pass 2's triangles (counts, offsets: pass 1's and their scan) as three vertex numbers each
hipError_t vr_launch_mesh_index_emit(const MeshLaunch &a, const uint32_t *counts, const unsigned long long *offsets,
                                     const unsigned long long *slots, const unsigned long long *row_masks,
                                     const uint32_t *row_bases, uint32_t *indices, hipStream_t stream);
// volume statistics (vrhip_volume_statistics): the blocks of 8^3 voxels b0 + (0 .. nb - 1) per axis, x fastest, of
// which the voxels lo <= v < hi are classified (lo < hi <= res, every block holds one).  cell_minmax as for MeshLaunch.
// lds_hist: the workgroups keep the table in (dynamic) LDS and flush it; else every count goes to `hist` at once.
// vr_stats.hip
struct StatsLaunch {
    VolView vol;
    int format;            // vrhip_format
    uint32_t lo[3], hi[3];
    uint32_t b0[3], nb[3];
    uint32_t bins_v, bins_g;
    float v_lo, v_hi, k_v, k_g;
    bool moments, lds_hist;
    const float2 *cell_minmax;
    int cell_shift, cell_cx, cell_cy;
    int num_cus;
};
// a block's, a chunk's or the call's moments
struct StatsRec {
    double sum, sum_sq;
    float mn, mx;
};
// counters[]: 64-bit words the launch adds to
enum { kStatsNan = 0, kStatsBelow, kStatsAbove, kStatsGradNan, kStatsBinned, kStatsFetched, kStatsSkipConst, kStatsSkipWindow,
       kStatsCounters };
constexpr uint32_t kStatsChunk = VRHIP_STATS_SUM_CHUNK;   // blocks per workgroup = per chunk of the moments' sum
constexpr uint32_t kStatsLdsBins = 16384;                 // the largest table a workgroup keeps in LDS (64 KiB)
inline size_t vr_stats_chunks(size_t n_blocks) { return (n_blocks + kStatsChunk - 1) / kStatsChunk; }
// hist (bins_g * bins_v words) and counters are zero before the launch; chunk_recs: vr_stats_chunks(n_blocks)
// records, written with a.moments only
hipError_t vr_launch_stats(const StatsLaunch &a, unsigned long long *hist, unsigned long long *counters,
                           StatsRec *chunk_recs, hipStream_t stream);
// the chunk records added in ascending order into *total
hipError_t vr_launch_stats_total(const StatsRec *chunk_recs, size_t n_chunks, StatsRec *total, hipStream_t stream);
// volume filters (vrhip_filter_volume): every block of 8^3 voxels of `vol` (x fastest) filtered into `dst`, a
// micro-bricked volume of the same layout and type that is not `vol.data`.  cell_minmax as for MeshLaunch: the
// (min, max) of vol's coarse cells, or nullptr: every block is fetched.  vr_filter.hip
struct FilterLaunch {
    VolView vol;
    int format;            // vrhip_format
    uint32_t kind;         // VRHIP_FILTER_*
    uint32_t radius[3];
    float taps[3][VRHIP_FILTER_MAX_RADIUS + 1];
    const float2 *cell_minmax;
    int cell_shift, cell_cx, cell_cy, cell_cz;
    int num_cus;
};
// counters[]: 64-bit words the launch adds to
enum { kFilterFetched = 0, kFilterSkipped, kFilterCounters };
inline size_t vr_filter_blocks(const VolView &v)
{
    return (size_t)((v.w + 7) / 8) * (size_t)((v.h + 7) / 8) * (size_t)((v.d + 7) / 8);
}
// counters are zero before the launch
hipError_t vr_launch_filter(const FilterLaunch &a, void *dst, unsigned long long *counters, hipStream_t stream);
// volume morphology (vrhip_morph_volume): one sweep over every block of 8^3 voxels of `vol` (x fastest) into `dst`, a
// micro-bricked volume of the same layout and type that is not `vol.data`.  vol is what the sweep takes its extremes
// of: the source, or the intermediate of a two-sweep op; f, for the two difference modes only, the source's voxels
// in the same layout.  cell_minmax: the (min, max) of the SOURCE's coarse cells, or nullptr: every block is fetched;
// skip_scale 1 for a first sweep, 2 for a second (the constant test's dilation in radii).  vr_morph.hip
enum { kMorphMin = 0, kMorphMax, kMorphMaxMin, kMorphFMinusMax, kMorphMinMinusF };
struct MorphLaunch {
    VolView vol;
    const void *f;
    int format;            // vrhip_format
    uint32_t mode;         // kMorph*
    uint32_t shape;        // VRHIP_MORPH_BOX / _BALL
    uint32_t radius[3];
    uint32_t skip_scale;
    const float2 *cell_minmax;
    int cell_shift, cell_cx, cell_cy, cell_cz;
    int num_cus;
};
// counters[]: 64-bit words the launch adds to, zero before it
enum { kMorphFetched = 0, kMorphSkipped, kMorphCounters };
hipError_t vr_launch_morph(const MorphLaunch &a, void *dst, unsigned long long *counters, hipStream_t stream);
// the frame launch for a.render.technique
inline hipError_t vr_launch_frame(const RaycastLaunch &a, hipStream_t stream)
{
    return a.render.technique == VRHIP_TECHNIQUE_PREINT ? vr_launch_preint(a, stream)
           : a.render.technique == VRHIP_TECHNIQUE_TF2D ? vr_launch_tf2d(a, stream)
           : a.render.technique == VRHIP_TECHNIQUE_ISO ? vr_launch_iso(a, stream)
           : a.render.technique == VRHIP_TECHNIQUE_MIP ? vr_launch_mip(a, stream)
           : a.render.technique == 1                   ? vr_launch_pathtrace(a, stream)
                                                       : vr_launch_raycast(a, stream);
}

// skip bitmap from bricks + TF + prefix
hipError_t vr_launch_skipmap(const BrickView &bricks, int format, float inv_max, const TfView &tf,
                             uint32_t *bits, uint32_t n_words, hipStream_t stream);
// SkipView::near_bits from the skip bitmap: scratch = 2 bytes per brick
hipError_t vr_launch_skip_near(const BrickView &bricks, const uint32_t *bits, uint32_t n_words, uint32_t radius,
                               uint8_t *scratch, uint32_t *near_bits, hipStream_t stream);

hipError_t vr_launch_build_bricks(const VolView &vol, int format, const uint32_t tex[3],
                                  void *bricks_out, hipStream_t stream);
// downsampling kernel (volumeraycast.cl:966-994): lo = low-res size, vpc = voxels per cell
hipError_t vr_launch_downsample(const VolView &vol, int format, const int lo[3], const int vpc[3],
                                void *out_dense, hipStream_t stream);
// synthetic field written straight into the micro-brick layout
hipError_t vr_launch_synth(int kind, const VolView &vol, int format, hipStream_t stream);
// dense x-fastest slices [z0, z0+nz) (device memory, `dense` points at slice z0) <-> bricks
hipError_t vr_launch_retile(const VolView &vol, int format, const void *dense, int z0, int nz,
                            bool to_bricks, hipStream_t stream);

// Blocks per CU of `kernel` (block_dim threads, `lds` bytes of dynamic LDS), after raising the
// kernel's dynamic LDS limit where needed.  Both are per device (hipFuncSetAttribute acts on the
// current device's copy of the function), so the answers are cached per (kernel address, device,
// LDS size), under a lock: renderers on several devices or host threads share this code.  The
// kernel's address is part of the key because the function-local statics exist once per pointer
// TYPE K, and many instantiations (ESS / INSTR / XS / FP variants) share one signature.
template <typename K>
hipError_t vr_prepare_kernel(K kernel, int block_dim, size_t lds, int *nb_out, const char *what, int num_cus)
{
    static std::mutex mu;
    static std::map<std::tuple<const void *, int, size_t>, int> cache;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple((const void *)kernel, dev, lds);
    const auto it = cache.find(key);
    if (it != cache.end()) { *nb_out = it->second; return hipSuccess; }
    if (lds > 48 * 1024) {
        e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block_dim, lds) != hipSuccess || nb < 1)
        nb = 1;
    if (const char *ev = getenv("VRHIP_BLOCKS_PER_CU")) {   // tuning / experiments
        const int v = atoi(ev);
        if (v > 0) nb = v;
    }
    if (getenv("VRHIP_DEBUG"))
        fprintf(stderr, "[vrhip] %s @%p: device %d, lds=%zu B, blocks/CU=%d, CUs=%d\n", what, (const void *)kernel, dev,
                lds, nb, num_cus);
    cache[key] = nb;
    *nb_out = nb;
    return hipSuccess;
}
