// vr_renderer.h -- the host state of one renderer (vrhip_renderer, include/vrhip.h), shared by the units that
// implement the C ABI: vrhip_api.hip, vrhip_gather.hip, vrhip_ingest_api.hip, vrhip_slice_api.hip, vrhip_depth_api.hip,
// vrhip_mesh_api.hip, vrhip_stats_api.hip, vrhip_filter_api.hip.  Host only.
//  * DevBuf / Handle: device memory, events and the stream, freed with the object that holds them;
//  * grow(): the one place that (re)allocates a renderer's buffer;
//  * the invalidation functions: one per cause, next to the table of what depends on what.
#ifndef VR_RENDERER_H
#define VR_RENDERER_H

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "vr_internal.h"

// Device memory that goes away with its holder.  Never an object of static storage duration: a free after the
// runtime has shut down is an error of its own.
template <class T = void>
struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;     // capacity (0 for a borrowed pointer)
    bool owned = true;    // false: somebody else's memory (borrow()), never freed from here

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), owned(o.owned) { o.forget(); }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; owned = o.owned;
            o.forget();
        }
        return *this;
    }
    ~DevBuf() { release(); }

    void release()   // (errors of the free are ignored)
    {
        if (p && owned) (void)hipFree(p);
        forget();
    }
    void borrow(T *other) { release(); p = other; owned = false; }
    operator T *() const { return p; }

private:
    void forget() { p = nullptr; bytes = 0; owned = true; }
};

// Pinned host memory that goes away with its holder (the staging block of a download).
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    void release()   // (errors of the free are ignored)
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// An event or a stream, destroyed with its holder.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using DevEvent = Handle<hipEvent_t, hipEventDestroy>;
using DevStream = Handle<hipStream_t, hipStreamDestroy>;

struct VolumeSlot {
    // owned, or -- in a `borrowed` slot -- pointers into the slot of the renderer that owns the voxels
    DevBuf<> dev;         // micro-bricked voxels (channel 0 of a multi-channel volume)
    DevBuf<> chan[3];     // channels 1..3 of CL_RG / CL_RGBA volumes
    DevBuf<> bricks;      // (min,max) grid
    bool bricks_built = false;
    DevBuf<float2> pt_minmax;     // path tracer: per-cell (min,max) incl. halo, built on demand
    bool pt_minmax_valid = false;
    DevBuf<float2> fine_minmax;   // ray caster: the same on the finer grid of the empty bits
    bool fine_minmax_valid = false;
    bool borrowed = false;        // dev / chan / bricks belong to another renderer (vrhip_share_volumes)
};

struct vrhip_renderer {
    int device = 0;
    int num_cus = 256;
    DevStream own_stream;             // (first: destroyed after everything that may still be freed behind it)
    hipStream_t stream = nullptr;
    mutable std::string err;
    std::string devname;

    uint32_t res[3] = {0, 0, 0};
    int format = -1;
    int channels = 1;                 // 1 = CL_R, 2 = CL_RG, 4 = CL_RGBA
    // HBM layout of a time step: 4x4x4-voxel micro-bricks (vr_internal.h, DESIGN.md "Data
    // layout"); nb = ceil(res / 4)
    uint32_t nb[3] = {0, 0, 0};
    std::vector<VolumeSlot> vols;
    uint32_t timestep = 0;

    DevBuf<float4> tff;
    uint32_t tff_n = 0;
    DevBuf<uint32_t> prefix;
    uint32_t prefix_n = 0;
    // the 2-D transfer function of technique 6 (Tf2dView): state of its own, made whole by
    // vrhip_set_transfer_function_2d and read by technique 6's frames alone
    DevBuf<float4> tf2d;
    DevBuf<uint32_t> tf2d_nz;
    uint32_t tf2d_nv = 0, tf2d_ng = 0;
    float tf2d_inv_ghi = 0.f;

    // the 1-D table as uploaded to `tff` (n entries of four floats): what ensure_preint integrates, without a read-back
    std::vector<float> tff_host;
    // technique 8's integral table and prefix count (PreintView), made from tff_host by ensure_preint when a
    // technique-8 frame first needs them; read by technique 8's frames alone
    DevBuf<double> preint_prefix;
    DevBuf<uint32_t> preint_nz;
    bool preint_valid = false;

    uint32_t brick_tex[3] = {0, 0, 0}, brick_edge[3] = {0, 0, 0};
    float brick_res[3] = {1, 1, 1};
    bool bricks_valid = false;

    // ESS skip bitmap of the current timestep
    DevBuf<uint32_t> skip_bits;
    uint32_t skip_words = 0;
    bool skip_dirty = true;
    // patch culling of the DDA pre-pass: the skip bitmap dilated by cull_radius bricks (SkipView::near_bits)
    DevBuf<uint32_t> near_bits;
    DevBuf<uint8_t> near_scratch;
    uint32_t cull_radius = 4;         // VRHIP_CULL_RADIUS (bricks; 0 = no patch culling)

    // cell grid of the current timestep + TF (CellView, vr_internal.h): opacity bound for the
    // path tracer, empty bits for the ray caster
    CellView cells = {nullptr, nullptr, 0, 0, 0, 3, 0, 0, 0, 3};
    DevBuf<float> cell_bound;
    DevBuf<uint32_t> cell_empty;
    DevBuf<float> cell_sparse;     // 13 x 4096 floats of scratch for the TF range-max table
    bool cells_have_bound = false, cells_have_empty = false;   // r->cells' tables match volume, time step and TF
    bool pt_cull = true;           // VRHIP_PT_NO_CULL=1 disables the path tracer's culling
    bool pt_leap = true;           // VRHIP_PT_NO_LEAP=1: no leaps over macro cells (A/B)
    bool pt_leap_far = true;       // VRHIP_PT_NO_FAR_LEAP=1: leaps stay inside one macro cell (A/B)
    DevBuf<uint8_t> cell_dist;     // CellView::cdist (two buffers)
    const uint8_t *cell_dist_table = nullptr;
    bool skip_empty = true;        // VRHIP_NO_EMPTY_SKIP=1 disables the ray caster's empty runs
    bool skip_empty_force = false; // VRHIP_EMPTY_SKIP=1: also where it is not expected to pay (see ray_skip_empty)

    vrhip_camera_params cam;
    vrhip_rendering_params render;
    vrhip_raycast_params raycast;
    vrhip_pathtrace_params pathtrace;
    vrhip_iso_params iso;
    bool use_ess = true;

    DevBuf<float4> fb;
    uint32_t fb_w = 0, fb_h = 0;

    DevBuf<DevStats> stats_dev;
    bool stats_enabled = false;

    // work queue of 8x8 wave tiles (centre first) for the current frame/tile set
    DevBuf<WaveTile> queue_dev;
    uint32_t queue_n = 0;
    DevBuf<uint32_t> queue_head;      // 2 x kControlWords (queue head, cont count, cont head, pad, sort bins + cursors):
                                      // the sets of launches alternate between the two blocks (FrameView::next_ctrl)
    DevBuf<uint8_t> patch_class;      // FrameView::patch_class of the current queue, camera, parameters and skip bitmaps
    std::vector<uint8_t> patch_class_key;   // what the classes were computed for (empty: nothing valid)
    uint32_t skip_version = 0;        // bumped whenever the skip bitmaps are rebuilt
    uint32_t queue_version = 0;       // bumped whenever the work queue is rebuilt
    uint32_t queue_frames = 1;        // frames per set of the current queue
    bool use_patch_classes = true;    // VRHIP_NO_PATCH_CLASS=1 disables
    int occ_force = 0;                // VRHIP_OCC=2|3: waves per SIMD of the default marching kernels (0 = by volume)
    int occ_force_split = 0;          // ... of phase 2 (VRHIP_OCC sets both, VRHIP_OCC_P1 / VRHIP_OCC_P2 one)
    uint32_t ctrl_sel = 0;            // the block the next set of launches uses
    bool ctrl_clean[2] = {false, false};   // that block is known to hold zeroes
    bool phase_timing = false;        // vrhip_set_phase_timing: an event between the phases of a frame
    int event_bind = 2;               // VRHIP_EVENT_BIND (launch_timed)
    bool frame_timing = true;         // vrhip_set_frame_timing: events around a frame's launches (vrhip_last_kernel_seconds)
    DevBuf<uint16_t> cost;            // per pixel: phase-2 rounds of the previous frame (sort key)
    DevBuf<uint32_t> order;           // sorted permutation of the suspended rays
    DevBuf<ContRec> live_rays;        // pre-pass output: live rays with their DDA state (phase 1's list)
    bool ray_list = true;             // VRHIP_NO_RAYLIST=1: phase 1 walks the live patches instead
    DevBuf<uint32_t> pm;              // FrameView::pm: the pixel-major block of a launch set (notes and index lists)
    bool pixel_major = true;          // VRHIP_PIXEL_MAJOR=0: launch sets keep the pre-pass's ray order (A/B)
    uint32_t pm_group = 64;           // VRHIP_PM_GROUP=1|32|64: a patch's index entries are padded to a multiple of it
    // vrhip_download_ray_order: the last render call was a pixel-major set, of pm_last_frames frames, on control block
    // pm_last_ctrl (queue, ray lists and block are as that set left them: prepare_render forgets it)
    bool pm_last = false;
    uint32_t pm_last_ctrl = 0, pm_last_frames = 0;
    DevBuf<uint32_t> seeds_dev;       // kMaxBatchFrames jitter seeds of a batch of frames
    DevBuf<vrhip_camera_params> cams_dev;   // kMaxBatchFrames cameras of a batch of per-frame views
    DevBuf<> samples_dev;             // vrhip_render_samples: the records and marks of a set of samples (lazily, reused)
    bool sort_cont = true;            // VRHIP_NO_SORT=1 disables
    DevBuf<LiveTile> live;            // DDA pre-pass output: patches with rays that sample
    bool prepass = true;              // VRHIP_NO_PREPASS=1 disables
    DevBuf<ContRec> cont;             // suspended rays of the two-phase march
    uint32_t round_budget = 10;       // phase-1 sample rounds per patch (0 = single phase)
    uint32_t refill_min = 16;         // phase 2: idle ray slots per wave before a refill (VRHIP_REFILL_MIN)
    std::vector<uint32_t> queue_key;   // W, H, tile_w, tile_h, tile ids...
    // image-order ESS: ping-pong hit images (volumerendercl.cpp:482-488, :524-530) + per-frame scratch
    DevBuf<uint8_t> hit_in, hit_out, hit_status, hit_any;
    uint32_t hit_w = 0, hit_h = 0;
    DevBuf<> fp;                      // footprint volume of the current time step (VolView::fp)
    bool fp_valid = false;
    uint32_t fp_timestep = 0;         // the time step `fp` was built for
    uint32_t fp_candidate = 0xffffffffu, fp_candidate_frames = 0;   // time series: see ensure_footprint
    bool fp_active = false;           // this frame reads it
    const void *fp_use = nullptr;     // what this frame reads: the renderer's own `fp` or its owner's
    vrhip_renderer *vol_owner = nullptr;   // vrhip_share_volumes: whose voxels (and footprint volume) this renderer renders from
    std::vector<vrhip_renderer *> sharers; // the renderers that render from THIS one's voxels (their vol_owner is this)
    size_t fp_failed_bytes = 0;       // a footprint allocation of this size failed: not retried until the volume or the cap changes
    bool use_fp = true;               // VRHIP_NO_FOOTPRINT=1 disables
    size_t fp_max_bytes = (size_t)96 << 30;   // VRHIP_FOOTPRINT_MAX_GB
    DevBuf<float4> env;               // environment map (float RGBA), or empty
    uint32_t env_w = 0, env_h = 0;

    // 8-bit frames to host memory (vrhip_quantise_rgba8 with a host destination, vr_rgba8.hip): the quantised words
    // on the device and the pinned block they are copied through; grown on demand, kept, freed with the renderer
    DevBuf<uint32_t> rgba8_dev;
    PinnedBuf rgba8_host;

    // slice views (vrhip_render_slices, vrhip_slice_api.hip): the parameter blocks of a call in device memory, and --
    // for a host destination -- the images on the device and the pinned block they are copied through; grown on
    // demand, kept, freed with the renderer.  No render entry point reads them.
    DevBuf<vrhip_slice_params> slice_params_dev;
    DevBuf<float4> slice_out_dev;
    PinnedBuf slice_host;

    // depth images (vrhip_render_depth, vrhip_depth_api.hip): for host destinations, the three outputs of a call in
    // one device block and the pinned block they are copied through; what the last call launched
    // (vrhip_last_depth_info).  Grown on demand, kept, freed with the renderer.  No render entry point reads them.
    DevBuf<> depth_out_dev;
    PinnedBuf depth_host;
    vrhip_depth_info depth_info;
    bool have_depth_info = false;

    // isosurface extraction (vrhip_isosurface_count / _extract, vrhip_mesh_api.hip): the per-block counts, their
    // prefix sum and its partial sums; for host destinations the triangles on the device and the pinned block they
    // are copied through (the totals always travel through mesh_totals_host); what the last call did
    // (vrhip_last_mesh_info).  Nothing is kept from one call to the next but the allocations: every call counts
    // anew.  Grown on demand, freed with the renderer.  No render entry point reads them.
    DevBuf<uint32_t> mesh_counts;
    DevBuf<unsigned long long> mesh_offsets, mesh_partials;
    DevBuf<float> mesh_out_dev;
    PinnedBuf mesh_host, mesh_totals_host;
    vrhip_mesh_info mesh_info;
    bool have_mesh_info = false;
    // ... and its indexed form (vrhip_isosurface_count_indexed / _extract_indexed): per point block the vertex count,
    // the holds-a-vertex flag and their two prefix sums, the partial sums of both scans, the rank tables of the
    // blocks that hold a vertex (vr_internal.h kMeshTableBytes each); the cube blocks' words are the ones above,
    // counted anew like them, and so is the staging of host destinations.  imesh_info: vrhip_last_indexed_mesh_info;
    // mesh_info is not touched.
    DevBuf<uint32_t> imesh_vcounts, imesh_vflags, imesh_row_bases;
    DevBuf<unsigned long long> imesh_voffsets, imesh_slots, imesh_partials, imesh_row_masks;
    PinnedBuf imesh_totals_host;
    vrhip_indexed_mesh_info imesh_info;
    bool have_imesh_info = false;

    // volume statistics (vrhip_volume_statistics, vrhip_stats_api.hip): the counters and the call's moments in one
    // device block, the chunks' moment records, for a host destination the table on the device, and the pinned block
    // all of it is copied through; what the last call did (vrhip_last_stats_info).  Nothing but the allocations is
    // kept from one call to the next.  Grown on demand, freed with the renderer.  No render, slice, depth or mesh
    // entry point reads them.
    DevBuf<unsigned long long> stats_ws, stats_hist_dev;
    DevBuf<StatsRec> stats_chunks;
    PinnedBuf stats_host;
    vrhip_stats_info stats_info;
    bool have_stats_info = false;

    // volume filters (vrhip_filter_volume, vrhip_filter_api.hip): the counters of a call in device memory, and what
    // the last call did (vrhip_last_filter_info).  The in-place scratch lives only inside a call.  No render, slice,
    // depth, mesh or statistics entry point reads them.
    DevBuf<unsigned long long> filter_ws;
    vrhip_filter_info filter_info;
    bool have_filter_info = false;

    // volume morphology (vrhip_morph_volume, vrhip_morph_api.hip): the counters of a call's two sweeps in device
    // memory, and what the last call did (vrhip_last_morph_info).  The intermediate and the in-place scratch live only
    // inside a call.  No render, slice, depth, mesh, statistics or filter entry point reads them.
    DevBuf<unsigned long long> morph_ws;
    vrhip_morph_info morph_info;
    bool have_morph_info = false;

    // device-side ingest (vrhip_ingest_raw, vrhip_volume_histogram): the running maximum and the 256 64-bit
    // histogram counters in device memory, the events around its kernels (all created on first use)
    size_t ingest_slab_bytes = (size_t)256 << 20;   // VRHIP_INGEST_SLAB_BYTES: staging per slab
    DevBuf<> ingest_ws;
    DevEvent evi0, evi1;
    double ingest_seconds = 0.0;

    DevEvent ev0, ev1, evm, evb0, evb1;
    bool timed = false, bricks_timed = false, phase_timed = false;
    vrhip_launch_info last_info;      // what the last render call launched (vrhip_last_launch_info)
    bool have_info = false;

    vrhip_renderer()
    {
        // defaults of volumerendercl.h:43-81
        std::memset(&cam, 0, sizeof cam);
        std::memset(&render, 0, sizeof render);
        std::memset(&raycast, 0, sizeof raycast);
        const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        std::memcpy(cam.viewMat, ident, sizeof ident);
        for (int i = 0; i < 3; ++i) { cam.bbox_bl[i] = -1.f; cam.bbox_tr[i] = 1.f; }
        for (int i = 0; i < 4; ++i) render.backgroundColor[i] = 1.f;
        for (int i = 0; i < 3; ++i) render.modelScale[i] = 1.f;
        render.illumType = 1;
        render.useLinear = 1;
        render.seed = 42;
        raycast.samplingRate = 1.5f;
        for (int i = 0; i < 3; ++i) raycast.brickRes[i] = 1.f;
        pathtrace.max_extinction = 100.f;
        iso.isoValue = 0.5f;
        iso.refineSteps = 4;
        iso.reserved[0] = iso.reserved[1] = 0;
    }
};

// ---- errors

inline std::string &create_error()   // what vrhip_last_error(NULL) answers: the last failed vrhip_create
{
    static std::string msg;
    return msg;
}

inline int fail(const vrhip_renderer *r, int code, const std::string &msg)
{
    if (r) r->err = msg;
    else create_error() = msg;
    return code;
}

#define VR_HIP(r, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(r, VRHIP_ERR_HIP,                                                     \
                        std::string("ERROR: " #call " (") + hipGetErrorString(e_) + ")");     \
    } while (0)

#define VR_REQUIRE(r, cond, code, msg)                                                        \
    do {                                                                                      \
        if (!(cond)) return fail(r, code, msg);                                               \
    } while (0)

inline int set_device(const vrhip_renderer *r)
{
    VR_HIP(r, hipSetDevice(r->device));
    return VRHIP_OK;
}

// ---- the one place that (re)allocates a buffer of a renderer

enum : unsigned {
    kGrowFresh = 1u,      // allocate anew whatever the capacity (the caller initialises the contents)
    kGrowTolerate = 2u,   // an allocation failure is not an error: the buffer stays empty, nothing is reported
};

// `b` holds at least `bytes` afterwards.  Nothing happens when it does already; otherwise the renderer's stream
// is waited for (it may be using the old allocation), the old one is freed and a new one made.  On failure the
// buffer is empty.
template <class T>
int grow(vrhip_renderer *r, DevBuf<T> &b, size_t bytes, unsigned flags = 0)
{
    if (!(flags & kGrowFresh) && b.p && bytes <= b.bytes) return VRHIP_OK;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    b.release();
    const hipError_t e = hipMalloc((void **)&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        if (flags & kGrowTolerate) {
            (void)hipGetLastError();
            return VRHIP_OK;
        }
        return fail(r, VRHIP_ERR_HIP, std::string("ERROR: hipMalloc of ") + std::to_string(bytes) + " bytes (" +
                                          hipGetErrorString(e) + ")");
    }
    b.bytes = bytes;
    return VRHIP_OK;
}

// The same for the pinned staging block: nothing uses the old one when this is called (its users wait for their
// copy before they return).
inline int grow_pinned(vrhip_renderer *r, PinnedBuf &b, size_t bytes)
{
    if (b.p && bytes <= b.bytes) return VRHIP_OK;
    b.release();
    const hipError_t e = hipHostMalloc(&b.p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(r, VRHIP_ERR_HIP, std::string("ERROR: hipHostMalloc of ") + std::to_string(bytes) + " bytes (" +
                                          hipGetErrorString(e) + ")");
    }
    b.bytes = bytes;
    return VRHIP_OK;
}

// the scan of the sparse gather message's head (vrhip_gather.hip), shared by the float and the 8-bit pack
void launch_pack_scan(hipStream_t st, int32_t *flags_pos, uint32_t n_slots, int32_t *slots, uint32_t *count);

// ---- views of the renderer's state for the launchers (vr_internal.h)

inline size_t fmt_bytes(int format) { return format == VRHIP_UCHAR ? 1 : format == VRHIP_USHORT ? 2 : 4; }

inline float inv_max_of(int format)
{
    return format == VRHIP_UCHAR ? 1.0f / 255.0f : format == VRHIP_USHORT ? 1.0f / 65535.0f : 1.0f;
}

inline VolView make_vol_view(const vrhip_renderer *r, const void *data)
{
    VolView v;
    v.data = data;
    v.w = (int)r->res[0]; v.h = (int)r->res[1]; v.d = (int)r->res[2];
    v.fw = (float)v.w; v.fh = (float)v.h; v.fd = (float)v.d;
    v.inv_max = inv_max_of(r->format);
    v.nbx = r->nb[0];
    v.nby = r->nb[1];
    v.nbz = r->nb[2];
    v.ystride = r->nb[0] * 64u;
    v.zstride = (unsigned long long)r->nb[0] * r->nb[1] * 64ull;
    v.chan[0] = v.chan[1] = v.chan[2] = nullptr;
    v.channels = 1;
    v.fp = nullptr;
    v.fp_nbx = (r->res[0] + 4u) >> 2;
    v.fp_nby = (r->res[1] + 4u) >> 2;
    return v;
}

// the render view of a time step: all channels
inline VolView make_render_view(const vrhip_renderer *r, const VolumeSlot &s)
{
    VolView v = make_vol_view(r, s.dev);
    for (int i = 0; i < 3; ++i) v.chan[i] = s.chan[i];
    v.channels = r->channels;
    v.fp = r->fp_active ? r->fp_use : nullptr;
    return v;
}

inline BrickView make_brick_view(const vrhip_renderer *r, const void *data)
{
    BrickView b;
    b.data = data;
    b.bw = (int)r->brick_tex[0];
    b.bh = (int)r->brick_tex[1];
    b.bd = (int)r->brick_tex[2];
    return b;
}

inline TfView make_tf_view(const vrhip_renderer *r)
{
    TfView t;
    t.tff = r->tff;
    t.tff_n = r->tff_n;
    t.prefix = r->prefix;
    t.prefix_n = r->prefix_n;
    return t;
}

inline Tf2dView make_tf2d_view(const vrhip_renderer *r)
{
    Tf2dView t;
    t.table = r->tf2d;
    t.nz = r->tf2d_nz;
    t.n_v = r->tf2d_nv;
    t.n_g = r->tf2d_ng;
    t.inv_ghi = r->tf2d_inv_ghi;
    return t;
}

inline PreintView make_preint_view(const vrhip_renderer *r)
{
    PreintView t;
    t.tff = r->tff;
    t.prefix = r->preint_prefix;
    t.nz = r->preint_nz;
    t.n = r->tff_n;
    return t;
}

// what make_ray derives the camera from: the frame size and the reference's padded launch size
inline void set_frame_geometry(FrameView *f, uint32_t width, uint32_t height)
{
    f->W = width;
    f->H = height;
    // padded NDRange of the reference (volumerendercl.cpp:513-514): a full extra group
    // when the size is already a multiple of 8; the camera is derived from it.
    f->gsx = width + (8u - width % 8u);
    f->gsy = height + (8u - height % 8u);
    const float gsx = (float)f->gsx, gsy = (float)f->gsy;
    float aspect = gsy / gsx;
    const float other = gsx / gsy;
    aspect = other < aspect ? other : aspect;   // vmin(aspect, other), vr_device_math.h
    f->ray_aspect = aspect;
    f->ray_psx = 2.f / gsx;
    f->ray_psy = 2.f / gsy;
}

// (re)allocate a slot for `timestep`, checking that res/format agree with other timesteps (vrhip_api.hip)
int prepare_slot(vrhip_renderer *r, const uint32_t res[3], int format, uint32_t timestep, VolumeSlot **slot,
                 int channels = 1);
// the cell grids of the current time step, and what the units outside vrhip_api.hip ask of them (vrhip_api.hip):
// ensure_cells builds what is stale (tables = false: the (min, max) pairs and the geometry only, nothing made from
// the transfer function); cell_minmax_of: the pairs as ensure_cells left them; mip_skips: do techniques 2 and 4 --
// and the depth images -- step over samples with object-order ESS on
int ensure_cells(vrhip_renderer *r, bool need_bound, bool need_empty, bool tables = true);
const float2 *cell_minmax_of(const vrhip_renderer *r, bool fine);
bool mip_skips(const vrhip_renderer *r);

// ---- derived state: what is built lazily from what, and what makes it stale
//
//   derived                                          | built by            | depends on
//   -------------------------------------------------+---------------------+-----------------------------------------
//   bricks of a slot (bricks_built)                  | vrhip_build_bricks  | that slot's voxels
//   bricks_valid, brick geometry                     | vrhip_build_bricks  | resolution; a build since the last voxel
//                                                    |                     | change of ANY slot (a sharer: its owner's)
//   skip bitmap + near bits (skip_dirty,             | ensure_skipmap      | bricks of the current step, TF, prefix
//     skip_version)                                  |                     | sum, current step
//   cell (min,max) of a slot, coarse and fine        | ensure_cells        | that slot's voxels
//     (pt_minmax_valid, fine_minmax_valid)           |                     |
//     (read as they are by techniques 2 and 4, which|                     |
//     derive nothing of their own from them)         |                     |
//   opacity bounds / macro bounds / leap radii,      | ensure_cells        | cell (min,max) of the current step, TF,
//     empty bits (cells_have_bound / _empty)         |                     | current step
//   footprint volume (fp_valid, fp_timestep;         | ensure_footprint    | voxels of the current step, current step
//     fp_failed_bytes: a size not to try again)      |                     | (fp_failed_bytes: any new voxels)
//   patch classes                                    | ensure_patch_classes| their byte key (patch_class_key), which
//                                                    |                     | holds skip_version and queue_version
//   2-D table, its column summary (tf2d, tf2d_nz,    | vrhip_set_transfer_ | the call's arguments alone: built whole at
//     tf2d_nv / _ng / _inv_ghi)                      |   function_2d       | set time, never stale, nothing derives
//                                                    |                     | from it (technique 6 reads it as it is,
//                                                    |                     | with the cell (min,max) like 2 and 4)
//   technique 8's integral table and prefix count    | ensure_preint       | TF
//     (preint_prefix, preint_nz; preint_valid)       |                     |
//
// A voxel write into ANY slot makes the renderer-wide tables stale, not only one into the current step (the code
// never looked at which).  fp_candidate / fp_candidate_frames count frames, and survive everything but a change
// of the step shown.  Mutation sites call one of the functions below and assign none of these members themselves;
// the ensure_* functions record what they built with the *_built functions.

inline void cells_tables_stale(vrhip_renderer *r) { r->cells_have_bound = r->cells_have_empty = false; }

// the voxels of time step `t` were (or are about to be) written: `r` and the renderers that share its volumes
inline void voxels_written(vrhip_renderer *r, uint32_t t)
{
    auto one = [t](vrhip_renderer *x) {
        if (t < x->vols.size()) {
            VolumeSlot &s = x->vols[t];
            s.bricks_built = s.pt_minmax_valid = s.fine_minmax_valid = false;
        }
        x->bricks_valid = false;
        x->skip_dirty = true;
        cells_tables_stale(x);
        x->fp_valid = false;
        x->fp_failed_bytes = 0;
    };
    one(r);
    for (vrhip_renderer *sh : r->sharers) one(sh);
}

// every slot is gone (their own flags with them)
inline void volumes_cleared(vrhip_renderer *r)
{
    r->bricks_valid = false;
    r->skip_dirty = true;
    cells_tables_stale(r);
    r->fp_valid = false;
    r->fp_failed_bytes = 0;
}

// the slots now point into `owner`'s, bricks included (after volumes_cleared)
inline void volumes_shared(vrhip_renderer *r, const vrhip_renderer *owner)
{
    r->bricks_valid = owner->bricks_valid;
    r->skip_dirty = true;
    cells_tables_stale(r);
    r->fp_valid = false;   // (its own footprint volume is not used while it shares: ensure_footprint)
}

inline void timestep_changed(vrhip_renderer *r)
{
    r->skip_dirty = true;
    cells_tables_stale(r);
    r->fp_valid = false;
}

// transfer function or its prefix sum
inline void tf_changed(vrhip_renderer *r)
{
    r->skip_dirty = true;
    cells_tables_stale(r);
    r->preint_valid = false;
}

// ensure_preint has made technique 8's tables from the transfer function as it is
inline void preint_built(vrhip_renderer *r) { r->preint_valid = true; }

// The 2-D transfer function (technique 6): the table is being replaced (n_v = 0: none is set until tf2d_set), then
// is whole.  No other derived state depends on it, and tf_changed does not touch it.
inline void tf2d_unset(vrhip_renderer *r) { r->tf2d_nv = r->tf2d_ng = 0; r->tf2d_inv_ghi = 0.f; }
inline void tf2d_set(vrhip_renderer *r, uint32_t n_v, uint32_t n_g, float inv_ghi)
{
    r->tf2d_nv = n_v;
    r->tf2d_ng = n_g;
    r->tf2d_inv_ghi = inv_ghi;
}

// vrhip_build_bricks has run: every slot's bricks match its voxels
inline void bricks_built(vrhip_renderer *r)
{
    r->bricks_valid = true;
    r->skip_dirty = true;
    cells_tables_stale(r);
}

inline void slot_bricks_built(VolumeSlot &s) { s.bricks_built = true; }
inline void cell_minmax_built(VolumeSlot &s, bool fine) { (fine ? s.fine_minmax_valid : s.pt_minmax_valid) = true; }
inline void cells_tables_built(vrhip_renderer *r, bool bound, bool empty)
{
    r->cells_have_bound = r->cells_have_bound || bound;
    r->cells_have_empty = r->cells_have_empty || empty;
}
inline void skipmap_built(vrhip_renderer *r) { r->skip_dirty = false; ++r->skip_version; }
inline void footprint_stale(vrhip_renderer *r) { r->fp_valid = false; }   // about to be overwritten
inline void footprint_alloc_failed(vrhip_renderer *r, size_t bytes) { r->fp_failed_bytes = bytes; }
inline void footprint_built(vrhip_renderer *r) { r->fp_valid = true; r->fp_timestep = r->timestep; }

#endif
