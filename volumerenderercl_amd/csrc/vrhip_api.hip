// vrhip_api.hip -- implementation of the C ABI in include/vrhip.h on the HIP runtime.
// Owns every device allocation of one renderer (like VolumeRenderCL owns its cl::Image
// objects, /root/reference/src/core/volumerendercl.h:446-463).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vr_renderer.h"

namespace {

constexpr uint32_t kSkipLdsMaxBytes = 64 * 1024;   // bitmap staged in LDS up to this size
// vrhip_render_samples: samples per launch set when the caller leaves it open -- the best of the sweep in DESIGN.md
// section 5.4 (4 ... 64 per set at 1024^2: the more the faster), as long as a set's scratch stays at what that sweep
// ran with (64 samples of 1024^2 pixels, 17 bytes each: 1.06 GiB); a caller that names a set size gets it
constexpr uint32_t kDefaultSamplesPerLaunch = 64;
constexpr unsigned long long kDefaultSampleRecords = 64ull << 20;

size_t volume_bytes(const vrhip_renderer *r)   // dense (host-side) size
{
    return (size_t)r->res[0] * r->res[1] * r->res[2] * fmt_bytes(r->format);
}

size_t volume_alloc_bytes(const vrhip_renderer *r)
{
    return (size_t)r->nb[0] * r->nb[1] * r->nb[2] * 64 * fmt_bytes(r->format);
}

void set_layout(vrhip_renderer *r)
{
    for (int i = 0; i < 3; ++i) r->nb[i] = (r->res[i] + 3) / 4;
}

// Dense x-fastest array (host memory, or device memory when dense_is_device) <-> micro-bricks,
// slab by slab (multiples of 4 slices) through a bounded device staging buffer.
hipError_t copy_volume(const vrhip_renderer *r, void *bricks_dev, void *dense, bool to_bricks,
                       bool dense_is_device, hipStream_t stream)
{
    const size_t bpv = fmt_bytes(r->format);
    const size_t slice_b = (size_t)r->res[0] * r->res[1] * bpv;
    const VolView v = make_vol_view(r, bricks_dev);
    if (dense_is_device) {
        hipError_t e = vr_launch_retile(v, r->format, dense, 0, (int)r->res[2], to_bricks, stream);
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    }
    int slab = (int)std::max<size_t>(4, ((size_t)256 << 20) / std::max<size_t>(slice_b, 1) / 4 * 4);
    slab = std::min<int>(slab, (int)((r->res[2] + 3) / 4 * 4));
    void *stage = nullptr;
    hipError_t e = hipMalloc(&stage, (size_t)slab * slice_b);
    if (e != hipSuccess) return e;
    for (int z0 = 0; z0 < (int)r->res[2] && e == hipSuccess; z0 += slab) {
        const int nz = std::min<int>(slab, (int)r->res[2] - z0);
        char *h = (char *)dense + (size_t)z0 * slice_b;
        if (to_bricks) {
            e = hipMemcpyAsync(stage, h, (size_t)nz * slice_b, hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = vr_launch_retile(v, r->format, stage, z0, nz, true, stream);
        } else {
            e = vr_launch_retile(v, r->format, stage, z0, nz, false, stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(h, stage, (size_t)nz * slice_b, hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);   // staging buffer is reused
    }
    (void)hipFree(stage);
    return e;
}

size_t bricks_bytes(const vrhip_renderer *r)
{
    return 2 * (size_t)r->brick_tex[0] * r->brick_tex[1] * r->brick_tex[2] * fmt_bytes(r->format);
}

// volumerendercl.cpp:39-54
uint32_t round_pow2(uint32_t n)
{
    uint32_t val = n - 1u;
    val |= val >> 1;
    val |= val >> 2;
    val |= val >> 4;
    val |= val >> 8;
    val |= val >> 16;
    val++;
    uint32_t x = val >> 1;
    return (val - n) > (n - x) ? x : val;
}

// log2 of the cell edges of the two cell grids (CellView): opacity bounds on at most 256 cells per axis,
// empty bits on at most 512 (edges 8 and 4 up to 2048^3)
void cell_shifts(const vrhip_renderer *r, int *shift, int *eshift)
{
    const uint32_t mres = std::max(r->res[0], std::max(r->res[1], r->res[2]));
    int sh = 3, es = 2;
    while (((mres + (1u << sh) - 1) >> sh) > 256u) ++sh;
    if (const char *e = getenv("VRHIP_CELL_SHIFT")) es = std::max(2, std::min(5, atoi(e)));   // A/B: 3 = one grid
    while (((mres + (1u << es) - 1) >> es) > 512u) ++es;
    *shift = sh;
    *eshift = std::min(es, sh);
}

// Does the ray caster step over empty cells (CellView::empty)?  Where the ESS bricks are not much
// larger than the cells the brick skipping has done the work already and the lookahead only costs.
// Measured on MI355X with cells of 4 voxels: -13 % frame time at 1024^3 (bricks of 16), -30 % at 2048^3
// (bricks of 32), +3 % at 256^3 (bricks of 4); with cells of 8 (round 1): +6 % at 1024^3 and 256^3,
// -25 % at 2048^3.  So: bricks of at least four cells.  Without ESS bricks the cells are all there is.
bool ray_skip_empty(const vrhip_renderer *r)
{
    if (!r->skip_empty || r->channels > 1) return false;
    if (r->skip_empty_force || !r->use_ess || !r->bricks_valid) return true;
    int shift, eshift;
    cell_shifts(r, &shift, &eshift);
    return std::max(r->brick_edge[0], std::max(r->brick_edge[1], r->brick_edge[2])) >= (4u << eshift);
}

// the techniques that are one launch over the cells' (min, max): maximum intensity projection, first-hit isosurface
// ... and the 2-D transfer function, which reads them the same way and no table made from the 1-D one; pre-integrated
// classification likewise (its own tables come from the 1-D one, but not through the cells)
bool minmax_technique(uint32_t t)
{
    return t == VRHIP_TECHNIQUE_MIP || t == VRHIP_TECHNIQUE_ISO || t == VRHIP_TECHNIQUE_TF2D ||
           t == VRHIP_TECHNIQUE_PREINT;
}

// Sharers of `owner` lose their (borrowed) volumes: nothing of theirs points into the owner any more.
void detach_sharers(vrhip_renderer *owner)
{
    std::vector<vrhip_renderer *> list;
    list.swap(owner->sharers);
    for (vrhip_renderer *sh : list) {
        sh->vol_owner = nullptr;           // (so that clearing does not look for itself in `owner->sharers`)
        (void)vrhip_clear_volumes(sh);     // waits for the sharer's stream; borrowed slots are not freed
    }
}

} // namespace

// Technique 8's tables (PreintView): made on the host from the host's copy of the 1-D table (tff_host, kept by
// vrhip_set_transfer_function) when a technique-8 frame first needs them after that call (tf_changed makes them
// stale).  Touches nothing else.  The stream is waited for only because a frame in flight may still read the old ones.
int ensure_preint(vrhip_renderer *r)
{
    if (r->preint_valid && r->preint_prefix && r->preint_nz) return VRHIP_OK;
    const uint32_t n = r->tff_n;
    std::vector<double> prefix(4 * (size_t)n);
    std::vector<uint32_t> nz(n + 1);
    VR_REQUIRE(r, r->tff_host.size() == 4 * (size_t)n &&
                      vrhip_preint_tables(r->tff_host.data(), n, prefix.data(), nz.data()) == VRHIP_OK, VRHIP_ERR_INVALID,
               "pre-integrated classification: the transfer function could not be integrated.");
    VR_HIP(r, hipStreamSynchronize(r->stream));
    int rc = grow(r, r->preint_prefix, prefix.size() * sizeof(double));
    if (!rc) rc = grow(r, r->preint_nz, nz.size() * sizeof(uint32_t));
    if (rc) return rc;
    VR_HIP(r, hipMemcpy(r->preint_prefix, prefix.data(), prefix.size() * sizeof(double), hipMemcpyHostToDevice));
    VR_HIP(r, hipMemcpy(r->preint_nz, nz.data(), nz.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    preint_built(r);
    return VRHIP_OK;
}

// (declared in vr_renderer.h: vrhip_depth_api.hip asks the same questions)
// Technique 2 steps over samples that cannot raise the running maximum when object-order ESS is on, technique 4
// over march samples that cannot reach isoValue (VRHIP_NO_EMPTY_SKIP=1 disables this like the ray caster's empty runs).
bool mip_skips(const vrhip_renderer *r) { return r->use_ess && r->skip_empty; }

// The (min, max) pairs of a cell grid of the current time step as ensure_cells left them: the renderer's own, or
// -- for a renderer that shares another one's voxels -- the owner's.  nullptr: not built.
const float2 *cell_minmax_of(const vrhip_renderer *r, bool fine)
{
    const VolumeSlot &s = r->vols[r->timestep];
    const float2 *src = fine ? (s.fine_minmax_valid ? s.fine_minmax.p : nullptr) : (s.pt_minmax_valid ? s.pt_minmax.p : nullptr);
    if (!src && r->vol_owner && r->timestep < r->vol_owner->vols.size()) {
        const VolumeSlot &os = r->vol_owner->vols[r->timestep];
        src = fine ? (os.fine_minmax_valid ? os.fine_minmax.p : nullptr) : (os.pt_minmax_valid ? os.pt_minmax.p : nullptr);
    }
    return src;
}

// (re)allocate a slot for `timestep`, checking that res/format agree with other timesteps
int prepare_slot(vrhip_renderer *r, const uint32_t res[3], int format, uint32_t timestep,
                 VolumeSlot **slot, int channels)
{
    VR_REQUIRE(r, res && res[0] && res[1] && res[2], VRHIP_ERR_INVALID,
               "Volume resolution must be non-zero.");
    VR_REQUIRE(r, format >= VRHIP_UCHAR && format <= VRHIP_FLOAT, VRHIP_ERR_INVALID,
               "Unknown or invalid volume data format.");   // volumerendercl.cpp:730
    VR_REQUIRE(r, res[0] <= 8192 && res[1] <= 8192 && res[2] <= 8192, VRHIP_ERR_INVALID,
               "Volume resolution above 8192 per axis is not supported.");
    bool same = r->format == format && r->res[0] == res[0] && r->res[1] == res[1] &&
                r->res[2] == res[2] && r->channels == channels;
    for (const VolumeSlot &vs : r->vols) same = same && !vs.borrowed;   // never write into shared voxels
    if (!same) {
        VR_REQUIRE(r, timestep == 0 || r->vols.empty(), VRHIP_ERR_INVALID,
                   "Volume size does not match size of the other time steps.");
        int rc = vrhip_clear_volumes(r);
        if (rc) return rc;
        std::memcpy(r->res, res, sizeof r->res);
        r->format = format;
        r->channels = channels;
        set_layout(r);
    }
    // Renderers that share these voxels hold copies of the slots' device pointers.  A slot that is
    // overwritten in place keeps its pointers: the sharers finish what they have in flight and drop
    // everything they derived from the old voxels.  A new time step would outgrow their slot lists, so
    // they are detached (they report "No volume data is loaded." until they share again).
    if (!r->sharers.empty()) {
        if (r->vols.size() <= timestep || !r->vols[timestep].dev) detach_sharers(r);
        for (vrhip_renderer *sh : r->sharers) VR_HIP(r, hipStreamSynchronize(sh->stream));
    }
    if (r->vols.size() <= timestep) r->vols.resize(timestep + 1);
    VolumeSlot &s = r->vols[timestep];
    int rc = grow(r, s.dev, volume_alloc_bytes(r));
    for (int c = 1; c < channels && !rc; ++c) rc = grow(r, s.chan[c - 1], volume_alloc_bytes(r));
    if (rc) return rc;
    voxels_written(r, timestep);
    *slot = &s;
    return VRHIP_OK;
}

namespace {

int ensure_fb(vrhip_renderer *r, uint32_t w, uint32_t h)
{
    if (r->fb && r->fb_w == w && r->fb_h == h) return VRHIP_OK;
    // a frame of another size starts from zeroes: the frame buffer accumulates, the cost map holds sort keys
    r->fb_w = r->fb_h = 0;
    int rc = grow(r, r->fb, (size_t)w * h * sizeof(float4), kGrowFresh);
    if (rc) return rc;
    VR_HIP(r, hipMemsetAsync(r->fb, 0, (size_t)w * h * sizeof(float4), r->stream));
    if ((rc = grow(r, r->cost, (size_t)w * h * sizeof(uint16_t), kGrowFresh))) return rc;
    VR_HIP(r, hipMemsetAsync(r->cost, 0, (size_t)w * h * sizeof(uint16_t), r->stream));
    r->fb_w = w;
    r->fb_h = h;
    return VRHIP_OK;
}

int check_renderable(vrhip_renderer *r, uint32_t width, uint32_t height)
{
    VR_REQUIRE(r, width > 0 && height > 0 && width <= 16384 && height <= 16384,
               VRHIP_ERR_INVALID, "Invalid output image size.");
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev,
               VRHIP_ERR_NODATA, "No volume data is loaded.");
    // (technique 6 neither reads nor requires the 1-D table: its own is asked for below)
    VR_REQUIRE(r, (r->tff && r->tff_n) || r->render.technique == VRHIP_TECHNIQUE_TF2D, VRHIP_ERR_NODATA,
               "No transfer function set.");
    if (r->use_ess && r->render.technique == 0) {
        VR_REQUIRE(r, r->bricks_valid && r->vols[r->timestep].bricks, VRHIP_ERR_NODATA,
                   "ESS bricks not built: call vrhip_build_bricks after the volume upload.");
        VR_REQUIRE(r, r->prefix && r->prefix_n, VRHIP_ERR_NODATA,
                   "No transfer function prefix sum set.");
    }
    VR_REQUIRE(r, r->render.technique <= VRHIP_TECHNIQUE_MIP || r->render.technique == VRHIP_TECHNIQUE_ISO ||
                      r->render.technique == VRHIP_TECHNIQUE_TF2D || r->render.technique == VRHIP_TECHNIQUE_PREINT,
               VRHIP_ERR_INVALID, "Unknown rendering technique.");   // (3, 5 and 7 are unassigned)
    // the path-tracing branch of the kernel returns before illumType is looked at (:686-706); technique 2 ignores it
    VR_REQUIRE(r, r->render.illumType <= 5 || r->render.technique != 0, VRHIP_ERR_INVALID,
               "Unknown illumination type.");
    VR_REQUIRE(r, r->render.technique != 1 || r->pathtrace.max_extinction > 0.f, VRHIP_ERR_INVALID,
               "max_extinction must be positive.");
    if (r->render.technique == VRHIP_TECHNIQUE_MIP) {   // what the maximum intensity projection does not define
        const vrhip_rendering_params &rp = r->render;
        VR_REQUIRE(r, !rp.imgEss && !rp.showEss, VRHIP_ERR_UNSUPPORTED,
                   "maximum intensity projection: image-order ESS and showEss are not supported.");
        VR_REQUIRE(r, !r->raycast.useAO, VRHIP_ERR_UNSUPPORTED,
                   "maximum intensity projection: ambient occlusion is not supported.");
        VR_REQUIRE(r, rp.iteration == 0, VRHIP_ERR_UNSUPPORTED,
                   "maximum intensity projection: frames do not accumulate (iteration must be 0).");
        VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED,
                   "maximum intensity projection: RG / RGBA volumes are not supported.");
        VR_REQUIRE(r, !r->env, VRHIP_ERR_UNSUPPORTED,
                   "maximum intensity projection: environment maps are not supported.");
    }
    if (r->render.technique == VRHIP_TECHNIQUE_ISO) {   // what the first-hit isosurface does not define
        const vrhip_rendering_params &rp = r->render;
        VR_REQUIRE(r, std::isfinite(r->iso.isoValue), VRHIP_ERR_INVALID, "isosurface: isoValue must be finite.");
        VR_REQUIRE(r, r->iso.refineSteps <= 16u, VRHIP_ERR_INVALID, "isosurface: refineSteps must be at most 16.");
        VR_REQUIRE(r, rp.illumType <= 1, VRHIP_ERR_UNSUPPORTED,
                   "isosurface: illumType 0 (flat) and 1 (central differences) only.");
        VR_REQUIRE(r, !rp.imgEss && !rp.showEss, VRHIP_ERR_UNSUPPORTED,
                   "isosurface: image-order ESS and showEss are not supported.");
        VR_REQUIRE(r, !r->raycast.useAO, VRHIP_ERR_UNSUPPORTED, "isosurface: ambient occlusion is not supported.");
        VR_REQUIRE(r, rp.iteration == 0, VRHIP_ERR_UNSUPPORTED,
                   "isosurface: frames do not accumulate (iteration must be 0).");
        VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "isosurface: RG / RGBA volumes are not supported.");
        VR_REQUIRE(r, !r->env, VRHIP_ERR_UNSUPPORTED, "isosurface: environment maps are not supported.");
    }
    if (r->render.technique == VRHIP_TECHNIQUE_TF2D) {   // what the 2-D transfer function does not define
        const vrhip_rendering_params &rp = r->render;
        VR_REQUIRE(r, r->tf2d && r->tf2d_nz && r->tf2d_nv && r->tf2d_ng, VRHIP_ERR_NODATA, "No 2-D transfer function set.");
        VR_REQUIRE(r, rp.illumType <= 1, VRHIP_ERR_UNSUPPORTED,
                   "2-D transfer function: illumType 0 (flat) and 1 (central differences) only.");
        VR_REQUIRE(r, !rp.imgEss && !rp.showEss, VRHIP_ERR_UNSUPPORTED,
                   "2-D transfer function: image-order ESS and showEss are not supported.");
        VR_REQUIRE(r, !r->raycast.useAO, VRHIP_ERR_UNSUPPORTED, "2-D transfer function: ambient occlusion is not supported.");
        VR_REQUIRE(r, rp.iteration == 0, VRHIP_ERR_UNSUPPORTED,
                   "2-D transfer function: frames do not accumulate (iteration must be 0).");
        VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "2-D transfer function: RG / RGBA volumes are not supported.");
        VR_REQUIRE(r, !r->env, VRHIP_ERR_UNSUPPORTED, "2-D transfer function: environment maps are not supported.");
    }
    if (r->render.technique == VRHIP_TECHNIQUE_PREINT) {   // what pre-integrated classification does not define
        const vrhip_rendering_params &rp = r->render;
        VR_REQUIRE(r, rp.illumType <= 1, VRHIP_ERR_UNSUPPORTED,
                   "pre-integrated classification: illumType 0 (flat) and 1 (central differences) only.");
        VR_REQUIRE(r, !rp.imgEss && !rp.showEss, VRHIP_ERR_UNSUPPORTED,
                   "pre-integrated classification: image-order ESS and showEss are not supported.");
        VR_REQUIRE(r, !r->raycast.useAO, VRHIP_ERR_UNSUPPORTED,
                   "pre-integrated classification: ambient occlusion is not supported.");
        VR_REQUIRE(r, rp.iteration == 0, VRHIP_ERR_UNSUPPORTED,
                   "pre-integrated classification: frames do not accumulate (iteration must be 0).");
        VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED,
                   "pre-integrated classification: RG / RGBA volumes are not supported.");
        VR_REQUIRE(r, !r->env, VRHIP_ERR_UNSUPPORTED, "pre-integrated classification: environment maps are not supported.");
    }
    // technique 1 and the traffic / downsampling helpers read channel 0 only, like the kernel's
    // .x readers; nothing else to check for CL_RG / CL_RGBA volumes
    // the path-tracing branch returns before the hit image is written (:686-706): its state
    // would never change
    VR_REQUIRE(r, !(r->render.imgEss && r->render.technique == 1), VRHIP_ERR_UNSUPPORTED,
               "image-order ESS is not supported with the path tracer.");
    return VRHIP_OK;
}

// The two hit images of image-order ESS, (W/8 + 1) x (H/8 + 1) texels, as updateOutputImg
// creates them (volumerendercl.cpp:482-488): the input image is initialised from a vector of
// 32-bit ones read as one byte per texel (bytes 1,0,0,0,1,...); the output image is left
// uninitialised there, zero here.
int ensure_hit_images(vrhip_renderer *r, uint32_t w, uint32_t h)
{
    const uint32_t hw = w / 8u + 1u, hh = h / 8u + 1u;
    if (r->hit_in && r->hit_w == hw && r->hit_h == hh) return VRHIP_OK;
    r->hit_w = r->hit_h = 0;
    const size_t n = (size_t)hw * hh;
    for (DevBuf<uint8_t> *p : {&r->hit_in, &r->hit_out, &r->hit_status, &r->hit_any}) {
        int rc = grow(r, *p, n, kGrowFresh);
        if (rc) return rc;
        VR_HIP(r, hipMemset(*p, 0, n));
    }
    std::vector<uint8_t> init(n, 0);
    for (size_t i = 0; i < n; i += 4) init[i] = 1;
    VR_HIP(r, hipMemcpy(r->hit_in, init.data(), n, hipMemcpyHostToDevice));
    r->hit_w = hw;
    r->hit_h = hh;
    return VRHIP_OK;
}

// Footprint volume of the current time step (VolView::fp, DESIGN.md "Footprint volume"): 8x the
// volume's bytes, so that a trilinear fetch is one load and none of the micro-brick address
// arithmetic.  The march is bound by VALU issue, so the instructions saved are frame time: -12 % at
// 2048^3 UCHAR in throughput mode (69 GB; 0.297 -> 0.261 ms), -4 % one frame at a time, -7 % on the
// dense "haze" volume (round 2; round 1 had measured +-0 one frame at a time and capped it at 33 GB).
// 288 GB of HBM are what this is for: the cap is 96 GB, one copy per GPU (renderers that share an
// owner's voxels read the owner's).  Built on first use, kept until the volume or the time step
// changes.
int ensure_footprint(vrhip_renderer *r)
{
    r->fp_active = false;
    const vrhip_rendering_params &rp = r->render;
    if (!r->use_fp || r->channels > 1 || r->stats_enabled || rp.technique != 0 || rp.illumType >= 2 ||
        r->raycast.useAO || rp.showEss || rp.imgEss)
        return VRHIP_OK;   // (the launcher uses it in the default kernels only)
    const VolView v = make_vol_view(r, r->vols[r->timestep].dev);
    const size_t bytes = (size_t)v.fp_nbx * v.fp_nby * ((size_t)(r->res[2] + 4u) >> 2) * 64u * 8u *
                         fmt_bytes(r->format);
    if (bytes > r->fp_max_bytes) return VRHIP_OK;
    // a renderer that shares an owner's voxels reads the owner's footprint volume of the same time step
    // (69 GB at 2048^3: one copy per GPU, not one per frame in flight); the owner builds it with its
    // first frame, which in every driver here comes before the twins' frames
    if (r->vol_owner) {
        const vrhip_renderer *o = r->vol_owner;
        if (o->fp && o->fp_valid && o->fp_timestep == r->timestep) {
            r->fp_use = o->fp;
            r->fp_active = true;
        }
        return VRHIP_OK;   // (no copy of its own: the plain layout until the owner has one)
    }
    if (!r->fp_valid || r->fp_timestep != r->timestep) {
        // A time series that moves on with every frame would rebuild 8x the volume per frame (40 ms at
        // 2048^3 against 0.6 ms for the frame from the plain layout): with more than one time step the
        // footprint volume is built for a step only once three frames in a row have shown it.
        if (r->vols.size() > 1) {
            if (r->fp_candidate != r->timestep) { r->fp_candidate = r->timestep; r->fp_candidate_frames = 0; }
            if (++r->fp_candidate_frames < 3u) return VRHIP_OK;
        }
        if (bytes == r->fp_failed_bytes) return VRHIP_OK;   // this allocation failed before: plain layout
        // renderers that share this one's volumes may be reading the old one on their own streams
        if (r->fp)
            for (vrhip_renderer *sh : r->sharers) VR_HIP(r, hipStreamSynchronize(sh->stream));
        footprint_stale(r);
        const int rc = grow(r, r->fp, bytes, kGrowTolerate);
        if (rc) return rc;
        if (!r->fp) {   // not enough HBM left: plain layout
            footprint_alloc_failed(r, bytes);
            return VRHIP_OK;
        }
        VolView fv = v;
        fv.fp = r->fp;
        VR_HIP(r, vr_launch_build_footprint(fv, r->format, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));   // sharers render on other streams
        footprint_built(r);
    }
    r->fp_use = r->fp;
    r->fp_active = true;
    return VRHIP_OK;
}

// Recompute the ESS skip bitmap when bricks, TF, prefix sum or timestep changed.
int ensure_skipmap(vrhip_renderer *r)
{
    if (!r->use_ess || !r->skip_dirty) return VRHIP_OK;
    const size_t n = (size_t)r->brick_tex[0] * r->brick_tex[1] * r->brick_tex[2];
    const uint32_t words = (uint32_t)(2 * ((n + 63) / 64));
    int rc = grow(r, r->skip_bits, ((size_t)words + 1) * sizeof(uint32_t));
    if (!rc) rc = grow(r, r->near_bits, ((size_t)words + 1) * sizeof(uint32_t));
    if (!rc) rc = grow(r, r->near_scratch, 2 * n);
    if (rc) return rc;
    r->skip_words = words;
    VR_HIP(r, vr_launch_skipmap(make_brick_view(r, r->vols[r->timestep].bricks), r->format,
                                inv_max_of(r->format), make_tf_view(r), r->skip_bits, words,
                                r->stream));
    if (r->cull_radius)
        VR_HIP(r, vr_launch_skip_near(make_brick_view(r, r->vols[r->timestep].bricks), r->skip_bits, words,
                                      r->cull_radius, r->near_scratch, r->near_bits, r->stream));
    skipmap_built(r);
    return VRHIP_OK;
}

// The (min, max) of one cell grid of the current time step (geometry: g.cx.., g.shift), built with the
// separable streaming kernels where they apply.
static int build_cell_minmax(vrhip_renderer *r, VolumeSlot &s, const CellView &g, float2 *out)
{
    // scratch for the separable build (one (min, max) per cell column and voxel slice), held only
    // while it runs
    DevBuf<> records;   // (without it -- the allocation may fail -- the kernels that need none)
    const size_t n_rec = (size_t)g.cx * g.cy * r->res[2];
    if (g.shift <= 4 && r->nb[0] <= 1600u && !getenv("VRHIP_CELLS_PER_WAVE") &&
        hipMalloc((void **)&records.p, n_rec * vr_cell_record_bytes(r->format)) != hipSuccess) {
        (void)hipGetLastError();
        records.p = nullptr;
    }
    hipError_t e = vr_launch_cell_minmax(make_vol_view(r, s.dev), r->format, g, out, r->stream, records);
    if (records && e == hipSuccess) e = hipStreamSynchronize(r->stream);
    VR_HIP(r, e);
    return VRHIP_OK;
}

} // namespace

// (Re)build what the coming frame needs of the cell grids when the volume, the timestep or the TF
// changed: the opacity bounds (path tracer; cells of 2^shift voxels, at most 256 per axis: shift 3
// up to 2048^3) and / or the empty bits (ray caster; cells of 2^eshift voxels, at most 512 per axis:
// shift 2 up to 2048^3, 16 MiB of bits).
int ensure_cells(vrhip_renderer *r, bool need_bound, bool need_empty, bool tables)
{
    if ((!need_bound || r->cells_have_bound) && (!need_empty || r->cells_have_empty)) return VRHIP_OK;
    VolumeSlot &s = r->vols[r->timestep];
    int shift, eshift;
    cell_shifts(r, &shift, &eshift);
    CellView g = r->cells;
    g.shift = shift;
    g.cx = (int)((r->res[0] + (1u << shift) - 1) >> shift);
    g.cy = (int)((r->res[1] + (1u << shift) - 1) >> shift);
    g.cz = (int)((r->res[2] + (1u << shift) - 1) >> shift);
    g.eshift = eshift;
    g.ecx = (int)((r->res[0] + (1u << eshift) - 1) >> eshift);
    g.ecy = (int)((r->res[1] + (1u << eshift) - 1) >> eshift);
    g.ecz = (int)((r->res[2] + (1u << eshift) - 1) >> eshift);
    const size_t n_cells = (size_t)g.cx * g.cy * g.cz, n_fine = (size_t)g.ecx * g.ecy * g.ecz;
    CellView fine = g;   // the fine grid's geometry for the kernels that take one grid
    fine.shift = eshift; fine.cx = g.ecx; fine.cy = g.ecy; fine.cz = g.ecz;
    int rc = grow(r, r->cell_sparse, 13 * 4096 * sizeof(float));
    if (rc) return rc;

    // ---- (min, max) per cell: a property of the voxels, kept per time step.  A renderer that shares
    // another one's voxels (vrhip_share_volumes) reads the owner's tables where the owner has built them.
    const bool one_grid = eshift == shift;
    const float2 *fine_mm = nullptr, *coarse_mm = nullptr;
    if (r->vol_owner && r->timestep < r->vol_owner->vols.size()) {
        const VolumeSlot &os = r->vol_owner->vols[r->timestep];
        if (os.dev == s.dev) {
            bool use = false;
            if (os.fine_minmax_valid && !s.fine_minmax_valid) { fine_mm = os.fine_minmax; use = true; }
            if (os.pt_minmax_valid && !s.pt_minmax_valid) { coarse_mm = os.pt_minmax; use = true; }
            // (what the owner's stream has written must be complete before this renderer's stream reads it)
            if (use && r->vol_owner->stream != r->stream) VR_HIP(r, hipStreamSynchronize(r->vol_owner->stream));
        }
    }
    if (need_empty && !one_grid && !s.fine_minmax_valid && !fine_mm) {
        if ((rc = grow(r, s.fine_minmax, n_fine * sizeof(float2)))) return rc;
        if ((rc = build_cell_minmax(r, s, fine, s.fine_minmax))) return rc;
        cell_minmax_built(s, true);
    }
    if (s.fine_minmax_valid) fine_mm = s.fine_minmax;
    if ((need_bound || one_grid) && !s.pt_minmax_valid && !coarse_mm) {
        if ((rc = grow(r, s.pt_minmax, n_cells * sizeof(float2)))) return rc;
        if (fine_mm && !one_grid) {
            VR_HIP(r, vr_launch_cell_reduce(fine_mm, g, s.pt_minmax, r->stream));
        } else if ((rc = build_cell_minmax(r, s, g, s.pt_minmax))) {
            return rc;
        }
        cell_minmax_built(s, false);
    }
    if (s.pt_minmax_valid) coarse_mm = s.pt_minmax;

    // ---- with the transfer function: bounds, empty bits (tables = false: a caller that reads the (min, max) alone and
    // may have no transfer function -- vrhip_render_depth; the tables stay stale and the next caller builds them)
    // (With tables = false nothing sets cells_have_empty, so the early return above does not hold for the next such
    // call either: it walks through here again, down to `r->cells = g`.  That is host arithmetic and grow() calls that
    // find their buffers large enough -- the (min, max) pairs are cached per slot and are not rebuilt.)
    // (the macro cells' bounds -- CellView::cbound -- sit behind the cells' in the same allocation)
    g.ccx = (g.cx + (1 << kLeapShift) - 1) >> kLeapShift;
    g.ccy = (g.cy + (1 << kLeapShift) - 1) >> kLeapShift;
    g.ccz = (g.cz + (1 << kLeapShift) - 1) >> kLeapShift;
    const size_t n_macro = (size_t)g.ccx * g.ccy * g.ccz;
    if (tables && need_bound && !r->cells_have_bound) {
        if ((rc = grow(r, r->cell_bound, (n_cells + n_macro) * sizeof(float)))) return rc;
        VR_HIP(r, vr_launch_cell_bounds(coarse_mm, g, inv_max_of(r->format), make_tf_view(r),
                                        r->cell_sparse, r->cell_bound, nullptr, r->stream));
        g.bound = r->cell_bound;
        VR_HIP(r, vr_launch_cell_coarse_bounds(g, r->cell_bound + n_cells, r->stream));
        // how far the macro cells around one are free too (CellView::cdist)
        if ((rc = grow(r, r->cell_dist, 2 * (size_t)kLeapLevels * n_macro))) return rc;
        VR_HIP(r, vr_launch_cell_leap_radius(g, r->cell_bound + n_cells, r->cell_dist, &r->cell_dist_table, r->stream));
        cells_tables_built(r, true, false);
    }
    g.bound = r->cells_have_bound ? r->cell_bound : nullptr;
    g.cbound = (r->cells_have_bound && r->pt_leap) ? r->cell_bound + n_cells : nullptr;
    g.cdist = (g.cbound && r->pt_leap_far) ? r->cell_dist_table : nullptr;
    if (tables && need_empty && !r->cells_have_empty) {
        if ((rc = grow(r, r->cell_empty, ((n_fine + 63) / 64) * 2 * sizeof(uint32_t)))) return rc;
        VR_HIP(r, vr_launch_cell_bounds(one_grid ? coarse_mm : fine_mm, fine, inv_max_of(r->format),
                                        make_tf_view(r), r->cell_sparse, nullptr, r->cell_empty, r->stream));
        cells_tables_built(r, false, true);
        g.empty = r->cell_empty;
    }
    if (!r->cells_have_empty) g.empty = nullptr;
    r->cells = g;
    return VRHIP_OK;
}

namespace {

// Build (or reuse) the centre-first queue of 8x8 wave tiles.  tile_ids == nullptr: the whole
// frame, `out` in frame layout; else the listed tiles, `out` compact [n][tile_h][tile_w].
int ensure_queue(vrhip_renderer *r, uint32_t W, uint32_t H, uint32_t tile_w, uint32_t tile_h,
                 const uint32_t *tile_ids, uint32_t n_tiles, uint32_t n_frames = 1,
                 uint32_t frame_stride = 0)
{
    std::vector<uint32_t> key = {W, H, tile_w, tile_h, tile_ids ? 1u : 0u, n_frames, frame_stride};
    if (tile_ids) key.insert(key.end(), tile_ids, tile_ids + n_tiles);
    if (key == r->queue_key && r->queue_dev) return VRHIP_OK;

    struct Item { float d2; WaveTile wt; };
    std::vector<Item> items;
    const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
    auto push = [&](uint32_t px0, uint32_t py0, uint32_t out_base) {
        if (px0 >= W || py0 >= H) return;
        Item it;
        float dx = (float)px0 + 4.f - cx, dy = (float)py0 + 4.f - cy;
        it.d2 = dx * dx + dy * dy;
        it.wt.tx8 = (uint16_t)(px0 / 8);
        it.wt.ty8 = (uint16_t)(py0 / 8);
        it.wt.out_base = out_base;
        items.push_back(it);
    };
    if (!tile_ids) {
        for (uint32_t y = 0; y < H; y += 8)
            for (uint32_t x = 0; x < W; x += 8) push(x, y, y * W + x);
    } else {
        const uint32_t tiles_x = (W + tile_w - 1) / tile_w;
        for (uint32_t k = 0; k < n_tiles; ++k) {
            const uint32_t tx = tile_ids[k] % tiles_x, ty = tile_ids[k] / tiles_x;
            for (uint32_t y = 0; y < tile_h; y += 8)
                for (uint32_t x = 0; x < tile_w; x += 8)
                    push(tx * tile_w + x, ty * tile_h + y, (k * tile_h + y) * tile_w + x);
        }
    }
    std::stable_sort(items.begin(), items.end(),
                     [](const Item &a, const Item &b) { return a.d2 < b.d2; });
    // a batch of frames: every patch once per frame (frame index in the upper bits of ty8 / tx8), the
    // frames' outputs one after the other
    const uint32_t frame_pixels = frame_stride ? frame_stride : (tile_ids ? n_tiles * tile_w * tile_h : W * H);
    std::vector<WaveTile> q(items.size() * n_frames);
    for (size_t i = 0; i < items.size(); ++i)
        for (uint32_t f = 0; f < n_frames; ++f) {
            WaveTile wt = items[i].wt;
            wt_set_frame(wt, f);
            wt.out_base += f * frame_pixels;
            q[i * n_frames + f] = wt;
        }

    VR_HIP(r, hipStreamSynchronize(r->stream));
    int rc = grow(r, r->live, q.size() * sizeof(LiveTile));
    if (!rc) rc = grow(r, r->queue_dev, q.size() * sizeof(WaveTile));
    if (rc) return rc;
    if (!q.empty())
        VR_HIP(r, hipMemcpy(r->queue_dev, q.data(), q.size() * sizeof(WaveTile),
                            hipMemcpyHostToDevice));
    r->queue_n = (uint32_t)q.size();
    r->queue_key.swap(key);
    r->queue_frames = n_frames;
    ++r->queue_version;
    // continuation buffer of the two-phase march: worst case every ray is suspended
    const size_t need = q.size() * 64;
    rc = grow(r, r->cont, need * sizeof(ContRec));
    if (!rc) rc = grow(r, r->order, need * sizeof(uint32_t));
    if (!rc) rc = grow(r, r->live_rays, (size_t)kLiveLists * live_list_cap((uint32_t)q.size()) * sizeof(ContRec));
    return rc;
}

void fill_launch(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t out_stride,
                 RaycastLaunch *a)
{
    std::memset(a, 0, sizeof *a);
    const VolumeSlot &s = r->vols[r->timestep];
    a->vol = make_render_view(r, s);
    a->bricks = make_brick_view(r, s.bricks);
    a->tf = make_tf_view(r);
    a->skip.bits = r->skip_bits;
    a->skip.n_words = r->skip_words;
    a->skip.in_lds = ((size_t)r->skip_words + 1) * sizeof(uint32_t) <= kSkipLdsMaxBytes ? 1u : 0u;
    if (getenv("VRHIP_SKIP_GLOBAL")) a->skip.in_lds = 0;   // experiments: bitmap from L2/HBM
    a->skip.near_bits = r->cull_radius ? r->near_bits : nullptr;
    a->skip.near_r = r->cull_radius;
    set_frame_geometry(&a->frame, width, height);
    a->frame.queue = r->queue_dev;
    a->frame.n_wave_tiles = r->queue_n;
    a->frame.out_stride = out_stride;
    uint32_t *const ctrl = r->queue_head + (size_t)r->ctrl_sel * kControlWords;
    a->frame.queue_head = ctrl;
    a->frame.next_ctrl = r->queue_head + (size_t)(r->ctrl_sel ^ 1u) * kControlWords;
    a->frame.patch_class = nullptr;   // (launch_timed: ensure_patch_classes)
    a->frame.set_frames = 1;
    a->frame.cont = r->cont;
    a->frame.cont_count = ctrl + 1;
    a->frame.cont_head = ctrl + 2;
    a->frame.round_budget = r->cont ? r->round_budget : 0;
    a->frame.refill_min = r->refill_min;
    a->frame.live = r->prepass ? r->live : nullptr;
    a->frame.live_rays = (r->prepass && r->ray_list) ? r->live_rays : nullptr;
    a->frame.live_count = ctrl + 3;
    a->frame.live_list_count = ctrl + kLiveBase;
    a->frame.draw_count = ctrl + kDrawBase;
    a->frame.cost = r->sort_cont ? r->cost : nullptr;
    a->frame.order = r->sort_cont && r->cost ? r->order : nullptr;
    a->frame.sort_ws = ctrl + 4;
    a->frame.fb = r->fb;
    if (r->render.imgEss && r->render.technique == 0) {
        a->frame.hit_in = r->hit_in;
        a->frame.hit_status = r->hit_status;
        a->frame.hit_any = r->hit_any;
        a->frame.hit_w = r->hit_w;
        a->frame.hit_h = r->hit_h;
    }
    a->frame.env = r->env;
    a->frame.env_w = r->env_w;
    a->frame.env_h = r->env_h;
    // showEss needs the position of every ray's last sample: it is kept in registers, not in the
    // continuation records, so the march runs in a single phase
    if (r->render.showEss) a->frame.round_budget = 0;
    a->cam = r->cam;
    a->render = r->render;
    a->raycast = r->raycast;
    a->pathtrace = r->pathtrace;
    a->iso = r->iso;
    a->cells = r->cells;
    if (!r->pt_cull) { a->cells.bound = a->cells.cbound = nullptr; a->cells.cdist = nullptr; }
    // the empty bits are those of TF(channel 0): not what a CL_RG / CL_RGBA sample's opacity is
    if (!ray_skip_empty(r)) a->cells.empty = nullptr;
    if (minmax_technique(r->render.technique)) {
        // (the kernel reads no table made from the transfer function: only the cells' (min, max) and their geometry)
        a->cells.bound = a->cells.cbound = nullptr;
        a->cells.cdist = nullptr;
        a->cells.empty = nullptr;
        if (mip_skips(r)) {
            a->cell_minmax_fine = r->cells.eshift != r->cells.shift;
            a->cell_minmax = cell_minmax_of(r, a->cell_minmax_fine != 0);
        }
    }
    if (r->render.technique == VRHIP_TECHNIQUE_TF2D) a->tf2d = make_tf2d_view(r);
    if (r->render.technique == VRHIP_TECHNIQUE_PREINT) a->preint = make_preint_view(r);
    a->format = r->format;
    a->use_ess = r->use_ess ? 1 : 0;
    a->instr = r->stats_enabled ? 1 : 0;
    // Three waves per SIMD -- one workgroup of 12 waves per CU that share one transfer function and one skip bitmap
    // in LDS, 168 VGPRs per lane (vr_raycast_kernels.h kWavesWide) -- where waves wait more than they issue:
    //  * volumes whose ESS bricks are too small for the empty-run lookahead (ray_skip_empty): the march waits for its
    //    fetches instead of stepping over empty cells (256^3: -12 % per frame, -6 % one frame at a time);
    //  * launch sets of several frames (the throughput schedule, a rank's tile share): enough rays for a third wave
    //    per SIMD, and no chain of one frame's longest rays that a third wave would stretch (2048^3, 16 frames per
    //    set and two renderers: "shells" -6 %, "haze" -8 %, 1024^3 USHORT -8 %; both phases -- one of them alone
    //    gains half of it or nothing).
    // One frame at a time with the lookahead: two waves ("shells" +10 % with three, the longest rays' chain).
    // VRHIP_OCC=2|3 forces both phases, VRHIP_OCC_P1 / VRHIP_OCC_P2 one of them (tools/ab_env.sh).
    const bool three = r->use_ess && (!ray_skip_empty(r) || r->queue_frames >= 4u);
    a->occ3 = r->occ_force ? (r->occ_force == 3) : three;
    a->occ3_split = r->occ_force_split ? (r->occ_force_split == 3) : three;
    a->stats = r->stats_dev;
    a->num_cus = r->num_cus;
}

// FrameView::patch_class for this launch (vr_patch_class_kernel), recomputed only when something it depends on
// has changed: camera, rendering / ray-cast parameters (the jitter seed does not count), frame geometry and
// work queue, skip bitmaps.  A static camera pays it once.
int ensure_patch_classes(vrhip_renderer *r, RaycastLaunch *a)
{
    a->frame.patch_class = nullptr;
    a->frame.set_frames = r->queue_frames;
    const vrhip_rendering_params &rp = a->render;
    // (a batch of per-frame views runs without: classes hold for one camera -- DESIGN.md "Per-frame cameras")
    if (!r->use_patch_classes || a->frame.cams || rp.technique != 0 || !a->use_ess || a->instr != 0 || !a->frame.live || !a->skip.near_bits ||
        rp.useGradient || a->frame.env || rp.showEss || rp.imgEss || rp.iteration != 0)
        return VRHIP_OK;
    const uint32_t n_patches = r->queue_n / r->queue_frames;
    std::vector<uint8_t> key;
    auto put = [&key](const void *p, size_t n) { key.insert(key.end(), (const uint8_t *)p, (const uint8_t *)p + n); };
    vrhip_rendering_params rk = rp;
    rk.seed = 0;   // (frames of one camera differ in the seed only; iteration is 0 here)
    put(&a->cam, sizeof a->cam);
    put(&rk, sizeof rk);
    put(&a->raycast, sizeof a->raycast);
    const uint32_t misc[10] = {a->frame.W, a->frame.H, a->frame.gsx, a->frame.gsy, r->queue_version, r->skip_version,
                               a->skip.near_r, n_patches, r->queue_frames, (uint32_t)a->bricks.bw};
    put(misc, sizeof misc);
    if (key != r->patch_class_key) {
        const int rc = grow(r, r->patch_class, n_patches);
        if (rc) return rc;
        r->patch_class_key.clear();
        VR_HIP(r, vr_launch_patch_classes(*a, n_patches, r->queue_frames, r->patch_class, r->stream));
        r->patch_class_key.swap(key);
        if (getenv("VRHIP_DEBUG")) {   // how many patches skip their ray set-up
            std::vector<uint8_t> h(n_patches);
            VR_HIP(r, hipMemcpyAsync(h.data(), r->patch_class, n_patches, hipMemcpyDeviceToHost, r->stream));
            VR_HIP(r, hipStreamSynchronize(r->stream));
            size_t n1 = 0;
            for (uint8_t v : h) n1 += v;
            fprintf(stderr, "[vrhip] patch classes: %zu of %u patches are background for every jitter\n", n1, n_patches);
        }
    }
    a->frame.patch_class = r->patch_class;
    return VRHIP_OK;
}

int launch_timed(vrhip_renderer *r, const RaycastLaunch &a)
{
    if (a.instr && !a.keep_stats) VR_HIP(r, hipMemsetAsync(r->stats_dev, 0, sizeof(DevStats), r->stream));
    // control words: the block of this set was zeroed by the first kernel of the previous set (memset
    // only for the first set, or after something else has used the block)
    if (!r->ctrl_clean[r->ctrl_sel])
        VR_HIP(r, hipMemsetAsync(a.frame.queue_head, 0, kControlWords * sizeof(uint32_t), r->stream));
    r->ctrl_clean[r->ctrl_sel] = false;
    RaycastLaunch b = a;
    {
        const int rc = ensure_patch_classes(r, &b);   // (before the frame's timing starts: once per camera)
        if (rc) return rc;
    }
    // The frame's events are bound to its launches (hipExtLaunchKernelGGL: the first launch's start, phase 1's end, the
    // last launch's end) -- a RECORDED event is a marker packet of its own between two launches, ~6 us of GPU time
    // each; VRHIP_EVENT_BIND=0 records them (A/B), =1 binds the ends only.  What the launchers did not bind -- no
    // launch at all -- is recorded here.
    bool start_bound = false, stop_bound = false;
    b.bind_events = r->event_bind;
    if (r->frame_timing) {
        b.stop_event = r->ev1;
        b.stop_bound = &stop_bound;
        if (r->event_bind >= 2) {
            b.start_event = r->ev0;
            b.start_bound = &start_bound;
        } else {
            VR_HIP(r, hipEventRecord(r->ev0, r->stream));
            start_bound = true;
        }
    }
    b.mid_event = r->phase_timing && r->frame_timing ? r->evm : nullptr;
    r->phase_timed = r->phase_timing && r->frame_timing;
    if (b.frame.hit_in) {
        VR_HIP(r, hipMemsetAsync(r->hit_any, 0, (size_t)r->hit_w * r->hit_h, r->stream));
        b.hit_out = r->hit_out;
    }
    std::memset(&r->last_info, 0, sizeof r->last_info);
    r->last_info.frames = b.frame.seeds ? r->queue_frames : 1u;
    r->last_info.views = b.frame.cams ? 1u : 0u;
    b.info = &r->last_info;
    r->have_info = false;
    VR_HIP(r, vr_launch_frame(b, r->stream));
    r->have_info = true;
    // the first kernel of this set has zeroed the other block (VR_ZERO_NEXT_CTRL) -- unless the set was empty and
    // nothing ran: then the other block keeps whatever it held, and the next set clears it with a memset
    r->ctrl_sel ^= 1u;
    r->ctrl_clean[r->ctrl_sel] = b.frame.n_wave_tiles != 0;
    if (r->frame_timing && !start_bound) VR_HIP(r, hipEventRecord(r->ev0, r->stream));
    if (r->frame_timing && !stop_bound) VR_HIP(r, hipEventRecord(r->ev1, r->stream));
    r->timed = r->frame_timing;
    if (b.frame.hit_in) std::swap(r->hit_in, r->hit_out);   // runRaycast, volumerendercl.cpp:524-530
    return VRHIP_OK;
}

int prepare_render(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                   uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles, uint32_t n_frames = 1,
                   uint32_t frame_stride = 0)
{
    r->pm_last = false;   // (whatever renders next rebuilds or reuses the queue, the ray lists and a control block)
    int rc = check_renderable(r, width, height);
    if (rc) return rc;
    if (tile_ids) {
        VR_REQUIRE(r, tile_w && tile_h && tile_w % 16 == 0 && tile_h % 16 == 0, VRHIP_ERR_INVALID,
                   "Tile size must be a positive multiple of 16.");
        const uint32_t nt = ((width + tile_w - 1) / tile_w) * ((height + tile_h - 1) / tile_h);
        for (uint32_t i = 0; i < n_tiles; ++i)
            VR_REQUIRE(r, tile_ids[i] < nt, VRHIP_ERR_INVALID, "Tile id out of range.");
    }
    rc = ensure_fb(r, width, height);
    if (rc) return rc;
    r->fp_active = false;
    if (r->render.imgEss) {
        rc = ensure_hit_images(r, width, height);
        if (rc) return rc;
    }
    if (r->render.technique == 0) {
        rc = ensure_skipmap(r);
        if (rc) return rc;
        rc = ensure_footprint(r);
        if (rc) return rc;
    }
    if (r->render.technique == 1 ? r->pt_cull : minmax_technique(r->render.technique) ? mip_skips(r) : ray_skip_empty(r)) {
        // (techniques 2 and 4 read the (min, max) of the grid the empty bits live on: built with them)
        // (technique 6 may have no 1-D transfer function to make the tables from: the pairs and the geometry alone)
        // (technique 8 reads none of them either: it is held to building nothing another technique reads)
        rc = ensure_cells(r, r->render.technique == 1, r->render.technique != 1,
                          r->render.technique != VRHIP_TECHNIQUE_TF2D && r->render.technique != VRHIP_TECHNIQUE_PREINT);
        if (rc) return rc;
    }
    if (r->render.technique == VRHIP_TECHNIQUE_PREINT) {
        rc = ensure_preint(r);
        if (rc) return rc;
    }
    return ensure_queue(r, width, height, tile_w, tile_h, tile_ids, n_tiles, n_frames, frame_stride);
}

int count_touched_impl(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                       uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                       uint64_t *microbricks_touched, uint8_t *bitmap_host, size_t bitmap_bytes,
                       bool fetched_only = false)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, r->render.technique != VRHIP_TECHNIQUE_MIP, VRHIP_ERR_UNSUPPORTED,
               "vrhip_count_touched / vrhip_count_fetched: not supported with maximum intensity projection.");
    VR_REQUIRE(r, r->render.technique != VRHIP_TECHNIQUE_ISO, VRHIP_ERR_UNSUPPORTED,
               "vrhip_count_touched / vrhip_count_fetched: not supported with isosurface rendering.");
    VR_REQUIRE(r, r->render.technique != VRHIP_TECHNIQUE_TF2D, VRHIP_ERR_UNSUPPORTED,
               "vrhip_count_touched / vrhip_count_fetched: not supported with the 2-D transfer function.");
    VR_REQUIRE(r, r->render.technique != VRHIP_TECHNIQUE_PREINT, VRHIP_ERR_UNSUPPORTED,
               "vrhip_count_touched / vrhip_count_fetched: not supported with pre-integrated classification.");
    int rc = prepare_render(r, width, height, tile_w, tile_h, tile_ids, n_tiles);
    if (rc) return rc;
    const size_t mb = (size_t)((r->res[0] + 3) / 4) * ((r->res[1] + 3) / 4) * ((r->res[2] + 3) / 4);
    const size_t words = (mb + 31) / 32;
    VR_REQUIRE(r, !bitmap_host || bitmap_bytes == (mb + 7) / 8, VRHIP_ERR_INVALID,
               "vrhip_count_touched: bitmap size mismatch");
    uint32_t *bits = nullptr;
    VR_HIP(r, hipMalloc((void **)&bits, words * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(bits, 0, words * sizeof(uint32_t), r->stream);
    RaycastLaunch a;
    fill_launch(r, width, height, tile_ids ? tile_w : width, &a);
    a.instr = fetched_only ? 3 : 2;
    a.touched = bits;
    // the instrumented pass must not disturb the accumulate buffer: render into a scratch
    float4 *scratch = nullptr;
    if (e == hipSuccess) e = hipMalloc((void **)&scratch, (size_t)width * height * sizeof(float4));
    if (e == hipSuccess && r->render.iteration != 0)
        e = hipMemcpyAsync(scratch, r->fb, (size_t)width * height * sizeof(float4),
                           hipMemcpyDeviceToDevice, r->stream);
    a.frame.fb = scratch;
    if (e == hipSuccess) e = hipMemsetAsync(r->stats_dev, 0, sizeof(DevStats), r->stream);
    a.frame.round_budget = 0;   // the traffic pass runs single-phase (no speculative touches)
    // image-order ESS: the pass skips what the next frame will skip, and leaves the hit images alone
    if (a.frame.hit_in && e == hipSuccess)
        e = hipMemsetAsync(r->hit_any, 0, (size_t)r->hit_w * r->hit_h, r->stream);
    a.frame.next_ctrl = nullptr;   // (this pass does not take part in the alternation of the control blocks)
    if (e == hipSuccess) e = hipMemsetAsync(a.frame.queue_head, 0, kControlWords * sizeof(uint32_t), r->stream);
    r->ctrl_clean[r->ctrl_sel] = false;
    if (e == hipSuccess) e = vr_launch_frame(a, r->stream);
    std::vector<uint32_t> host(words);
    if (e == hipSuccess)
        e = hipMemcpyAsync(host.data(), bits, words * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    (void)hipFree(bits);
    if (scratch) (void)hipFree(scratch);
    if (e != hipSuccess)
        return fail(r, VRHIP_ERR_HIP,
                    std::string("ERROR: vrhip_count_touched (") + hipGetErrorString(e) + ")");
    uint64_t cnt = 0;
    for (size_t i = 0; i < words; ++i) cnt += (uint64_t)__builtin_popcount(host[i]);
    if (microbricks_touched) *microbricks_touched = cnt;
    if (bitmap_host) std::memcpy(bitmap_host, host.data(), bitmap_bytes);
    return VRHIP_OK;
}

} // namespace

extern "C" {

int vrhip_abi_version(void) { return VRHIP_ABI_VERSION; }

int vrhip_create(int device_id, vrhip_renderer **out)
{
    if (!out) return fail(nullptr, VRHIP_ERR_INVALID, "vrhip_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, VRHIP_ERR_HIP,
                    std::string("ERROR: no HIP device available (") + hipGetErrorString(e) + ")");
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, VRHIP_ERR_INVALID, "vrhip_create: device id out of range");
    vrhip_renderer *r = new vrhip_renderer();
    r->device = device_id;
    hipDeviceProp_t prop;
    // the frame's timing events order nothing for the host (results leave by stream-ordered copies that fence for
    // themselves): no system-scope fence -- a write-back of the L2 -- when one of them completes.  VRHIP_EVENT_FENCE=1: A/B
    const unsigned ev_flags = getenv("VRHIP_EVENT_FENCE") && atoi(getenv("VRHIP_EVENT_FENCE")) ? hipEventDefault
                                                                                                 : hipEventDisableSystemFence;
    if ((e = hipSetDevice(device_id)) != hipSuccess ||
        (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&r->own_stream.h, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&r->ev0.h, ev_flags)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&r->ev1.h, ev_flags)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&r->evm.h, ev_flags)) != hipSuccess ||
        (e = hipEventCreate(&r->evb0.h)) != hipSuccess ||
        (e = hipEventCreate(&r->evb1.h)) != hipSuccess ||
        (e = hipMalloc((void **)&r->stats_dev.p, sizeof(DevStats))) != hipSuccess ||
        (e = hipMalloc((void **)&r->queue_head.p, 2 * kControlWords * sizeof(uint32_t))) != hipSuccess) {
        std::string msg = std::string("ERROR: vrhip_create (") + hipGetErrorString(e) + ")";
        delete r;   // (with whatever it holds by now)
        return fail(nullptr, VRHIP_ERR_HIP, msg);
    }
    r->stream = r->own_stream;
    // the switches of the removed experiment kernels fail loudly instead of silently rendering with the default ones
    if (getenv("VRHIP_MARCH") || getenv("VRHIP_LDS_STAGE") || getenv("VRHIP_MARCH_MICRO")) {
        vrhip_destroy(r);
        return fail(nullptr, VRHIP_ERR_UNSUPPORTED,
                    "VRHIP_MARCH / VRHIP_LDS_STAGE / VRHIP_MARCH_MICRO: the VR_EXPERIMENTS kernels were removed "
                    "(commit 858be18 holds them)");
    }
    if (const char *b = getenv("VRHIP_ROUND_BUDGET")) r->round_budget = (uint32_t)atoi(b);   // tuning
    if (getenv("VRHIP_NO_PREPASS")) r->prepass = false;        // experiments: phase 1 walks every patch
    if (getenv("VRHIP_NO_RAYLIST")) r->ray_list = false;       // experiments: phase 1 on live patches
    if (const char *e = getenv("VRHIP_CULL_RADIUS")) {
        const int v = atoi(e);
        if (v >= 0 && v <= 64) r->cull_radius = (uint32_t)v;
    }
    if (getenv("VRHIP_NO_SORT")) r->sort_cont = false;         // experiments: phase 2 in append order
    if (const char *e = getenv("VRHIP_PIXEL_MAJOR")) r->pixel_major = atoi(e) != 0;   // A/B: the ray order of launch sets
    if (const char *e = getenv("VRHIP_PM_GROUP")) {
        const int v = atoi(e);
        if (v == 1 || v == 32 || v == 64) r->pm_group = (uint32_t)v;
    }
    if (getenv("VRHIP_NO_PATCH_CLASS")) r->use_patch_classes = false;   // A/B: every patch sets up its rays
    auto occ_env = [](const char *name, int dflt) {
        const char *e = getenv(name);
        return e ? (atoi(e) == 3 ? 3 : atoi(e) == 2 ? 2 : 0) : dflt;
    };
    if (const char *e = getenv("VRHIP_FRAME_TIMING")) r->frame_timing = atoi(e) != 0;   // A/B (tools/ab_env.sh)
    if (const char *e = getenv("VRHIP_EVENT_BIND")) r->event_bind = atoi(e);
    r->occ_force = r->occ_force_split = occ_env("VRHIP_OCC", 0);
    r->occ_force = occ_env("VRHIP_OCC_P1", r->occ_force);
    r->occ_force_split = occ_env("VRHIP_OCC_P2", r->occ_force_split);
    if (getenv("VRHIP_PT_NO_CULL")) r->pt_cull = false;        // experiments: no opacity-bound culling
    if (getenv("VRHIP_PT_NO_LEAP")) r->pt_leap = false;        // A/B: every tracking step on its own
    if (getenv("VRHIP_PT_NO_FAR_LEAP")) r->pt_leap_far = false;
    if (getenv("VRHIP_NO_EMPTY_SKIP")) r->skip_empty = false;  // experiments: no empty-run skipping
    if (getenv("VRHIP_EMPTY_SKIP")) r->skip_empty_force = true;   // ... or everywhere
    if (getenv("VRHIP_NO_FOOTPRINT")) r->use_fp = false;       // plain volume layout only
    if (const char *e = getenv("VRHIP_REFILL_MIN")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 16) r->refill_min = (uint32_t)v;
    }
    if (const char *e = getenv("VRHIP_INGEST_SLAB_BYTES")) {   // tests: a small volume over many slabs
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v > 0) r->ingest_slab_bytes = (size_t)v;
    }
    if (const char *e = getenv("VRHIP_FOOTPRINT_MAX_GB")) {
        const double gb = atof(e);
        if (gb >= 0.0) r->fp_max_bytes = (size_t)(gb * 1073741824.0);   // (fp_failed_bytes starts at 0)
    }
    r->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    r->devname = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    *out = r;
    return VRHIP_OK;
}

void vrhip_destroy(vrhip_renderer *r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    vrhip_clear_volumes(r);   // detaches the sharers, leaves the owner's list
    delete r;
}

const char *vrhip_last_error(const vrhip_renderer *r)
{
    return r ? r->err.c_str() : create_error().c_str();
}

int vrhip_device_name(const vrhip_renderer *r, char *buf, size_t buf_len)
{
    if (!r || !buf || !buf_len) return VRHIP_ERR_INVALID;
    std::snprintf(buf, buf_len, "%s", r->devname.c_str());
    return VRHIP_OK;
}

int vrhip_set_stream(vrhip_renderer *r, void *hip_stream, int use_own)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    r->stream = use_own ? r->own_stream : (hipStream_t)hip_stream;
    return VRHIP_OK;
}

static int download_cells_impl(vrhip_renderer *r, bool fine, float *out_minmax, size_t n_floats, uint32_t dims[3],
                               uint32_t *shift)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev,
               VRHIP_ERR_NODATA, "No volume data is loaded.");
    VR_REQUIRE(r, r->tff && r->tff_n, VRHIP_ERR_NODATA, "No transfer function set.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    cells_tables_stale(r);   // (this call always rebuilds the table it asks for)
    // (only the grid asked for: the coarse one is then built directly unless the fine one exists already,
    // in which case it is reduced from it -- the tests take both routes)
    int rc = ensure_cells(r, !fine, fine);
    if (rc) return rc;
    const CellView &g = r->cells;
    const bool second = fine && g.eshift != g.shift;
    const int cx = second ? g.ecx : g.cx, cy = second ? g.ecy : g.cy, cz = second ? g.ecz : g.cz;
    const size_t n_cells = (size_t)cx * cy * cz;
    if (dims) { dims[0] = (uint32_t)cx; dims[1] = (uint32_t)cy; dims[2] = (uint32_t)cz; }
    if (shift) *shift = (uint32_t)(second ? g.eshift : g.shift);
    if (!out_minmax) return VRHIP_OK;
    VR_REQUIRE(r, n_floats == 2 * n_cells, VRHIP_ERR_INVALID, "vrhip_download_cells: size mismatch");
    VR_HIP(r, hipStreamSynchronize(r->stream));
    const float2 *src = cell_minmax_of(r, second);   // (its own tables, or the volumes' owner's)
    VR_REQUIRE(r, src, VRHIP_ERR_NODATA, "vrhip_download_cells: no cell grid");
    VR_HIP(r, hipMemcpy(out_minmax, src, n_cells * sizeof(float2), hipMemcpyDeviceToHost));
    return VRHIP_OK;
}

int vrhip_download_cells(vrhip_renderer *r, float *out_minmax, size_t n_floats, uint32_t dims[3],
                         uint32_t *shift)
{
    return download_cells_impl(r, false, out_minmax, n_floats, dims, shift);
}

int vrhip_download_empty_cells(vrhip_renderer *r, float *out_minmax, size_t n_floats, uint32_t dims[3],
                               uint32_t *shift)
{
    return download_cells_impl(r, true, out_minmax, n_floats, dims, shift);
}

int vrhip_download_cell_tables(vrhip_renderer *r, float *out_bound, size_t n_bound, float *out_macro, size_t n_macro,
                               uint8_t *out_leap, size_t n_leap, uint32_t *out_empty, size_t n_empty, uint32_t dims[9],
                               uint32_t shifts[2])
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev,
               VRHIP_ERR_NODATA, "No volume data is loaded.");
    VR_REQUIRE(r, r->tff && r->tff_n, VRHIP_ERR_NODATA, "No transfer function set.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    cells_tables_stale(r);   // (this call always rebuilds the tables)
    int rc = ensure_cells(r, true, true);
    if (rc) return rc;
    const CellView &g = r->cells;
    const size_t cells = (size_t)g.cx * g.cy * g.cz, macro = (size_t)g.ccx * g.ccy * g.ccz;
    const size_t words = ((size_t)g.ecx * g.ecy * g.ecz + 31) / 32;
    if (dims) {
        const int d[9] = {g.cx, g.cy, g.cz, g.ccx, g.ccy, g.ccz, g.ecx, g.ecy, g.ecz};
        for (int i = 0; i < 9; ++i) dims[i] = (uint32_t)d[i];
    }
    if (shifts) { shifts[0] = (uint32_t)g.shift; shifts[1] = (uint32_t)g.eshift; }
    if (!out_bound && !out_macro && !out_leap && !out_empty) return VRHIP_OK;
    VR_REQUIRE(r, (!out_bound || n_bound == cells) && (!out_macro || n_macro == macro) &&
                  (!out_leap || n_leap == (size_t)kLeapLevels * macro) && (!out_empty || n_empty == words),
               VRHIP_ERR_INVALID, "vrhip_download_cell_tables: size mismatch");
    VR_REQUIRE(r, r->cell_bound && r->cell_dist_table && r->cell_empty, VRHIP_ERR_NODATA,
               "vrhip_download_cell_tables: no cell tables");
    VR_HIP(r, hipStreamSynchronize(r->stream));
    if (out_bound) VR_HIP(r, hipMemcpy(out_bound, r->cell_bound, cells * sizeof(float), hipMemcpyDeviceToHost));
    if (out_macro) VR_HIP(r, hipMemcpy(out_macro, r->cell_bound + cells, macro * sizeof(float), hipMemcpyDeviceToHost));
    if (out_leap) VR_HIP(r, hipMemcpy(out_leap, r->cell_dist_table, (size_t)kLeapLevels * macro, hipMemcpyDeviceToHost));
    if (out_empty) VR_HIP(r, hipMemcpy(out_empty, r->cell_empty, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VRHIP_OK;
}

int vrhip_get_stream(const vrhip_renderer *r, void **hip_stream)
{
    if (!r || !hip_stream) return VRHIP_ERR_INVALID;
    *hip_stream = (void *)r->stream;
    return VRHIP_OK;
}

int vrhip_upload_volume(vrhip_renderer *r, const void *host_voxels, const uint32_t res[3],
                        int format, uint32_t timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, host_voxels, VRHIP_ERR_INVALID, "vrhip_upload_volume: NULL voxel pointer");
    if (set_device(r)) return VRHIP_ERR_HIP;
    VolumeSlot *s;
    int rc = prepare_slot(r, res, format, timestep, &s);
    if (rc) return rc;
    VR_HIP(r, copy_volume(r, s->dev, const_cast<void *>(host_voxels), true, false, r->stream));
    return VRHIP_OK;
}

int vrhip_upload_volume_channels(vrhip_renderer *r, const void *host_voxels, const uint32_t res[3],
                                 int format, int channels, uint32_t timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (channels == 1) return vrhip_upload_volume(r, host_voxels, res, format, timestep);
    VR_REQUIRE(r, host_voxels, VRHIP_ERR_INVALID, "vrhip_upload_volume: NULL voxel pointer");
    VR_REQUIRE(r, channels == 2 || channels == 4, VRHIP_ERR_INVALID,
               "Unknown or invalid volume color format.");   // volumerendercl.cpp:711
    if (set_device(r)) return VRHIP_ERR_HIP;
    VolumeSlot *s;
    int rc = prepare_slot(r, res, format, timestep, &s, channels);
    if (rc) return rc;
    // interleaved texels -> one planar array per channel, each re-tiled like a CL_R volume
    const size_t n = (size_t)res[0] * res[1] * res[2], bpv = fmt_bytes(format);
    std::vector<unsigned char> plane(n * bpv);
    const unsigned char *src = static_cast<const unsigned char *>(host_voxels);
    for (int c = 0; c < channels; ++c) {
        for (size_t i = 0; i < n; ++i)
            std::memcpy(&plane[i * bpv], src + (i * (size_t)channels + (size_t)c) * bpv, bpv);
        VR_HIP(r, copy_volume(r, c == 0 ? s->dev : s->chan[c - 1], plane.data(), true, false,
                              r->stream));
    }
    return VRHIP_OK;
}

int vrhip_upload_volume_device(vrhip_renderer *r, const void *dev_voxels, const uint32_t res[3],
                               int format, uint32_t timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, dev_voxels, VRHIP_ERR_INVALID, "vrhip_upload_volume_device: NULL pointer");
    if (set_device(r)) return VRHIP_ERR_HIP;
    VolumeSlot *s;
    int rc = prepare_slot(r, res, format, timestep, &s);
    if (rc) return rc;
    VR_HIP(r, copy_volume(r, s->dev, const_cast<void *>(dev_voxels), true, true, r->stream));
    return VRHIP_OK;
}

int vrhip_synth_volume(vrhip_renderer *r, int kind, const uint32_t res[3], int format,
                       uint32_t timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, kind == 0 || kind == 1, VRHIP_ERR_INVALID, "vrhip_synth_volume: kind must be 0/1");
    if (set_device(r)) return VRHIP_ERR_HIP;
    VolumeSlot *s;
    int rc = prepare_slot(r, res, format, timestep, &s);
    if (rc) return rc;
    VR_HIP(r, vr_launch_synth(kind, make_vol_view(r, s->dev), format, r->stream));
    VR_HIP(r, hipStreamSynchronize(r->stream));
    return VRHIP_OK;
}

int vrhip_download_volume(vrhip_renderer *r, uint32_t timestep, void *host_dst, size_t bytes)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, timestep < r->vols.size() && r->vols[timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, host_dst && bytes == volume_bytes(r), VRHIP_ERR_INVALID,
               "vrhip_download_volume: size mismatch");
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_HIP(r, copy_volume(r, r->vols[timestep].dev, host_dst, false, false, r->stream));
    return VRHIP_OK;
}

int vrhip_downsample_volume(vrhip_renderer *r, uint32_t timestep, int factor, void *host_dst,
                            size_t bytes, uint32_t out_res[3])
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, timestep < r->vols.size() && r->vols[timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, factor >= 2, VRHIP_ERR_INVALID, "Factor must be greater or equal 2.");
    int lo[3], vpc[3];
    for (int i = 0; i < 3; ++i) {
        lo[i] = (int)std::ceil((double)r->res[i] / (double)factor);        // volumerendercl.cpp:245-251
        vpc[i] = (int)std::ceil((float)r->res[i] / (float)lo[i]);           // volumeraycast.cl:974-975
        if (out_res) out_res[i] = (uint32_t)lo[i];
    }
    VR_REQUIRE(r, lo[0] >= 64, VRHIP_ERR_INVALID,
               "Could not create down-sampled volume data set, because the resolution would be "
               "smaller than the minimum (64x64x64).");   // :253-259
    if (!host_dst) return VRHIP_OK;
    const size_t need = (size_t)lo[0] * lo[1] * lo[2] * fmt_bytes(r->format);
    VR_REQUIRE(r, bytes == need, VRHIP_ERR_INVALID, "vrhip_downsample_volume: size mismatch");
    if (set_device(r)) return VRHIP_ERR_HIP;
    void *dev = nullptr;
    VR_HIP(r, hipMalloc(&dev, need));
    hipError_t e = vr_launch_downsample(make_vol_view(r, r->vols[timestep].dev), r->format, lo, vpc,
                                        dev, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(host_dst, dev, need, hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    (void)hipFree(dev);
    if (e != hipSuccess)
        return fail(r, VRHIP_ERR_HIP,
                    std::string("ERROR: vrhip_downsample_volume (") + hipGetErrorString(e) + ")");
    return VRHIP_OK;
}

int vrhip_clear_volumes(vrhip_renderer *r)
{
    if (!r) return VRHIP_ERR_INVALID;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    // renderers that render from these voxels (vrhip_share_volumes) stop doing so before they are freed
    detach_sharers(r);
    r->vols.clear();   // (frees what the slots own: not the voxels and bricks of a borrowed slot)
    if (r->vol_owner) {   // a sharer leaves its owner's list
        std::vector<vrhip_renderer *> &v = r->vol_owner->sharers;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
        r->vol_owner = nullptr;
    }

    volumes_cleared(r);
    r->format = -1;
    r->channels = 1;
    r->res[0] = r->res[1] = r->res[2] = 0;
    r->timestep = 0;
    return VRHIP_OK;
}

int vrhip_set_round_budget(vrhip_renderer *r, uint32_t rounds)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, rounds <= 100000u, VRHIP_ERR_INVALID, "vrhip_set_round_budget: out of range");
    r->round_budget = rounds;
    return VRHIP_OK;
}

int vrhip_share_volumes(vrhip_renderer *r, vrhip_renderer *owner)
{
    if (!r || !owner || r == owner) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, r->device == owner->device, VRHIP_ERR_INVALID,
               "vrhip_share_volumes: both renderers must live on the same device.");
    VR_REQUIRE(r, !owner->vols.empty(), VRHIP_ERR_NODATA, "No volume data is loaded.");
    for (const VolumeSlot &s : owner->vols)
        VR_REQUIRE(r, s.dev && !s.borrowed, VRHIP_ERR_INVALID,
                   "vrhip_share_volumes: the owner must hold its own, complete volumes.");
    int rc = vrhip_clear_volumes(r);
    if (rc) return rc;
    // what the owner has written must be complete before this renderer's stream reads it
    if (hipStreamSynchronize(owner->stream) != hipSuccess)
        return fail(r, VRHIP_ERR_HIP, "ERROR: vrhip_share_volumes (stream synchronize)");
    std::memcpy(r->res, owner->res, sizeof r->res);
    r->format = owner->format;
    r->channels = owner->channels;
    set_layout(r);
    for (int i = 0; i < 3; ++i) {
        r->brick_edge[i] = owner->brick_edge[i];
        r->brick_res[i] = owner->brick_res[i];
        r->brick_tex[i] = owner->brick_tex[i];
        r->raycast.brickRes[i] = owner->raycast.brickRes[i];
    }
    r->vols.resize(owner->vols.size());
    for (size_t t = 0; t < owner->vols.size(); ++t) {
        VolumeSlot &d = r->vols[t];
        const VolumeSlot &s = owner->vols[t];
        d.dev.borrow(s.dev);
        for (int c = 0; c < 3; ++c) d.chan[c].borrow(s.chan[c]);
        d.bricks.borrow(s.bricks);
        d.borrowed = true;
    }
    r->timestep = owner->timestep < r->vols.size() ? owner->timestep : 0;
    r->vol_owner = owner;
    owner->sharers.push_back(r);
    volumes_shared(r, owner);
    return VRHIP_OK;
}

int vrhip_set_timestep(vrhip_renderer *r, uint32_t timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    // volumerendercl.cpp:1169-1170: silently ignored when out of range
    if (!r->vols.empty() && timestep >= r->vols.size()) return VRHIP_OK;
    if (r->timestep != timestep) timestep_changed(r);
    r->timestep = timestep;
    return VRHIP_OK;
}

int vrhip_get_resolution(const vrhip_renderer *r, uint32_t res_xyzt[4])
{
    if (!r || !res_xyzt) return VRHIP_ERR_INVALID;
    res_xyzt[0] = r->res[0];
    res_xyzt[1] = r->res[1];
    res_xyzt[2] = r->res[2];
    res_xyzt[3] = r->vols.empty() ? 1u : (uint32_t)r->vols.size();
    return VRHIP_OK;
}

int vrhip_set_transfer_function(vrhip_renderer *r, const uint8_t *rgba8, uint32_t n_entries)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, rgba8 && n_entries > 0, VRHIP_ERR_INVALID, "Empty transfer function.");
    VR_REQUIRE(r, n_entries <= 4096, VRHIP_ERR_UNSUPPORTED,
               "Transfer functions above 4096 entries are not supported.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    // CL_UNORM_INT8 -> float: c / 255.0f (OpenCL 1.2 spec 8.3.1.1)
    std::vector<float4> table(n_entries);
    for (uint32_t i = 0; i < n_entries; ++i) {
        table[i].x = (float)rgba8[4 * i + 0] / 255.0f;
        table[i].y = (float)rgba8[4 * i + 1] / 255.0f;
        table[i].z = (float)rgba8[4 * i + 2] / 255.0f;
        table[i].w = (float)rgba8[4 * i + 3] / 255.0f;
    }
    VR_HIP(r, hipStreamSynchronize(r->stream));
    r->tff_n = 0;
    const int rc = grow(r, r->tff, n_entries * sizeof(float4));
    if (rc) return rc;
    VR_HIP(r, hipMemcpy(r->tff, table.data(), n_entries * sizeof(float4), hipMemcpyHostToDevice));
    r->tff_host.assign(&table[0].x, &table[0].x + 4 * (size_t)n_entries);   // (technique 8 integrates it: ensure_preint)
    r->tff_n = n_entries;
    tf_changed(r);
    return VRHIP_OK;
}

int vrhip_set_transfer_function_2d(vrhip_renderer *r, const uint8_t *rgba8, uint32_t n_v, uint32_t n_g, float g_hi)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, rgba8, VRHIP_ERR_INVALID, "Empty 2-D transfer function.");
    VR_REQUIRE(r, vrhip_tf2d_params_check(n_v, n_g, g_hi) == VRHIP_OK, VRHIP_ERR_INVALID,
               "2-D transfer function: n_v must be 1..4096, n_g 1..256, their product at most 65536, g_hi finite and > 0.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    // the table as float4 (c / 255.0f, like the 1-D one) and the columns' opacity summary (Tf2dView::nz)
    const size_t n = (size_t)n_v * n_g;
    std::vector<float4> table(n);
    std::vector<uint32_t> nz(n_v + 1, 0u);
    for (size_t k = 0; k < n; ++k) {
        table[k].x = (float)rgba8[4 * k + 0] / 255.0f;
        table[k].y = (float)rgba8[4 * k + 1] / 255.0f;
        table[k].z = (float)rgba8[4 * k + 2] / 255.0f;
        table[k].w = (float)rgba8[4 * k + 3] / 255.0f;
        if (rgba8[4 * k + 3]) nz[k % n_v + 1] = 1u;
    }
    for (uint32_t i = 0; i < n_v; ++i) nz[i + 1] += nz[i];
    const volatile float inv_ghi = 1.0f / g_hi;   // (volatile: rounded to fp32 here, whatever the host's flags)
    VR_HIP(r, hipStreamSynchronize(r->stream));
    tf2d_unset(r);
    int rc = grow(r, r->tf2d, n * sizeof(float4));
    if (!rc) rc = grow(r, r->tf2d_nz, nz.size() * sizeof(uint32_t));
    if (rc) return rc;
    VR_HIP(r, hipMemcpy(r->tf2d, table.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    VR_HIP(r, hipMemcpy(r->tf2d_nz, nz.data(), nz.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    tf2d_set(r, n_v, n_g, inv_ghi);
    return VRHIP_OK;
}

int vrhip_set_tff_prefix_sum(vrhip_renderer *r, const uint32_t *prefix, uint32_t n)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, prefix && n > 0, VRHIP_ERR_INVALID, "Empty prefix sum.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    r->prefix_n = 0;
    const int rc = grow(r, r->prefix, n * sizeof(uint32_t));
    if (rc) return rc;
    VR_HIP(r, hipMemcpy(r->prefix, prefix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    r->prefix_n = n;
    tf_changed(r);
    return VRHIP_OK;
}

int vrhip_build_bricks(vrhip_renderer *r)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, !r->vols.empty(), VRHIP_ERR_NODATA, "No volume data is loaded.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    // brick size / grid: volumerendercl.cpp:620-636
    for (int i = 0; i < 3; ++i) {
        uint32_t e = round_pow2(r->res[i] / 64u);
        r->brick_edge[i] = e > 1u ? e : 1u;
        r->brick_res[i] = (float)r->res[i] / (float)r->brick_edge[i];
        r->brick_tex[i] = (uint32_t)std::ceil((double)r->brick_res[i]);
        r->raycast.brickRes[i] = r->brick_res[i];   // :630-631
    }
    // The bricks depend on the voxels alone, and renderers created with vrhip_share_volumes keep
    // the pointer: an allocation is made once per slot and lives as long as the voxels do, and a
    // slot whose voxels have not changed since its last build is left alone (the reference
    // rebuilds on every setTransferFunction, :877 -- same values).
    for (size_t t = 0; t < r->vols.size(); ++t) {
        VolumeSlot &s = r->vols[t];
        if (!s.dev) return fail(r, VRHIP_ERR_NODATA,
                                "Error loading timeseries data: size mismatch.");   // :227
        if (s.borrowed) {   // shared voxels come with their bricks (they depend on nothing else)
            const vrhip_renderer *o = r->vol_owner;
            VR_REQUIRE(r, o && t < o->vols.size() && o->vols[t].bricks && o->vols[t].bricks_built, VRHIP_ERR_NODATA,
                       "vrhip_build_bricks: the owner of the shared volumes has to build its bricks first.");
            s.bricks.borrow(o->vols[t].bricks);
            continue;
        }
        const int rc = grow(r, s.bricks, bricks_bytes(r));   // (a slot without bricks is one with bricks_built unset)
        if (rc) return rc;
    }
    bool any = false;
    for (const VolumeSlot &s : r->vols) any = any || (!s.borrowed && !s.bricks_built);
    if (any) {   // (vrhip_last_bricks_seconds keeps reporting the last build that did something)
        VR_HIP(r, hipEventRecord(r->evb0, r->stream));
        for (VolumeSlot &s : r->vols) {
            if (s.borrowed || s.bricks_built) continue;
            VolView v = make_vol_view(r, s.dev);
            VR_HIP(r, vr_launch_build_bricks(v, r->format, r->brick_tex, s.bricks, r->stream));
            slot_bricks_built(s);
        }
        VR_HIP(r, hipEventRecord(r->evb1, r->stream));
        r->bricks_timed = true;
    }
    VR_HIP(r, hipStreamSynchronize(r->stream));   // reference: _queueCL.finish() (:670)
    bricks_built(r);
    return VRHIP_OK;
}

int vrhip_get_brick_info(const vrhip_renderer *r, uint32_t tex[3], float brick_res[3],
                         uint32_t edge[3])
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, r->bricks_valid, VRHIP_ERR_NODATA, "ESS bricks not built.");
    for (int i = 0; i < 3; ++i) {
        if (tex) tex[i] = r->brick_tex[i];
        if (brick_res) brick_res[i] = r->brick_res[i];
        if (edge) edge[i] = r->brick_edge[i];
    }
    return VRHIP_OK;
}

int vrhip_download_bricks(vrhip_renderer *r, uint32_t timestep, void *host_dst, size_t bytes)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, r->bricks_valid && timestep < r->vols.size() && r->vols[timestep].bricks,
               VRHIP_ERR_NODATA, "ESS bricks not built.");
    VR_REQUIRE(r, host_dst && bytes == bricks_bytes(r), VRHIP_ERR_INVALID,
               "vrhip_download_bricks: size mismatch");
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_HIP(r, hipMemcpyAsync(host_dst, r->vols[timestep].bricks, bytes, hipMemcpyDeviceToHost,
                             r->stream));
    VR_HIP(r, hipStreamSynchronize(r->stream));
    return VRHIP_OK;
}

double vrhip_last_bricks_seconds(const vrhip_renderer *r)
{
    if (!r || !r->bricks_timed) return 0.0;
    float ms = 0.f;
    if (hipEventSynchronize(r->evb1) != hipSuccess) return 0.0;
    if (hipEventElapsedTime(&ms, r->evb0, r->evb1) != hipSuccess) return 0.0;
    return (double)ms * 1e-3;
}

int vrhip_set_camera_params(vrhip_renderer *r, const vrhip_camera_params *p)
{
    if (!r || !p) return VRHIP_ERR_INVALID;
    r->cam = *p;
    return VRHIP_OK;
}

int vrhip_set_rendering_params(vrhip_renderer *r, const vrhip_rendering_params *p)
{
    if (!r || !p) return VRHIP_ERR_INVALID;
    r->render = *p;
    return VRHIP_OK;
}

int vrhip_set_raycast_params(vrhip_renderer *r, const vrhip_raycast_params *p)
{
    if (!r || !p) return VRHIP_ERR_INVALID;
    r->raycast = *p;
    return VRHIP_OK;
}

int vrhip_set_pathtrace_params(vrhip_renderer *r, const vrhip_pathtrace_params *p)
{
    if (!r || !p) return VRHIP_ERR_INVALID;
    r->pathtrace = *p;
    return VRHIP_OK;
}

int vrhip_set_iso_params(vrhip_renderer *r, const vrhip_iso_params *p)
{
    if (!r || !p) return VRHIP_ERR_INVALID;
    r->iso = *p;   // (checked at render time, and only when technique 4 is selected: check_renderable)
    return VRHIP_OK;
}

int vrhip_set_object_ess(vrhip_renderer *r, int enabled)
{
    if (!r) return VRHIP_ERR_INVALID;
    r->use_ess = enabled != 0;
    return VRHIP_OK;
}

int vrhip_render_frame(vrhip_renderer *r, uint32_t width, uint32_t height, float *out_rgba,
                       int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    int rc = prepare_render(r, width, height, 0, 0, nullptr, 0);
    if (rc) return rc;
    RaycastLaunch a;
    fill_launch(r, width, height, width, &a);
    if (out_rgba && out_is_device) a.frame.out = (float4 *)out_rgba;
    rc = launch_timed(r, a);
    if (rc) return rc;
    if (out_rgba && !out_is_device) {
        VR_HIP(r, hipMemcpyAsync(out_rgba, r->fb, (size_t)width * height * sizeof(float4),
                                 hipMemcpyDeviceToHost, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
    }
    return VRHIP_OK;
}

int vrhip_render_tiles(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                       uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                       float *out_tiles_dev)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, out_tiles_dev, VRHIP_ERR_INVALID, "vrhip_render_tiles: NULL output");
    if (n_tiles == 0) return VRHIP_OK;
    VR_REQUIRE(r, tile_ids, VRHIP_ERR_INVALID, "vrhip_render_tiles: NULL tile list");
    int rc = prepare_render(r, width, height, tile_w, tile_h, tile_ids, n_tiles);
    if (rc) return rc;
    RaycastLaunch a;
    fill_launch(r, width, height, tile_w, &a);
    a.frame.out = (float4 *)out_tiles_dev;
    return launch_timed(r, a);
}

int vrhip_render_batch(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                       uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                       const uint32_t *seeds, uint32_t n_frames, float *out_dev,
                       uint32_t out_frame_stride)
{
    return vrhip_render_batch_views(r, width, height, tile_w, tile_h, tile_ids, n_tiles, seeds, nullptr, n_frames,
                                    out_dev, out_frame_stride);
}

int vrhip_render_batch_views(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                             uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                             const uint32_t *seeds, const vrhip_camera_params *cams, uint32_t n_frames,
                             float *out_dev, uint32_t out_frame_stride)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, out_dev && seeds, VRHIP_ERR_INVALID, "vrhip_render_batch: NULL argument");
    VR_REQUIRE(r, n_frames >= 1 && n_frames <= kMaxBatchFrames, VRHIP_ERR_INVALID,
               "vrhip_render_batch: 1..256 frames per batch");
    VR_REQUIRE(r, height <= (8u << kFrameShift) && width <= (8u << kFrameShift), VRHIP_ERR_INVALID,
               "Invalid output image size.");
    VR_REQUIRE(r, !tile_ids || n_tiles > 0, VRHIP_ERR_INVALID, "vrhip_render_batch: empty tile list");
    // the frames of a batch are independent: nothing that chains frames, nothing that draws from
    // rendering_params.seed outside the ray set-up
    const vrhip_rendering_params &rp = r->render;
    VR_REQUIRE(r, (rp.technique == 0 || minmax_technique(rp.technique)) && rp.iteration == 0 && !rp.imgEss &&
                      !r->raycast.useAO,
               VRHIP_ERR_UNSUPPORTED,
               "vrhip_render_batch: technique 0, 2, 4, 6 or 8 only, iteration 0, no image-order ESS, no ambient occlusion");
    const uint32_t packed = tile_ids ? n_tiles * tile_w * tile_h : width * height;
    VR_REQUIRE(r, out_frame_stride == 0 || out_frame_stride >= packed, VRHIP_ERR_INVALID,
               "vrhip_render_batch: frame stride smaller than a frame");
    VR_REQUIRE(r, (unsigned long long)n_frames * (out_frame_stride ? out_frame_stride : packed) <= 0xffffffffull,
               VRHIP_ERR_INVALID, "vrhip_render_batch: the frames of a batch must hold fewer than 2^32 pixels together");
    int rc = prepare_render(r, width, height, tile_w, tile_h, tile_ids, n_tiles, n_frames,
                            out_frame_stride);
    if (rc) return rc;
    if ((rc = grow(r, r->seeds_dev, kMaxBatchFrames * sizeof(uint32_t)))) return rc;
    VR_HIP(r, hipMemcpyAsync(r->seeds_dev, seeds, n_frames * sizeof(uint32_t), hipMemcpyHostToDevice,
                             r->stream));
    if (cams) {
        if ((rc = grow(r, r->cams_dev, kMaxBatchFrames * sizeof(vrhip_camera_params)))) return rc;
        VR_HIP(r, hipMemcpyAsync(r->cams_dev, cams, n_frames * sizeof(vrhip_camera_params), hipMemcpyHostToDevice,
                                 r->stream));
    }
    RaycastLaunch a;
    fill_launch(r, width, height, tile_ids ? tile_w : width, &a);
    a.frame.out = (float4 *)out_dev;
    a.frame.seeds = r->seeds_dev;
    a.frame.cams = cams ? r->cams_dev : nullptr;
    // Pixel-major ray order (vr_internal.h): the frames of ONE camera differ in the jitter only, so the rays of a pixel
    // march alike and phase 1 draws them side by side.  A camera per frame: the same pixel is not the same ray.
    if (r->pixel_major && !cams && n_frames >= 2 && rp.technique == 0 && a.frame.live_rays) {
        // The block is sized for the worst case, every ray of the set live: 268 bytes per work item (140 MB for 1024^2
        // x 32 frames, beside the 2 GB of ray records that case needs).  It is optional: where it does not fit 32-bit
        // indices or cannot be allocated, the set keeps the pre-pass's order and the launch info says so.
        const unsigned long long words = pm_block_words(r->queue_n, n_frames);
        if (words <= 0xffffffffull) {
            if ((rc = grow(r, r->pm, (size_t)words * sizeof(uint32_t), kGrowTolerate))) return rc;
            if (r->pm.p) {
                a.frame.pm = r->pm;
                a.pm_group = r->pm_group;
            }
        }
    }
    const uint32_t ctrl_used = r->ctrl_sel;
    rc = launch_timed(r, a);
    if (!rc && r->last_info.pixel_major) {   // vrhip_download_ray_order
        r->pm_last = true;
        r->pm_last_ctrl = ctrl_used;
        r->pm_last_frames = n_frames;
    }
    return rc;
}

int vrhip_render_samples(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h,
                         const uint32_t *tile_ids, uint32_t n_tiles, const uint32_t *seeds, uint32_t n_samples,
                         uint32_t samples_per_launch, float *out_rgba, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, seeds && n_samples >= 1, VRHIP_ERR_INVALID, "vrhip_render_samples: no seeds");
    VR_REQUIRE(r, r->render.technique == 1, VRHIP_ERR_UNSUPPORTED,
               "vrhip_render_samples: path tracer only (technique 1); the ray caster's frames do not accumulate here");
    VR_REQUIRE(r, height <= (8u << kFrameShift) && width <= (8u << kFrameShift), VRHIP_ERR_INVALID,
               "Invalid output image size.");
    VR_REQUIRE(r, !tile_ids || n_tiles > 0, VRHIP_ERR_INVALID, "vrhip_render_samples: empty tile list");
    const unsigned long long plane = tile_ids ? (unsigned long long)n_tiles * tile_w * tile_h
                                              : (unsigned long long)width * height;
    VR_REQUIRE(r, plane >= 1 && plane <= 0xffffffffull, VRHIP_ERR_INVALID, "vrhip_render_samples: too many pixels");
    // samples per set: what was asked for (0: kDefaultSamplesPerLaunch), within the queue's frame bits and 2^32 records
    unsigned long long per = samples_per_launch ? samples_per_launch : kDefaultSamplesPerLaunch;
    if (!samples_per_launch && per * plane > kDefaultSampleRecords) per = kDefaultSampleRecords / plane ? kDefaultSampleRecords / plane : 1;
    if (per > kMaxBatchFrames) per = kMaxBatchFrames;
    if (per > n_samples) per = n_samples;
    if (per * plane > 0xffffffffull) per = 0xffffffffull / plane;
    // a tile subset for the host has no place of its own to land in: one more plane of the scratch
    const bool stage = tile_ids && out_rgba && !out_is_device;
    const uint32_t first = r->render.iteration;
    for (uint32_t done = 0; done < n_samples;) {
        const uint32_t m = (uint32_t)(per < n_samples - done ? per : n_samples - done);
        int rc = prepare_render(r, width, height, tile_w, tile_h, tile_ids, n_tiles, m, 0);
        if (rc) return rc;
        const size_t rec_bytes = ((size_t)per + (stage ? 1u : 0u)) * (size_t)plane * sizeof(float4);
        const size_t need = rec_bytes + (size_t)per * (size_t)plane;
        if ((rc = grow(r, r->samples_dev, need))) return rc;
        if ((rc = grow(r, r->seeds_dev, kMaxBatchFrames * sizeof(uint32_t)))) return rc;
        VR_HIP(r, hipMemcpyAsync(r->seeds_dev, seeds + done, m * sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
        RaycastLaunch a;
        fill_launch(r, width, height, tile_ids ? tile_w : width, &a);
        float4 *const planes = (float4 *)r->samples_dev.p;
        a.frame.out = planes;
        a.frame.sample_mark = (uint8_t *)r->samples_dev.p + rec_bytes;
        a.frame.seeds = r->seeds_dev;
        a.render.iteration = first + done;
        a.samples = 1;
        a.sample_plane = (uint32_t)plane;
        a.fold_out = stage ? planes + (size_t)per * (size_t)plane : out_is_device ? (float4 *)out_rgba : nullptr;
        a.keep_stats = done != 0;
        rc = launch_timed(r, a);
        if (rc) return rc;
        done += m;
    }
    if (out_rgba && !out_is_device) {
        const float4 *src = stage ? (const float4 *)r->samples_dev.p + (size_t)per * (size_t)plane : r->fb;
        VR_HIP(r, hipMemcpyAsync(out_rgba, src, (size_t)plane * sizeof(float4), hipMemcpyDeviceToHost, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
    }
    return VRHIP_OK;
}

double vrhip_last_kernel_seconds(const vrhip_renderer *r)
{
    if (!r || !r->timed) return 0.0;
    float ms = 0.f;
    if (hipEventSynchronize(r->ev1) != hipSuccess) return 0.0;
    if (hipEventElapsedTime(&ms, r->ev0, r->ev1) != hipSuccess) return 0.0;
    return (double)ms * 1e-3;
}

int vrhip_last_phase_seconds(const vrhip_renderer *r, double *phase1, double *phase2)
{
    if (!r || !r->timed || !r->phase_timed) return VRHIP_ERR_NODATA;
    float a = 0.f, b = 0.f;
    if (hipEventSynchronize(r->ev1) != hipSuccess) return VRHIP_ERR_HIP;
    if (hipEventElapsedTime(&a, r->ev0, r->evm) != hipSuccess) return VRHIP_ERR_HIP;
    if (hipEventElapsedTime(&b, r->evm, r->ev1) != hipSuccess) return VRHIP_ERR_HIP;
    if (phase1) *phase1 = (double)a * 1e-3;
    if (phase2) *phase2 = (double)b * 1e-3;
    return VRHIP_OK;
}

int vrhip_last_launch_info(const vrhip_renderer *r, vrhip_launch_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_info) return fail(r, VRHIP_ERR_NODATA, "vrhip_last_launch_info: nothing has been rendered yet");
    *out = r->last_info;
    return VRHIP_OK;
}

int vrhip_download_cost_map(vrhip_renderer *r, uint16_t *out, size_t n)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, r->cost && n == (size_t)r->fb_w * r->fb_h, VRHIP_ERR_NODATA,
               "vrhip_download_cost_map: no cost map of this size (render a frame first)");
    VR_HIP(r, hipStreamSynchronize(r->stream));
    VR_HIP(r, hipMemcpy(out, r->cost, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return VRHIP_OK;
}

int vrhip_download_ray_order(vrhip_renderer *r, uint32_t sizes[8], uint32_t *out_items, size_t n_items,
                             uint32_t *out_notes, size_t n_notes, uint32_t out_counters[16], uint32_t *out_records,
                             size_t n_records, uint32_t *out_index, size_t n_index)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, r->pm_last && r->pm && r->live_rays && r->queue_dev && r->queue_head, VRHIP_ERR_NODATA,
               "vrhip_download_ray_order: the last render call was not a launch set in pixel-major order");
    const uint32_t n = r->queue_n, sf = r->pm_last_frames;
    const uint32_t ray_cap = live_list_cap(n), idx_cap = pm_list_cap(n, sf);
    VR_HIP(r, hipStreamSynchronize(r->stream));
    // the control words of that set: the set after next clears them (FrameView::next_ctrl), nothing before
    std::vector<uint32_t> ctrl(kControlWords);
    VR_HIP(r, hipMemcpy(ctrl.data(), r->queue_head + (size_t)r->pm_last_ctrl * kControlWords, kControlWords * sizeof(uint32_t),
                        hipMemcpyDeviceToHost));
    uint32_t counters[2 * kLiveLists], take[2 * kLiveLists];
    size_t n_rec = 0, n_ent = 0;
    for (uint32_t k = 0; k < kLiveLists; ++k) {
        counters[k] = ctrl[kLiveBase + k * kLiveStride];
        counters[kLiveLists + k] = ctrl[kPmBase + k * kLiveStride];
        take[k] = counters[k] < ray_cap ? counters[k] : ray_cap;
        take[kLiveLists + k] = counters[kLiveLists + k] < idx_cap ? counters[kLiveLists + k] : idx_cap;
        n_rec += take[k];
        n_ent += take[kLiveLists + k];
    }
    if (sizes) {
        const uint32_t s[8] = {sf, n, r->pm_group, ray_cap, idx_cap, (uint32_t)n_rec, (uint32_t)n_ent, 0u};
        std::memcpy(sizes, s, sizeof s);
    }
    if (out_counters) std::memcpy(out_counters, counters, sizeof counters);
    VR_REQUIRE(r, (!out_items || n_items == 3 * (size_t)n) && (!out_notes || n_notes == 3 * (size_t)n) &&
                  (!out_records || n_records == 4 * n_rec) && (!out_index || n_index == n_ent),
               VRHIP_ERR_INVALID, "vrhip_download_ray_order: size mismatch");
    if (out_items) {
        std::vector<WaveTile> q(n);
        if (n) VR_HIP(r, hipMemcpy(q.data(), r->queue_dev, (size_t)n * sizeof(WaveTile), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) {
            out_items[3 * (size_t)i] = wt_col(q[i]);
            out_items[3 * (size_t)i + 1] = wt_row(q[i]);
            out_items[3 * (size_t)i + 2] = wt_frame(q[i]);
        }
    }
    if (out_notes && n) VR_HIP(r, hipMemcpy(out_notes, r->pm, 3 * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_records) {
        std::vector<ContRec> recs;
        for (uint32_t k = 0; k < kLiveLists; ++k) {
            recs.resize(take[k]);
            if (take[k])
                VR_HIP(r, hipMemcpy(recs.data(), r->live_rays + (size_t)k * ray_cap, (size_t)take[k] * sizeof(ContRec),
                                    hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < take[k]; ++i) {
                out_records[0] = rec_gx(recs[i]);
                out_records[1] = rec_gy(recs[i]);
                out_records[2] = rec_frame(recs[i]);
                out_records[3] = k * ray_cap + i;
                out_records += 4;
            }
        }
    }
    if (out_index)
        for (uint32_t k = 0; k < kLiveLists; ++k) {
            const uint32_t c = take[kLiveLists + k];
            if (c)
                VR_HIP(r, hipMemcpy(out_index, r->pm + 3 * (size_t)n + (size_t)k * idx_cap, (size_t)c * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost));
            out_index += c;
        }
    return VRHIP_OK;
}

int vrhip_set_phase_timing(vrhip_renderer *r, int enabled)
{
    if (!r) return VRHIP_ERR_INVALID;
    r->phase_timing = enabled != 0;
    return VRHIP_OK;
}

int vrhip_set_frame_timing(vrhip_renderer *r, int enabled)
{
    if (!r) return VRHIP_ERR_INVALID;
    r->frame_timing = enabled != 0;
    if (!r->frame_timing) r->timed = r->phase_timed = false;
    return VRHIP_OK;
}

int vrhip_set_stats_enabled(vrhip_renderer *r, int enabled)
{
    if (!r) return VRHIP_ERR_INVALID;
    r->stats_enabled = enabled != 0;
    return VRHIP_OK;
}

int vrhip_get_stats(const vrhip_renderer *r, vrhip_stats *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (hipSetDevice(r->device) != hipSuccess) return VRHIP_ERR_HIP;
    DevStats s;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    VR_HIP(r, hipMemcpy(&s, r->stats_dev, sizeof s, hipMemcpyDeviceToHost));
    out->samples_taken = s.v[0];
    out->samples_nominal = s.v[1];
    out->samples_shaded = s.v[2];
    out->bricks_visited = s.v[3];
    out->bricks_skipped = s.v[4];
    out->rays_hit = s.v[5];
    return VRHIP_OK;
}

int vrhip_set_environment_map(vrhip_renderer *r, const float *rgba, uint32_t width,
                              uint32_t height)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    r->env.release();
    r->env_w = r->env_h = 0;
    // the kernel only samples maps wider than one texel (:655); createEnvironmentMap("")
    // installs a 1x1 white one, i.e. none
    if (!rgba || width <= 1 || height == 0) return VRHIP_OK;
    VR_REQUIRE(r, width <= 16384 && height <= 16384, VRHIP_ERR_INVALID,
               "Environment map too large.");
    const size_t bytes = (size_t)width * height * sizeof(float4);
    const int rc = grow(r, r->env, bytes);
    if (rc) return rc;
    VR_HIP(r, hipMemcpy(r->env, rgba, bytes, hipMemcpyHostToDevice));
    r->env_w = width;
    r->env_h = height;
    return VRHIP_OK;
}

int vrhip_reset_image_ess(vrhip_renderer *r)
{
    if (!r) return VRHIP_ERR_INVALID;
    r->hit_w = r->hit_h = 0;   // re-created (and re-initialised) by the next imgEss frame
    return VRHIP_OK;
}

int vrhip_get_image_ess(vrhip_renderer *r, uint32_t width, uint32_t height, uint8_t *hit_in,
                        uint8_t *hit_out)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, width > 0 && height > 0 && width <= 16384 && height <= 16384, VRHIP_ERR_INVALID,
               "Invalid output image size.");
    int rc = ensure_hit_images(r, width, height);
    if (rc) return rc;
    const size_t n = (size_t)r->hit_w * r->hit_h;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    if (hit_in) VR_HIP(r, hipMemcpy(hit_in, r->hit_in, n, hipMemcpyDeviceToHost));
    if (hit_out) VR_HIP(r, hipMemcpy(hit_out, r->hit_out, n, hipMemcpyDeviceToHost));
    return VRHIP_OK;
}

int vrhip_set_image_ess(vrhip_renderer *r, uint32_t width, uint32_t height, const uint8_t *hit_in,
                        const uint8_t *hit_out)
{
    if (!r) return VRHIP_ERR_INVALID;
    if (set_device(r)) return VRHIP_ERR_HIP;
    VR_REQUIRE(r, width > 0 && height > 0 && width <= 16384 && height <= 16384, VRHIP_ERR_INVALID,
               "Invalid output image size.");
    int rc = ensure_hit_images(r, width, height);
    if (rc) return rc;
    const size_t n = (size_t)r->hit_w * r->hit_h;
    VR_HIP(r, hipStreamSynchronize(r->stream));
    if (hit_in) VR_HIP(r, hipMemcpy(r->hit_in, hit_in, n, hipMemcpyHostToDevice));
    if (hit_out) VR_HIP(r, hipMemcpy(r->hit_out, hit_out, n, hipMemcpyHostToDevice));
    return VRHIP_OK;
}

int vrhip_count_touched(vrhip_renderer *r, uint32_t width, uint32_t height,
                        uint64_t *microbricks_touched, uint8_t *bitmap_host, size_t bitmap_bytes)
{
    return count_touched_impl(r, width, height, 0, 0, nullptr, 0, microbricks_touched,
                              bitmap_host, bitmap_bytes);
}

int vrhip_count_fetched(vrhip_renderer *r, uint32_t width, uint32_t height, uint64_t *microbricks_fetched)
{
    if (r && r->render.technique != 1)
        return fail(r, VRHIP_ERR_UNSUPPORTED, "vrhip_count_fetched: technique 1 (path tracer) only");
    return count_touched_impl(r, width, height, 0, 0, nullptr, 0, microbricks_fetched, nullptr, 0, true);
}

int vrhip_count_touched_tiles(vrhip_renderer *r, uint32_t width, uint32_t height,
                              uint32_t tile_w, uint32_t tile_h, const uint32_t *tile_ids,
                              uint32_t n_tiles, uint64_t *microbricks_touched)
{
    if (r && (!tile_ids || !n_tiles))
        return fail(r, VRHIP_ERR_INVALID, "vrhip_count_touched_tiles: empty tile list");
    return count_touched_impl(r, width, height, tile_w, tile_h, tile_ids, n_tiles,
                              microbricks_touched, nullptr, 0);
}

} // extern "C"
