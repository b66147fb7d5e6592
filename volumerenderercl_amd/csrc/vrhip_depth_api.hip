// vrhip_depth_api.hip -- vrhip_render_depth and vrhip_last_depth_info (include/vrhip.h "depth images and picking"):
// the checks, the cell grid for skipping, the launch (vr_depth.hip) and the copy to host destinations.  It reads the
// volume of the current time step, the camera, seed, useLinear, samplingRate, the object-ESS switch and -- in OPACITY
// mode -- the transfer function, and writes only the buffers the renderer keeps for it (vr_renderer.h): not the frame
// buffer, the hit images, the control words or vrhip_last_launch_info.  (The cell grid it may build is derived state
// every technique builds on demand and reads as it is: vr_renderer.h "derived state".)
#include <cmath>

#include "vr_renderer.h"

extern "C" {

int vrhip_render_depth(vrhip_renderer *r, uint32_t width, uint32_t height, const vrhip_depth_params *p,
                       float *out_xyzt, float *out_aux, uint8_t *out_kind, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p, VRHIP_ERR_INVALID, "vrhip_render_depth: NULL argument");
    VR_REQUIRE(r, out_xyzt || out_aux || out_kind, VRHIP_ERR_INVALID, "vrhip_render_depth: no output");
    VR_REQUIRE(r, p->mode <= VRHIP_DEPTH_OPACITY, VRHIP_ERR_INVALID, "vrhip_render_depth: unknown mode.");
    VR_REQUIRE(r, p->reserved == 0, VRHIP_ERR_INVALID, "vrhip_render_depth: reserved must be 0.");
    VR_REQUIRE(r, p->mode == VRHIP_DEPTH_MAX || std::isfinite(p->threshold), VRHIP_ERR_INVALID,
               "vrhip_render_depth: threshold must be finite.");
    VR_REQUIRE(r, p->mode != VRHIP_DEPTH_ISO || p->refineSteps <= 16u, VRHIP_ERR_INVALID,
               "vrhip_render_depth: refineSteps must be at most 16.");
    VR_REQUIRE(r, width > 0 && height > 0 && width <= 16384 && height <= 16384, VRHIP_ERR_INVALID,
               "Invalid output image size.");
    vrhip_depth_params dp = *p;
    if (dp.w == 0 && dp.h == 0) {   // the whole frame
        VR_REQUIRE(r, dp.x0 == 0 && dp.y0 == 0, VRHIP_ERR_INVALID, "vrhip_render_depth: the rectangle is not inside the frame.");
        dp.w = width;
        dp.h = height;
    }
    VR_REQUIRE(r, dp.w > 0 && dp.h > 0, VRHIP_ERR_INVALID, "vrhip_render_depth: exactly one of w, h is zero.");
    VR_REQUIRE(r, dp.x0 < width && dp.w <= width - dp.x0 && dp.y0 < height && dp.h <= height - dp.y0, VRHIP_ERR_INVALID,
               "vrhip_render_depth: the rectangle is not inside the frame.");
    VR_REQUIRE(r, !out_is_device || ((uintptr_t)out_xyzt & 15u) == 0, VRHIP_ERR_INVALID,
               "vrhip_render_depth: a device out_xyzt must be 16-byte aligned.");
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, dp.mode != VRHIP_DEPTH_OPACITY || (r->tff && r->tff_n), VRHIP_ERR_NODATA, "No transfer function set.");
    VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "depth images: RG / RGBA volumes are not supported.");
    if (set_device(r)) return VRHIP_ERR_HIP;

    DepthLaunch a;
    std::memset(&a, 0, sizeof a);
    a.vol = make_vol_view(r, r->vols[r->timestep].dev);
    a.tf = make_tf_view(r);
    set_frame_geometry(&a.frame, width, height);
    a.cam = r->cam;
    a.render = r->render;
    a.raycast = r->raycast;
    a.params = dp;
    a.format = r->format;

    // ---- object-order ESS on: the cell grid, as techniques 2 and 4 take it (ISO, MAX: the (min, max) pairs, which need
    // no transfer function) or with the ray caster's empty bits (OPACITY)
    int rc;
    if (mip_skips(r)) {
        const bool have_tf = r->tff && r->tff_n;
        if ((rc = ensure_cells(r, false, true, have_tf))) return rc;
        a.cells = r->cells;
        a.cells.bound = a.cells.cbound = nullptr;
        a.cells.cdist = nullptr;
        if (dp.mode == VRHIP_DEPTH_OPACITY) {
            VR_REQUIRE(r, a.cells.empty, VRHIP_ERR_HIP, "vrhip_render_depth: the empty bits were not built.");
        } else {
            a.cells.empty = nullptr;
            const bool fine = r->cells.eshift != r->cells.shift;
            a.cell_minmax = cell_minmax_of(r, fine);
            VR_REQUIRE(r, a.cell_minmax, VRHIP_ERR_HIP, "vrhip_render_depth: the cells' (min, max) were not built.");
            // the grid the pairs live on, in the e* fields: the fine grid, or the only one (vr_launch_mip)
            if (!fine) { a.cells.ecx = a.cells.cx; a.cells.ecy = a.cells.cy; a.cells.ecz = a.cells.cz; a.cells.eshift = a.cells.shift; }
        }
    }

    // ---- destinations: the caller's device memory, or one device block of the renderer's: xyzt, aux, kind
    const size_t n = (size_t)dp.w * dp.h;
    const size_t off_aux = n * sizeof(float4), off_kind = off_aux + n * sizeof(float), bytes = off_kind + n;
    if (out_is_device) {
        a.out_xyzt = (float4 *)out_xyzt;
        a.out_aux = out_aux;
        a.out_kind = out_kind;
    } else {
        if ((rc = grow(r, r->depth_out_dev, bytes))) return rc;
        if ((rc = grow_pinned(r, r->depth_host, bytes))) return rc;
        uint8_t *base = (uint8_t *)r->depth_out_dev.p;
        a.out_xyzt = out_xyzt ? (float4 *)base : nullptr;
        a.out_aux = out_aux ? (float *)(base + off_aux) : nullptr;
        a.out_kind = out_kind ? base + off_kind : nullptr;
    }

    r->have_depth_info = false;
    VR_HIP(r, vr_launch_depth(a, r->stream));
    std::memset(&r->depth_info, 0, sizeof r->depth_info);
    r->depth_info.mode = dp.mode;
    r->depth_info.work_items = ((dp.w + 7u) / 8u) * ((dp.h + 7u) / 8u);
    r->depth_info.empty_skip = (a.cell_minmax || a.cells.empty) ? 1u : 0u;
    r->have_depth_info = true;

    if (!out_is_device) {
        const uint8_t *dev = (const uint8_t *)r->depth_out_dev.p;
        uint8_t *host = (uint8_t *)r->depth_host.p;
        if (out_xyzt) VR_HIP(r, hipMemcpyAsync(host, dev, off_aux, hipMemcpyDeviceToHost, r->stream));
        if (out_aux) VR_HIP(r, hipMemcpyAsync(host + off_aux, dev + off_aux, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
        if (out_kind) VR_HIP(r, hipMemcpyAsync(host + off_kind, dev + off_kind, n, hipMemcpyDeviceToHost, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
        if (out_xyzt) std::memcpy(out_xyzt, host, off_aux);
        if (out_aux) std::memcpy(out_aux, host + off_aux, n * sizeof(float));
        if (out_kind) std::memcpy(out_kind, host + off_kind, n);
    }
    return VRHIP_OK;
}

int vrhip_last_depth_info(const vrhip_renderer *r, vrhip_depth_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_depth_info) return fail(r, VRHIP_ERR_NODATA, "vrhip_last_depth_info: no depth image has been rendered yet");
    *out = r->depth_info;
    return VRHIP_OK;
}

} // extern "C"
