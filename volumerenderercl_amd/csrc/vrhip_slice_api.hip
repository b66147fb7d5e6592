// vrhip_slice_api.hip -- vrhip_render_slices (include/vrhip.h "slice views"): the checks, the upload of a call's
// parameter blocks, the launch (vr_slice.hip) and the copy to a host destination.  It reads the volume of the
// current time step, the transfer function, useLinear and backgroundColor, and writes only the three buffers the
// renderer keeps for it (vr_renderer.h): nothing a render entry point reads later.
#include <cmath>

#include "vr_renderer.h"

extern "C" {

int vrhip_render_slices(vrhip_renderer *r, uint32_t width, uint32_t height, const vrhip_slice_params *slices,
                        uint32_t n_slices, float *out_rgba, int out_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, slices && out_rgba, VRHIP_ERR_INVALID, "vrhip_render_slices: NULL argument");
    VR_REQUIRE(r, n_slices > 0, VRHIP_ERR_INVALID, "vrhip_render_slices: no slices");
    VR_REQUIRE(r, width > 0 && height > 0 && width <= 16384 && height <= 16384, VRHIP_ERR_INVALID,
               "Invalid output image size.");
    bool need_tf = false;
    for (uint32_t i = 0; i < n_slices; ++i) {
        const vrhip_slice_params &s = slices[i];
        VR_REQUIRE(r, s.samples >= 1 && s.samples <= VRHIP_SLICE_MAX_SAMPLES, VRHIP_ERR_INVALID,
                   "vrhip_render_slices: samples must be 1 .. 256.");
        VR_REQUIRE(r, s.mode <= VRHIP_SLICE_MEAN, VRHIP_ERR_INVALID, "vrhip_render_slices: unknown mode.");
        VR_REQUIRE(r, s.output <= VRHIP_SLICE_VALUE, VRHIP_ERR_INVALID, "vrhip_render_slices: unknown output.");
        VR_REQUIRE(r, s.reserved == 0, VRHIP_ERR_INVALID, "vrhip_render_slices: reserved must be 0.");
        for (int c = 0; c < 3; ++c)
            VR_REQUIRE(r, std::isfinite(s.origin[c]) && std::isfinite(s.u[c]) && std::isfinite(s.v[c]) && std::isfinite(s.w[c]),
                       VRHIP_ERR_INVALID, "vrhip_render_slices: origin, u, v and w must be finite.");
        need_tf = need_tf || s.output == VRHIP_SLICE_TF;
    }
    const unsigned long long patches = (unsigned long long)((width + 7u) / 8u) * ((height + 7u) / 8u);
    VR_REQUIRE(r, patches * n_slices <= 0xffffffffull, VRHIP_ERR_INVALID,
               "vrhip_render_slices: more than 2^32 - 1 patches in one call.");
    VR_REQUIRE(r, !out_is_device || ((uintptr_t)out_rgba & 15u) == 0, VRHIP_ERR_INVALID,
               "vrhip_render_slices: a device destination must be 16-byte aligned.");
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, !need_tf || (r->tff && r->tff_n), VRHIP_ERR_NODATA, "No transfer function set.");
    VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "slice views: RG / RGBA volumes are not supported.");
    if (set_device(r)) return VRHIP_ERR_HIP;

    const size_t param_bytes = (size_t)n_slices * sizeof(vrhip_slice_params);
    const size_t out_bytes = (size_t)n_slices * width * height * sizeof(float4);
    int rc = grow(r, r->slice_params_dev, param_bytes);
    if (rc) return rc;
    float4 *out_dev = (float4 *)out_rgba;
    if (!out_is_device) {
        if ((rc = grow(r, r->slice_out_dev, out_bytes))) return rc;
        if ((rc = grow_pinned(r, r->slice_host, out_bytes))) return rc;
        out_dev = r->slice_out_dev;
    }
    // (pageable source: the copy has left the caller's array when the call returns)
    VR_HIP(r, hipMemcpyAsync(r->slice_params_dev, slices, param_bytes, hipMemcpyHostToDevice, r->stream));
    VR_HIP(r, vr_launch_slices(make_vol_view(r, r->vols[r->timestep].dev), r->format, make_tf_view(r), r->slice_params_dev,
                               n_slices, width, height, r->render.useLinear, r->render.backgroundColor, out_dev, r->stream));
    if (!out_is_device) {
        VR_HIP(r, hipMemcpyAsync(r->slice_host.p, out_dev, out_bytes, hipMemcpyDeviceToHost, r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
        std::memcpy(out_rgba, r->slice_host.p, out_bytes);
    }
    return VRHIP_OK;
}

} // extern "C"
