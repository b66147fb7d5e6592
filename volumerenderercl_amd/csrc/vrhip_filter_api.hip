// vrhip_filter_api.hip -- vrhip_filter_volume, vrhip_last_filter_info, vrhip_filter_params_check and
// vrhip_filter_gaussian_taps (include/vrhip.h "volume filters"): the checks, the cell grid for skipping, the
// destination slot (prepare_slot, as an upload takes it), the launch (vr_filter.hip) and the counters.  It reads the
// volume of the current time step and the object-ESS switch and writes the voxels of the destination step; what
// depends on those voxels goes stale as after an upload (vr_renderer.h "derived state").
#include <cmath>
#include <utility>

#include "vr_renderer.h"

namespace {

// the checks that need no volume, in the header's order
int filter_check(vrhip_renderer *r, const vrhip_filter_params *p)
{
    VR_REQUIRE(r, p->kind == VRHIP_FILTER_SEPARABLE || p->kind == VRHIP_FILTER_MEDIAN3, VRHIP_ERR_INVALID,
               "filter: unknown kind.");
    for (int a = 0; a < 3; ++a) {
        VR_REQUIRE(r, p->radius[a] <= VRHIP_FILTER_MAX_RADIUS, VRHIP_ERR_INVALID, "filter: a radius above 8.");
        VR_REQUIRE(r, p->kind != VRHIP_FILTER_MEDIAN3 || p->radius[a] == 0, VRHIP_ERR_INVALID,
                   "filter: the median takes no radius (it must be 0).");
        if (p->kind == VRHIP_FILTER_SEPARABLE)
            for (uint32_t k = 0; k <= p->radius[a]; ++k)
                VR_REQUIRE(r, std::isfinite(p->taps[a][k]), VRHIP_ERR_INVALID, "filter: a tap within the radius is not finite.");
    }
    VR_REQUIRE(r, !(p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]), VRHIP_ERR_INVALID,
               "filter: reserved must be 0.");
    return VRHIP_OK;
}

} // namespace

extern "C" {

int vrhip_filter_volume(vrhip_renderer *r, const vrhip_filter_params *p, uint32_t dst_timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p, VRHIP_ERR_INVALID, "vrhip_filter_volume: NULL argument");
    int rc;
    if ((rc = filter_check(r, p))) return rc;
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "filter: RG / RGBA volumes are not supported.");
    for (const VolumeSlot &s : r->vols)   // (before anything is touched: prepare_slot would clear a sharer)
        VR_REQUIRE(r, !s.borrowed, VRHIP_ERR_UNSUPPORTED, "filter: this renderer's volumes belong to another renderer.");
    VR_REQUIRE(r, dst_timestep <= r->vols.size(), VRHIP_ERR_INVALID, "filter: dst_timestep is above the number of time steps.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    r->have_filter_info = false;
    vrhip_filter_info info;
    std::memset(&info, 0, sizeof info);
    const bool in_place = dst_timestep == r->timestep;

    FilterLaunch a;
    std::memset(&a, 0, sizeof a);
    a.format = r->format;
    a.kind = p->kind;
    for (int i = 0; i < 3; ++i) {
        a.radius[i] = p->radius[i];
        for (uint32_t k = 0; k <= VRHIP_FILTER_MAX_RADIUS; ++k) a.taps[i][k] = p->taps[i][k];
    }
    a.num_cus = r->num_cus;
    if (mip_skips(r)) {   // object-order ESS: the coarse cells' (min, max) of the source, built before it may go stale
        if ((rc = ensure_cells(r, true, false, false))) return rc;
        a.cell_minmax = cell_minmax_of(r, false);
        VR_REQUIRE(r, a.cell_minmax, VRHIP_ERR_HIP, "filter: the cells' (min, max) were not built.");
        a.cell_shift = r->cells.shift;
        a.cell_cx = r->cells.cx;
        a.cell_cy = r->cells.cy;
        a.cell_cz = r->cells.cz;
        VR_REQUIRE(r, a.cell_shift >= 3, VRHIP_ERR_HIP, "filter: the cells are smaller than a block.");
    }
    const size_t vol_bytes = (size_t)r->nb[0] * r->nb[1] * r->nb[2] * 64 * fmt_bytes(r->format);
    const size_t ws_bytes = kFilterCounters * sizeof(unsigned long long);
    if ((rc = grow(r, r->filter_ws, ws_bytes))) return rc;
    DevBuf<> scratch;   // in place: the result, until it takes the slot's place; freed on every way out
    if (in_place && (rc = grow(r, scratch, vol_bytes))) return rc;
    // the destination, as an upload takes it: the sharers, the slot, what is stale from here on.  (The slots may move:
    // the source is looked up afterwards.  The cells' pairs stay where they are until somebody rebuilds them.)
    const uint32_t res[3] = {r->res[0], r->res[1], r->res[2]};
    VolumeSlot *dst_slot;
    if ((rc = prepare_slot(r, res, r->format, dst_timestep, &dst_slot))) return rc;
    a.vol = make_vol_view(r, r->vols[r->timestep].dev);
    void *dst = in_place ? scratch.p : dst_slot->dev.p;
    VR_HIP(r, hipMemsetAsync(r->filter_ws.p, 0, ws_bytes, r->stream));
    VR_HIP(r, vr_launch_filter(a, dst, r->filter_ws, r->stream));
    unsigned long long c[kFilterCounters];
    VR_HIP(r, hipMemcpyAsync(c, r->filter_ws.p, ws_bytes, hipMemcpyDeviceToHost, r->stream));
    if (in_place && !r->sharers.empty())   // (they hold the slot's address: the bytes move, not the slot)
        VR_HIP(r, hipMemcpyAsync(dst_slot->dev.p, scratch.p, vol_bytes, hipMemcpyDeviceToDevice, r->stream));
    VR_HIP(r, hipStreamSynchronize(r->stream));
    if (in_place && r->sharers.empty()) std::swap(dst_slot->dev, scratch);
    info.blocks = vr_filter_blocks(a.vol);
    info.blocks_fetched = c[kFilterFetched];
    info.blocks_skipped = c[kFilterSkipped];
    info.scratch_bytes = ws_bytes + (in_place ? vol_bytes : 0u);
    info.empty_skip = a.cell_minmax ? 1u : 0u;
    info.in_place = in_place ? 1u : 0u;
    r->filter_info = info;
    r->have_filter_info = true;
    return VRHIP_OK;
}

int vrhip_filter_params_check(const vrhip_filter_params *p)
{
    if (!p) return VRHIP_ERR_INVALID;
    vrhip_renderer scratch;   // (holds the message, owns nothing)
    return filter_check(&scratch, p);
}

int vrhip_filter_gaussian_taps(double sigma, uint32_t radius, float taps[VRHIP_FILTER_MAX_RADIUS + 1])
{
    if (!taps || !std::isfinite(sigma) || !(sigma > 0.0) || radius > VRHIP_FILTER_MAX_RADIUS) return VRHIP_ERR_INVALID;
    double t[VRHIP_FILTER_MAX_RADIUS + 1];
    const double d = 2.0 * sigma * sigma;
    for (uint32_t k = 0; k <= radius; ++k) t[k] = std::exp(-((double)k * (double)k) / d);
    double tail = 0.0;
    for (uint32_t k = 1; k <= radius; ++k) tail = tail + t[k];
    const double sum = t[0] + 2.0 * tail;
    for (uint32_t k = 0; k <= VRHIP_FILTER_MAX_RADIUS; ++k) taps[k] = k <= radius ? (float)(t[k] / sum) : 0.f;
    return VRHIP_OK;
}

int vrhip_last_filter_info(const vrhip_renderer *r, vrhip_filter_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_filter_info) return fail(r, VRHIP_ERR_NODATA, "vrhip_last_filter_info: no filter has run yet");
    *out = r->filter_info;
    return VRHIP_OK;
}

} // extern "C"
