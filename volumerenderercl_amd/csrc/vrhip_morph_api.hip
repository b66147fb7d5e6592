// vrhip_morph_api.hip -- vrhip_morph_volume and vrhip_last_morph_info (include/vrhip.h "volume morphology"; the two
// host-only functions are vrhip_morph_host.hip's): the checks, the cell grid for skipping, the destination slot
// (prepare_slot, as an upload takes it), the intermediate and the in-place scratch, the one or two launches
// (vr_morph.hip) and the counters.  It reads the volume of the current time step and the object-ESS switch and writes
// the voxels of the destination step; what depends on those voxels goes stale as after an upload (vr_renderer.h
// "derived state").
#include <utility>

#include "vr_morph_math.h"
#include "vr_renderer.h"

namespace {

// the checks that need no volume, in the header's order (vr_morph_math.h)
int morph_check(vrhip_renderer *r, const vrhip_morph_params *p)
{
    const char *problem = morph::params_problem(p->op, p->shape, p->radius, p->reserved);
    VR_REQUIRE(r, !problem, VRHIP_ERR_INVALID, problem);
    return VRHIP_OK;
}

// the modes of an op's sweeps; the second is -1 for a one-sweep op
void morph_modes(uint32_t op, int mode[2])
{
    switch (op) {
    case VRHIP_MORPH_ERODE: mode[0] = kMorphMin, mode[1] = -1; break;
    case VRHIP_MORPH_DILATE: mode[0] = kMorphMax, mode[1] = -1; break;
    case VRHIP_MORPH_GRADIENT: mode[0] = kMorphMaxMin, mode[1] = -1; break;
    case VRHIP_MORPH_OPEN: mode[0] = kMorphMin, mode[1] = kMorphMax; break;
    case VRHIP_MORPH_CLOSE: mode[0] = kMorphMax, mode[1] = kMorphMin; break;
    case VRHIP_MORPH_TOPHAT: mode[0] = kMorphMin, mode[1] = kMorphFMinusMax; break;
    default: mode[0] = kMorphMax, mode[1] = kMorphMinMinusF; break;   // BLACKHAT
    }
}

} // namespace

extern "C" {

int vrhip_morph_volume(vrhip_renderer *r, const vrhip_morph_params *p, uint32_t dst_timestep)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p, VRHIP_ERR_INVALID, "vrhip_morph_volume: NULL argument");
    int rc;
    if ((rc = morph_check(r, p))) return rc;
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "morph: RG / RGBA volumes are not supported.");
    for (const VolumeSlot &s : r->vols)   // (before anything is touched: prepare_slot would clear a sharer)
        VR_REQUIRE(r, !s.borrowed, VRHIP_ERR_UNSUPPORTED, "morph: this renderer's volumes belong to another renderer.");
    VR_REQUIRE(r, dst_timestep <= r->vols.size(), VRHIP_ERR_INVALID, "morph: dst_timestep is above the number of time steps.");
    if (set_device(r)) return VRHIP_ERR_HIP;
    r->have_morph_info = false;
    vrhip_morph_info info;
    std::memset(&info, 0, sizeof info);
    const bool in_place = dst_timestep == r->timestep;
    int mode[2];
    morph_modes(p->op, mode);
    const bool two = mode[1] >= 0;
    // OPEN / CLOSE in place without sharers: the second sweep reads the intermediate alone and writes the slot itself
    const bool direct = in_place && two && (p->op == VRHIP_MORPH_OPEN || p->op == VRHIP_MORPH_CLOSE) && r->sharers.empty();

    MorphLaunch a;
    std::memset(&a, 0, sizeof a);
    a.format = r->format;
    a.shape = p->shape;
    for (int i = 0; i < 3; ++i) a.radius[i] = p->radius[i];
    a.num_cus = r->num_cus;
    if (mip_skips(r)) {   // object-order ESS: the coarse cells' (min, max) of the source, built before it may go stale
        if ((rc = ensure_cells(r, true, false, false))) return rc;
        a.cell_minmax = cell_minmax_of(r, false);
        VR_REQUIRE(r, a.cell_minmax, VRHIP_ERR_HIP, "morph: the cells' (min, max) were not built.");
        a.cell_shift = r->cells.shift;
        a.cell_cx = r->cells.cx;
        a.cell_cy = r->cells.cy;
        a.cell_cz = r->cells.cz;
        VR_REQUIRE(r, a.cell_shift >= 3, VRHIP_ERR_HIP, "morph: the cells are smaller than a block.");
    }
    const size_t vol_bytes = (size_t)r->nb[0] * r->nb[1] * r->nb[2] * 64 * fmt_bytes(r->format);
    const size_t ws_bytes = 2 * kMorphCounters * sizeof(unsigned long long);
    if ((rc = grow(r, r->morph_ws, ws_bytes))) return rc;
    DevBuf<> mid, result;   // the intermediate; in place: the result, until it takes the slot's place.  Freed on every way out
    if (two && (rc = grow(r, mid, vol_bytes))) return rc;
    if (in_place && !direct && (rc = grow(r, result, vol_bytes))) return rc;
    // the destination, as an upload takes it: the sharers, the slot, what is stale from here on.  (The slots may move:
    // the source is looked up afterwards.  The cells' pairs stay where they are until somebody rebuilds them.)
    const uint32_t res[3] = {r->res[0], r->res[1], r->res[2]};
    VolumeSlot *dst_slot;
    if ((rc = prepare_slot(r, res, r->format, dst_timestep, &dst_slot))) return rc;
    const VolView source = make_vol_view(r, r->vols[r->timestep].dev);
    void *dst = in_place && !direct ? result.p : dst_slot->dev.p;
    VR_HIP(r, hipMemsetAsync(r->morph_ws.p, 0, ws_bytes, r->stream));
    a.vol = source;
    a.mode = (uint32_t)mode[0];
    a.skip_scale = 1u;
    VR_HIP(r, vr_launch_morph(a, two ? mid.p : dst, r->morph_ws, r->stream));
    if (two) {
        a.vol.data = mid.p;   // (the source's layout and type)
        a.mode = (uint32_t)mode[1];
        a.f = mode[1] == kMorphFMinusMax || mode[1] == kMorphMinMinusF ? source.data : nullptr;
        a.skip_scale = 2u;
        VR_HIP(r, vr_launch_morph(a, dst, r->morph_ws.p + kMorphCounters, r->stream));
    }
    unsigned long long c[2 * kMorphCounters];
    VR_HIP(r, hipMemcpyAsync(c, r->morph_ws.p, ws_bytes, hipMemcpyDeviceToHost, r->stream));
    if (in_place && !direct && !r->sharers.empty())   // (they hold the slot's address: the bytes move, not the slot)
        VR_HIP(r, hipMemcpyAsync(dst_slot->dev.p, result.p, vol_bytes, hipMemcpyDeviceToDevice, r->stream));
    VR_HIP(r, hipStreamSynchronize(r->stream));
    if (in_place && !direct && r->sharers.empty()) std::swap(dst_slot->dev, result);
    info.sweeps = two ? 2u : 1u;
    for (uint32_t s = 0; s < info.sweeps; ++s) {
        info.sweep[s].blocks = vr_filter_blocks(source);
        info.sweep[s].blocks_fetched = c[s * kMorphCounters + kMorphFetched];
        info.sweep[s].blocks_skipped = c[s * kMorphCounters + kMorphSkipped];
    }
    info.scratch_bytes = ws_bytes + ((two ? 1u : 0u) + (in_place && !direct ? 1u : 0u)) * vol_bytes;
    info.empty_skip = a.cell_minmax ? 1u : 0u;
    info.in_place = in_place ? 1u : 0u;
    r->morph_info = info;
    r->have_morph_info = true;
    return VRHIP_OK;
}

int vrhip_last_morph_info(const vrhip_renderer *r, vrhip_morph_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_morph_info) return fail(r, VRHIP_ERR_NODATA, "vrhip_last_morph_info: no morphology call has run yet");
    *out = r->morph_info;
    return VRHIP_OK;
}

} // extern "C"
