// vrhip_stats_api.hip -- vrhip_volume_statistics, vrhip_last_stats_info and vrhip_stats_params_check (include/vrhip.h
// "volume statistics"): the checks, the cell grid for skipping, the launches (vr_stats.hip) and the copies to the host.  It reads the volume of
// the current time step and the object-ESS switch, and writes only the buffers the renderer keeps for it
// (vr_renderer.h) and the caller's destinations.  (The cell grid it may build is derived state every technique builds
// on demand and reads as it is: vr_renderer.h "derived state".)  Every call counts anew: nothing but allocations is
// kept between calls, so nothing here can go stale.
#include <cmath>
#include <cstdlib>

#include "vr_renderer.h"

namespace {

// the checks that need no volume, in the header's order; k_v, k_g: the scales, computed once in fp32
int stats_check(vrhip_renderer *r, const vrhip_stats_params *p, float *k_v, float *k_g)
{
    VR_REQUIRE(r, p->bins_v >= 1 && p->bins_v <= VRHIP_STATS_MAX_BINS_V && p->bins_g >= 1 && p->bins_g <= VRHIP_STATS_MAX_BINS_G &&
                      (uint64_t)p->bins_v * p->bins_g <= VRHIP_STATS_MAX_BINS,
               VRHIP_ERR_INVALID, "statistics: bins_v must be 1..4096, bins_g 1..256 and their product at most 65536.");
    VR_REQUIRE(r, std::isfinite(p->v_lo) && std::isfinite(p->v_hi) && p->v_hi > p->v_lo, VRHIP_ERR_INVALID,
               "statistics: v_lo and v_hi must be finite, v_lo < v_hi.");
    const volatile float span = p->v_hi - p->v_lo;   // (volatile: rounded to fp32 here, whatever the host's flags)
    const volatile float kv = (float)p->bins_v / span;
    VR_REQUIRE(r, std::isfinite((float)span) && std::isfinite((float)kv), VRHIP_ERR_INVALID,
               "statistics: bins_v / (v_hi - v_lo) is not finite in fp32.");
    *k_v = kv;
    *k_g = 0.f;
    if (p->bins_g > 1) {
        VR_REQUIRE(r, std::isfinite(p->g_hi) && p->g_hi > 0.f, VRHIP_ERR_INVALID,
                   "statistics: g_hi must be finite and positive when bins_g > 1.");
        const volatile float kg = (float)p->bins_g / p->g_hi;
        VR_REQUIRE(r, std::isfinite((float)kg), VRHIP_ERR_INVALID, "statistics: bins_g / g_hi is not finite in fp32.");
        *k_g = kg;
    }
    VR_REQUIRE(r, !(p->flags & ~VRHIP_STATS_MOMENTS), VRHIP_ERR_INVALID, "statistics: unknown flags.");
    VR_REQUIRE(r, !(p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]), VRHIP_ERR_INVALID,
               "statistics: reserved must be 0.");
    return VRHIP_OK;
}

// the largest table the workgroups keep in LDS: kStatsLdsBins, or VRHIP_STATS_LDS_BINS below it (A/B runs; 0: none)
uint32_t stats_lds_bins()
{
    if (const char *ev = getenv("VRHIP_STATS_LDS_BINS")) {
        const long v = atol(ev);
        if (v >= 0 && v < (long)kStatsLdsBins) return (uint32_t)v;
    }
    return kStatsLdsBins;
}

} // namespace

extern "C" {

int vrhip_volume_statistics(vrhip_renderer *r, const vrhip_stats_params *p, vrhip_volume_stats *out, uint64_t *hist,
                            int hist_is_device)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, p && out && hist, VRHIP_ERR_INVALID, "vrhip_volume_statistics: NULL argument");
    StatsLaunch a;
    std::memset(&a, 0, sizeof a);
    int rc;
    if ((rc = stats_check(r, p, &a.k_v, &a.k_g))) return rc;
    VR_REQUIRE(r, !hist_is_device || ((uintptr_t)hist & 15u) == 0, VRHIP_ERR_INVALID,
               "vrhip_volume_statistics: a device destination must be 16-byte aligned.");
    VR_REQUIRE(r, !r->vols.empty() && r->timestep < r->vols.size() && r->vols[r->timestep].dev, VRHIP_ERR_NODATA,
               "No volume data is loaded.");
    VR_REQUIRE(r, r->channels == 1, VRHIP_ERR_UNSUPPORTED, "statistics: RG / RGBA volumes are not supported.");
    const bool whole = !(p->lo[0] | p->lo[1] | p->lo[2] | p->hi[0] | p->hi[1] | p->hi[2]);
    bool voxels = true;
    uint64_t n_voxels = 1;
    for (int i = 0; i < 3; ++i) {
        uint32_t lo = 0, hi = r->res[i];
        if (!whole) {
            lo = p->lo[i];
            hi = p->hi[i];
            VR_REQUIRE(r, hi != 0 && hi <= r->res[i] && lo <= hi, VRHIP_ERR_INVALID,
                       "statistics: the region is not a box inside the volume.");
        }
        if (hi <= lo) voxels = false;
        a.lo[i] = lo;
        a.hi[i] = hi;
        n_voxels *= hi - lo;
    }
    const bool moments = (p->flags & VRHIP_STATS_MOMENTS) != 0;
    const size_t n_bins = (size_t)p->bins_v * p->bins_g, hist_bytes = n_bins * sizeof(uint64_t);
    if (set_device(r)) return VRHIP_ERR_HIP;
    r->have_stats_info = false;
    vrhip_stats_info info;
    std::memset(&info, 0, sizeof info);
    std::memset(out, 0, sizeof *out);
    if (moments) {
        out->min = INFINITY;
        out->max = -INFINITY;
    }

    unsigned long long *hist_dev = reinterpret_cast<unsigned long long *>(hist);
    if (!hist_is_device) {
        if ((rc = grow(r, r->stats_hist_dev, hist_bytes))) return rc;
        hist_dev = r->stats_hist_dev.p;
    }
    VR_HIP(r, hipMemsetAsync(hist_dev, 0, hist_bytes, r->stream));
    info.hist_path = n_bins <= stats_lds_bins() ? VRHIP_STATS_PATH_LDS : VRHIP_STATS_PATH_GLOBAL;
    if (voxels) {
        for (int i = 0; i < 3; ++i) {
            a.b0[i] = a.lo[i] / VRHIP_MESH_BLOCK;
            a.nb[i] = (a.hi[i] - 1u) / VRHIP_MESH_BLOCK - a.b0[i] + 1u;
        }
        a.vol = make_vol_view(r, r->vols[r->timestep].dev);
        a.format = r->format;
        a.bins_v = p->bins_v;
        a.bins_g = p->bins_g;
        a.v_lo = p->v_lo;
        a.v_hi = p->v_hi;
        a.moments = moments;
        a.lds_hist = info.hist_path == VRHIP_STATS_PATH_LDS;
        a.num_cus = r->num_cus;
        if (mip_skips(r)) {   // object-order ESS: the coarse cells' (min, max), which need no transfer function
            if ((rc = ensure_cells(r, true, false, false))) return rc;
            a.cell_minmax = cell_minmax_of(r, false);
            VR_REQUIRE(r, a.cell_minmax, VRHIP_ERR_HIP, "statistics: the cells' (min, max) were not built.");
            a.cell_shift = r->cells.shift;
            a.cell_cx = r->cells.cx;
            a.cell_cy = r->cells.cy;
            VR_REQUIRE(r, a.cell_shift >= 3, VRHIP_ERR_HIP, "statistics: the cells are smaller than a block.");
        }
        const size_t n_blocks = (size_t)a.nb[0] * a.nb[1] * a.nb[2], n_chunks = vr_stats_chunks(n_blocks);
        VR_REQUIRE(r, n_blocks < 0x7fffffffull, VRHIP_ERR_UNSUPPORTED, "statistics: too many blocks for one launch.");
        // the counters, and behind them the call's moments
        const size_t ws_bytes = kStatsCounters * sizeof(unsigned long long) + sizeof(StatsRec);
        if ((rc = grow(r, r->stats_ws, ws_bytes))) return rc;
        if (moments && (rc = grow(r, r->stats_chunks, n_chunks * sizeof(StatsRec)))) return rc;
        if ((rc = grow_pinned(r, r->stats_host, ws_bytes + (hist_is_device ? 0u : hist_bytes)))) return rc;
        StatsRec *total = reinterpret_cast<StatsRec *>(r->stats_ws.p + kStatsCounters);
        VR_HIP(r, hipMemsetAsync(r->stats_ws.p, 0, ws_bytes, r->stream));
        VR_HIP(r, vr_launch_stats(a, hist_dev, r->stats_ws, moments ? r->stats_chunks.p : nullptr, r->stream));
        if (moments) VR_HIP(r, vr_launch_stats_total(r->stats_chunks, n_chunks, total, r->stream));
        VR_HIP(r, hipMemcpyAsync(r->stats_host.p, r->stats_ws.p, ws_bytes, hipMemcpyDeviceToHost, r->stream));
        if (!hist_is_device)
            VR_HIP(r, hipMemcpyAsync((uint8_t *)r->stats_host.p + ws_bytes, hist_dev, hist_bytes, hipMemcpyDeviceToHost,
                                     r->stream));
        VR_HIP(r, hipStreamSynchronize(r->stream));
        const unsigned long long *c = (const unsigned long long *)r->stats_host.p;
        out->voxels = n_voxels;
        out->nan = c[kStatsNan];
        out->below = c[kStatsBelow];
        out->above = c[kStatsAbove];
        out->gradient_nan = c[kStatsGradNan];
        out->binned = c[kStatsBinned];
        if (moments) {
            StatsRec t;
            std::memcpy(&t, c + kStatsCounters, sizeof t);
            out->min = t.mn;
            out->max = t.mx;
            out->sum = t.sum;
            out->sum_sq = t.sum_sq;
        }
        if (!hist_is_device) std::memcpy(hist, (const uint8_t *)r->stats_host.p + ws_bytes, hist_bytes);
        info.blocks = n_blocks;
        info.blocks_fetched = c[kStatsFetched];
        info.blocks_skipped_constant = c[kStatsSkipConst];
        info.blocks_skipped_window = c[kStatsSkipWindow];
        info.scratch_bytes = ws_bytes + (moments ? n_chunks * sizeof(StatsRec) : 0u);
        info.empty_skip = a.cell_minmax ? 1u : 0u;
    } else {   // a region without a voxel: the table of zeros
        if (hist_is_device) VR_HIP(r, hipStreamSynchronize(r->stream));
        else std::memset(hist, 0, hist_bytes);
    }
    r->stats_info = info;
    r->have_stats_info = true;
    return VRHIP_OK;
}

int vrhip_stats_params_check(const vrhip_stats_params *p)
{
    if (!p) return VRHIP_ERR_INVALID;
    vrhip_renderer scratch;   // (holds the message, owns nothing)
    float k_v, k_g;
    return stats_check(&scratch, p, &k_v, &k_g);
}

int vrhip_last_stats_info(const vrhip_renderer *r, vrhip_stats_info *out)
{
    if (!r || !out) return VRHIP_ERR_INVALID;
    if (!r->have_stats_info) return fail(r, VRHIP_ERR_NODATA, "vrhip_last_stats_info: no statistics have been computed yet");
    *out = r->stats_info;
    return VRHIP_OK;
}

} // extern "C"
