// vrhip_ingest_api.hip -- the device-side ingest entry points of the C ABI (include/vrhip.h) over the kernels of
// vr_ingest.hip: vrhip_ingest_raw, vrhip_volume_histogram, vrhip_last_ingest_seconds.
#include <algorithm>
#include <string>

#include "vr_renderer.h"
#include "vr_ingest.h"

namespace {

constexpr size_t kIngestHistOffset = 16;   // bytes: the maximum word sits in front of the counters
constexpr size_t kIngestWsBytes = kIngestHistOffset + 256 * sizeof(unsigned long long);

int ensure_ingest_ws(vrhip_renderer *r)
{
    const int rc = grow(r, r->ingest_ws, kIngestWsBytes);
    if (rc) return rc;
    if (!r->evi0) VR_HIP(r, hipEventCreate(&r->evi0.h));
    if (!r->evi1) VR_HIP(r, hipEventCreate(&r->evi1.h));
    return VRHIP_OK;
}

unsigned long long *ingest_hist(const vrhip_renderer *r)
{
    return reinterpret_cast<unsigned long long *>(static_cast<char *>(r->ingest_ws.p) + kIngestHistOffset);
}

// waits for the stream and adds the time between the two ingest events to *seconds
hipError_t ingest_elapsed(vrhip_renderer *r, double *seconds)
{
    hipError_t e = hipStreamSynchronize(r->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, r->evi0, r->evi1);
    if (e == hipSuccess) *seconds += (double)ms * 1e-3;
    return e;
}

// the counters, as the doubles the loader keeps
hipError_t ingest_read_hist(vrhip_renderer *r, double hist[256])
{
    unsigned long long h[256];
    hipError_t e = hipMemcpyAsync(h, ingest_hist(r), sizeof h, hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e == hipSuccess)
        for (int i = 0; i < 256; ++i) hist[i] = (double)h[i];
    return e;
}

// The two passes of vrhip_ingest_raw over a prepared slot; `stage` holds stage_bytes of interleaved staging
// followed (channels > 1) by the planar staging of `channels` planes of plane_stride elements.
hipError_t ingest_passes(vrhip_renderer *r, VolumeSlot *s, const char *raw, size_t bytes, int format, int channels,
                         int big_endian, int slab, char *stage, size_t stage_bytes, size_t plane_stride,
                         double hist[256], float *max_value, double *seconds)
{
    const size_t bpv = fmt_bytes(format);
    const size_t slice_texels = (size_t)r->res[0] * r->res[1], slice_b = slice_texels * bpv * (size_t)channels;
    const size_t need = slice_b * r->res[2];
    // what the loader's flat loops run over: every whole word of the file, the ones beyond the volume included
    const size_t tail_words = bytes / bpv - need / bpv, stage_words = stage_bytes / bpv;
    uint32_t *max_dev = static_cast<uint32_t *>(r->ingest_ws.p);
    hipStream_t st = r->stream;
    void *planes[4] = {s->dev, s->chan[0], s->chan[1], s->chan[2]};
    char *planar = stage + stage_bytes;
    hipError_t e = hipSuccess;
#define VR_TRY(call)                                  \
    do {                                              \
        if ((e = (call)) != hipSuccess) return e;     \
    } while (0)
    // the words beyond the volume, stage_words at a time, each piece handed to fn(words in the piece)
    auto for_tail = [&](auto fn) -> hipError_t {
        for (size_t w0 = 0; w0 < tail_words; w0 += stage_words) {
            const size_t nw = std::min(stage_words, tail_words - w0);
            VR_TRY(hipMemcpyAsync(stage, raw + need + w0 * bpv, nw * bpv, hipMemcpyHostToDevice, st));
            VR_TRY(hipEventRecord(r->evi0, st));
            VR_TRY(fn(nw));
            VR_TRY(hipEventRecord(r->evi1, st));
            VR_TRY(ingest_elapsed(r, seconds));   // (the staging buffer is reused)
        }
        return hipSuccess;
    };

    // ---- pass 1, slab by slab: copy, maximum, de-interleave, re-tile the raw words
    const uint32_t max_init = vr_ingest_max_init(format);
    VR_TRY(hipMemcpyAsync(max_dev, &max_init, sizeof max_init, hipMemcpyHostToDevice, st));
    VR_TRY(hipStreamSynchronize(st));   // (max_init leaves the stack)
    for (int z0 = 0; z0 < (int)r->res[2]; z0 += slab) {
        const int nz = std::min<int>(slab, (int)r->res[2] - z0);
        const size_t texels = (size_t)nz * slice_texels;
        VR_TRY(hipMemcpyAsync(stage, raw + (size_t)z0 * slice_b, (size_t)nz * slice_b, hipMemcpyHostToDevice, st));
        VR_TRY(hipEventRecord(r->evi0, st));
        VR_TRY(vr_launch_ingest_max(stage, texels * (size_t)channels, format, big_endian, max_dev, r->num_cus, st));
        if (channels > 1) {
            VR_TRY(vr_launch_deinterleave(stage, planar, plane_stride, texels, format, channels, st));
            for (int c = 0; c < channels; ++c)
                VR_TRY(vr_launch_retile(make_vol_view(r, planes[c]), format, planar + (size_t)c * plane_stride * bpv, z0,
                                        nz, true, st));
        } else {
            VR_TRY(vr_launch_retile(make_vol_view(r, s->dev), format, stage, z0, nz, true, st));
        }
        VR_TRY(hipEventRecord(r->evi1, st));
        VR_TRY(ingest_elapsed(r, seconds));
    }
    VR_TRY(for_tail([&](size_t nw) { return vr_launch_ingest_max(stage, nw, format, big_endian, max_dev, r->num_cus, st); }));
    uint32_t max_word = 0;
    VR_TRY(hipMemcpyAsync(&max_word, max_dev, sizeof max_word, hipMemcpyDeviceToHost, st));
    VR_TRY(hipStreamSynchronize(st));
    IngestParams p;
    p.max_value = vr_ingest_max_decode(format, max_word);
    p.stretch = 65535.f / p.max_value;   // datrawreader.cpp: numeric_limits<unsigned short>::max() / float(max)
    p.big_endian = big_endian;

    // ---- pass 2: convert in place and count
    VR_TRY(hipMemsetAsync(ingest_hist(r), 0, 256 * sizeof(unsigned long long), st));
    VR_TRY(hipEventRecord(r->evi0, st));
    for (int c = 0; c < channels; ++c)
        VR_TRY(vr_launch_ingest_convert(make_vol_view(r, planes[c]), format, p, 1, ingest_hist(r), r->num_cus, st));
    VR_TRY(hipEventRecord(r->evi1, st));
    VR_TRY(ingest_elapsed(r, seconds));
    VR_TRY(for_tail([&](size_t nw) { return vr_launch_ingest_count(stage, nw, format, p, ingest_hist(r), r->num_cus, st); }));
    VR_TRY(ingest_read_hist(r, hist));
#undef VR_TRY
    *max_value = p.max_value;
    return hipSuccess;
}

} // namespace

extern "C" {

int vrhip_ingest_raw(vrhip_renderer *r, const void *raw, size_t bytes, const uint32_t res[3], int format, int channels,
                     int big_endian, uint32_t timestep, double hist[256], float *max_value)
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, raw && hist && max_value, VRHIP_ERR_INVALID, "vrhip_ingest_raw: NULL pointer");
    VR_REQUIRE(r, channels == 1 || channels == 2 || channels == 4, VRHIP_ERR_INVALID,
               "Unknown or invalid volume color format.");   // volumerendercl.cpp:711
    VR_REQUIRE(r, res && res[0] && res[1] && res[2], VRHIP_ERR_INVALID, "Volume resolution must be non-zero.");
    VR_REQUIRE(r, format >= VRHIP_UCHAR && format <= VRHIP_FLOAT, VRHIP_ERR_INVALID,
               "Unknown or invalid volume data format.");
    const size_t bpv = fmt_bytes(format);
    const size_t slice_texels = (size_t)res[0] * res[1], slice_b = slice_texels * bpv * (size_t)channels;
    VR_REQUIRE(r, bytes / slice_b >= res[2], VRHIP_ERR_INVALID,
               "Volume size does not match size specified in dat file.");   // volumerendercl.cpp:740-742
    if (set_device(r)) return VRHIP_ERR_HIP;
    VolumeSlot *s;
    int rc = prepare_slot(r, res, format, timestep, &s, channels);
    if (rc) return rc;
    if ((rc = ensure_ingest_ws(r))) return rc;
    // slabs of whole multiples of 4 slices (micro-brick rows are written whole), at least 4
    int slab = (int)std::max<size_t>(4, r->ingest_slab_bytes / slice_b / 4 * 4);
    slab = std::min<int>(slab, (int)((res[2] + 3) / 4 * 4));
    const size_t stage_bytes = ((size_t)slab * slice_b + 15) / 16 * 16;
    const size_t per16 = 16 / bpv;
    const size_t plane_stride = channels > 1 ? ((size_t)slab * slice_texels + per16 - 1) / per16 * per16 : 0;
    void *stage = nullptr;
    VR_HIP(r, hipMalloc(&stage, stage_bytes + (size_t)channels * plane_stride * bpv));
    double seconds = 0.0;
    const hipError_t e = ingest_passes(r, s, static_cast<const char *>(raw), bytes, format, channels, big_endian ? 1 : 0,
                                       slab, static_cast<char *>(stage), stage_bytes, plane_stride, hist, max_value,
                                       &seconds);
    (void)hipFree(stage);
    if (e != hipSuccess)
        return fail(r, VRHIP_ERR_HIP, std::string("ERROR: vrhip_ingest_raw (") + hipGetErrorString(e) + ")");
    r->ingest_seconds = seconds;
    return VRHIP_OK;
}

int vrhip_volume_histogram(vrhip_renderer *r, uint32_t timestep, double hist[256])
{
    if (!r) return VRHIP_ERR_INVALID;
    VR_REQUIRE(r, timestep < r->vols.size() && r->vols[timestep].dev, VRHIP_ERR_NODATA, "No volume data is loaded.");
    VR_REQUIRE(r, hist, VRHIP_ERR_INVALID, "vrhip_volume_histogram: NULL pointer");
    if (set_device(r)) return VRHIP_ERR_HIP;
    int rc = ensure_ingest_ws(r);
    if (rc) return rc;
    const VolumeSlot &s = r->vols[timestep];
    const void *planes[4] = {s.dev, s.chan[0], s.chan[1], s.chan[2]};
    const IngestParams p = {1.f, 1.f, 0};
    VR_HIP(r, hipMemsetAsync(ingest_hist(r), 0, 256 * sizeof(unsigned long long), r->stream));
    for (int c = 0; c < r->channels; ++c)
        VR_HIP(r, vr_launch_ingest_convert(make_vol_view(r, planes[c]), r->format, p, 0, ingest_hist(r), r->num_cus,
                                           r->stream));
    VR_HIP(r, ingest_read_hist(r, hist));
    return VRHIP_OK;
}

double vrhip_last_ingest_seconds(const vrhip_renderer *r) { return r ? r->ingest_seconds : 0.0; }

} // extern "C"
