// A caller of the volume statistics through the C++ class, compiled against include/ ALONE (tests/test_gpu_stats.py):
// VolumeRenderCL::volumeStatistics on the whole volume with moments and a 2-D table, and on a region with a 1-D one.
// Writes to argv[1], raw, per call: the six counts (uint64), min and max (float32), sum and sum_sq (float64), then the
// table (uint64, bins_g * bins_v).
#include <volumerendercl.h>

#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        VolumeRenderCL vr;
        vr.initialize(false, false);
        vr.loadSyntheticVolume("shells", 32, DatRawReader::UCHAR);
        static_assert(sizeof(vrhip_stats_params) == 64 && sizeof(vrhip_volume_stats) == 72 && sizeof(vrhip_stats_info) == 48,
                      "64, 72 and 48 bytes");
        VolumeRenderCL::stats_params whole;
        whole.vBins = 64;
        whole.gBins = 16;
        whole.gHi = 0.5f;
        whole.moments = true;
        VolumeRenderCL::stats_params part;
        part.vBins = 256;
        part.vLo = 0.1f;
        part.vHi = 0.9f;
        part.region.lo = {{3u, 5u, 2u}};
        part.region.hi = {{29u, 30u, 31u}};
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        auto put = [&](const void *p, size_t size, size_t n) { return std::fwrite(p, size, n, f) == n; };
        for (const VolumeRenderCL::stats_params *sp : {&whole, &part}) {
            const VolumeRenderCL::volume_stats st = vr.volumeStatistics(*sp);
            if (st.hist.size() != size_t(sp->vBins) * sp->gBins) return 5;
            const uint64_t counts[6] = {st.voxels, st.nan, st.below, st.above, st.gradientNan, st.binned};
            if (!put(counts, 8, 6) || !put(&st.min, 4, 1) || !put(&st.max, 4, 1) || !put(&st.sum, 8, 1) || !put(&st.sumSq, 8, 1) ||
                !put(st.hist.data(), 8, st.hist.size()))
                return 4;
        }
        std::fclose(f);
        VolumeRenderCL::stats_params bad;
        bad.vBins = 0;
        try {
            (void)vr.volumeStatistics(bad);
            return 6;
        } catch (const std::invalid_argument &) {
        }
        std::printf("ok\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
