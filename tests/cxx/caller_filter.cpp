// A caller of the volume filters through the C++ class, compiled against include/ ALONE (tests/test_gpu_filter.py):
// a synthetic volume smoothed in place with gaussianFilter, then medianFilter, then filterVolume with explicit taps
// into a new time step.  Writes to argv[1], raw, after each of the three: the 256-bin histogram of the filtered step
// (uint64) and the info block (blocks, fetched, skipped, scratch bytes: uint64; empty skip, in place: uint32).
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
        static_assert(sizeof(vrhip_filter_params) == 140 && sizeof(vrhip_filter_info) == 40, "140 and 40 bytes");
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        auto put = [&](const void *p, size_t size, size_t n) { return std::fwrite(p, size, n, f) == n; };
        auto report = [&]() {
            const VolumeRenderCL::volume_stats st = vr.volumeStatistics(VolumeRenderCL::stats_params());
            const VolumeRenderCL::filter_info fi = vr.lastFilterInfo();
            const uint64_t words[4] = {fi.blocks, fi.blocksFetched, fi.blocksSkipped, fi.scratchBytes};
            const uint32_t flags[2] = {fi.emptySkip ? 1u : 0u, fi.inPlace ? 1u : 0u};
            return st.hist.size() == 256 && put(st.hist.data(), 8, 256) && put(words, 8, 4) && put(flags, 4, 2);
        };
        vr.gaussianFilter(1.5);
        if (!report()) return 4;
        vr.medianFilter();
        if (!report()) return 4;
        VolumeRenderCL::FilterParams fp;
        fp.radius = {{1u, 0u, 2u}};
        fp.taps[0] = {{0.5f, 0.25f}};
        fp.taps[1] = {{1.f}};
        fp.taps[2] = {{0.5f, 0.5f, -0.25f}};
        vr.filterVolume(fp, 1);   // a new step
        vr.setTimestep(1);
        if (vr.getTimestep() != 1 || !report()) return 4;
        std::fclose(f);
        VolumeRenderCL::FilterParams bad;
        bad.radius = {{9u, 0u, 0u}};
        try {
            vr.filterVolume(bad, 0);
            return 6;
        } catch (const std::invalid_argument &) {
        }
        try {
            vr.filterVolume(fp, 3);   // above the number of steps
            return 7;
        } catch (const std::invalid_argument &) {
        }
        std::printf("ok\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
