// A caller of the volume morphology through the C++ class, compiled against include/ ALONE (tests/test_gpu_morph.py):
// a synthetic volume opened in place with open(2), then closed with a box (close(1, false)), then morphVolume with an
// anisotropic gradient into a new time step.  Writes to argv[1], raw, after each of the three: the 256-bin histogram
// of the written step (uint64) and the info block (per sweep blocks, fetched, skipped, then scratch bytes: uint64;
// sweeps, empty skip, in place: uint32).
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
        static_assert(sizeof(vrhip_morph_params) == 32 && sizeof(vrhip_morph_info) == 72, "32 and 72 bytes");
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        auto put = [&](const void *p, size_t size, size_t n) { return std::fwrite(p, size, n, f) == n; };
        auto report = [&]() {
            const VolumeRenderCL::volume_stats st = vr.volumeStatistics(VolumeRenderCL::stats_params());
            const VolumeRenderCL::morph_info mi = vr.lastMorphInfo();
            const uint64_t words[7] = {mi.blocks[0], mi.blocksFetched[0], mi.blocksSkipped[0], mi.blocks[1], mi.blocksFetched[1],
                                       mi.blocksSkipped[1], mi.scratchBytes};
            const uint32_t flags[3] = {mi.sweeps, mi.emptySkip ? 1u : 0u, mi.inPlace ? 1u : 0u};
            return st.hist.size() == 256 && put(st.hist.data(), 8, 256) && put(words, 8, 7) && put(flags, 4, 3);
        };
        vr.open(2);
        if (!report()) return 4;
        vr.close(1, false);
        if (!report()) return 4;
        VolumeRenderCL::MorphParams mp;
        mp.op = VolumeRenderCL::MorphOp::Gradient;
        mp.ball = true;
        mp.radius = {{3u, 0u, 1u}};
        vr.morphVolume(mp, 1);   // a new step
        vr.setTimestep(1);
        if (vr.getTimestep() != 1 || !report()) return 4;
        std::fclose(f);
        VolumeRenderCL::MorphParams bad;
        bad.radius = {{9u, 0u, 0u}};
        try {
            vr.morphVolume(bad, 0);
            return 6;
        } catch (const std::invalid_argument &) {
        }
        try {
            vr.morphVolume(mp, 3);   // above the number of steps
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
