// A caller of the progressive path tracer's many-samples call, compiled against include/ ALONE
// (tests/test_samples_abi.py): 16 samples per pixel into host memory, into device memory and for a tile subset.
// Compiled only; it is never run without a GPU.
#include <volumerendercl.h>

#include <cstdlib>
#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        VolumeRenderCL vr;
        vr.initialize(false, false);
        DatRawReader::Properties props;
        props.dat_file_name = argv[1];
        vr.loadVolumeData(props);
        std::vector<unsigned char> tff(1024 * 4, 0);
        for (size_t i = 0; i < 1024; ++i) tff[4 * i + 3] = (unsigned char)(i / 4);
        vr.setTransferFunction(tff);
        vr.setTechnique(VolumeRenderCL::TECH_PATHTRACE);
        const size_t W = 64, H = 48;
        const std::vector<unsigned int> seeds = vr.drawSeeds(16);
        std::vector<float> image;
        vr.renderSamples(W, H, seeds, image);                 // iterations 0..15, the library's set size
        float *dev = nullptr;   // caller-owned device memory: W x H RGBA floats
        if (argc > 2) dev = reinterpret_cast<float *>(std::strtoull(argv[2], nullptr, 16));
        vr.renderSamples(W, H, vr.drawSeeds(16), dev, 4u);    // iterations 16..31 in sets of 4
        vr.renderSamples(W, H, 16, 16, std::vector<unsigned int>{0, 1}, vr.drawSeeds(8), dev);
        vrhip_launch_info li;
        if (vrhip_last_launch_info(vr.handle(), &li) != VRHIP_OK || !li.samples) return 3;
        std::printf("%zu floats, iteration %u\n", image.size(), vr.renderingParams().iteration);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
