// A caller of the throughput path with per-frame cameras, compiled against include/ ALONE (tests/test_views.py): a
// turntable of views rendered as one launch set, through a renderer and through a twin that shares its volume.
// Compiled only; it is never run without a GPU.
#include <volumerendercl.h>

#include <cmath>
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
        const size_t n = 8, W = 64, H = 48;
        std::vector<std::array<float, 16>> views(n);
        for (size_t k = 0; k < n; ++k) {   // rotation about y by k * 45 degrees, 2 units from the centre
            const float a = float(k) * 0.785398163f, c = std::cos(a), s = std::sin(a);
            views[k] = {{2 * c, 0, 2 * s, 2 * s, 0, 2, 0, 0, -2 * s, 0, 2 * c, 2 * c, 0, 0, 0, 1}};
        }
        const std::vector<unsigned int> seeds = vr.drawSeeds(n);
        float *dev = nullptr;   // caller-owned device memory: n frames of W x H RGBA floats
        if (argc > 2) dev = reinterpret_cast<float *>(std::strtoull(argv[2], nullptr, 16));
        vr.renderFrames(W, H, seeds, views, dev);
        std::unique_ptr<VolumeRenderCL> twin = vr.shareVolumes();
        twin->renderFramesTiles(W, H, 16, 16, std::vector<unsigned int>{0, 1}, seeds, views, dev, W * H);
        std::printf("%zu views\n", views.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
