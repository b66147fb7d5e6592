// A caller of the slice views through the C++ class, compiled against include/ ALONE (tests/test_gpu_slice.py):
// VolumeRenderCL::axisSlice / planeSlice / sliceStack build six slices, renderSlices renders them in one call between
// two progressive ray-cast frames of the same renderer.  Writes to argv[1]: the six 80-byte parameter blocks, then the
// six slice images and the two frames, raw float32.
#include <volumerendercl.h>

#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const size_t W = 37, H = 21;
        VolumeRenderCL vr;
        vr.initialize(false, false);
        vr.loadSyntheticVolume("sphere", 32, DatRawReader::UCHAR);
        std::vector<unsigned char> tff(256 * 4, 0);
        for (size_t i = 0; i < 256; ++i) {
            tff[4 * i] = (unsigned char)i;
            tff[4 * i + 1] = (unsigned char)(255 - i);
            tff[4 * i + 2] = 40;
            tff[4 * i + 3] = (unsigned char)i;
        }
        vr.setTransferFunction(tff);
        vr.updateSamplingRate(1.5);
        vr.updateOutputImg(W, H, 0);
        vr.updateView({{2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1}});
        vr.setSeed(77);
        static_assert(sizeof(VolumeRenderCL::slice_params) == 80, "vrhip_slice_params is 80 bytes");
        std::vector<VolumeRenderCL::slice_params> slices;
        slices.push_back(VolumeRenderCL::axisSlice(2, 0.1f));
        slices.push_back(VolumeRenderCL::axisSlice(0, -0.3f, 0.5f, 5, VolumeRenderCL::SLICE_MEAN, VolumeRenderCL::SLICE_VALUE));
        slices.push_back(VolumeRenderCL::planeSlice({{0.1f, 0.f, -0.1f}}, {{1.f, 1.f, 1.f}}, {{0.f, 0.f, 1.f}}, 0.9f, 0.8f, 0.3f, 4,
                                                    VolumeRenderCL::SLICE_MIN));
        for (const auto &s : VolumeRenderCL::sliceStack(VolumeRenderCL::axisSlice(1, 0.f), 3, 2.f)) slices.push_back(s);
        std::vector<float> a, b, img;
        vr.runRaycastNoGL(W, H, a);          // iteration 0
        vr.renderSlices(W, H, slices, img);
        vr.runRaycastNoGL(W, H, b);          // iteration 1: accumulates on a
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        if (std::fwrite(slices.data(), sizeof(slices[0]), slices.size(), f) != slices.size()) return 4;
        if (img.size() != slices.size() * W * H * 4 || a.size() != W * H * 4 || b.size() != W * H * 4) return 4;
        for (const std::vector<float> *v : {&img, &a, &b})
            if (std::fwrite(v->data(), sizeof(float), v->size(), f) != v->size()) return 4;
        std::fclose(f);
        std::printf("%zu slices\n", slices.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
