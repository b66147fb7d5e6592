// A caller of the maximum intensity projection through the C++ class, compiled against include/ ALONE
// (tests/test_gpu_mip.py): VolumeRenderCL::setTechnique(TECH_MIP), two frames in a row from one renderer (a
// projection does not accumulate: the second is iteration 0 like the first), with and without object-order ESS,
// then a ray-cast frame from the same renderer.  Writes the three frames, raw float32, to argv[1].
#include <volumerendercl.h>

#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const size_t W = 56, H = 40;
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
        vr.setIllumination(1);   // ignored by the projection
        vr.updateSamplingRate(1.5);
        vr.updateOutputImg(W, H, 0);
        vr.updateView({{2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1}});
        vr.setSeed(77);
        vr.setTechnique(VolumeRenderCL::TECH_MIP);
        std::vector<float> a, b, c;
        vr.setObjEss(true);
        vr.runRaycastNoGL(W, H, a);
        vr.setObjEss(false);
        vr.runRaycastNoGL(W, H, b);
        vr.setObjEss(true);
        vr.setTechnique(VolumeRenderCL::TECH_RAYCAST);
        vr.runRaycastNoGL(W, H, c);
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        for (const std::vector<float> *v : {&a, &b, &c})
            if (v->size() != W * H * 4 || std::fwrite(v->data(), sizeof(float), v->size(), f) != v->size()) return 4;
        std::fclose(f);
        std::printf("%zu floats per frame\n", a.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
