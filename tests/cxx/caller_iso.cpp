// A caller of the first-hit isosurface through the C++ class, compiled against include/ ALONE
// (tests/test_gpu_iso.py): VolumeRenderCL::setTechnique(TECH_ISO) with setIsoValue / setIsoRefinement, two shaded
// frames in a row from one renderer (an isosurface does not accumulate: the second is iteration 0 like the first),
// with and without object-order ESS, a flat frame, then a ray-cast frame from the same renderer.  Writes the four
// frames, raw float32, to argv[1].
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
        vr.setIllumination(1);
        vr.updateSamplingRate(1.5);
        vr.updateOutputImg(W, H, 0);
        vr.updateView({{2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1}});
        vr.setSeed(77);
        vr.setTechnique(VolumeRenderCL::TECH_ISO);
        vr.setIsoValue(0.4f);
        vr.setIsoRefinement(6);
        std::vector<float> a, b, c, d;
        vr.setObjEss(true);
        vr.runRaycastNoGL(W, H, a);
        vr.setObjEss(false);
        vr.runRaycastNoGL(W, H, b);
        vr.setObjEss(true);
        vr.setIllumination(0);
        vr.runRaycastNoGL(W, H, c);
        vr.setIllumination(1);
        vr.setTechnique(VolumeRenderCL::TECH_RAYCAST);
        vr.runRaycastNoGL(W, H, d);
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        for (const std::vector<float> *v : {&a, &b, &c, &d})
            if (v->size() != W * H * 4 || std::fwrite(v->data(), sizeof(float), v->size(), f) != v->size()) return 4;
        std::fclose(f);
        std::printf("%zu floats per frame\n", a.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
