// A caller of technique 8 (pre-integrated classification), compiled against include/ ALONE (tests/test_preint_abi.py):
// the C++ mirror's technique constant and host-only slab, and the C ABI's two host-only entry points.  Compiled only;
// the C++ route is run on a GPU through vrhip_render --preint (tests/test_gpu_preint.py).
#include <volumerendercl.h>

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
        std::vector<unsigned char> tff(256 * 4, 0);
        for (int i = 127; i < 129; ++i) tff[4 * i + 0] = tff[4 * i + 3] = 255;
        vr.setTransferFunction(tff);
        vr.setTechnique(VolumeRenderCL::TECH_PREINT);
        static_assert(VolumeRenderCL::TECH_PREINT == VRHIP_TECHNIQUE_PREINT, "the mirror's value is the C ABI's");
        static_assert(VRHIP_TECHNIQUE_PREINT == 8u, "technique 8");
        std::vector<float> image;
        vr.runRaycastNoGL(40, 32, image);
        const std::array<float, 4> c = VolumeRenderCL::preintSlab(tff, 0.2f, 0.8f);
        // the C ABI directly
        std::vector<float> entries(tff.size());
        for (size_t i = 0; i < tff.size(); ++i) entries[i] = float(tff[i]) / 255.0f;
        float d[4];
        if (vrhip_preint_slab(entries.data(), 256u, 0, 0.2f, 0.8f, d) != VRHIP_OK) return 3;
        std::vector<double> prefix(4 * 256);
        std::vector<uint32_t> nz(257);
        if (vrhip_preint_tables(entries.data(), 256u, prefix.data(), nz.data()) != VRHIP_OK) return 3;
        std::printf("%zu floats, abar %g %g, %u entries show\n", image.size(), double(c[3]), double(d[3]), nz[256]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
