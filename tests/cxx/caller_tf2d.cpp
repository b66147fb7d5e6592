// A caller of technique 6 (2-D transfer function), compiled against include/ ALONE (tests/test_tf2d_abi.py): the
// C++ mirror's ramp table and setter, and the C ABI's four entry points.  Compiled only; it is never run without a GPU.
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
        std::vector<unsigned char> tff(256 * 4, 200);
        const unsigned int nG = 8;
        const float gHi = 0.25f;
        const std::vector<unsigned char> table = VolumeRenderCL::rampTransferFunction2D(tff, nG, gHi, 0.02f, 0.1f);
        vr.setTransferFunction2D(table, 256u, nG, gHi);
        vr.setTechnique(VolumeRenderCL::TECH_TF2D);
        static_assert(VolumeRenderCL::TECH_TF2D == VRHIP_TECHNIQUE_TF2D, "the mirror's value is the C ABI's");
        std::vector<float> image;
        vr.runRaycastNoGL(64, 48, image);
        // the C ABI directly
        float c[4];
        if (vrhip_tf2d_params_check(256u, nG, gHi) != VRHIP_OK) return 3;
        if (vrhip_tf2d_lookup(table.data(), 256u, nG, gHi, 0.5f, 0.05f, c) != VRHIP_OK) return 3;
        std::vector<unsigned char> again(table.size());
        if (vrhip_tf2d_build_ramp(tff.data(), 256u, nG, gHi, 0.02f, 0.1f, again.data()) != VRHIP_OK) return 3;
        if (vrhip_set_transfer_function_2d(vr.handle(), again.data(), 256u, nG, gHi) != VRHIP_OK) return 3;
        std::printf("%zu floats, alpha %g\n", image.size(), double(c[3]));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
