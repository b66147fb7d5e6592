// A stand-alone program around the host-only functions of technique 6 (volumerenderercl_amd/csrc/vrhip_tf2d_api.hip),
// for the host sanitizers: tests/test_tf2d_abi.py compiles that file as C++ together with this one with
// -fsanitize=address,undefined and runs the result.  No device, no library: every table size at its limits, every
// kind of coordinate, exact-size buffers on the heap so that one entry too far is an error the sanitizer reports.
#include <vrhip.h>

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const unsigned sizes[][2] = {{1, 1}, {2, 1}, {1, 256}, {7, 5}, {256, 256}, {4096, 16}};
    const float coords[] = {-inf, -3.e38f, -1.5f, -1.f, -0.f, 0.f, 1.e-45f, 0.07f, 0.5f, 0.999999f, 1.f, 1.5f, 2.f, 7.f, 3.e38f, inf, nan};
    unsigned long long sum = 0;
    for (const auto &sz : sizes) {
        const unsigned nv = sz[0], ng = sz[1];
        std::vector<unsigned char> tf1(4 * size_t(nv)), table(4 * size_t(nv) * ng);
        for (size_t i = 0; i < tf1.size(); ++i) tf1[i] = (unsigned char)((i * 37u + 11u) & 255u);
        for (float ghi : {1.e-30f, 0.25f, 3.e38f}) {
            if (vrhip_tf2d_params_check(nv, ng, ghi) != VRHIP_OK) return 1;
            if (vrhip_tf2d_build_ramp(tf1.data(), nv, ng, ghi, 0.f, ghi, table.data()) != VRHIP_OK) return 1;
            if (vrhip_tf2d_build_ramp(tf1.data(), nv, ng, ghi, ghi * 0.25f, ghi * 0.5f, table.data()) != VRHIP_OK) return 1;
            for (float s : coords)
                for (float m : coords) {
                    float c[4];
                    if (vrhip_tf2d_lookup(table.data(), nv, ng, ghi, s, m, c) != VRHIP_OK) return 1;
                    for (float v : c) {
                        if (!(v >= 0.f && v <= 1.f)) return 2;   // a blend of entries in [0, 1], never a NaN
                        sum += (unsigned long long)(v * 255.f);
                    }
                }
        }
    }
    // what is refused is refused before anything is read or written
    float c[4] = {9.f, 9.f, 9.f, 9.f};
    unsigned char one[4] = {1, 2, 3, 4};
    if (vrhip_tf2d_params_check(0, 1, 1.f) != VRHIP_ERR_INVALID || vrhip_tf2d_params_check(4097, 1, 1.f) != VRHIP_ERR_INVALID ||
        vrhip_tf2d_params_check(1, 257, 1.f) != VRHIP_ERR_INVALID || vrhip_tf2d_params_check(4096, 17, 1.f) != VRHIP_ERR_INVALID ||
        vrhip_tf2d_params_check(1, 1, 0.f) != VRHIP_ERR_INVALID || vrhip_tf2d_params_check(1, 1, nan) != VRHIP_ERR_INVALID)
        return 3;
    if (vrhip_tf2d_lookup(nullptr, 1, 1, 1.f, 0.f, 0.f, c) != VRHIP_ERR_INVALID || vrhip_tf2d_lookup(one, 1, 1, inf, 0.f, 0.f, c) != VRHIP_ERR_INVALID ||
        vrhip_tf2d_lookup(one, 1, 1, 1.f, 0.f, 0.f, nullptr) != VRHIP_ERR_INVALID || c[0] != 9.f)
        return 3;
    if (vrhip_tf2d_build_ramp(one, 1, 1, 1.f, 0.5f, 0.5f, one) != VRHIP_ERR_INVALID || vrhip_tf2d_build_ramp(one, 1, 1, 1.f, -0.1f, 0.5f, one) != VRHIP_ERR_INVALID ||
        vrhip_tf2d_build_ramp(one, 1, 1, 1.f, 0.f, inf, one) != VRHIP_ERR_INVALID || one[3] != 4)
        return 3;
    std::printf("tf2d host functions: ok (%llu)\n", sum);
    return 0;
}
