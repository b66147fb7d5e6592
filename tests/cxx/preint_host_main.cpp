// The host-only functions of technique 8 (vrhip_preint_api.hip: vrhip_preint_tables, vrhip_preint_slab) in a
// stand-alone program, for the host sanitizers (tests/test_preint_abi.py builds this file and vrhip_preint_api.hip
// with -fsanitize=address,undefined and runs it): table sizes 1, 2, 256 and 4096, slabs inside, across and beyond
// the table, reversed, RAW values with infinities and NaN, and the refusals.
#include <vrhip.h>

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    unsigned long slabs = 0;
    uint32_t state = 12345u;
    auto rnd = [&state]() { state = state * 1664525u + 1013904223u; return float(state >> 8) / 16777216.0f; };
    for (uint32_t n : {1u, 2u, 256u, 4096u}) {
        std::vector<float> tff(4 * size_t(n));
        for (float &v : tff) v = std::floor(rnd() * 256.0f) / 255.0f > 1.0f ? 1.0f : std::floor(rnd() * 255.0f) / 255.0f;
        for (uint32_t i = 0; i < n; i += 3) tff[4 * i + 3] = 0.0f;
        std::vector<double> prefix(4 * size_t(n));
        std::vector<uint32_t> nz(n + 1);
        if (vrhip_preint_tables(tff.data(), n, prefix.data(), nz.data()) != VRHIP_OK) return 1;
        for (uint32_t i = 1; i < n; ++i)
            for (int c = 0; c < 4; ++c)
                if (!(prefix[4 * i + c] >= prefix[4 * (i - 1) + c])) return 2;   // non-decreasing
        if (nz[n] > n) return 2;
        float out[4];
        const float special[] = {-inf, -3e38f, -2.0f, -1.0f, -0.0f, 0.0f, 0.5f, 1.0f, 2.0f, 3e38f, inf, nan};
        for (float sf : special)
            for (float sb : special) {
                if (vrhip_preint_slab(tff.data(), n, 1, sf, sb, out) != VRHIP_OK) return 3;
                for (float v : out) if (!(v >= 0.0f) || !std::isfinite(v)) return 4;
                ++slabs;
            }
        for (int k = 0; k < 2000; ++k) {
            const float sf = rnd() * 1.4f - 0.2f, sb = k % 5 ? rnd() * 1.4f - 0.2f : std::nextafter(sf, 2.0f);
            if (vrhip_preint_slab(tff.data(), n, k & 1, sf, sb, out) != VRHIP_OK) return 3;
            if (vrhip_preint_slab(tff.data(), n, k & 1, sb, sf, out) != VRHIP_OK) return 3;
            if (!(out[3] >= 0.0f && out[3] <= 1.0f)) return 4;
            slabs += 2;
        }
        if (vrhip_preint_slab(tff.data(), n, 0, 0.0f, 2.5f, out) != VRHIP_ERR_INVALID) return 5;
        if (vrhip_preint_slab(tff.data(), n, 0, nan, 0.5f, out) != VRHIP_ERR_INVALID) return 5;
        tff[1] = 1.5f;
        if (vrhip_preint_slab(tff.data(), n, 0, 0.0f, 1.0f, out) != VRHIP_ERR_INVALID) return 5;
    }
    float out[4];
    const float one[4] = {1, 1, 1, 1};
    if (vrhip_preint_slab(nullptr, 1, 0, 0.f, 1.f, out) != VRHIP_ERR_INVALID) return 6;
    if (vrhip_preint_slab(one, 0, 0, 0.f, 1.f, out) != VRHIP_ERR_INVALID) return 6;
    if (vrhip_preint_slab(one, 4097, 0, 0.f, 1.f, out) != VRHIP_ERR_INVALID) return 6;
    if (vrhip_preint_slab(one, 1, 0, 0.f, 1.f, nullptr) != VRHIP_ERR_INVALID) return 6;
    if (vrhip_preint_tables(one, 1, nullptr, nullptr) != VRHIP_ERR_INVALID) return 6;
    std::printf("preint host functions: ok (%lu slabs)\n", slabs);
    return 0;
}
