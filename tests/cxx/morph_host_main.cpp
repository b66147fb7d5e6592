// The host-only functions of the volume morphology (vrhip_morph_host.hip: vrhip_morph_params_check,
// vrhip_morph_element) in a stand-alone program, for the host sanitizers (tests/test_morph_abi.py builds this file and
// vrhip_morph_host.hip with -fsanitize=address,undefined and runs it): every radius triple 0..8 of both shapes into a
// buffer of exactly the element's size (a write past it is the sanitizer's to find), the quoted counts, symmetry, the
// order, the capacity-too-small return and the refusals.
#include <vrhip.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static vrhip_morph_params make(uint32_t shape, uint32_t rx, uint32_t ry, uint32_t rz)
{
    vrhip_morph_params p;
    std::memset(&p, 0, sizeof p);
    p.op = VRHIP_MORPH_ERODE;
    p.shape = shape;
    p.radius[0] = rx;
    p.radius[1] = ry;
    p.radius[2] = rz;
    return p;
}

int main()
{
    unsigned long elements = 0;
    for (uint32_t shape : {uint32_t(VRHIP_MORPH_BOX), uint32_t(VRHIP_MORPH_BALL)})
        for (uint32_t rz = 0; rz <= 8; ++rz)
            for (uint32_t ry = 0; ry <= 8; ++ry)
                for (uint32_t rx = 0; rx <= 8; ++rx) {
                    const vrhip_morph_params p = make(shape, rx, ry, rz);
                    if (vrhip_morph_params_check(&p) != VRHIP_OK) return 1;
                    uint32_t n = 0;
                    const int rc0 = vrhip_morph_element(&p, nullptr, 0, &n);   // the count alone
                    if (rc0 != VRHIP_ERR_INVALID || n == 0) return 2;
                    if (shape == VRHIP_MORPH_BOX && n != (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1)) return 3;
                    std::vector<int8_t> e(3 * size_t(n));
                    uint32_t m = 0;
                    if (n > 1) {   // one too few: refused, nothing written
                        std::vector<int8_t> small(3 * size_t(n - 1), int8_t(99));
                        if (vrhip_morph_element(&p, small.data(), n - 1, &m) != VRHIP_ERR_INVALID || m != n) return 4;
                        for (int8_t v : small) if (v != 99) return 4;
                    }
                    if (vrhip_morph_element(&p, e.data(), n, &m) != VRHIP_OK || m != n) return 5;
                    bool centre = false;
                    for (uint32_t i = 0; i < n; ++i) {
                        const int dx = e[3 * i], dy = e[3 * i + 1], dz = e[3 * i + 2];
                        if (std::abs(dx) > int(rx) || std::abs(dy) > int(ry) || std::abs(dz) > int(rz)) return 6;
                        centre = centre || (!dx && !dy && !dz);
                        const uint32_t j = n - 1 - i;   // z, y, x ascending and symmetric: the mirror image reversed
                        if (e[3 * j] != -dx || e[3 * j + 1] != -dy || e[3 * j + 2] != -dz) return 7;
                        if (i) {
                            const int px = e[3 * i - 3], py = e[3 * i - 2], pz = e[3 * i - 1];
                            if (!(pz < dz || (pz == dz && (py < dy || (py == dy && px < dx))))) return 8;
                        }
                    }
                    if (!centre) return 9;
                    ++elements;
                }
    const uint32_t quoted[][4] = {{1, 1, 1, 7}, {2, 2, 2, 33}, {4, 4, 4, 257}, {8, 8, 8, 2109}, {2, 0, 3, 19}, {0, 0, 0, 1}};
    for (const auto &q : quoted) {
        const vrhip_morph_params p = make(VRHIP_MORPH_BALL, q[0], q[1], q[2]);
        uint32_t n = 0;
        vrhip_morph_element(&p, nullptr, 0, &n);
        if (n != q[3]) return 10;
    }
    // the refusals
    uint32_t n = 0;
    int8_t buf[3];
    vrhip_morph_params p = make(VRHIP_MORPH_BALL, 0, 0, 0);
    if (vrhip_morph_params_check(nullptr) != VRHIP_ERR_INVALID) return 11;
    if (vrhip_morph_element(nullptr, buf, 1, &n) != VRHIP_ERR_INVALID || vrhip_morph_element(&p, buf, 1, nullptr) != VRHIP_ERR_INVALID ||
        vrhip_morph_element(&p, nullptr, 1, &n) != VRHIP_ERR_INVALID)
        return 11;
    if (vrhip_morph_element(&p, buf, 1, &n) != VRHIP_OK || n != 1 || buf[0] || buf[1] || buf[2]) return 11;
    p.op = 7;
    if (vrhip_morph_params_check(&p) != VRHIP_ERR_INVALID) return 12;
    p = make(2, 1, 1, 1);
    if (vrhip_morph_params_check(&p) != VRHIP_ERR_INVALID || vrhip_morph_element(&p, buf, 1, &n) != VRHIP_ERR_INVALID) return 12;
    for (int a = 0; a < 3; ++a) {
        p = make(VRHIP_MORPH_BOX, 1, 1, 1);
        p.radius[a] = 9;
        if (vrhip_morph_params_check(&p) != VRHIP_ERR_INVALID) return 13;
        p.radius[a] = 0xffffffffu;
        if (vrhip_morph_params_check(&p) != VRHIP_ERR_INVALID || vrhip_morph_element(&p, buf, 1, &n) != VRHIP_ERR_INVALID) return 13;
        p = make(VRHIP_MORPH_BOX, 1, 1, 1);
        p.reserved[a] = 1;
        if (vrhip_morph_params_check(&p) != VRHIP_ERR_INVALID) return 14;
    }
    std::printf("morph host functions: ok (%lu elements)\n", elements);
    return 0;
}
