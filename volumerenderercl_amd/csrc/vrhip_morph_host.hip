// vrhip_morph_host.hip -- the host-only functions of the volume morphology (include/vrhip.h "volume morphology"):
// vrhip_morph_params_check and vrhip_morph_element, on the element test the kernel uses (vr_morph_math.h).  Plain
// C++, no HIP header: tests/test_morph_abi.py builds this file with a C++ compiler and the host sanitizers too.
#include <cstdint>

#include "../../include/vrhip.h"
#include "vr_morph_math.h"

static_assert(morph::kMaxRadius == VRHIP_MORPH_MAX_RADIUS && morph::kBox == VRHIP_MORPH_BOX && morph::kBall == VRHIP_MORPH_BALL &&
                  VRHIP_MORPH_BLACKHAT == 6,
              "vr_morph_math.h states the header's constants");
static_assert(sizeof(vrhip_morph_params) == 32 && sizeof(vrhip_morph_info) == 72, "the sizes the header states");

extern "C" {

int vrhip_morph_params_check(const vrhip_morph_params *p)
{
    if (!p) return VRHIP_ERR_INVALID;
    return morph::params_problem(p->op, p->shape, p->radius, p->reserved) ? VRHIP_ERR_INVALID : VRHIP_OK;
}

int vrhip_morph_element(const vrhip_morph_params *p, int8_t *offsets_xyz, uint32_t capacity, uint32_t *n)
{
    if (!p || !n || (!offsets_xyz && capacity)) return VRHIP_ERR_INVALID;
    if (vrhip_morph_params_check(p) != VRHIP_OK) return VRHIP_ERR_INVALID;
    const int R[3] = {(int)p->radius[0], (int)p->radius[1], (int)p->radius[2]};
    uint32_t count = 0;
    for (int dz = -R[2]; dz <= R[2]; ++dz)
        for (int dy = -R[1]; dy <= R[1]; ++dy) {
            const int h = morph::half_width(p->shape, p->radius, dy, dz);
            if (h >= 0) count += (uint32_t)(2 * h + 1);
        }
    *n = count;
    if (capacity < count) return VRHIP_ERR_INVALID;
    int8_t *o = offsets_xyz;
    for (int dz = -R[2]; dz <= R[2]; ++dz)
        for (int dy = -R[1]; dy <= R[1]; ++dy) {
            const int h = morph::half_width(p->shape, p->radius, dy, dz);   // (the runs the kernel walks)
            for (int dx = -h; dx <= h; ++dx) {
                *o++ = (int8_t)dx;
                *o++ = (int8_t)dy;
                *o++ = (int8_t)dz;
            }
        }
    return VRHIP_OK;
}

} // extern "C"
