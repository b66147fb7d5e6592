// vrhip_preint_api.hip -- the host-only functions of technique 8's contract (include/vrhip.h "technique == 8"):
// vrhip_preint_tables, the integral table and the prefix count the renderer uploads, and vrhip_preint_slab, the slab
// classification.  No renderer, no device, no HIP call: plain C++ that a C++ compiler builds as well
// (tests/cxx/preint_host_main.cpp runs it under the host sanitizers).  The arithmetic is vr_preint_math.h's, the very
// text the kernel compiles (the library is built without contraction).
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/vrhip.h"
#include "vr_preint_math.h"

extern "C" {

int vrhip_preint_tables(const float *tff_rgba, uint32_t n, double *prefix, uint32_t *nz)
{
    if (!tff_rgba || !prefix || !nz || n < 1 || n > VRHIP_PREINT_MAX_ENTRIES) return VRHIP_ERR_INVALID;
    for (uint32_t i = 0; i < 4 * n; ++i)
        if (!(tff_rgba[i] >= 0.0f && tff_rgba[i] <= 1.0f)) return VRHIP_ERR_INVALID;
    preint::build_tables(tff_rgba, (int)n, prefix, nz);
    return VRHIP_OK;
}

int vrhip_preint_slab(const float *tff_rgba, uint32_t n, int raw, float sf, float sb, float out[4])
{
    if (!tff_rgba || !out || n < 1 || n > VRHIP_PREINT_MAX_ENTRIES) return VRHIP_ERR_INVALID;
    // a value that is not RAW is a normalised one: inside [-1, 2], where tff_coord's clamp changes nothing
    if (!raw && !(sf >= -1.0f && sf <= 2.0f && sb >= -1.0f && sb <= 2.0f)) return VRHIP_ERR_INVALID;
    std::vector<double> prefix(4 * (size_t)n);
    std::vector<uint32_t> nz(n + 1);
    if (vrhip_preint_tables(tff_rgba, n, prefix.data(), nz.data())) return VRHIP_ERR_INVALID;
    const float ua = preint::table_coord(raw != 0, sf, (int)n), ub = preint::table_coord(raw != 0, sb, (int)n);
    preint::slab(tff_rgba, prefix.data(), (int)n, ua, ub, out);
    return VRHIP_OK;
}

} // extern "C"
