// vrhip_tf2d_api.hip -- the host-only functions of technique 6's contract (include/vrhip.h "technique == 6"):
// vrhip_tf2d_params_check, vrhip_tf2d_lookup and vrhip_tf2d_build_ramp.  No renderer, no device, no HIP call: plain
// C++ that a C++ compiler builds as well (tests/cxx/tf2d_host_main.cpp runs it under the host sanitizers).  fp32, one
// rounded operation per line of the header's statement (the library is built without contraction); the lookup is
// vr_tf2d.hip's tf2d_lookup on the RGBA8 table.  vrhip_set_transfer_function_2d is vrhip_api.hip's.
#include <cmath>
#include <cstdint>

#include "../../include/vrhip.h"

namespace {

// tff_coord (vr_sampling.h): every x outside [-1, 2] reads what -1 or 2 reads, a NaN reads -1
float coord(float x)
{
    const float c = x > -1.0f ? x : -1.0f;
    return c < 2.0f ? c : 2.0f;
}

int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

float lerpf(float p, float q, float w) { return std::fmaf(w, q - p, p); }

// tff_linear's index arithmetic on an axis of n entries
void axis(float x, uint32_t n, int *i0, int *i1, float *w)
{
    const float ub = coord(x) * (float)n - 0.5f;
    const float fl = std::floor(ub);
    *w = ub - fl;
    const int i = (int)fl;
    *i0 = clampi(i, 0, (int)n - 1);
    *i1 = clampi(i + 1, 0, (int)n - 1);
}

} // namespace

extern "C" {

int vrhip_tf2d_params_check(uint32_t n_v, uint32_t n_g, float g_hi)
{
    if (n_v < 1 || n_v > VRHIP_TF2D_MAX_NV || n_g < 1 || n_g > VRHIP_TF2D_MAX_NG ||
        (uint64_t)n_v * n_g > VRHIP_TF2D_MAX_ENTRIES)
        return VRHIP_ERR_INVALID;
    if (!std::isfinite(g_hi) || !(g_hi > 0.f)) return VRHIP_ERR_INVALID;
    return VRHIP_OK;
}

int vrhip_tf2d_lookup(const uint8_t *rgba8, uint32_t n_v, uint32_t n_g, float g_hi, float s, float m, float out_rgba[4])
{
    if (!rgba8 || !out_rgba || vrhip_tf2d_params_check(n_v, n_g, g_hi)) return VRHIP_ERR_INVALID;
    int i0, i1, j0, j1;
    float a, b;
    axis(s, n_v, &i0, &i1, &a);
    const float inv_ghi = 1.0f / g_hi;
    axis(m * inv_ghi, n_g, &j0, &j1, &b);
    for (int ch = 0; ch < 4; ++ch) {
        const float e00 = (float)rgba8[4 * ((size_t)j0 * n_v + i0) + ch] / 255.0f;
        const float e01 = (float)rgba8[4 * ((size_t)j0 * n_v + i1) + ch] / 255.0f;
        const float e10 = (float)rgba8[4 * ((size_t)j1 * n_v + i0) + ch] / 255.0f;
        const float e11 = (float)rgba8[4 * ((size_t)j1 * n_v + i1) + ch] / 255.0f;
        out_rgba[ch] = lerpf(lerpf(e00, e01, a), lerpf(e10, e11, a), b);
    }
    return VRHIP_OK;
}

int vrhip_tf2d_build_ramp(const uint8_t *tf1d_rgba8, uint32_t n_v, uint32_t n_g, float g_hi, float g0, float g1,
                          uint8_t *out_rgba8)
{
    if (!tf1d_rgba8 || !out_rgba8 || vrhip_tf2d_params_check(n_v, n_g, g_hi)) return VRHIP_ERR_INVALID;
    if (!std::isfinite(g0) || !std::isfinite(g1) || !(g0 >= 0.f) || !(g1 > g0)) return VRHIP_ERR_INVALID;
    const float span = g1 - g0;
    for (uint32_t j = 0; j < n_g; ++j) {
        const float gj = (((float)j + 0.5f) * g_hi) / (float)n_g;
        const float w = (gj - g0) / span;
        const float wj = w < 0.f ? 0.f : (w > 1.f ? 1.f : w);
        for (uint32_t i = 0; i < n_v; ++i) {
            const uint8_t *src = tf1d_rgba8 + 4 * (size_t)i;
            uint8_t *dst = out_rgba8 + 4 * ((size_t)j * n_v + i);
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            const float x = (float)src[3] * wj;
            const float q = std::floor(x);
            dst[3] = (uint8_t)(q + (x - q >= 0.5f ? 1.0f : 0.0f));
        }
    }
    return VRHIP_OK;
}

} // extern "C"
