// vr_morph_math.h -- the structuring element and the keys of the volume morphology (vrhip_morph_volume,
// include/vrhip.h "volume morphology"), written once for the host (vrhip_morph_api.hip:
// vrhip_morph_element, vrhip_morph_params_check) and for the device (vr_morph.hip).  Plain C++: no HIP header, no
// library call, so that a C++ compiler builds it for the stand-alone sanitizer program as well.
// tests/ref/morph_ref.c restates these lines in C.
//
// Element.  B holds the integer offsets (dx, dy, dz) with |d_a| <= R_a; BOX takes all of them, BALL those with
//   dx^2 R'y^2 R'z^2 + dy^2 R'x^2 R'z^2 + dz^2 R'x^2 R'y^2 <= R'x^2 R'y^2 R'z^2,   R'_a = max(R_a, 1),
// in integers (R <= 8: the right side is at most 2^18).  B is symmetric and down-closed in every |d_a|, so the row
// (dy, dz) of B is the run dx = -h .. h with h = half_width(dy, dz), or empty (h < 0).
// Keys.  UCHAR / USHORT: the raw integer.  FLOAT: the order-preserving key of the volume filters (vr_filter.hip,
// filter_key / filter_unkey): the sign bit flipped for words with a clear sign bit, all bits for the others, every
// NaN 0xffffffff; the word stored for a key is a NaN as 0x7fc00000 and a zero of either sign as +0.
#ifndef VR_MORPH_MATH_H
#define VR_MORPH_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define VR_MORPH_FN __host__ __device__ inline
#else
#define VR_MORPH_FN inline
#endif

namespace morph {

constexpr uint32_t kMaxRadius = 8u;   // VRHIP_MORPH_MAX_RADIUS
constexpr uint32_t kBox = 0u, kBall = 1u;   // VRHIP_MORPH_BOX, VRHIP_MORPH_BALL

// is (dx, dy, dz) an offset of B?  R[a] <= 8
VR_MORPH_FN bool in_element(uint32_t shape, const uint32_t R[3], int dx, int dy, int dz)
{
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
    if (ax > (int)R[0] || ay > (int)R[1] || az > (int)R[2]) return false;
    if (shape != kBall) return true;
    const uint32_t rx = R[0] ? R[0] : 1u, ry = R[1] ? R[1] : 1u, rz = R[2] ? R[2] : 1u;
    const uint32_t x2 = rx * rx, y2 = ry * ry, z2 = rz * rz;
    return (uint32_t)(ax * ax) * y2 * z2 + (uint32_t)(ay * ay) * x2 * z2 + (uint32_t)(az * az) * x2 * y2 <= x2 * y2 * z2;
}

// the largest dx with (dx, dy, dz) in B, or -1 when the row (dy, dz) holds no offset
VR_MORPH_FN int half_width(uint32_t shape, const uint32_t R[3], int dy, int dz)
{
    int h = -1;
    for (int dx = 0; dx <= (int)R[0]; ++dx) {
        if (!in_element(shape, R, dx, dy, dz)) break;
        h = dx;
    }
    return h;
}

// what vrhip_morph_params_check refuses, in the header's order, or nullptr.  Ops are 0 .. 6 (VRHIP_MORPH_BLACKHAT).
inline const char *params_problem(uint32_t op, uint32_t shape, const uint32_t radius[3], const uint32_t reserved[3])
{
    if (op > 6u) return "morph: unknown op.";
    if (shape != kBox && shape != kBall) return "morph: unknown shape.";
    for (int a = 0; a < 3; ++a)
        if (radius[a] > kMaxRadius) return "morph: a radius above 8.";
    if (reserved[0] | reserved[1] | reserved[2]) return "morph: reserved must be 0.";
    return nullptr;
}

VR_MORPH_FN uint32_t key_of_float(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u;
}
VR_MORPH_FN uint32_t float_of_key(uint32_t key)
{
    if (key == 0xffffffffu) return 0x7fc00000u;
    const uint32_t bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    return bits == 0x80000000u ? 0u : bits;
}

} // namespace morph

#endif
