// vr_raycast_int.hip -- the ray-cast kernels for the integer voxel types, UCHAR and USHORT: this unit's instantiations
// of vr_raycast_kernels.h.  The two share a unit on purpose: compiled in a unit of their own, ten USHORT kernels (the
// 4-wave footprint variants of phase 1 on the ray list and of phase 2) come out with another scalar register
// allocation than behind the UCHAR kernels -- see DESIGN.md "Build".
#include "vr_raycast_kernels.h"

hipError_t vr_launch_raycast_u8(const RaycastLaunch &a, hipStream_t stream)
{
    return a.frame.cams ? launch_typed<uint8_t, true>(a, stream) : launch_typed<uint8_t, false>(a, stream);
}

hipError_t vr_launch_raycast_u16(const RaycastLaunch &a, hipStream_t stream)
{
    return a.frame.cams ? launch_typed<uint16_t, true>(a, stream) : launch_typed<uint16_t, false>(a, stream);
}

#if defined(VR_MARCH_STATS) || defined(VR_STAMPS)
int vr_raycast_debug_int(int which, unsigned long long *sum, size_t n, int reset) { return debug_add(which, sum, n, reset); }
#endif
