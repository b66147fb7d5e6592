// vr_raycast_f32.hip -- the ray-cast kernels for FLOAT volumes: this unit's instantiations of vr_raycast_kernels.h
#include "vr_raycast_kernels.h"

hipError_t vr_launch_raycast_f32(const RaycastLaunch &a, hipStream_t stream)
{
    return a.frame.cams ? launch_typed<float, true>(a, stream) : launch_typed<float, false>(a, stream);
}

#if defined(VR_MARCH_STATS) || defined(VR_STAMPS)
int vr_raycast_debug_f32(int which, unsigned long long *sum, size_t n, int reset) { return debug_add(which, sum, n, reset); }
#endif
