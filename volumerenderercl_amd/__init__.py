"""volumerenderercl_amd -- MI355X-native (gfx950, hand-written HIP) replacement for the
ray-cast hot path of vbruder/VolumeRendererCL, behind the reference's VolumeRenderCL
interface.  The product is `libvrhip.so` (csrc/, C ABI in include/vrhip.h); this package is
the thin host-side mirror used by tests, bench.py and the multi-GPU tile driver."""
from . import _lib, frontend
from ._lib import (CameraParams, DepthInfo, DepthParams, IndexedMeshInfo, IsoParams, MeshInfo, MeshParams, PathtraceParams, RaycastParams, RenderingParams, SliceParams, Stats,
                   UCHAR, USHORT, FLOAT, TECH_RAYCAST, TECH_PATHTRACE, TECH_MIP, TECH_ISO, TECH_TF2D, TECH_PREINT)
from .renderer import VolumeRenderCL

__all__ = ["VolumeRenderCL", "frontend", "_lib", "CameraParams", "RenderingParams",
           "RaycastParams", "PathtraceParams", "IsoParams", "SliceParams", "DepthParams", "DepthInfo", "MeshParams", "MeshInfo", "IndexedMeshInfo", "Stats", "UCHAR", "USHORT", "FLOAT",
           "TECH_RAYCAST", "TECH_PATHTRACE", "TECH_MIP", "TECH_ISO", "TECH_TF2D", "TECH_PREINT"]
