"""ctypes binding of libvrhip.so (include/vrhip.h).

The HIP library is the product: there is no CPU fallback.  Loading fails loudly when the
in-tree shared library has not been built (`python -c "import __graft_entry__ as g; g.build()"`
or `make -C volumerenderercl_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VRHIP_LIB_PATH selects an alternative build of the same library (tools/mkvariant.sh: -D variants for A/B runs)
LIB_PATH = os.environ.get("VRHIP_LIB_PATH") or os.path.join(_HERE, "libvrhip.so")

OK, ERR_INVALID, ERR_HIP, ERR_NODATA, ERR_UNSUPPORTED = range(5)
UCHAR, USHORT, FLOAT = 0, 1, 2
# rendering_params.technique: ray caster, path tracer, maximum intensity projection (VRHIP_TECHNIQUE_MIP), first-hit
# isosurface (VRHIP_TECHNIQUE_ISO; 3 is unassigned), 2-D transfer function (VRHIP_TECHNIQUE_TF2D; 5 is unassigned)
TECH_RAYCAST, TECH_PATHTRACE, TECH_MIP = 0, 1, 2
TECH_ISO = 4
TECH_TF2D = 6
# pre-integrated classification (VRHIP_TECHNIQUE_PREINT; 7 is unassigned)
TECH_PREINT = 8
# the limits of a 2-D transfer function (vrhip_tf2d_params_check): those of the statistics histogram
TF2D_MAX_NV, TF2D_MAX_NG, TF2D_MAX_ENTRIES = 4096, 256, 65536


class CameraParams(C.Structure):
    """vrhip_camera_params == VolumeRenderCL::camera_params (volumerendercl.h:43-49)."""
    _fields_ = [("viewMat", C.c_float * 16), ("bbox_bl", C.c_float * 4),
                ("bbox_tr", C.c_float * 4), ("ortho", C.c_uint32), ("_pad", C.c_uint32 * 7)]


class RenderingParams(C.Structure):
    """vrhip_rendering_params == VolumeRenderCL::rendering_params (volumerendercl.h:51-66)."""
    _fields_ = [("backgroundColor", C.c_float * 4), ("modelScale", C.c_float * 4),
                ("illumType", C.c_uint32), ("imgEss", C.c_uint32), ("showEss", C.c_uint32),
                ("useLinear", C.c_uint32), ("useGradient", C.c_uint32),
                ("technique", C.c_uint32), ("seed", C.c_uint32), ("iteration", C.c_uint32)]


class RaycastParams(C.Structure):
    """vrhip_raycast_params == VolumeRenderCL::raycast_params (volumerendercl.h:68-76)."""
    _fields_ = [("samplingRate", C.c_float), ("useAO", C.c_uint32), ("contours", C.c_uint32),
                ("aerial", C.c_uint32), ("brickRes", C.c_float * 4)]


class PathtraceParams(C.Structure):
    """vrhip_pathtrace_params == VolumeRenderCL::pathtrace_params (volumerendercl.h:78-81)."""
    _fields_ = [("max_extinction", C.c_float)]


class IsoParams(C.Structure):
    """vrhip_iso_params: the parameters of technique 4 (no reference counterpart)."""
    _fields_ = [("isoValue", C.c_float), ("refineSteps", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# vrhip_slice_params.mode / .output (slice views, vrhip_render_slices)
SLICE_MAX, SLICE_MIN, SLICE_MEAN = 0, 1, 2
SLICE_TF, SLICE_VALUE = 0, 1
SLICE_MAX_SAMPLES = 256


class SliceParams(C.Structure):
    """vrhip_slice_params: one slice view -- a plane or a slab through the box [-1, 1]^3 (no reference counterpart)."""
    _fields_ = [("origin", C.c_float * 4), ("u", C.c_float * 4), ("v", C.c_float * 4), ("w", C.c_float * 4),
                ("samples", C.c_uint32), ("mode", C.c_uint32), ("output", C.c_uint32), ("reserved", C.c_uint32)]


# vrhip_depth_params.mode and the bytes of out_kind (depth images, vrhip_render_depth)
DEPTH_ISO, DEPTH_MAX, DEPTH_OPACITY = 0, 1, 2
DEPTH_MISS, DEPTH_NO_HIT, DEPTH_HIT = 0, 1, 2


class DepthParams(C.Structure):
    """vrhip_depth_params: what a depth image looks for, and the rectangle of the frame it answers."""
    _fields_ = [("mode", C.c_uint32), ("threshold", C.c_float), ("refineSteps", C.c_uint32), ("x0", C.c_uint32),
                ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("reserved", C.c_uint32)]


class DepthInfo(C.Structure):
    """vrhip_depth_info: what the last vrhip_render_depth launched."""
    _fields_ = [("mode", C.c_uint32), ("work_items", C.c_uint32), ("empty_skip", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


# vrhip_mesh_params.normals (isosurface extraction, vrhip_isosurface_extract)
MESH_NORMALS_NONE, MESH_NORMALS_GRADIENT = 0, 1
MESH_BLOCK = 8


class MeshParams(C.Structure):
    """vrhip_mesh_params: the iso value, the normals wanted and the region of an isosurface extraction."""
    _fields_ = [("isoValue", C.c_float), ("normals", C.c_uint32), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3),
                ("reserved", C.c_uint32 * 4)]


class MeshInfo(C.Structure):
    """vrhip_mesh_info: what the last vrhip_isosurface_count / _extract did."""
    _fields_ = [("triangles", C.c_uint64), ("blocks", C.c_uint64), ("blocks_skipped", C.c_uint64),
                ("empty_skip", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class IndexedMeshInfo(C.Structure):
    """vrhip_indexed_mesh_info: what the last vrhip_isosurface_count_indexed / _extract_indexed did."""
    _fields_ = [("vertices", C.c_uint64), ("triangles", C.c_uint64), ("point_blocks", C.c_uint64),
                ("point_blocks_skipped", C.c_uint64), ("blocks", C.c_uint64), ("blocks_skipped", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("empty_skip", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


# vrhip_stats_params.flags, the chunk of the moments' sum and vrhip_stats_info.hist_path (volume statistics,
# vrhip_volume_statistics)
STATS_MOMENTS = 1
STATS_SUM_CHUNK = 256
STATS_PATH_LDS, STATS_PATH_GLOBAL = 0, 1


class StatsParams(C.Structure):
    """vrhip_stats_params: the region, the bins, the window and the flags of a vrhip_volume_statistics call."""
    _fields_ = [("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("bins_v", C.c_uint32), ("bins_g", C.c_uint32),
                ("v_lo", C.c_float), ("v_hi", C.c_float), ("g_hi", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class VolumeStats(C.Structure):
    """vrhip_volume_stats: the counts and the moments of a region."""
    _fields_ = [("voxels", C.c_uint64), ("nan", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64),
                ("gradient_nan", C.c_uint64), ("binned", C.c_uint64), ("min", C.c_float), ("max", C.c_float),
                ("sum", C.c_double), ("sum_sq", C.c_double)]

    def as_dict(self):
        return {n: (float if t in (C.c_float, C.c_double) else int)(getattr(self, n)) for n, t in self._fields_}


class StatsInfo(C.Structure):
    """vrhip_stats_info: what the last vrhip_volume_statistics did."""
    _fields_ = [("blocks", C.c_uint64), ("blocks_fetched", C.c_uint64), ("blocks_skipped_constant", C.c_uint64),
                ("blocks_skipped_window", C.c_uint64), ("scratch_bytes", C.c_uint64), ("empty_skip", C.c_uint32),
                ("hist_path", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# vrhip_filter_params.kind and the largest radius (volume filters, vrhip_filter_volume)
FILTER_SEPARABLE, FILTER_MEDIAN3 = 0, 1
FILTER_MAX_RADIUS = 8


class FilterParams(C.Structure):
    """vrhip_filter_params: the kind, the radii and the taps of a vrhip_filter_volume call."""
    _fields_ = [("kind", C.c_uint32), ("radius", C.c_uint32 * 3), ("taps", (C.c_float * (FILTER_MAX_RADIUS + 1)) * 3),
                ("reserved", C.c_uint32 * 4)]


class FilterInfo(C.Structure):
    """vrhip_filter_info: what the last vrhip_filter_volume did."""
    _fields_ = [("blocks", C.c_uint64), ("blocks_fetched", C.c_uint64), ("blocks_skipped", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("empty_skip", C.c_uint32), ("in_place", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# vrhip_morph_params.op / .shape and the largest radius (volume morphology, vrhip_morph_volume)
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_GRADIENT, MORPH_TOPHAT, MORPH_BLACKHAT = range(7)
MORPH_BOX, MORPH_BALL = 0, 1
MORPH_MAX_RADIUS = 8


class MorphParams(C.Structure):
    """vrhip_morph_params: the op, the shape and the radii of a vrhip_morph_volume call."""
    _fields_ = [("op", C.c_uint32), ("shape", C.c_uint32), ("radius", C.c_uint32 * 3), ("reserved", C.c_uint32 * 3)]


class MorphSweepInfo(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("blocks_fetched", C.c_uint64), ("blocks_skipped", C.c_uint64)]


class MorphInfo(C.Structure):
    """vrhip_morph_info: what the last vrhip_morph_volume did."""
    _fields_ = [("sweep", MorphSweepInfo * 2), ("scratch_bytes", C.c_uint64), ("sweeps", C.c_uint32),
                ("empty_skip", C.c_uint32), ("in_place", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in ("scratch_bytes", "sweeps", "empty_skip", "in_place")}
        for n, _ in MorphSweepInfo._fields_:
            d[n] = [int(getattr(self.sweep[s], n)) for s in range(2)]
        return d


class Stats(C.Structure):
    _fields_ = [("samples_taken", C.c_uint64), ("samples_nominal", C.c_uint64),
                ("samples_shaded", C.c_uint64), ("bricks_visited", C.c_uint64),
                ("bricks_skipped", C.c_uint64), ("rays_hit", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class LaunchInfo(C.Structure):
    """vrhip_launch_info: what the last render call launched."""
    _fields_ = [(n, C.c_uint32) for n in (
        "technique", "frames", "work_items", "prepass", "ray_list", "phase1_waves", "phase2_waves", "round_budget",
        "footprint", "empty_skip", "skip_in_lds", "instrumented", "extras", "patch_classes", "sorted_phase2",
        "views", "samples")] + [("reserved", C.c_uint32 * 14), ("pixel_major", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


assert C.sizeof(LaunchInfo) == 128
assert C.sizeof(CameraParams) == 128 and C.sizeof(RenderingParams) == 64
assert C.sizeof(RaycastParams) == 32 and C.sizeof(PathtraceParams) == 4 and C.sizeof(IsoParams) == 16
assert C.sizeof(SliceParams) == 80
assert C.sizeof(DepthParams) == 32 and C.sizeof(DepthInfo) == 32
assert C.sizeof(MeshParams) == 48 and C.sizeof(MeshInfo) == 32 and C.sizeof(IndexedMeshInfo) == 64
assert C.sizeof(StatsParams) == 64 and C.sizeof(VolumeStats) == 72 and C.sizeof(StatsInfo) == 48
assert C.sizeof(FilterParams) == 140 and C.sizeof(FilterInfo) == 40
assert C.sizeof(MorphParams) == 32 and C.sizeof(MorphInfo) == 72

_H = C.c_void_p
_U3 = C.POINTER(C.c_uint32)

# name -> (restype, argtypes): every symbol include/vrhip.h declares
SYMBOLS = {
    "vrhip_abi_version": (C.c_int, []),
    "vrhip_create": (C.c_int, [C.c_int, C.POINTER(_H)]),
    "vrhip_destroy": (None, [_H]),
    "vrhip_last_error": (C.c_char_p, [_H]),
    "vrhip_device_name": (C.c_int, [_H, C.c_char_p, C.c_size_t]),
    "vrhip_set_stream": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "vrhip_get_stream": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "vrhip_download_cells": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vrhip_download_empty_cells": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32)]),
    "vrhip_download_cell_tables": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vrhip_assemble_batch": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_void_p]),
    "vrhip_pack_tiles": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrhip_quantise_rgba8": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "vrhip_render_frame_rgba8": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "vrhip_frame_rgba8": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "vrhip_pack_tiles_rgba8": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "vrhip_assemble_batch_rgba8": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_void_p]),
    "vrhip_message_positions": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32,
                                          C.c_uint32, C.c_void_p]),
    "vrhip_assemble_frame": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_void_p]),
    "vrhip_upload_volume": (C.c_int, [_H, C.c_void_p, _U3, C.c_int, C.c_uint32]),
    "vrhip_upload_volume_channels": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_uint32), C.c_int,
                                               C.c_int, C.c_uint32]),
    "vrhip_share_volumes": (C.c_int, [_H, _H]),
    "vrhip_render_batch": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "vrhip_render_batch_views": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_uint32]),
    "vrhip_render_samples": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "vrhip_set_round_budget": (C.c_int, [_H, C.c_uint32]),
    "vrhip_upload_volume_device": (C.c_int, [_H, C.c_void_p, _U3, C.c_int, C.c_uint32]),
    "vrhip_synth_volume": (C.c_int, [_H, C.c_int, _U3, C.c_int, C.c_uint32]),
    "vrhip_ingest_raw": (C.c_int, [_H, C.c_void_p, C.c_size_t, _U3, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                   C.POINTER(C.c_double), C.POINTER(C.c_float)]),
    "vrhip_volume_histogram": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_double)]),
    "vrhip_last_ingest_seconds": (C.c_double, [_H]),
    "vrhip_download_volume": (C.c_int, [_H, C.c_uint32, C.c_void_p, C.c_size_t]),
    "vrhip_downsample_volume": (C.c_int, [_H, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, _U3]),
    "vrhip_clear_volumes": (C.c_int, [_H]),
    "vrhip_set_timestep": (C.c_int, [_H, C.c_uint32]),
    "vrhip_get_resolution": (C.c_int, [_H, C.POINTER(C.c_uint32)]),
    "vrhip_set_transfer_function": (C.c_int, [_H, C.c_void_p, C.c_uint32]),
    "vrhip_set_tff_prefix_sum": (C.c_int, [_H, C.c_void_p, C.c_uint32]),
    "vrhip_set_transfer_function_2d": (C.c_int, [_H, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float]),
    "vrhip_tf2d_params_check": (C.c_int, [C.c_uint32, C.c_uint32, C.c_float]),
    "vrhip_tf2d_lookup": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                    C.POINTER(C.c_float)]),
    "vrhip_tf2d_build_ramp": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "vrhip_preint_slab": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "vrhip_preint_tables": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "vrhip_build_bricks": (C.c_int, [_H]),
    "vrhip_get_brick_info": (C.c_int, [_H, _U3, C.POINTER(C.c_float), _U3]),
    "vrhip_download_bricks": (C.c_int, [_H, C.c_uint32, C.c_void_p, C.c_size_t]),
    "vrhip_last_bricks_seconds": (C.c_double, [_H]),
    "vrhip_set_camera_params": (C.c_int, [_H, C.POINTER(CameraParams)]),
    "vrhip_set_rendering_params": (C.c_int, [_H, C.POINTER(RenderingParams)]),
    "vrhip_set_raycast_params": (C.c_int, [_H, C.POINTER(RaycastParams)]),
    "vrhip_set_pathtrace_params": (C.c_int, [_H, C.POINTER(PathtraceParams)]),
    "vrhip_set_iso_params": (C.c_int, [_H, C.POINTER(IsoParams)]),
    "vrhip_set_object_ess": (C.c_int, [_H, C.c_int]),
    "vrhip_render_frame": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "vrhip_render_slices": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]),
    "vrhip_render_depth": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.POINTER(DepthParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int]),
    "vrhip_last_depth_info": (C.c_int, [_H, C.POINTER(DepthInfo)]),
    "vrhip_isosurface_count": (C.c_int, [_H, C.POINTER(MeshParams), C.POINTER(C.c_uint64)]),
    "vrhip_isosurface_extract": (C.c_int, [_H, C.POINTER(MeshParams), C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.POINTER(C.c_uint64), C.c_int]),
    "vrhip_last_mesh_info": (C.c_int, [_H, C.POINTER(MeshInfo)]),
    "vrhip_isosurface_count_indexed": (C.c_int, [_H, C.POINTER(MeshParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vrhip_isosurface_extract_indexed": (C.c_int, [_H, C.POINTER(MeshParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                   C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "vrhip_last_indexed_mesh_info": (C.c_int, [_H, C.POINTER(IndexedMeshInfo)]),
    "vrhip_volume_statistics": (C.c_int, [_H, C.POINTER(StatsParams), C.POINTER(VolumeStats), C.c_void_p, C.c_int]),
    "vrhip_last_stats_info": (C.c_int, [_H, C.POINTER(StatsInfo)]),
    "vrhip_stats_params_check": (C.c_int, [C.POINTER(StatsParams)]),
    "vrhip_filter_volume": (C.c_int, [_H, C.POINTER(FilterParams), C.c_uint32]),
    "vrhip_filter_params_check": (C.c_int, [C.POINTER(FilterParams)]),
    "vrhip_filter_gaussian_taps": (C.c_int, [C.c_double, C.c_uint32, C.POINTER(C.c_float)]),
    "vrhip_last_filter_info": (C.c_int, [_H, C.POINTER(FilterInfo)]),
    "vrhip_morph_volume": (C.c_int, [_H, C.POINTER(MorphParams), C.c_uint32]),
    "vrhip_morph_params_check": (C.c_int, [C.POINTER(MorphParams)]),
    "vrhip_morph_element": (C.c_int, [C.POINTER(MorphParams), C.POINTER(C.c_int8), C.c_uint32, _U3]),
    "vrhip_last_morph_info": (C.c_int, [_H, C.POINTER(MorphInfo)]),
    "vrhip_render_tiles": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_uint32, C.c_void_p]),
    "vrhip_set_environment_map": (C.c_int, [_H, C.c_void_p, C.c_uint32, C.c_uint32]),
    "vrhip_reset_image_ess": (C.c_int, [_H]),
    "vrhip_get_image_ess": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "vrhip_set_image_ess": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "vrhip_last_kernel_seconds": (C.c_double, [_H]),
    "vrhip_last_phase_seconds": (C.c_int, [_H, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vrhip_last_launch_info": (C.c_int, [_H, C.POINTER(LaunchInfo)]),
    "vrhip_download_cost_map": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "vrhip_download_ray_order": (C.c_int, [_H, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "vrhip_set_phase_timing": (C.c_int, [_H, C.c_int]),
    "vrhip_set_frame_timing": (C.c_int, [_H, C.c_int]),
    "vrhip_build_source_hash": (C.c_char_p, []),
    "vrhip_set_stats_enabled": (C.c_int, [_H, C.c_int]),
    "vrhip_get_stats": (C.c_int, [_H, C.POINTER(Stats)]),
    "vrhip_count_touched": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                      C.c_void_p, C.c_size_t]),
    "vrhip_count_fetched": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "vrhip_count_touched_tiles": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
}

_lib = None


def load():
    """Load libvrhip.so and bind every declared symbol.  Raises (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libvrhip.so is not built (%s missing). Build it with "
            "`make -C volumerenderercl_amd/csrc` or __graft_entry__.build(); there is no "
            "CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.vrhip_abi_version() != 1:
        raise RuntimeError("libvrhip.so ABI version mismatch")
    _lib = lib
    return lib
