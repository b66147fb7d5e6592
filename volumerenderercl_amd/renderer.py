"""Host-side mirror of the reference's `VolumeRenderCL` interface over the C ABI.

The production host is the C++ class in csrc/host/ (same interface, the reference is
compiled code); this Python twin exists so tests and bench.py can drive libvrhip.so
through exactly the calls the reference's caller makes (volumerenderwidget.cpp), with
the reference's method names, argument meaning, call order and error behaviour
(/root/reference/src/core/volumerendercl.h:123-356).
"""
import ctypes as C

import numpy as np

from . import _lib, frontend
from ._lib import (CameraParams, IsoParams, PathtraceParams, RaycastParams, RenderingParams, Stats,
                   UCHAR, USHORT, FLOAT, TECH_MIP, TECH_ISO, TECH_TF2D, TECH_PREINT)

NP_DTYPE = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
_MT19937_DEFAULT_SEED = 5489   # std::mt19937 default constructor


def _u3(v):
    return (C.c_uint32 * 3)(*[int(x) for x in v])


class VolumeRenderCL:
    TECH_RAYCAST, TECH_PATHTRACE = 0, 1

    def __init__(self):
        self._lib = None
        self._h = C.c_void_p()
        self._vol_loaded = False
        self._model_scale = np.ones(3, dtype=np.float32)
        self._camera = CameraParams()
        self._camera.viewMat[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
        self._camera.bbox_bl[:] = [-1, -1, -1, 0]
        self._camera.bbox_tr[:] = [1, 1, 1, 0]
        self._rendering = RenderingParams()
        self._rendering.backgroundColor[:] = [1, 1, 1, 1]
        self._rendering.modelScale[:] = [1, 1, 1, 0]
        self._rendering.illumType = 1
        self._rendering.useLinear = 1
        self._rendering.seed = 42
        self._raycast = RaycastParams()
        self._raycast.samplingRate = 1.5
        self._raycast.brickRes[:] = [1, 1, 1, 0]
        self._pathtrace = PathtraceParams(100.0)
        self._iso = IsoParams(0.5, 4)
        self._timestep = 0
        self._res = [0, 0, 0, 1]
        self._thickness = [1.0, 1.0, 1.0]
        self._format = None
        self._histograms = []
        # the reference's member generator is default-seeded (volumerendercl.cpp:67 shadows it)
        self._generator = frontend.Mt19937(_MT19937_DEFAULT_SEED)
        self._fixed_seed = None
        self._out_size = (0, 0)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != _lib.OK:
            msg = self._lib.vrhip_last_error(self._h)
            msg = msg.decode() if msg else "vrhip error %d" % rc
            if rc == _lib.ERR_INVALID:
                raise ValueError(msg)        # std::invalid_argument
            raise RuntimeError(msg)          # std::runtime_error

    def _push_params(self):
        ms = self._model_scale
        self._rendering.modelScale[:] = [float(ms[0]), float(ms[1]), float(ms[2]), 0.0]
        self._check(self._lib.vrhip_set_camera_params(self._h, C.byref(self._camera)))
        self._check(self._lib.vrhip_set_rendering_params(self._h, C.byref(self._rendering)))
        self._check(self._lib.vrhip_set_raycast_params(self._h, C.byref(self._raycast)))
        self._check(self._lib.vrhip_set_pathtrace_params(self._h, C.byref(self._pathtrace)))
        self._check(self._lib.vrhip_set_iso_params(self._h, C.byref(self._iso)))

    @property
    def handle(self):
        return self._h

    @property
    def lib(self):
        return self._lib

    # ------------------------------------------------------------------ interface
    def initialize(self, useGL=False, useCPU=False, vendor=None, deviceName="", platformId=-1,
                   device_id=0):
        """volumerendercl.cpp:95-159.  useGL / useCPU / vendor select OpenCL plumbing that
        does not exist here; useCPU is refused loudly (no CPU path in the product)."""
        if useCPU:
            raise RuntimeError("ERROR: no CPU device path; libvrhip renders on MI355X only")
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.vrhip_create(int(device_id), C.byref(h))
        if rc != _lib.OK:
            msg = self._lib.vrhip_last_error(None)
            raise RuntimeError(msg.decode() if msg else "vrhip_create failed")
        self._h = h
        self._device_id = int(device_id)

    def setRoundBudget(self, rounds):
        """Scheduling knob of the two-phase march (vrhip_set_round_budget): 10 (default) for the
        shortest single frame, ~32 when several frames are in flight.  No effect on pixels."""
        self._round_budget = int(rounds)
        self._check(self._lib.vrhip_set_round_budget(self._h, int(rounds)))

    def shareVolumes(self):
        """A second renderer on the same GPU that renders from THIS renderer's voxels and ESS
        bricks (vrhip_share_volumes) with everything else of its own -- transfer function, kernel
        arguments, frame buffer, scratch, stream: one frame each can be in flight on two streams
        over a single copy of the volume.  Starts as a copy of this renderer's settings; this
        renderer must keep its volumes (no load / clear / close) while the twin is alive."""
        if not self._vol_loaded:
            raise RuntimeError("No volume data is loaded.")
        twin = VolumeRenderCL()
        twin.initialize(device_id=getattr(self, "_device_id", 0))
        twin._check(twin._lib.vrhip_share_volumes(twin._h, self._h))
        for name in ("_res", "_thickness", "_histograms"):
            setattr(twin, name, list(getattr(self, name)))
        twin._format = self._format
        twin._model_scale = self._model_scale.copy()
        twin._timestep = self._timestep
        twin._props = getattr(self, "_props", None)
        for name in ("_camera", "_rendering", "_raycast", "_pathtrace", "_iso"):
            C.memmove(C.byref(getattr(twin, name)), C.byref(getattr(self, name)),
                      C.sizeof(getattr(self, name)))
        twin._fixed_seed = self._fixed_seed
        twin._vol_loaded = True
        twin._check(twin._lib.vrhip_set_timestep(twin._h, int(self._timestep)))
        twin._check(twin._lib.vrhip_set_object_ess(twin._h, 1 if getattr(self, "_obj_ess", True) else 0))
        if getattr(self, "_tff", None) is not None:
            twin.setTransferFunction(self._tff)
            if getattr(self, "_prefix", None) is not None:
                twin.setTffPrefixSum(self._prefix)
        if getattr(self, "_tf2d", None) is not None:
            twin.setTransferFunction2D(*self._tf2d)
        twin._rendering.iteration = self._rendering.iteration
        if getattr(self, "_round_budget", None) is not None:
            twin.setRoundBudget(self._round_budget)
        return twin

    def close(self):
        self._batch_f32 = None      # (the float frames behind render_batch(rgba8=True))
        if self._lib is not None and self._h:
            self._lib.vrhip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr, use_own=False):
        """Launch on the given hipStream_t handle (0 = legacy default stream)."""
        self._check(self._lib.vrhip_set_stream(self._h, C.c_void_p(stream_ptr),
                                               1 if use_own else 0))

    def get_stream(self):
        """The hipStream_t handle (int, 0 = legacy default stream) render calls are enqueued on."""
        p = C.c_void_p()
        self._check(self._lib.vrhip_get_stream(self._h, C.byref(p)))
        return p.value or 0

    def getPlatformNames(self):
        """volumerendercl.cpp:1062-1079 (OpenCL platforms): there is one, the HIP runtime."""
        return ["AMD HIP (ROCm)"]

    def getDeviceNames(self, platformId=0, type="GPU"):
        """volumerendercl.cpp:1087-1108: the devices of a platform by type; no CPU device here."""
        return [] if type == "CPU" else [self.getCurrentDeviceName()]

    def getCurrentDeviceName(self):
        buf = C.create_string_buffer(256)
        self._check(self._lib.vrhip_device_name(self._h, buf, 256))
        return buf.value.decode()

    def updateView(self, viewMat):
        """volumerendercl.cpp:379-390: 16 floats, row-major; silently ignored without data."""
        if not self._vol_loaded:
            return
        self._camera.viewMat[:] = [float(x) for x in viewMat]
        self._rendering.iteration = 0

    def updateSamplingRate(self, samplingRate):
        self._raycast.samplingRate = float(samplingRate)

    def updateOutputImg(self, width, height, texId=0):
        """volumerendercl.cpp:465-499: output buffers are sized by the render call; the hit images
        of image-order ESS are re-created with their initial contents (:482-488)."""
        self._out_size = (int(width), int(height))
        if self._h:
            self._check(self._lib.vrhip_reset_image_ess(self._h))

    def getImageEss(self, width, height):
        """(hit_in, hit_out) of image-order ESS for a width x height frame: uint8
        [(height/8+1), (width/8+1)]; hit_in is what the next imgEss frame reads."""
        shape = (int(height) // 8 + 1, int(width) // 8 + 1)
        a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        self._check(self._lib.vrhip_get_image_ess(self._h, int(width), int(height),
                                                  a.ctypes.data, b.ctypes.data))
        return a, b

    def setImageEss(self, width, height, hit_in=None, hit_out=None):
        shape = (int(height) // 8 + 1, int(width) // 8 + 1)
        ptrs = []
        keep = []
        for h in (hit_in, hit_out):
            if h is None:
                ptrs.append(None)
                continue
            h = np.ascontiguousarray(h, dtype=np.uint8)
            if h.shape != shape:
                raise ValueError("hit image must have shape %r" % (shape,))
            keep.append(h)
            ptrs.append(h.ctypes.data)
        self._check(self._lib.vrhip_set_image_ess(self._h, int(width), int(height), *ptrs))

    def _begin_frame(self):
        # setMemObjectsRaycast: fresh seed per frame (volumerendercl.cpp:212)
        if self._fixed_seed is None:
            self._rendering.seed = self._generator()
        else:
            self._rendering.seed = self._fixed_seed
        self._push_params()

    def _advance_iteration(self):
        # a maximum intensity projection, an isosurface, a 2-D transfer function or a pre-integrated frame does not
        # accumulate: every frame of it is iteration 0
        if self._rendering.technique not in (TECH_MIP, TECH_ISO, TECH_TF2D, TECH_PREINT):
            self._rendering.iteration += 1

    def runRaycast(self, width, height, out_dev_ptr=None):
        """volumerendercl.cpp:506-558: frame stays on the GPU; iteration advances (:540)."""
        if not self._vol_loaded:
            return
        self._begin_frame()
        self._check(self._lib.vrhip_render_frame(self._h, int(width), int(height),
                                                 C.c_void_p(out_dev_ptr), 1 if out_dev_ptr else 0))
        self._advance_iteration()

    def runRaycastNoGL(self, width, height, output=None):
        """volumerendercl.cpp:568-607 with the documented contract honoured:
        returns width*height*4 float32, row-major RGBA, row 0 = top."""
        if not self._vol_loaded:
            return output
        self._begin_frame()
        out = np.empty((int(height), int(width), 4), dtype=np.float32)
        self._check(self._lib.vrhip_render_frame(self._h, int(width), int(height),
                                                 out.ctypes.data_as(C.c_void_p), 0))
        self._advance_iteration()   # accumulation advances in both paths
        if output is not None:
            output[:] = out.reshape(-1).tolist()
        return out

    # ---- 8-bit frames (the reference's CL_UNORM_INT8 output image; frontend.quantise_rgba8 states the conversion)
    @staticmethod
    def _rgba8_out(out, shape):
        """(array to return, pointer, is_device) of an 8-bit destination: `out` (numpy uint8, or a torch uint8
        device tensor) or a fresh numpy array of `shape`."""
        if out is None:
            out = np.empty(shape, dtype=np.uint8)
        n = int(np.prod(shape))
        if isinstance(out, np.ndarray):
            if out.dtype != np.uint8 or out.size != n or not out.flags.c_contiguous:
                raise ValueError("out must be a contiguous uint8 array of %d bytes" % n)
            return out, out.ctypes.data, 0
        import torch
        if out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a numpy array or a contiguous uint8 device tensor of %d bytes" % n)
        return out, out.data_ptr(), 1

    def render_frame_rgba8(self, width, height, out=None):
        """runRaycastNoGL as the reference reads it back: the frame as uint8 [height, width, 4]
        (vrhip_render_frame_rgba8: the frame of runRaycast, then quantised on the same stream; the float
        frame buffer keeps the unquantised frame, so accumulation carries on as with runRaycast).  out: a
        numpy uint8 array or a torch uint8 device tensor to fill; returned."""
        if not self._vol_loaded:
            return out
        out, ptr, dev = self._rgba8_out(out, (int(height), int(width), 4))
        self._begin_frame()
        self._check(self._lib.vrhip_render_frame_rgba8(self._h, int(width), int(height), C.c_void_p(ptr), dev))
        self._advance_iteration()
        return out

    def quantise_rgba8(self, frames, out=None, stream=None):
        """A contiguous float32 device tensor [..., 4] as uint8 of the same shape (vrhip_quantise_rgba8), on
        torch's current stream (or the hipStream_t handle `stream`).  out: a numpy uint8 array (the call
        returns when it is filled) or a torch uint8 device tensor; None: a new device tensor."""
        import torch
        if (frames.dtype != torch.float32 or not frames.is_cuda or not frames.is_contiguous() or frames.dim() < 1
                or frames.shape[-1] != 4):
            raise ValueError("quantise_rgba8: a contiguous float32 device tensor [..., 4]")
        if out is None:
            out = torch.empty(frames.shape, dtype=torch.uint8, device=frames.device)
        out, ptr, dev = self._rgba8_out(out, tuple(frames.shape))
        n = frames.numel() // 4
        if n:
            if stream is None:
                stream = torch.cuda.current_stream(frames.device).cuda_stream
            self._check(self._lib.vrhip_quantise_rgba8(self._h, C.c_void_p(stream), C.c_void_p(frames.data_ptr()), 1, n, n,
                                                       C.c_void_p(ptr), dev))
        return out

    def render_tiles(self, width, height, tile_w, tile_h, tile_ids, out_dev_ptr):
        """Image-tile decomposition entry; no reference counterpart."""
        if not self._vol_loaded:
            return
        self._begin_frame()
        ids = np.ascontiguousarray(tile_ids, dtype=np.uint32)
        self._check(self._lib.vrhip_render_tiles(self._h, int(width), int(height), int(tile_w),
                                                 int(tile_h), ids.ctypes.data_as(C.c_void_p),
                                                 int(ids.size), C.c_void_p(out_dev_ptr)))

    def render_batch(self, width, height, seeds, out_dev_ptr=None, tile_w=0, tile_h=0, tile_ids=None,
                     frame_stride=0, views=None, rgba8=False, out=None):
        """len(seeds) <= 256 independent frames (frame f jittered by seeds[f]) in one set of
        launches (vrhip_render_batch): whole frames into out[f][height][width][4], or -- with
        tile_ids -- the tile subset into out[f][n_tiles][tile_h][tile_w][4] (device memory);
        frame_stride: pixels between the frames of `out` when they are not packed.
        views: one row-major 16-float view matrix per frame (as updateView takes it): frame f is
        rendered from views[f] with the renderer's bbox and ortho setting (vrhip_render_batch_views);
        None: every frame from the renderer's view.
        rgba8=True: the frames as 8-bit pixels from the same launch set -- the floats are rendered into a
        buffer this object keeps until close() and quantised on the renderer's stream (vrhip_quantise_rgba8)
        -- into `out`, a torch uint8 device tensor [n, height, width, 4] (tiles: [n, n_tiles, tile_h, tile_w, 4]),
        or None for a new one; returned.  out_dev_ptr and frame_stride belong to the float form and must be
        left alone then, as `out` must without rgba8."""
        if not self._vol_loaded:
            return
        if rgba8:
            if out_dev_ptr is not None or frame_stride:
                raise ValueError("render_batch: with rgba8 the frames go to `out`, packed")
            return self._render_batch_rgba8(width, height, seeds, out, tile_w, tile_h, tile_ids, views)
        if out_dev_ptr is None or out is not None:
            raise ValueError("render_batch: a device pointer for the float frames")
        self._rendering.iteration = 0
        self._push_params()
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        ids = None if tile_ids is None else np.ascontiguousarray(tile_ids, dtype=np.uint32)
        cams = None
        if views is not None:
            if len(views) != sd.size:
                raise ValueError("render_batch: one view per frame (%d views, %d seeds)" % (len(views), sd.size))
            cams = (CameraParams * max(1, sd.size))()
            for f, v in enumerate(views):
                m = [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]
                if len(m) != 16:
                    raise ValueError("render_batch: a view is 16 floats")
                C.memmove(C.byref(cams[f]), C.byref(self._camera), C.sizeof(CameraParams))
                cams[f].viewMat[:] = m
        self._check(self._lib.vrhip_render_batch_views(
            self._h, int(width), int(height), int(tile_w), int(tile_h),
            None if ids is None else ids.ctypes.data_as(C.c_void_p), 0 if ids is None else int(ids.size),
            sd.ctypes.data_as(C.c_void_p), None if cams is None else C.cast(cams, C.c_void_p), int(sd.size),
            C.c_void_p(out_dev_ptr), int(frame_stride)))

    def _render_batch_rgba8(self, width, height, seeds, out, tile_w, tile_h, tile_ids, views):
        import torch
        n = len(seeds)
        shape = ((n, int(height), int(width), 4) if tile_ids is None
                 else (n, len(tile_ids), int(tile_h), int(tile_w), 4))
        dev = torch.device("cuda", getattr(self, "_device_id", 0))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        elif tuple(out.shape) != shape:
            raise ValueError("render_batch: out must have shape %r" % (shape,))
        out, ptr, is_dev = self._rgba8_out(out, shape)
        if not is_dev:
            raise ValueError("render_batch: out must be a torch uint8 device tensor")
        f32 = getattr(self, "_batch_f32", None)
        if f32 is None or f32.numel() < int(np.prod(shape)):
            f32 = self._batch_f32 = torch.zeros(int(np.prod(shape)), dtype=torch.float32, device=dev)
        # the renderer's stream follows torch's current one (the float buffer's last reader, `out`'s producer) and
        # the other way round afterwards, as TileDriver brackets a render
        rs = torch.cuda.ExternalStream(self.get_stream(), device=dev)
        cur = torch.cuda.current_stream(dev)
        rs.wait_stream(cur)
        self.render_batch(width, height, seeds, f32.data_ptr(), tile_w, tile_h, tile_ids, views=views)
        self.quantise_rgba8(f32[: int(np.prod(shape))].view(shape), out, stream=self.get_stream())
        cur.wait_stream(rs)
        return out

    def render_samples(self, width, height, seeds, out_dev_ptr=None, tile_w=0, tile_h=0, tile_ids=None,
                       samples_per_launch=0):
        """Progressive path tracer (technique 1): len(seeds) consecutive iterations of the accumulated
        image -- sample k jittered by seeds[k] at iteration (current iteration + k) -- in as few launch
        sets as possible (vrhip_render_samples), bit for bit what len(seeds) runRaycastNoGL calls with
        those seeds leave in the frame buffer.  samples_per_launch: samples per set (0 = the library's
        default).  With tile_ids the tile subset, compact [n_tiles][tile_h][tile_w][4].  Returns the
        accumulated image as numpy when no device pointer is given, else writes it there and returns
        None.  Advances the iteration by len(seeds)."""
        if not self._vol_loaded:
            return None
        sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        self._push_params()
        ids = None if tile_ids is None else np.ascontiguousarray(tile_ids, dtype=np.uint32).reshape(-1)
        out = None
        if out_dev_ptr is None:
            shape = (int(height), int(width), 4) if ids is None else (int(ids.size), int(tile_h), int(tile_w), 4)
            out = np.zeros(shape, dtype=np.float32)
        self._check(self._lib.vrhip_render_samples(
            self._h, int(width), int(height), int(tile_w), int(tile_h),
            None if ids is None else ids.ctypes.data_as(C.c_void_p), 0 if ids is None else int(ids.size),
            sd.ctypes.data_as(C.c_void_p) if sd.size else None, int(sd.size), int(samples_per_launch),
            out.ctypes.data_as(C.c_void_p) if out is not None else C.c_void_p(out_dev_ptr),
            0 if out is not None else 1))
        self._rendering.iteration += int(sd.size)
        return out

    # ---- slice views (no reference counterpart; include/vrhip.h "slice views")
    def render_slices(self, width, height, slices, out_dev_ptr=None):
        """2-D cuts through the voxels (vrhip_render_slices): `slices` is a SliceParams or a sequence of them
        (frontend.axis_slice, plane_slice, slice_stack build them), all rendered by one launch at width x height.
        Returns float32 [n, height, width, 4], row 0 = top; with out_dev_ptr (device memory of that size, 16-byte
        aligned) the images are written there without a wait and None is returned.  Reads the volume of the current
        time step, the transfer function, setLinearInterpolation and setBackground; the camera, the technique, the
        iteration and the seed are neither read nor touched: progressive frames carry on around it bit for bit."""
        if not self._vol_loaded:
            raise RuntimeError("No volume data is loaded.")
        if isinstance(slices, _lib.SliceParams):
            slices = [slices]
        slices = list(slices)
        for s in slices:
            if not isinstance(s, _lib.SliceParams):
                raise ValueError("render_slices: a sequence of SliceParams")
        arr = (_lib.SliceParams * max(1, len(slices)))(*slices)
        self._push_params()
        out = None
        if out_dev_ptr is None:
            out = np.empty((len(slices), int(height), int(width), 4), dtype=np.float32)
        self._check(self._lib.vrhip_render_slices(
            self._h, int(width), int(height), C.cast(arr, C.c_void_p), len(slices),
            out.ctypes.data_as(C.c_void_p) if out is not None else C.c_void_p(out_dev_ptr),
            0 if out is not None else 1))
        return out

    # ---- depth images and picking (no reference counterpart; include/vrhip.h "depth images and picking")
    _DEPTH_MODES = {"iso": _lib.DEPTH_ISO, "max": _lib.DEPTH_MAX, "opacity": _lib.DEPTH_OPACITY}

    def _depth_params(self, mode, threshold, refine, rect):
        if isinstance(mode, str):
            if mode not in self._DEPTH_MODES:
                raise ValueError("depth mode must be 'iso', 'max' or 'opacity'")
            mode = self._DEPTH_MODES[mode]
        p = _lib.DepthParams()
        p.mode, p.threshold, p.refineSteps, p.reserved = int(mode), float(threshold), int(refine), 0
        if rect is not None:
            p.x0, p.y0, p.w, p.h = (int(v) for v in rect)
        return p

    def render_depth(self, width, height, mode, threshold=0.5, refine=4, rect=None, out_dev_ptrs=None):
        """Where along its ray each pixel's "thing" lies (vrhip_render_depth).  mode "iso" (the first sample at or above
        `threshold`, refined by `refine` bisections as technique 4 does), "max" (the first sample that attains the ray's
        maximum) or "opacity" (the sample at which the ray caster's accumulated opacity reaches `threshold`); the
        DEPTH_* numbers do as well.  rect = (x0, y0, w, h): that rectangle of the width x height frame only.
        Returns (xyzt float32 [h, w, 4], aux float32 [h, w], kind uint8 [h, w]), row 0 = top: the hit position in
        box space ([-1, 1]^3) and the ray parameter t, (0, 0, 0, inf) without a hit; the value found (iso: the sample
        at the hit, max: the maximum, opacity: the opacity reached); DEPTH_MISS / DEPTH_NO_HIT / DEPTH_HIT.
        With out_dev_ptrs = (xyzt, aux, kind) device addresses (0 or None: not wanted; xyzt 16-byte aligned) the
        answer is written there without a wait and None is returned.  The rays are the current camera's and seed's;
        the technique, the iteration and the frame buffer are neither read nor touched."""
        p = self._depth_params(mode, threshold, refine, rect)
        self._push_params()
        if out_dev_ptrs is not None:
            ptrs = [C.c_void_p(int(a)) if a else None for a in out_dev_ptrs]
            self._check(self._lib.vrhip_render_depth(self._h, int(width), int(height), C.byref(p), ptrs[0], ptrs[1],
                                                     ptrs[2], 1))
            return None
        w, h = (int(p.w), int(p.h)) if rect is not None else (int(width), int(height))
        xyzt = np.empty((h, w, 4), dtype=np.float32)
        aux = np.empty((h, w), dtype=np.float32)
        kind = np.empty((h, w), dtype=np.uint8)
        self._check(self._lib.vrhip_render_depth(self._h, int(width), int(height), C.byref(p),
                                                 xyzt.ctypes.data_as(C.c_void_p), aux.ctypes.data_as(C.c_void_p),
                                                 kind.ctypes.data_as(C.c_void_p), 0))
        return xyzt, aux, kind

    def pick(self, width, height, x, y, mode, threshold=0.5, refine=4):
        """The 3-D point under pixel (x, y) of the width x height frame: render_depth on a 1 x 1 rectangle.  None when
        the ray finds nothing; else a dict: pos (box space, float32 [3]), t, aux, and voxel = (pos * 0.5 + 0.5) * res,
        the continuous voxel coordinates (float64 [3], x y z)."""
        xyzt, aux, kind = self.render_depth(width, height, mode, threshold, refine, rect=(int(x), int(y), 1, 1))
        if kind[0, 0] != _lib.DEPTH_HIT:
            return None
        pos = xyzt[0, 0, :3].copy()
        voxel = frontend.box_to_voxel(pos, self._res[:3])
        return {"pos": pos, "t": float(xyzt[0, 0, 3]), "aux": float(aux[0, 0]), "voxel": voxel}

    def lastDepthInfo(self):
        """What the last render_depth / pick launched (vrhip_last_depth_info): mode, work_items (8 x 8 patches),
        empty_skip (1: the kernel stepped over samples by the cell grid) -- as a dict."""
        di = _lib.DepthInfo()
        self._check(self._lib.vrhip_last_depth_info(self._h, C.byref(di)))
        return di.as_dict()

    # ---- isosurface extraction (no reference counterpart; include/vrhip.h "isosurface extraction")
    @staticmethod
    def _mesh_params(iso, normals, region):
        p = _lib.MeshParams()
        p.isoValue = float(iso)
        p.normals = _lib.MESH_NORMALS_GRADIENT if normals else _lib.MESH_NORMALS_NONE
        if region is not None:
            lo, hi = region
            p.lo[:] = [int(v) for v in lo]
            p.hi[:] = [int(v) for v in hi]
        return p

    def isosurface_count(self, iso, region=None):
        """The number of triangles of the isosurface at `iso` (units of isoValue of setIsoParams) of the current time
        step (vrhip_isosurface_count).  region = ((x0, y0, z0), (x1, y1, z1)) in voxels: the cubes with lo <= corner
        and corner + 1 <= hi only; None: the whole volume."""
        p = self._mesh_params(iso, False, region)
        n = C.c_uint64(0)
        self._check(self._lib.vrhip_isosurface_count(self._h, C.byref(p), C.byref(n)))
        return int(n.value)

    def extract_isosurface(self, iso, normals=False, region=None, out_dev_ptrs=None):
        """The isosurface at `iso` as a triangle list (vrhip_isosurface_extract): (positions float32 [n, 3, 3] in box
        space -- the volume is [-1, 1]^3 --, normals float32 [n, 3, 3] or None).  The list is deterministic and
        ordered (blocks of 8^3 cubes, cubes, tetrahedra); shared vertices are bit-equal, so frontend.weld_mesh turns it
        into an indexed, watertight mesh.  normals: technique 4's shading normal per vertex.
        With out_dev_ptrs = (positions, normals or None, capacity in triangles) -- device addresses, 16-byte aligned --
        the triangles are written there and their number is returned; a capacity that is too small raises, and
        isosurface_count tells what is needed.  The camera, the technique and the frame buffer are neither read nor
        touched."""
        p = self._mesh_params(iso, normals, region)
        n = C.c_uint64(0)
        if out_dev_ptrs is not None:
            pos, nrm, cap = out_dev_ptrs
            self._check(self._lib.vrhip_isosurface_extract(self._h, C.byref(p), C.c_void_p(int(pos)),
                                                           C.c_void_p(int(nrm)) if nrm else None, int(cap), C.byref(n), 1))
            return int(n.value)
        self._check(self._lib.vrhip_isosurface_count(self._h, C.byref(p), C.byref(n)))
        count = int(n.value)
        pos = np.empty((count, 3, 3), dtype=np.float32)
        nrm = np.empty((count, 3, 3), dtype=np.float32) if normals else None
        if count:
            self._check(self._lib.vrhip_isosurface_extract(
                self._h, C.byref(p), pos.ctypes.data_as(C.c_void_p),
                nrm.ctypes.data_as(C.c_void_p) if normals else None, count, C.byref(n), 0))
            if int(n.value) != count:
                raise RuntimeError("extract_isosurface: the volume changed between the count and the extraction")
        return pos, nrm

    def lastMeshInfo(self):
        """What the last isosurface_count / extract_isosurface did (vrhip_last_mesh_info): triangles, blocks (of 8^3
        cubes that hold a cube of the region), blocks_skipped (by the cell grid, object-order ESS on), empty_skip (1:
        the cell grid was handed to the kernel) -- as a dict."""
        mi = _lib.MeshInfo()
        self._check(self._lib.vrhip_last_mesh_info(self._h, C.byref(mi)))
        return mi.as_dict()

    # ---- indexed isosurface extraction (include/vrhip.h "indexed isosurface extraction")
    def isosurface_count_indexed(self, iso, region=None):
        """(vertices, triangles) of the indexed isosurface at `iso` (vrhip_isosurface_count_indexed): one vertex per
        crossed lattice edge of the region, the triangles of isosurface_count."""
        p = self._mesh_params(iso, False, region)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.vrhip_isosurface_count_indexed(self._h, C.byref(p), C.byref(nv), C.byref(nt)))
        return int(nv.value), int(nt.value)

    def extract_isosurface_indexed(self, iso, normals=False, region=None, out_dev_ptrs=None):
        """The isosurface at `iso` as an indexed mesh made on the device (vrhip_isosurface_extract_indexed): (vertices
        float32 [m, 3] in box space, normals float32 [m, 3] or None, indices uint32 [n, 3]).  vertices[indices] is
        extract_isosurface's list bit for bit; a vertex is a lattice edge, so edges that meet in a grid point equal to
        `iso` stay separate vertices with equal positions, which frontend.weld_mesh would merge.
        With out_dev_ptrs = (vertices, normals or None, indices, capacity in vertices, capacity in triangles) --
        device addresses, 16-byte aligned -- the mesh is written there and (m, n) is returned; a capacity that is too
        small raises, and isosurface_count_indexed tells what is needed."""
        p = self._mesh_params(iso, normals, region)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        if out_dev_ptrs is not None:
            vtx, nrm, idx, cap_v, cap_t = out_dev_ptrs
            self._check(self._lib.vrhip_isosurface_extract_indexed(
                self._h, C.byref(p), C.c_void_p(int(vtx)), C.c_void_p(int(nrm)) if nrm else None, C.c_void_p(int(idx)),
                int(cap_v), int(cap_t), C.byref(nv), C.byref(nt), 1))
            return int(nv.value), int(nt.value)
        self._check(self._lib.vrhip_isosurface_count_indexed(self._h, C.byref(p), C.byref(nv), C.byref(nt)))
        m, n = int(nv.value), int(nt.value)
        vtx = np.empty((m, 3), dtype=np.float32)
        nrm = np.empty((m, 3), dtype=np.float32) if normals else None
        idx = np.empty((n, 3), dtype=np.uint32)
        if n:
            self._check(self._lib.vrhip_isosurface_extract_indexed(
                self._h, C.byref(p), vtx.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p) if normals else None,
                idx.ctypes.data_as(C.c_void_p), m, n, C.byref(nv), C.byref(nt), 0))
            if (int(nv.value), int(nt.value)) != (m, n):
                raise RuntimeError("extract_isosurface_indexed: the volume changed between the count and the extraction")
        return vtx, nrm, idx

    def lastIndexedMeshInfo(self):
        """What the last isosurface_count_indexed / extract_isosurface_indexed did (vrhip_last_indexed_mesh_info):
        vertices, triangles, point_blocks (of 8^3 grid points that own an edge of the region), point_blocks_skipped,
        blocks, blocks_skipped (the cube blocks, as lastMeshInfo), scratch_bytes (device memory beyond the
        destinations), empty_skip -- as a dict."""
        mi = _lib.IndexedMeshInfo()
        self._check(self._lib.vrhip_last_indexed_mesh_info(self._h, C.byref(mi)))
        return mi.as_dict()

    # ---- volume statistics (include/vrhip.h "volume statistics")
    @staticmethod
    def _stats_params(bins, window, region, moments):
        p = _lib.StatsParams()
        p.bins_v, p.bins_g = int(bins[0]), int(bins[1])
        p.v_lo, p.v_hi, p.g_hi = float(window[0]), float(window[1]), float(window[2])
        p.flags = _lib.STATS_MOMENTS if moments else 0
        if region is not None:
            lo, hi = region
            p.lo[:] = [int(v) for v in lo]
            p.hi[:] = [int(v) for v in hi]
        return p

    def volume_statistics(self, bins=(256, 1), window=(0.0, 1.0, 1.0), region=None, moments=False, out_dev_ptr=None):
        """What is in the current time step (vrhip_volume_statistics), computed on the device: (stats, hist).  stats is
        a dict -- voxels, nan, below, above, gradient_nan, binned, and with moments min, max, sum, sum_sq of the
        normalised value s (0 without) --, hist a uint64 ndarray [bins_g, bins_v]: value bins over window[0] <= s <=
        window[1], gradient-magnitude bins (central differences in index space) over [0, window[2]), the top one
        open-ended.  region = ((x0, y0, z0), (x1, y1, z1)) in voxels, lo <= v < hi; None: the whole volume.
        frontend.mean_std and frontend.otsu_threshold turn the result into a mean and an isoValue.
        With out_dev_ptr -- a device address, 16-byte aligned, of bins_g * bins_v 64-bit words -- the table is
        written there and only stats is returned.  The camera, the technique and the frame buffer are neither read
        nor touched."""
        p = self._stats_params(bins, window, region, moments)
        if self._lib.vrhip_stats_params_check(C.byref(p)) != _lib.OK:   # (before the table is sized by the bins)
            raise ValueError("volume_statistics: bins, window or gradient range out of range")
        st = _lib.VolumeStats()
        if out_dev_ptr is not None:
            self._check(self._lib.vrhip_volume_statistics(self._h, C.byref(p), C.byref(st), C.c_void_p(int(out_dev_ptr)), 1))
            return st.as_dict()
        hist = np.empty((p.bins_g, p.bins_v), dtype=np.uint64)
        self._check(self._lib.vrhip_volume_statistics(self._h, C.byref(p), C.byref(st), hist.ctypes.data_as(C.c_void_p), 0))
        return st.as_dict(), hist

    def lastStatsInfo(self):
        """What the last volume_statistics did (vrhip_last_stats_info): blocks (of 8^3 voxels that hold a voxel of the
        region), blocks_fetched, blocks_skipped_constant, blocks_skipped_window (by the cell grid, object-order ESS
        on), scratch_bytes, empty_skip (1: the cell grid was handed to the kernel), hist_path (_lib.STATS_PATH_LDS or
        _lib.STATS_PATH_GLOBAL) -- as a dict."""
        si = _lib.StatsInfo()
        self._check(self._lib.vrhip_last_stats_info(self._h, C.byref(si)))
        return si.as_dict()

    # ---- volume filters (include/vrhip.h "volume filters")
    @staticmethod
    def _filter_params(kind, taps, radius):
        p = _lib.FilterParams()
        kinds = {"separable": _lib.FILTER_SEPARABLE, "median3": _lib.FILTER_MEDIAN3}
        if kind not in kinds:
            raise ValueError("filter_volume: kind must be 'separable' or 'median3'")
        p.kind = kinds[kind]
        if kind == "median3":
            if taps is not None or (radius is not None and any(int(v) for v in np.atleast_1d(radius))):
                raise ValueError("filter_volume: the median takes neither taps nor a radius")
            return p
        if taps is None:
            raise ValueError("filter_volume: separable needs taps")
        taps = list(taps)
        if len(taps) and np.isscalar(taps[0]):   # one tap vector: the same on every axis
            taps = [taps, taps, taps]
        if len(taps) != 3:
            raise ValueError("filter_volume: taps is one sequence of weights, or one per axis")
        taps = [np.asarray(t, dtype=np.float32).ravel() for t in taps]
        if radius is None:
            radius = [max(t.size - 1, 0) for t in taps]
        elif np.isscalar(radius):
            radius = [radius] * 3
        radius = [int(v) for v in radius]
        for a in range(3):
            if not 0 <= radius[a] <= _lib.FILTER_MAX_RADIUS or taps[a].size < radius[a] + 1:
                raise ValueError("filter_volume: a radius is 0..8 and needs radius + 1 taps")
            p.radius[a] = radius[a]
            for k in range(radius[a] + 1):
                p.taps[a][k] = float(taps[a][k])
        return p

    def filter_volume(self, kind="separable", taps=None, radius=None, dst=None):
        """Filter channel 0 of the current time step on the device (vrhip_filter_volume) into time step dst -- None:
        the current one, in place; the number of steps: a new one.  kind "separable": taps is one sequence of weights
        w[0 .. R] (the weight at distance k, used on both sides) for all axes or one per axis (x, y, z), radius the
        R per axis (None: len(taps) - 1); three fp32 passes x, y, z with neighbours clamped to the volume
        (frontend.gaussian_taps makes Gaussian weights).  kind "median3": the median of the 3x3x3 neighbourhood.
        The destination is a step like an uploaded one: the ESS bricks are rebuilt here, as loadVolumeData does,
        when a transfer function is set.  Returns dst."""
        if not self._vol_loaded:
            raise RuntimeError("No volume data is loaded.")
        p = self._filter_params(kind, taps, radius)
        if self._lib.vrhip_filter_params_check(C.byref(p)) != _lib.OK:
            raise ValueError("filter_volume: radius or taps out of range")
        dst = self._timestep if dst is None else int(dst)
        self._check(self._lib.vrhip_filter_volume(self._h, C.byref(p), dst))
        if dst >= self._res[3]:
            self._res[3] = dst + 1
        if self._histograms:
            h = self.volumeHistogram(dst)
            if dst < len(self._histograms):
                self._histograms[dst] = h
            else:
                self._histograms.append(h)
        if getattr(self, "_tff", None) is not None:
            self._generate_bricks()
        if dst == self._timestep:
            self._rendering.iteration = 0
        return dst

    def lastFilterInfo(self):
        """What the last filter_volume did (vrhip_last_filter_info): blocks (of 8^3 voxels), blocks_fetched,
        blocks_skipped (constant by the cell grid, object-order ESS on), scratch_bytes (device memory the call held:
        the in-place copy and the counters), empty_skip (1: the cell grid was handed to the kernel), in_place -- as a
        dict."""
        fi = _lib.FilterInfo()
        self._check(self._lib.vrhip_last_filter_info(self._h, C.byref(fi)))
        return fi.as_dict()

    # ---- volume morphology (include/vrhip.h "volume morphology")
    def morph_volume(self, op, radius, shape="ball", dst=None):
        """Grey-scale morphology of channel 0 of the current time step on the device (vrhip_morph_volume) into time step
        dst -- None: the current one, in place; the number of steps: a new one.  op: "erode", "dilate", "open", "close",
        "gradient", "tophat" or "blackhat"; shape "box" or "ball"; radius 0..8, one for all axes or (x, y, z);
        neighbours clamped to the volume (frontend.morph_element lists the structuring element).  The destination is
        a step like an uploaded one: the ESS bricks are rebuilt here, as loadVolumeData does, when a transfer function
        is set.  Returns dst."""
        if not self._vol_loaded:
            raise RuntimeError("No volume data is loaded.")
        p = frontend.morph_params(op, radius, shape)
        if self._lib.vrhip_morph_params_check(C.byref(p)) != _lib.OK:
            raise ValueError("morph_volume: op, shape or radius out of range")
        dst = self._timestep if dst is None else int(dst)
        self._check(self._lib.vrhip_morph_volume(self._h, C.byref(p), dst))
        if dst >= self._res[3]:
            self._res[3] = dst + 1
        if self._histograms:
            h = self.volumeHistogram(dst)
            if dst < len(self._histograms):
                self._histograms[dst] = h
            else:
                self._histograms.append(h)
        if getattr(self, "_tff", None) is not None:
            self._generate_bricks()
        if dst == self._timestep:
            self._rendering.iteration = 0
        return dst

    def lastMorphInfo(self):
        """What the last morph_volume did (vrhip_last_morph_info): per sweep (lists of two) blocks (of 8^3 voxels),
        blocks_fetched and blocks_skipped (constant by the cell grid, object-order ESS on); sweeps (1 or 2),
        scratch_bytes (device memory the call held: full-size scratches and the counters), empty_skip (1: the cell
        grid was handed to the kernel), in_place -- as a dict."""
        mi = _lib.MorphInfo()
        self._check(self._lib.vrhip_last_morph_info(self._h, C.byref(mi)))
        return mi.as_dict()

    # ---- volume
    def loadVolumeData(self, props, ingest="host"):
        """volumerendercl.cpp:765-805. `props` is a datraw.Properties (dat_file_name or
        raw_file_names set).  ingest="device": the loader only reads the files; maximum, USHORT
        stretch / FLOAT normalisation and histogram are computed in HBM (vrhip_ingest_raw), bit for
        bit what the host loader (ingest="host", the default) computes."""
        from . import datraw
        if ingest not in ("host", "device"):
            raise ValueError("ingest must be 'host' or 'device'")
        self._vol_loaded = False
        try:
            reader = datraw.DatRawReader()
            reader.read_files(props, convert=(ingest == "host"))
        except ValueError as e:      # std::invalid_argument -> runtime_error (:784-787)
            raise RuntimeError(str(e))
        p = reader.properties()
        vols = reader.data()
        self._histograms = reader.histograms()
        self._props = p
        co = p.image_channel_order
        if co in ("R", "", "I", "LUMINANCE"):
            channels = 1
        elif co == "RG":
            channels = 2
        elif co == "RGBA":
            channels = 4
        elif co in ("ARGB", "BGRA"):   # uploaded by the reference, but its kernel has no branch for them
            raise RuntimeError("ARGB / BGRA volumes are not supported.")
        else:
            raise RuntimeError("Unknown or invalid volume color format.")   # :711
        if ingest == "device":
            return self._ingest_raw(vols, p, channels)
        return self.loadVolumeArrays(vols, p.format, p.slice_thickness, p.volume_res[:3],
                                     channels=channels)

    def _ingest_raw(self, raws, p, channels):
        """The device-ingest half of loadVolumeData: raw file bytes -> vrhip_ingest_raw per time step;
        fills the histograms and the properties' min_value / max_value as the host loader does."""
        if p.format not in NP_DTYPE:
            raise RuntimeError("Unknown or invalid volume data format.")
        self._check(self._lib.vrhip_clear_volumes(self._h))
        self._histograms = []
        for t, raw in enumerate(raws):
            raw = np.ascontiguousarray(raw, dtype=np.uint8)
            hist, vmax = (C.c_double * 256)(), C.c_float()
            rc = self._lib.vrhip_ingest_raw(self._h, raw.ctypes.data_as(C.c_void_p), raw.nbytes,
                                            _u3(p.volume_res[:3]), p.format, int(channels),
                                            int(p.endianness), t, hist, C.byref(vmax))
            if rc == _lib.ERR_INVALID:   # the size check of loadVolumeData throws std::runtime_error
                raise RuntimeError(self._lib.vrhip_last_error(self._h).decode())
            self._check(rc)
            self._histograms.append(np.array(hist))
            p.min_value, p.max_value = 0.0, float(vmax.value)
        self._finish_load(p.volume_res[:3], len(raws), p.format, p.slice_thickness)
        return len(raws)

    def lastIngestSeconds(self):
        return float(self._lib.vrhip_last_ingest_seconds(self._h))

    def volumeHistogram(self, t=0):
        """vrhip_volume_histogram: the loader's binning of the values stored in time step t."""
        hist = (C.c_double * 256)()
        self._check(self._lib.vrhip_volume_histogram(self._h, int(t), hist))
        return np.array(hist)

    def _finish_load(self, r, n_steps, fmt, thickness):
        self._res = [int(r[0]), int(r[1]), int(r[2]), int(n_steps)]
        self._format = fmt
        self._thickness = [float(x) for x in thickness]
        self._calc_scaling()
        # default prefix sum of the linear ramp (volumerendercl.cpp:795-801)
        prefix = np.cumsum(np.arange(1024, dtype=np.uint64) * 4).astype(np.uint32)
        self._vol_loaded = True
        self.setTffPrefixSum(prefix)

    def loadVolumeArrays(self, volumes, fmt, thickness=(1.0, 1.0, 1.0), res=None, channels=None):
        """Upload already-decoded time steps (ndarray [z, y, x], [z, y, x, c] for CL_RG / CL_RGBA
        volumes, or flat with `res` and `channels`) -- the volDataToCLmem + calcScaling + default
        prefix-sum part of loadVolumeData."""
        self._vol_loaded = False
        self._check(self._lib.vrhip_clear_volumes(self._h))
        for t, v in enumerate(volumes):
            v = np.ascontiguousarray(v, dtype=NP_DTYPE[fmt])
            r = res if res is not None else (v.shape[2], v.shape[1], v.shape[0])
            nch = channels if channels is not None else (v.shape[3] if v.ndim == 4 else 1)
            if v.size < int(r[0]) * int(r[1]) * int(r[2]) * nch:
                raise RuntimeError("Volume size does not match size specified in dat file.")
            self._check(self._lib.vrhip_upload_volume_channels(
                self._h, v.ctypes.data_as(C.c_void_p), _u3(r), fmt, int(nch), t))
        self._finish_load(r, len(volumes), fmt, thickness)
        return len(volumes)

    def synthVolume(self, kind, res, fmt):
        """SURVEY 8(d) synthetic input generated in HBM (no host copy)."""
        self._vol_loaded = False
        self._check(self._lib.vrhip_clear_volumes(self._h))
        self._check(self._lib.vrhip_synth_volume(self._h, {"sphere": 0, "shells": 1}[kind],
                                                 _u3(res), fmt, 0))
        self._res = [int(res[0]), int(res[1]), int(res[2]), 1]
        self._format = fmt
        self._thickness = [1.0, 1.0, 1.0]
        self._calc_scaling()
        self._vol_loaded = True
        self._histograms = [self.volumeHistogram(0)]   # what the TF editor draws under the curve

    def downsampleVolume(self, t, factor):
        """Device part of volumeDownsampling (volumerendercl.cpp:238-300 + kernel
        `downsampling`): returns the low-res ndarray [z, y, x] of time step t."""
        lo = (C.c_uint32 * 3)()
        self._check(self._lib.vrhip_downsample_volume(self._h, int(t), int(factor), None, 0, lo))
        out = np.empty((lo[2], lo[1], lo[0]), dtype=NP_DTYPE[self._format])
        self._check(self._lib.vrhip_downsample_volume(self._h, int(t), int(factor),
                                                      out.ctypes.data_as(C.c_void_p), out.nbytes, lo))
        return out

    def volumeDownsampling(self, t, factor):
        """volumerendercl.cpp:238-341: down-sample time step t on the GPU and write
        <dat name>_<N>.raw / .dat next to the loaded .dat (the reference's text, quirks included:
        `Format:` carries the enum's integer, `ObjectFileName:` is cut with substr(first + 1,
        lastindex)).  Returns the path without extension."""
        props = getattr(self, "_props", None)
        if not self._vol_loaded or props is None or not props.dat_file_name:
            raise RuntimeError("No volume data is loaded.")
        if factor < 2:
            raise ValueError("Factor must be greater or equal 2.")
        low = self.downsampleVolume(t, factor)
        name = props.dat_file_name
        dot = name.rfind(".")
        rawname = (name[:dot] if dot >= 0 else name) + "_" + str(low.shape[2])
        low.tofile(rawname + ".raw")
        last = rawname.rfind(".")
        first = max(rawname.rfind("/"), rawname.rfind("\\"))
        short = rawname[first + 1:] if last < 0 else rawname[first + 1:first + 1 + last]
        with open(rawname + ".dat", "w") as f:
            f.write("ObjectFileName: \t%s.raw\n" % short)
            f.write("Resolution: \t\t%d %d %d\n" % (low.shape[2], low.shape[1], low.shape[0]))
            f.write("SliceThickness: \t%g %g %g\n" % tuple(props.slice_thickness[:3]))
            f.write("Format: \t\t\t%d\n" % int(props.format))
        return rawname

    def downloadVolume(self, t=0):
        out = np.empty((self._res[2], self._res[1], self._res[0]), dtype=NP_DTYPE[self._format])
        self._check(self._lib.vrhip_download_volume(self._h, t, out.ctypes.data_as(C.c_void_p),
                                                    out.nbytes))
        return out

    def _calc_scaling(self):
        """calcScaling, volumerendercl.cpp:347-362 (valarray<float> arithmetic)."""
        res = np.array(self._res[:3], dtype=np.float32)
        th = np.array(self._thickness, dtype=np.float32)
        s = res * (th * (np.float32(1.0) / th[0]))
        self._model_scale = (s.max() / s).astype(np.float32)

    def hasData(self):
        return self._vol_loaded

    def getResolution(self):
        if not self._vol_loaded:
            return [0, 0, 0, 1]
        return list(self._res)

    def createEnvironmentMap(self, file_name):
        """volumerendercl.cpp:1121-1150: Radiance .hdr file -> float RGBA environment map; an
        empty name installs the reference's 1x1 white map, which the kernel never samples."""
        if not file_name:
            self.setEnvironmentMap(None)
            return
        from . import datraw
        self.setEnvironmentMap(datraw.load_hdr(file_name))

    def setEnvironmentMap(self, rgba):
        """float32 [height, width, 4] texels, or None to remove the map."""
        if rgba is None:
            self._check(self._lib.vrhip_set_environment_map(self._h, None, 0, 0))
            return
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("environment map must be [height, width, 4]")
        self._check(self._lib.vrhip_set_environment_map(self._h, rgba.ctypes.data,
                                                        rgba.shape[1], rgba.shape[0]))

    def getHistogram(self, timestep=0):
        if not self._vol_loaded:
            raise ValueError("Invalid timestep for histogram data.")
        return self._histograms[timestep]

    def scaleVolume(self, scale):
        self._model_scale = (self._model_scale * np.asarray(scale, dtype=np.float32)).astype(
            np.float32)

    # ---- transfer function
    def setTransferFunction(self, tff):
        """volumerendercl.cpp:864-891: upload RGBA8 table, rebuild the ESS bricks, set the
        inclusive prefix sum of the alpha bytes, reset the iteration."""
        if not self._vol_loaded:
            return
        tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1)
        self._tff = tff.copy()
        self._check(self._lib.vrhip_set_transfer_function(
            self._h, tff.ctypes.data_as(C.c_void_p), tff.size // 4))
        self._generate_bricks()
        prefix = np.cumsum(tff[3::4].astype(np.uint64)).astype(np.uint32)
        self.setTffPrefixSum(prefix)
        self._rendering.iteration = 0

    def setTffPrefixSum(self, prefix):
        if not self._vol_loaded:
            return
        prefix = np.ascontiguousarray(prefix, dtype=np.uint32)
        self._prefix = prefix.copy()
        self._check(self._lib.vrhip_set_tff_prefix_sum(
            self._h, prefix.ctypes.data_as(C.c_void_p), prefix.size))

    def _generate_bricks(self):
        self._check(self._lib.vrhip_build_bricks(self._h))
        brf = (C.c_float * 3)()
        self._check(self._lib.vrhip_get_brick_info(self._h, None, brf, None))
        self._raycast.brickRes[:] = [brf[0], brf[1], brf[2], 0.0]   # :627-631

    def brickInfo(self):
        tex, brf, edge = (C.c_uint32 * 3)(), (C.c_float * 3)(), (C.c_uint32 * 3)()
        self._check(self._lib.vrhip_get_brick_info(self._h, tex, brf, edge))
        return list(tex), list(brf), list(edge)

    def downloadBricks(self, t=0):
        tex, _, _ = self.brickInfo()
        out = np.empty((tex[2], tex[1], tex[0], 2), dtype=NP_DTYPE[self._format])
        self._check(self._lib.vrhip_download_bricks(self._h, t, out.ctypes.data_as(C.c_void_p),
                                                    out.nbytes))
        return out

    def downloadCells(self, fine=False):
        """(min, max) of every cell of the cell grid (vrhip_download_cells; fine: the grid of the ray
        caster's empty bits, vrhip_download_empty_cells): ndarray [cz, cy, cx, 2], shift."""
        fn = self._lib.vrhip_download_empty_cells if fine else self._lib.vrhip_download_cells
        dims, shift = (C.c_uint32 * 3)(), C.c_uint32()
        self._check(fn(self._h, None, 0, dims, C.byref(shift)))
        out = np.empty((dims[2], dims[1], dims[0], 2), dtype=np.float32)
        self._check(fn(self._h, out.ctypes.data_as(C.c_void_p), out.size, dims, C.byref(shift)))
        return out, int(shift.value)

    def downloadCellTables(self):
        """What the renderer derives from the cell grids and the transfer function (vrhip_download_cell_tables), rebuilt
        and copied out: dict of bound [cz, cy, cx] and macro [ccz, ccy, ccx] float32, leap [7, ccz, ccy, ccx] uint8,
        empty (uint32 words of the fine grid's bits), fine_dims (ecz, ecy, ecx), shift, eshift."""
        fn = self._lib.vrhip_download_cell_tables
        dims, shifts = (C.c_uint32 * 9)(), (C.c_uint32 * 2)()
        self._check(fn(self._h, None, 0, None, 0, None, 0, None, 0, dims, shifts))
        cx, cy, cz, ccx, ccy, ccz, ecx, ecy, ecz = (int(d) for d in dims)
        bound = np.empty((cz, cy, cx), dtype=np.float32)
        macro = np.empty((ccz, ccy, ccx), dtype=np.float32)
        leap = np.empty((7, ccz, ccy, ccx), dtype=np.uint8)
        empty = np.empty((ecx * ecy * ecz + 31) // 32, dtype=np.uint32)
        self._check(fn(self._h, bound.ctypes.data_as(C.c_void_p), bound.size, macro.ctypes.data_as(C.c_void_p), macro.size,
                       leap.ctypes.data_as(C.c_void_p), leap.size, empty.ctypes.data_as(C.c_void_p), empty.size,
                       dims, shifts))
        return {"bound": bound, "macro": macro, "leap": leap, "empty": empty, "fine_dims": (ecz, ecy, ecx),
                "shift": int(shifts[0]), "eshift": int(shifts[1])}

    def lastBricksSeconds(self):
        return float(self._lib.vrhip_last_bricks_seconds(self._h))

    # ---- setters (volumerendercl.cpp:922-1047,1157-1174)
    def setCamOrtho(self, v):
        self._camera.ortho = 1 if v else 0

    def setIllumination(self, illum):
        self._rendering.illumType = int(illum)

    def setAmbientOcclusion(self, ao):
        self._raycast.useAO = 1 if ao else 0

    def setShowESS(self, v):
        self._rendering.showEss = 1 if v else 0

    def setLinearInterpolation(self, v):
        self._rendering.useLinear = 1 if v else 0

    def setContours(self, v):
        self._raycast.contours = 1 if v else 0

    def setAerial(self, v):
        self._raycast.aerial = 1 if v else 0

    def setImgEss(self, v):
        self._rendering.imgEss = 1 if v else 0

    def setObjEss(self, v):
        """The reference rebuilds its program with/without -DESS; here a variant switch."""
        self._obj_ess = bool(v)
        self._check(self._lib.vrhip_set_object_ess(self._h, 1 if v else 0))

    def setBackground(self, color):
        # the reference converts through cl_float3: alpha becomes 0 (volumerendercl.cpp:1027)
        self._rendering.backgroundColor[:] = [float(color[0]), float(color[1]), float(color[2]),
                                              0.0]

    def setUseGradient(self, v):
        self._rendering.useGradient = 1 if v else 0

    def setTechnique(self, tech):
        """TECH_RAYCAST (0), TECH_PATHTRACE (1), TECH_MIP (2, maximum intensity projection), TECH_ISO (4, first-hit
        isosurface: setIsoValue, setIsoRefinement), TECH_TF2D (6, 2-D transfer function: setTransferFunction2D) or
        TECH_PREINT (8, pre-integrated classification of the 1-D transfer function: no parameters of its own);
        include/vrhip.h."""
        self._rendering.technique = int(tech)
        self._rendering.iteration = 0

    def setExtinction(self, extinction):
        self._pathtrace.max_extinction = float(extinction)

    def setIsoValue(self, value):
        """TECH_ISO: the threshold, in the units of the transfer function's coordinate (normalised for UCHAR / USHORT
        volumes, the raw value for FLOAT).  Default 0.5."""
        self._iso.isoValue = float(value)

    def setIsoRefinement(self, steps):
        """TECH_ISO: bisection rounds between the last sample below and the first at or above the threshold (0-16).
        Default 4."""
        self._iso.refineSteps = int(steps)

    def setTransferFunction2D(self, table, g_hi):
        """TECH_TF2D: the 2-D transfer function TF2(value, gradient magnitude).  table: uint8 [n_g, n_v, 4] (row j =
        gradient bin j, value fastest); g_hi: the gradient magnitude at the table's upper edge, the g_hi of
        volume_statistics, whose bin centres the entries sit on (frontend.tf2d_from_1d, frontend.tf2d_ramp make
        tables).  State of its own: setTransferFunction does not touch it and is not needed by TECH_TF2D."""
        table = np.ascontiguousarray(table, dtype=np.uint8)
        if table.ndim != 3 or table.shape[2] != 4:
            raise ValueError("the 2-D transfer function must have shape (n_g, n_v, 4)")
        self._check(self._lib.vrhip_set_transfer_function_2d(self._h, table.ctypes.data, table.shape[1], table.shape[0],
                                                             float(g_hi)))
        self._tf2d = (table.copy(), float(g_hi))   # (shareVolumes hands it to the twin)
        self._rendering.iteration = 0

    def setBBox(self, bl_x, bl_y, bl_z, tr_x, tr_y, tr_z):
        self._camera.bbox_bl[:] = [bl_x, bl_y, bl_z, 0]
        self._camera.bbox_tr[:] = [tr_x, tr_y, tr_z, 0]
        self._rendering.iteration = 0

    def setTimestep(self, t):
        if self._vol_loaded and t >= self._res[3]:
            return
        self._timestep = int(t)
        self._check(self._lib.vrhip_set_timestep(self._h, int(t)))
        self._rendering.iteration = 0

    def getLastExecTime(self):
        return float(self._lib.vrhip_last_kernel_seconds(self._h))

    def setPhaseTiming(self, v):
        """Record an event between the two phases of a frame (vrhip_set_phase_timing; off by default:
        the event costs GPU time)."""
        self._check(self._lib.vrhip_set_phase_timing(self._h, 1 if v else 0))

    def setFrameTiming(self, v):
        """Record the two events around a frame's launches (vrhip_set_frame_timing; on by default, as the
        reference times every frame, volumerendercl.cpp:545-551).  Off: getLastExecTime() answers 0 and frames
        that follow each other without a wait lose the events' GPU time."""
        self._check(self._lib.vrhip_set_frame_timing(self._h, 1 if v else 0))

    def getLastPhaseTimes(self):
        """(phase-1 seconds, phase-2 seconds) of the last ray-cast pass rendered with setPhaseTiming(True);
        (0.0, 0.0) when the last pass was not phase-timed."""
        a, b = C.c_double(), C.c_double()
        if self._lib.vrhip_last_phase_seconds(self._h, C.byref(a), C.byref(b)) != _lib.OK:
            return 0.0, 0.0
        return float(a.value), float(b.value)

    def lastLaunchInfo(self):
        """What the last render call launched (vrhip_last_launch_info): kernel variants, waves per workgroup,
        round budget, lookahead, frames of the set -- as a dict."""
        li = _lib.LaunchInfo()
        self._check(self._lib.vrhip_last_launch_info(self._h, C.byref(li)))
        return li.as_dict()

    def downloadRayOrder(self):
        """The pixel-major ray order of the launch set just rendered (vrhip_download_ray_order; RuntimeError unless the
        last render call was a set with lastLaunchInfo()["pixel_major"] == 1), as a dict: set_frames, n_items, group,
        live_list_cap, pm_list_cap; items int64 [n, 3] (patch column, patch row, frame) in queue order; ballot uint64 [n]
        (bit = 8 * row + column of the patch) and first int64 [n] (position of the item's first record), from notes
        (the 3 n words as they are); ray_counts and index_counts (eight each); records, a list of eight int64
        [count, 4] (gx, gy, frame, position in the ray lists); index, a list of eight uint32 arrays (0xffffffff pads)."""
        fn = self._lib.vrhip_download_ray_order
        sizes, counters = (C.c_uint32 * 8)(), (C.c_uint32 * 16)()
        self._check(fn(self._h, sizes, None, 0, None, 0, counters, None, 0, None, 0))
        sf, n, group, ray_cap, idx_cap, n_rec, n_ent = (int(v) for v in sizes[:7])
        items = np.empty((n, 3), dtype=np.uint32)
        notes = np.empty(3 * n, dtype=np.uint32)
        recs = np.empty((n_rec, 4), dtype=np.uint32)
        ents = np.empty(n_ent, dtype=np.uint32)
        self._check(fn(self._h, sizes, items.ctypes.data_as(C.c_void_p), items.size, notes.ctypes.data_as(C.c_void_p),
                       notes.size, counters, recs.ctypes.data_as(C.c_void_p), recs.size, ents.ctypes.data_as(C.c_void_p),
                       ents.size))
        ray_counts = [int(v) for v in counters[:8]]
        index_counts = [int(v) for v in counters[8:]]
        rcut = np.cumsum([0] + [min(c, ray_cap) for c in ray_counts])
        icut = np.cumsum([0] + [min(c, idx_cap) for c in index_counts])
        ballot = notes[0:2 * n:2].astype(np.uint64) | (notes[1:2 * n:2].astype(np.uint64) << np.uint64(32))
        return {"set_frames": sf, "n_items": n, "group": group, "live_list_cap": ray_cap, "pm_list_cap": idx_cap,
                "items": items.astype(np.int64), "notes": notes, "ballot": ballot, "first": notes[2 * n:].astype(np.int64),
                "ray_counts": ray_counts, "index_counts": index_counts,
                "records": [recs[rcut[k]:rcut[k + 1]].astype(np.int64) for k in range(8)],
                "index": [ents[icut[k]:icut[k + 1]].copy() for k in range(8)]}

    # ---- test / bench conveniences (not in the reference)
    def setSeed(self, seed):
        """Pin the per-frame jitter seed (None restores the mt19937 sequence).  params() shows a pinned seed at
        once, not only after the next frame."""
        self._fixed_seed = None if seed is None else int(seed) & 0xFFFFFFFF
        if self._fixed_seed is not None:
            self._rendering.seed = self._fixed_seed

    def setIteration(self, it):
        self._rendering.iteration = int(it)

    def setStatsEnabled(self, v):
        self._check(self._lib.vrhip_set_stats_enabled(self._h, 1 if v else 0))

    def getStats(self):
        st = Stats()
        self._check(self._lib.vrhip_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def countTouched(self, width, height, want_bitmap=False):
        n = C.c_uint64()
        bm = None
        if want_bitmap:
            mb = [(r + 3) // 4 for r in self._res[:3]]
            bm = np.zeros((mb[0] * mb[1] * mb[2] + 7) // 8, dtype=np.uint8)
        self._push_params()
        self._check(self._lib.vrhip_count_touched(
            self._h, int(width), int(height), C.byref(n),
            bm.ctypes.data_as(C.c_void_p) if bm is not None else None,
            bm.nbytes if bm is not None else 0))
        return int(n.value), bm

    def countFetched(self, width, height):
        """technique 1: micro-bricks the product's own fetches touch (vrhip_count_fetched)."""
        n = C.c_uint64()
        self._push_params()
        self._check(self._lib.vrhip_count_fetched(self._h, int(width), int(height), C.byref(n)))
        return int(n.value)

    def countTouchedTiles(self, width, height, tile_w, tile_h, tile_ids):
        n = C.c_uint64()
        ids = np.ascontiguousarray(tile_ids, dtype=np.uint32)
        self._push_params()
        self._check(self._lib.vrhip_count_touched_tiles(
            self._h, int(width), int(height), int(tile_w), int(tile_h),
            ids.ctypes.data_as(C.c_void_p), int(ids.size), C.byref(n)))
        return int(n.value)

    def params(self):
        """Copies of the four kernel-argument structs as they will be pushed."""
        self._rendering.modelScale[:] = [float(self._model_scale[0]), float(self._model_scale[1]),
                                         float(self._model_scale[2]), 0.0]
        return self._camera, self._rendering, self._raycast, self._pathtrace

    def isoParams(self):
        """The IsoParams of TECH_ISO as they will be pushed (setIsoValue, setIsoRefinement)."""
        return self._iso
