#!/usr/bin/env python3
"""tools/slice_time.py [VIEWPORT] -- what the slice views (vrhip_render_slices) cost, on one GPU; prints one JSON line.
Scenes: 2048^3 UCHAR shells and 1024^3 FLOAT shells, VIEWPORT^2 pixels (default 1024), linear filter, transfer-function
output.  Per scene, in ms per call, HIP events, the median of 20 after 3 warm-ups, images left on the device:
  thin_axial       one thin slice perpendicular to z
  thin_oblique     one thin slice perpendicular to (1, 1, 1)
  slab64           one 64-sample mean slab, 0.25 box units thick, perpendicular to z
  stack64_one_call 64 thin axial slices spanning the box, one call
  stack64_64_calls the same 64 slices, one call each
For every case also `bytes`: a LOWER bound of the voxel bytes touched -- the distinct 64-byte lines that hold the voxel
floor(tex * res) of a taken sample (the eight taps of the linear filter touch these and more) -- and `hbm_fraction` =
bytes / time / HBM_PEAK.  Before anything is timed a small case is compared with the CPU restatement bit for bit."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from tests import slice_ref
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL, frontend

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
WARM, REPS = 3, 20
HBM_PEAK = 8.0e12   # bytes per second, MI355X
dev = torch.device("cuda", 0)


def median_of(fn):
    for _ in range(WARM):
        fn()
    return statistics.median(fn() for _ in range(REPS))


def events(fn):
    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)
    return timed


def parity():
    vr = VolumeRenderCL(); vr.initialize()
    vol = (np.random.default_rng(1).random((33, 9, 17), dtype=np.float32) * 255).astype(np.uint8)
    tff = frontend.tff_from_stops()
    vr.loadVolumeArrays([vol], UCHAR)
    vr.setTransferFunction(tff)
    slices = [frontend.axis_slice("z", 0.1), frontend.plane_slice([0, 0, 0], [1, 1, 1], [0, 0, 1], 1.5, 1.5, 0.5, 7, "mean"),
              frontend.axis_slice("x", -0.2, 0.6, 64, "min", "value")]
    got = vr.render_slices(37, 21, slices)
    ref = slice_ref.render_all(vol, slice_ref.UCHAR, tff, slices, True, list(vr.params()[1].backgroundColor), 37, 21)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "slice views differ from their restatement"
    vr.close()


def line_bytes(slices, n, fmt):
    """Lower bound of the bytes touched: distinct 64-byte lines of the voxels floor(tex * res) of the taken samples."""
    lines = []
    g = (2.0 * (torch.arange(V, device=dev, dtype=torch.float64) + 0.5)) / V - 1.0
    sx, sy = g[None, :, None], -g[:, None, None]
    nb = (n + 3) // 4
    for s in slices:
        o, u, v, w = (torch.tensor(list(getattr(s, k)[:3]), device=dev, dtype=torch.float64) for k in ("origin", "u", "v", "w"))
        p = o + sx * u + sy * v
        for k in range(s.samples):
            tex = (p + ((k + 0.5) / s.samples - 0.5) * w) * 0.5 + 0.5
            ok = ((tex >= 0) & (tex <= 1)).all(dim=-1)
            i = (tex[ok] * n).floor().clamp_(0, n - 1).to(torch.int64)
            brick = ((i[:, 2] >> 2) * nb + (i[:, 1] >> 2)) * nb + (i[:, 0] >> 2)
            # a micro-brick of 64 voxels: one line of UCHAR, four of FLOAT (one per z & 3)
            lines.append(torch.unique(brick if fmt == UCHAR else brick * 4 + (i[:, 2] & 3)))
    return int(torch.unique(torch.cat(lines)).numel()) * 64


parity()
out = {"tool": "slice_time", "viewport": V, "reps": REPS, "warmups": WARM, "hbm_peak_bytes_per_s": HBM_PEAK}
for name, n, fmt in (("shells2048_uchar", 2048, UCHAR), ("shells1024_float", 1024, FLOAT)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    img = torch.zeros((64, V, V, 4), dtype=torch.float32, device=dev)
    stack = frontend.slice_stack(frontend.axis_slice("z", 0.0), 64, 2.0)
    cases = {
        "thin_axial": [frontend.axis_slice("z", 0.1)],
        "thin_oblique": [frontend.plane_slice([0, 0, 0], [1, 1, 1], [0, 0, 1], 1.0, 1.0)],
        "slab64": [frontend.axis_slice("z", 0.1, 0.25, 64, "mean")],
        "stack64_one_call": stack,
    }
    res = {}
    for case, slices in cases.items():
        ms = median_of(events(lambda: vr.render_slices(V, V, slices, out_dev_ptr=img.data_ptr())))
        b = line_bytes(slices, n, fmt)
        res[case] = {"ms": round(ms, 4), "bytes": b, "hbm_fraction": round(b / (ms * 1e-3) / HBM_PEAK, 4)}

    def one_by_one():
        for i, s in enumerate(stack):
            vr.render_slices(V, V, [s], out_dev_ptr=img[i].data_ptr())
    ms = median_of(events(one_by_one))
    b = res["stack64_one_call"]["bytes"]
    res["stack64_64_calls"] = {"ms": round(ms, 4), "bytes": b, "hbm_fraction": round(b / (ms * 1e-3) / HBM_PEAK, 4)}
    out[name] = res
    vr.close()
    del img
print(json.dumps(out))
