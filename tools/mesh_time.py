#!/usr/bin/env python3
"""tools/mesh_time.py [OUT.json] -- what an isosurface extraction (vrhip_isosurface_count / _extract) costs, on one
GPU; prints one JSON line and, with an argument, writes it there too.
Scenes: the benchmark's headline volume (2048^3 UCHAR shells) and 1024^3 FLOAT shells, isoValue 0.5, no normals, the
whole volume.  Per scene and with object-order ESS on / off, in ms per call, a host clock around a call that ends in a
synchronise, the median of 20 after 3 warm-ups, with the spread (max - min of the 20) beside it as *_spread_ms:
  count_{ess,noess}     vrhip_isosurface_count: pass 1, the reduce and the scan of its sums, the totals to the host
  extract_{ess,noess}   vrhip_isosurface_extract into device memory: the same with the offsets, then pass 2
and: triangles, blocks, the share of blocks the cell grid skips, triangles per second of an extraction, and the bytes
pass 1 must read -- every voxel once -- over the count's time against the 8 TB/s HBM peak of DESIGN 5.2 (with ESS on
the skipped blocks' voxels are not read: the figure is then the rate at which the volume is dealt with, not traffic).
Before anything is timed the ESS-on and ESS-off lists are compared byte for byte."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL

WARM, REPS = 3, 20
ISO = 0.5
HBM_PEAK = 8.0e12
dev = torch.device("cuda", 0)


def timed(fn):
    def one():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(WARM):
        one()
    t = [one() for _ in range(REPS)]
    return round(statistics.median(t), 4), round(max(t) - min(t), 4)


out = {"tool": "mesh_time", "reps": REPS, "warmups": WARM, "iso_value": ISO, "hbm_peak_bytes_per_s": HBM_PEAK}
for name, n, fmt, size in (("shells2048_uchar", 2048, UCHAR, 1), ("shells1024_float", 1024, FLOAT, 4)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    vr.setObjEss(True)
    tris = vr.isosurface_count(ISO)
    info = vr.lastMeshInfo()
    out[name + "_triangles"], out[name + "_blocks"] = tris, info["blocks"]
    out[name + "_blocks_skipped_share"] = round(info["blocks_skipped"] / info["blocks"], 4)
    a = torch.zeros((tris * 9,), dtype=torch.float32, device=dev)
    b = torch.zeros((tris * 9,), dtype=torch.float32, device=dev)
    for buf, ess in ((a, True), (b, False)):
        vr.setObjEss(ess)
        assert vr.extract_isosurface(ISO, out_dev_ptrs=(buf.data_ptr(), None, tris)) == tris
        torch.cuda.synchronize()
        mi = vr.lastMeshInfo()
        assert mi["empty_skip"] == int(ess) and (ess or mi["blocks_skipped"] == 0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    del b
    volume_bytes = n ** 3 * size
    out[name + "_pass1_bytes"] = volume_bytes
    for ess in (True, False):
        vr.setObjEss(ess)
        tag = "%s_%%s_%s" % (name, "ess" if ess else "noess")
        ms, sp = timed(lambda: vr.isosurface_count(ISO))
        out[tag % "count" + "_ms"], out[tag % "count" + "_spread_ms"] = ms, sp
        out[tag % "count" + "_hbm_share"] = round(volume_bytes / (ms * 1e-3) / HBM_PEAK, 4)
        ms, sp = timed(lambda: vr.extract_isosurface(ISO, out_dev_ptrs=(a.data_ptr(), None, tris)))
        out[tag % "extract" + "_ms"], out[tag % "extract" + "_spread_ms"] = ms, sp
        out[tag % "extract" + "_triangles_per_s"] = round(tris / (ms * 1e-3), 1)
    del a
    vr.close()
line = json.dumps(out)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
