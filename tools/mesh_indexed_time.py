#!/usr/bin/env python3
"""tools/mesh_indexed_time.py [OUT.json] [--host-route] -- what an indexed isosurface extraction
(vrhip_isosurface_count_indexed / _extract_indexed) costs next to the triangle list of the same run, on one GPU; prints
one JSON line and, with an argument, writes it there too.
Scenes: the benchmark's headline volume (2048^3 UCHAR shells) and 1024^3 FLOAT shells, isoValue 0.5, the whole volume,
into device memory.  Per scene: vertices, triangles, the point blocks and the share the cell grid skips, scratch_bytes
and the bytes of both forms of the surface.  Per scene, with object-order ESS on / off and without / with normals, in
ms per call, a host clock around a call that ends in a synchronise, the median of 20 after 3 warm-ups, with the spread
(max - min of the 20) beside it as *_spread_ms:
  count_indexed_*     vrhip_isosurface_count_indexed: pass 1 and its scan, the vertex count and its two scans
  extract_indexed_*   vrhip_isosurface_extract_indexed: the same with the offsets, the vertex emit, the index emit
  extract_soup_*      vrhip_isosurface_extract of the same surface
Before anything is timed vertices[indices] is compared with the triangle list bit for bit, ESS on against ESS off too.
--host-route: the way from the volume to an indexed mesh in host memory without these calls -- the triangle list to
host memory, then frontend.weld_mesh -- timed once, at 1024^3 only (at 2048^3 it takes minutes), next to one indexed
extraction into host memory; without the flag "host_route" says that it was left out."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL, frontend

WARM, REPS = 3, 20
ISO = 0.5
dev = torch.device("cuda", 0)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
HOST_ROUTE = "--host-route" in sys.argv[1:]


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


out = {"tool": "mesh_indexed_time", "reps": REPS, "warmups": WARM, "iso_value": ISO,
       "host_route": "left out (run with --host-route)"}
for name, n, fmt in (("shells2048_uchar", 2048, UCHAR), ("shells1024_float", 1024, FLOAT)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    vr.setObjEss(True)
    nv, nt = vr.isosurface_count_indexed(ISO)
    info = vr.lastIndexedMeshInfo()
    out[name + "_vertices"], out[name + "_triangles"] = nv, nt
    out[name + "_point_blocks"] = info["point_blocks"]
    out[name + "_point_blocks_skipped_share"] = round(info["point_blocks_skipped"] / info["point_blocks"], 4)
    out[name + "_indexed_bytes"], out[name + "_soup_bytes"] = 12 * (nv + nt), 36 * nt
    vtx = torch.zeros((nv, 3), dtype=torch.float32, device=dev)
    nrm = torch.zeros((nv, 3), dtype=torch.float32, device=dev)
    idx = torch.zeros((nt, 3), dtype=torch.int32, device=dev)
    soup = torch.zeros((nt, 3, 3), dtype=torch.float32, device=dev)
    snrm = torch.zeros((nt, 3, 3), dtype=torch.float32, device=dev)
    first = None
    for ess in (True, False):
        vr.setObjEss(ess)
        assert vr.extract_isosurface_indexed(ISO, True, out_dev_ptrs=(vtx.data_ptr(), nrm.data_ptr(), idx.data_ptr(), nv, nt)) == (nv, nt)
        assert vr.extract_isosurface(ISO, True, out_dev_ptrs=(soup.data_ptr(), snrm.data_ptr(), nt)) == nt
        torch.cuda.synchronize()
        mi = vr.lastIndexedMeshInfo()
        assert mi["empty_skip"] == int(ess) and (ess or mi["point_blocks_skipped"] == 0)
        out[name + "_scratch_bytes"] = mi["scratch_bytes"]
        flat = idx.view(-1).long()
        assert torch.equal(vtx[flat].view(torch.int32), soup.view(-1, 3).view(torch.int32)), name
        assert torch.equal(nrm[flat].view(torch.int32), snrm.view(-1, 3).view(torch.int32)), name
        del flat
        if first is None:
            first = (vtx.clone(), idx.clone())
        else:
            assert torch.equal(first[0].view(torch.int32), vtx.view(torch.int32)) and torch.equal(first[1], idx), name
    del first
    for ess in (True, False):
        vr.setObjEss(ess)
        tag = name + "_%s_" + ("ess" if ess else "noess")
        ms, sp = timed(lambda: vr.isosurface_count_indexed(ISO))
        out[tag % "count_indexed" + "_ms"], out[tag % "count_indexed" + "_spread_ms"] = ms, sp
        for normals in (False, True):
            t2 = tag + ("_normals" if normals else "")
            np_ = nrm.data_ptr() if normals else None
            ms, sp = timed(lambda: vr.extract_isosurface_indexed(ISO, normals, out_dev_ptrs=(vtx.data_ptr(), np_, idx.data_ptr(), nv, nt)))
            out[t2 % "extract_indexed" + "_ms"], out[t2 % "extract_indexed" + "_spread_ms"] = ms, sp
            sn = snrm.data_ptr() if normals else None
            ms, sp = timed(lambda: vr.extract_isosurface(ISO, normals, out_dev_ptrs=(soup.data_ptr(), sn, nt)))
            out[t2 % "extract_soup" + "_ms"], out[t2 % "extract_soup" + "_spread_ms"] = ms, sp
    del vtx, nrm, idx, soup, snrm
    if HOST_ROUTE and n == 1024:
        vr.setObjEss(True)
        vr.extract_isosurface_indexed(ISO)   # (warm: the staging is allocated)
        t0 = time.perf_counter()
        hv, _, hi = vr.extract_isosurface_indexed(ISO)
        t1 = time.perf_counter()
        pos, _ = vr.extract_isosurface(ISO)
        pos, _ = vr.extract_isosurface(ISO)
        t2 = time.perf_counter()
        pos, _ = vr.extract_isosurface(ISO)
        t3 = time.perf_counter()
        wv, _, wi = frontend.weld_mesh(pos)
        t4 = time.perf_counter()
        assert (hv[hi].view("u4") == pos.view("u4")).all()
        out["host_route"] = "timed once at 1024^3"
        out[name + "_host_indexed_ms"] = round((t1 - t0) * 1e3, 1)
        out[name + "_host_soup_ms"] = round((t3 - t2) * 1e3, 1)
        out[name + "_host_weld_ms"] = round((t4 - t3) * 1e3, 1)
        out[name + "_host_weld_vertices"] = int(wv.shape[0])
    vr.close()
line = json.dumps(out)
print(line)
if args:
    with open(args[0], "w") as f:
        f.write(line + "\n")
