#!/usr/bin/env python3
"""tools/depth_time.py [VIEWPORT] -- what a depth image (vrhip_render_depth) costs, on one GPU; prints one JSON line.
Scenes: the benchmark's headline (2048^3 UCHAR shells) and 1024^3 FLOAT shells, VIEWPORT^2 pixels (default 1024), the
benchmark's view.  Per scene, in ms per call, HIP events, the median of 20 after 3 warm-ups, with the spread
(max - min of the 20) beside it as *_spread_ms:
  depth_{iso,max,opacity}_{ess,noess}   a whole-frame depth image into device memory, object-order ESS on / off
                                        (iso: threshold ISO, refineSteps 4; opacity: threshold 0.9)
  pick_{iso,max,opacity}                a 1 x 1 rectangle at the frame's centre, ESS on
  tech4_shaded, tech2                   the same scene's technique-4 shaded frame and technique-2 frame (ESS on, one
                                        frame at a time, left on the device): the same march with a pixel at its end
Before anything is timed the ESS-on and ESS-off depth images are compared bit for bit."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import FLOAT, TECH_ISO, TECH_MIP, TECH_RAYCAST, UCHAR, VolumeRenderCL, frontend

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
WARM, REPS = 3, 20
ISO, REFINE, OPACITY = 0.5, 4, 0.9
THRESHOLD = {"iso": ISO, "max": 0.0, "opacity": OPACITY}
dev = torch.device("cuda", 0)
VIEW = frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0))


def timed(fn):
    def one():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(WARM):
        one()
    t = [one() for _ in range(REPS)]
    return round(statistics.median(t), 4), round(max(t) - min(t), 4)


out = {"tool": "depth_time", "viewport": V, "reps": REPS, "warmups": WARM, "iso_value": ISO, "refine_steps": REFINE,
       "opacity_threshold": OPACITY}
for name, n, fmt in (("shells2048_uchar", 2048, UCHAR), ("shells1024_float", 1024, FLOAT)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.updateView(VIEW)
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    vr.setSeed(frontend.Mt19937()())
    vr.setBackground((1.0, 1.0, 1.0))
    vr.setIsoValue(ISO)
    vr.setIsoRefinement(REFINE)
    xyzt = torch.zeros((V, V, 4), dtype=torch.float32, device=dev)
    aux = torch.zeros((V, V), dtype=torch.float32, device=dev)
    kind = torch.zeros((V, V), dtype=torch.uint8, device=dev)
    ptrs = (xyzt.data_ptr(), aux.data_ptr(), kind.data_ptr())
    for mode in ("iso", "max", "opacity"):
        pair = []
        for ess in (True, False):
            vr.setObjEss(ess)
            vr.render_depth(V, V, mode, THRESHOLD[mode], REFINE, out_dev_ptrs=ptrs)
            torch.cuda.synchronize()
            assert vr.lastDepthInfo()["empty_skip"] == int(ess)
            pair.append((xyzt.clone(), aux.clone(), kind.clone()))
        for a, b in zip(*pair):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, mode)
        out["%s_%s_hit_fraction" % (name, mode)] = round(float((pair[0][2] == 2).float().mean()), 4)
        del pair
        for ess in (True, False):
            vr.setObjEss(ess)
            key = "%s_depth_%s_%s" % (name, mode, "ess" if ess else "noess")
            out[key + "_ms"], out[key + "_spread_ms"] = timed(
                lambda: vr.render_depth(V, V, mode, THRESHOLD[mode], REFINE, out_dev_ptrs=ptrs))
        vr.setObjEss(True)
        key = "%s_pick_%s" % (name, mode)
        out[key + "_ms"], out[key + "_spread_ms"] = timed(
            lambda: vr.render_depth(V, V, mode, THRESHOLD[mode], REFINE, rect=(V // 2, V // 2, 1, 1), out_dev_ptrs=ptrs))
    for key, tech in (("tech4_shaded", TECH_ISO), ("tech2", TECH_MIP)):
        vr.setTechnique(tech)
        vr.setObjEss(True)
        vr.setIllumination(1)

        def single():
            vr.setIteration(0); vr.runRaycast(V, V)

        k = "%s_%s" % (name, key)
        out[k + "_ms"], out[k + "_spread_ms"] = timed(single)
        assert vr.lastLaunchInfo()["technique"] == tech
    vr.setTechnique(TECH_RAYCAST)
    del xyzt, aux, kind
    vr.close()
print(json.dumps(out))
