#!/usr/bin/env python3
"""tools/mip_time.py [VIEWPORT] -- what a maximum intensity projection (technique 2) costs, on one GPU; prints one
JSON line.  Scenes: the benchmark's headline (2048^3 UCHAR shells) and 1024^3 FLOAT shells, VIEWPORT^2 pixels
(default 1024), the benchmark's view.  Per scene, in ms per frame, HIP events, the median of 20 after 3 warm-ups:
  mip_ess_*       technique 2 with object-order ESS (samples below the running maximum are not fetched)
  mip_noess_*     technique 2, every sample fetched
  raycast_*       technique 0 (ESS on, default illumination) on the same volume in the same run
  *_single_ms     one frame at a time (vrhip_render_frame, the frame left on the device)
  *_orbit32_ms    a 32-frame turntable in one launch set (vrhip_render_batch_views), per frame
Before anything is timed the ESS-on and ESS-off projections of one frame are compared bit for bit."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import FLOAT, TECH_MIP, TECH_RAYCAST, UCHAR, VolumeRenderCL, frontend

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
F, WARM, REPS = 32, 3, 20
dev = torch.device("cuda", 0)
ROT = frontend.quat_from_axis_angle((1, 1, 0), 30.0)
VIEW = frontend.view_matrix(ROT)
ORBIT = frontend.orbit_views((0, 1, 0), F, ROT)


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


out = {"tool": "mip_time", "viewport": V, "frames_per_set": F, "reps": REPS, "warmups": WARM}
for name, n, fmt in (("shells2048_uchar", 2048, UCHAR), ("shells1024_float", 1024, FLOAT)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.updateView(VIEW)
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    mt = frontend.Mt19937()
    seeds = [mt() for _ in range(F)]
    vr.setSeed(seeds[0])
    frames = torch.zeros((F, V, V, 4), dtype=torch.float32, device=dev)
    # the skipping changes no bit
    vr.setTechnique(TECH_MIP)
    pair = []
    for ess in (True, False):
        vr.setObjEss(ess)
        vr.runRaycast(V, V, frames[0].data_ptr())
        torch.cuda.synchronize()
        pair.append(frames[0].clone())
    assert torch.equal(pair[0].view(torch.int32), pair[1].view(torch.int32)), name
    del pair
    for key, tech, ess in (("mip_ess", TECH_MIP, True), ("mip_noess", TECH_MIP, False), ("raycast", TECH_RAYCAST, True)):
        vr.setTechnique(tech)
        vr.setObjEss(ess)
        vr.setRoundBudget(10)

        def single():
            vr.setIteration(0); vr.runRaycast(V, V)

        out["%s_%s_single_ms" % (name, key)] = round(median_of(events(single)), 4)
        assert vr.lastLaunchInfo()["technique"] == tech
        vr.setRoundBudget(48)   # (the ray caster's schedule for launch sets; nothing to technique 2)

        def orbit():
            vr.render_batch(V, V, seeds, frames.data_ptr(), views=ORBIT)

        out["%s_%s_orbit32_ms" % (name, key)] = round(median_of(events(orbit)) / F, 4)
        li = vr.lastLaunchInfo()
        assert li["technique"] == tech and li["frames"] == F and li["views"] == 1, li
    del frames
    vr.close()
print(json.dumps(out))
