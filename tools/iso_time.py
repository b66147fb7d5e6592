#!/usr/bin/env python3
"""tools/iso_time.py [VIEWPORT] -- what a first-hit isosurface (technique 4) costs, on one GPU; prints one JSON line.
Scenes: the benchmark's headline (2048^3 UCHAR shells) and 1024^3 FLOAT shells, VIEWPORT^2 pixels (default 1024), the
benchmark's view, isoValue ISO (a threshold that cuts the shells), refineSteps 4.  Per scene, in ms per frame, HIP
events, the median of 20 after 3 warm-ups:
  iso_ess_*        technique 4 with object-order ESS (march samples whose cell lies below isoValue are not fetched)
  iso_noess_*      technique 4, every sample fetched
  *_flat / *_shaded   illumType 0 / 1
  raycast_step_*   technique 0 (ESS on, shaded) with a step transfer function at the same threshold: the only way to
                   this picture without technique 4
  mip_*            technique 2 (ESS on) on the same volume, default transfer function
  *_single_ms      one frame at a time (vrhip_render_frame, the frame left on the device)
  *_orbit32_ms     a 32-frame turntable in one launch set (vrhip_render_batch_views), per frame
Before anything is timed the ESS-on and ESS-off isosurface frames (flat and shaded) are compared bit for bit."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from volumerenderercl_amd import FLOAT, TECH_ISO, TECH_MIP, TECH_RAYCAST, UCHAR, VolumeRenderCL, frontend

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
F, WARM, REPS = 32, 3, 20
ISO, REFINE = 0.5, 4
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


def step_tff(n=1024):
    """Transparent below ISO, opaque grey from ISO on: technique 0's way to a surface at the threshold."""
    t = np.zeros((n, 4), np.uint8)
    t[int(ISO * n):] = [160, 160, 160, 255]
    return t


out = {"tool": "iso_time", "viewport": V, "frames_per_set": F, "reps": REPS, "warmups": WARM, "iso_value": ISO,
       "refine_steps": REFINE}
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
    vr.setBackground((1.0, 1.0, 1.0))   # (alpha 0, as the CLI sets it: a hit is then alpha 1)
    vr.setIsoValue(ISO)
    vr.setIsoRefinement(REFINE)
    frames = torch.zeros((F, V, V, 4), dtype=torch.float32, device=dev)
    # the skipping changes no bit, and the threshold cuts the shells: some rays hit, some do not
    vr.setTechnique(TECH_ISO)
    for illum in (0, 1):
        vr.setIllumination(illum)
        pair = []
        for ess in (True, False):
            vr.setObjEss(ess)
            vr.runRaycast(V, V, frames[0].data_ptr())
            torch.cuda.synchronize()
            pair.append(frames[0].clone())
        assert torch.equal(pair[0].view(torch.int32), pair[1].view(torch.int32)), (name, illum)
        hit = float((pair[0][..., 3] == 1.0).float().mean())
        out["%s_hit_fraction" % name] = round(hit, 4)
        assert 0.01 < hit < 1.0, (name, hit)
        del pair
    runs = (("iso_ess_flat", TECH_ISO, True, 0, None), ("iso_ess_shaded", TECH_ISO, True, 1, None),
            ("iso_noess_flat", TECH_ISO, False, 0, None), ("iso_noess_shaded", TECH_ISO, False, 1, None),
            ("raycast_step", TECH_RAYCAST, True, 1, step_tff()), ("mip", TECH_MIP, True, 1, None))
    for key, tech, ess, illum, tff in runs:
        vr.setTransferFunction(frontend.tff_from_stops() if tff is None else tff)
        vr.setTechnique(tech)
        vr.setObjEss(ess)
        vr.setIllumination(illum)
        vr.setRoundBudget(10)

        def single():
            vr.setIteration(0); vr.runRaycast(V, V)

        out["%s_%s_single_ms" % (name, key)] = round(median_of(events(single)), 4)
        assert vr.lastLaunchInfo()["technique"] == tech
        vr.setRoundBudget(48)   # (the ray caster's schedule for launch sets; nothing to techniques 2 and 4)

        def orbit():
            vr.render_batch(V, V, seeds, frames.data_ptr(), views=ORBIT)

        out["%s_%s_orbit32_ms" % (name, key)] = round(median_of(events(orbit)) / F, 4)
        li = vr.lastLaunchInfo()
        assert li["technique"] == tech and li["frames"] == F and li["views"] == 1, li
    del frames
    vr.close()
print(json.dumps(out))
