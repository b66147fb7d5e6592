#!/usr/bin/env python3
"""tools/preint_time.py [VIEWPORT] [OUT.json] -- what a frame with pre-integrated classification (technique 8) costs,
on one GPU; prints one JSON line and writes it to OUT.json (default profiles/r4/preint_time.json).
Scenes: the benchmark's headline (2048^3 UCHAR shells) and 1024^3 FLOAT shells, VIEWPORT^2 pixels (default 1024), the
benchmark's view, shaded (illumType 1), one frame at a time (vrhip_render_frame, the frame left on the device).  Two
1-D tables: the default one, and a NARROW PEAK (256 entries, opaque in the two at 0.5, transparent elsewhere).  Per
scene and table, in ms per frame, HIP events, the median of 20 after 3 warm-ups, with the spread (max - min) beside it,
all in this one process:
  preint_*        technique 8
  raycast_*       technique 0 with the same table.  NOT the same march with ESS on and off: on, it walks the ESS
                  bricks, culls patches and ends rays by the step table; off, it is the plain loop technique 8 follows
  tf2d_*          technique 6 with every row of a 64-row table the same 1-D table (technique 0's picture)
  *_ess / *_noess object-order ESS on / off
and, for the peak table, what the feature saves: `raycast_rate` is the samplingRate, found by doubling from the
scene's own, at which technique 0 first has alpha > 0 on every pixel on which technique 8 has it at the scene's rate
(null: not up to 64 x), and raycast_at_rate_* technique 0's time there.
Before anything is timed the ESS-on and ESS-off technique-8 frames are compared bit for bit."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from volumerenderercl_amd import FLOAT, TECH_PREINT, TECH_RAYCAST, TECH_TF2D, UCHAR, VolumeRenderCL, frontend

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r4", "preint_time.json")
WARM, REPS = 3, 20
RATE, N_G, G_HI, MAX_DOUBLINGS = 1.5, 64, 0.25, 6
dev = torch.device("cuda", 0)
VIEW = frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0))


def timed(fn):
    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(WARM):
        once()
    ts = [once() for _ in range(REPS)]
    return round(statistics.median(ts), 4), round(max(ts) - min(ts), 4)


peak = np.zeros((256, 4), np.uint8)
peak[127:129] = 255
tffs = {"default": frontend.tff_from_stops(), "peak": peak}
out = {"tool": "preint_time", "viewport": V, "reps": REPS, "warmups": WARM, "sampling_rate": RATE, "tf2d_rows": N_G,
       "peak_table": "256 entries, 127 and 128 opaque white"}
for name, n, fmt in (("shells2048_uchar", 2048, UCHAR), ("shells1024_float", 1024, FLOAT)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.updateView(VIEW)
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    vr.setSeed(frontend.Mt19937()())
    vr.setBackground((1.0, 1.0, 1.0))
    vr.setIllumination(1)
    vr.setRoundBudget(10)
    frame = torch.zeros((V, V, 4), dtype=torch.float32, device=dev)

    def render(tech, ess, rate=RATE):
        vr.setTechnique(tech); vr.setObjEss(ess); vr.updateSamplingRate(rate); vr.setIteration(0)
        vr.runRaycast(V, V, frame.data_ptr())
        torch.cuda.synchronize()
        return frame.clone()

    def time_one(key, tech, ess, rate=RATE):
        vr.setTechnique(tech); vr.setObjEss(ess); vr.updateSamplingRate(rate)

        def single():
            vr.setIteration(0); vr.runRaycast(V, V)

        med, spread = timed(single)
        out[key + "_ms"], out[key + "_spread_ms"] = med, spread
        assert vr.lastLaunchInfo()["technique"] == tech

    for tname, tff in tffs.items():
        pre = "%s_%s_" % (name, tname)
        vr.setTransferFunction(tff)
        vr.setTransferFunction2D(frontend.tf2d_from_1d(tff, N_G), G_HI)
        a, b = render(TECH_PREINT, True), render(TECH_PREINT, False)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), pre   # no bit changes with the switch
        seen = a[..., 3] > 0
        out[pre + "preint_coverage"] = round(float(seen.float().mean()), 4)
        del a, b
        for tech_name, tech in (("preint", TECH_PREINT), ("raycast", TECH_RAYCAST), ("tf2d", TECH_TF2D)):
            for ess in (True, False):
                time_one(pre + tech_name + ("_ess" if ess else "_noess"), tech, ess)
        if tname == "peak":
            out[pre + "raycast_coverage"] = round(float((render(TECH_RAYCAST, False)[..., 3] > 0).float().mean()), 4)
            found = None
            for k in range(0, MAX_DOUBLINGS + 1):
                rate = RATE * 2 ** k
                missed = int((seen & ~(render(TECH_RAYCAST, False, rate)[..., 3] > 0)).sum())
                out[pre + "raycast_missed_at_%g" % rate] = missed
                if missed == 0:
                    found = rate
                    break
            out[pre + "raycast_rate"] = found
            if found is not None:
                for ess in (True, False):
                    time_one(pre + "raycast_at_rate" + ("_ess" if ess else "_noess"), TECH_RAYCAST, ess, found)
        del seen
    del frame
    vr.close()
print(json.dumps(out))
with open(OUT, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
