#!/usr/bin/env python3
"""tools/tf2d_time.py [VIEWPORT] [OUT.json] -- what a frame through a 2-D transfer function (technique 6) costs, on
one GPU; prints one JSON line and writes it to OUT.json (default profiles/r4/tf2d_time.json).
Scenes: the benchmark's headline (2048^3 UCHAR shells) and 1024^3 FLOAT shells, VIEWPORT^2 pixels (default 1024), the
benchmark's view, shaded (illumType 1), one frame at a time (vrhip_render_frame, the frame left on the device).  Per
scene, in ms per frame, HIP events, the median of 20 after 3 warm-ups, with the spread (max - min) beside it:
  tf2d_equal_*    technique 6, every row of the 1024 x 64 table the default 1-D table (technique 0's picture)
  tf2d_band_*     technique 6, the same rows with their opacity scaled by a gradient ramp (frontend.tf2d_ramp): opaque
                  only where the gradient magnitude is above G0
  raycast_*       technique 0 with the same 1-D table.  NOT the same march with ESS on and off: on, it walks the ESS
                  bricks, culls patches and ends rays by the step table; off, it is the plain loop technique 6 follows
  mip_ess, iso_ess   techniques 2 and 4 with ESS: the kernels that share technique 6's launch shape
  *_ess / *_noess    object-order ESS on / off
Before anything is timed the ESS-on and ESS-off technique-6 frames are compared bit for bit, and the rows-all-equal
frame with technique 0's ESS-off frame."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import FLOAT, TECH_ISO, TECH_MIP, TECH_RAYCAST, TECH_TF2D, UCHAR, VolumeRenderCL, frontend

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r4", "tf2d_time.json")
WARM, REPS = 3, 20
N_G, G_HI, G0, G1 = 64, 0.25, 0.02, 0.08
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


out = {"tool": "tf2d_time", "viewport": V, "reps": REPS, "warmups": WARM, "n_v": 1024, "n_g": N_G, "g_hi": G_HI,
       "ramp": [G0, G1]}
tff = frontend.tff_from_stops()
tables = {"equal": frontend.tf2d_from_1d(tff, N_G), "band": frontend.tf2d_ramp(tff, N_G, G_HI, G0, G1)}
for name, n, fmt in (("shells2048_uchar", 2048, UCHAR), ("shells1024_float", 1024, FLOAT)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    vr.setTransferFunction(tff)
    vr.updateView(VIEW)
    vr.set_stream(torch.cuda.current_stream().cuda_stream)
    vr.setSeed(frontend.Mt19937()())
    vr.setBackground((1.0, 1.0, 1.0))
    vr.setIllumination(1)
    vr.setRoundBudget(10)
    frame = torch.zeros((V, V, 4), dtype=torch.float32, device=dev)

    def render(tech, ess):
        vr.setTechnique(tech); vr.setObjEss(ess); vr.setIteration(0)
        vr.runRaycast(V, V, frame.data_ptr())
        torch.cuda.synchronize()
        return frame.clone()

    # no bit changes with the switch; rows all equal is technique 0's ESS-off frame
    for key, table in tables.items():
        vr.setTransferFunction2D(table, G_HI)
        a, b = render(TECH_TF2D, True), render(TECH_TF2D, False)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, key)
        out["%s_tf2d_%s_coverage" % (name, key)] = round(float((a[..., 3] > 0).float().mean()), 4)
        if key == "equal":
            c = render(TECH_RAYCAST, False)
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), name
        del a, b
    runs = [("tf2d_%s_%s" % (k, "ess" if e else "noess"), TECH_TF2D, e, k) for k in tables for e in (True, False)]
    runs += [("raycast_ess", TECH_RAYCAST, True, None), ("raycast_noess", TECH_RAYCAST, False, None),
             ("mip_ess", TECH_MIP, True, None), ("iso_ess", TECH_ISO, True, None)]
    for key, tech, ess, table in runs:
        if table is not None:
            vr.setTransferFunction2D(tables[table], G_HI)
        vr.setTechnique(tech)
        vr.setObjEss(ess)

        def single():
            vr.setIteration(0); vr.runRaycast(V, V)

        med, spread = timed(single)
        out["%s_%s_ms" % (name, key)], out["%s_%s_spread_ms" % (name, key)] = med, spread
        assert vr.lastLaunchInfo()["technique"] == tech
    del frame
    vr.close()
print(json.dumps(out))
with open(OUT, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
