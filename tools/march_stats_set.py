"""tools/march_stats_set.py -- round statistics of phase 1 for one 32-frame launch set of the headline (1024^2, budget 48),
per frame, from a -DVR_MARCH_STATS build (tools/mkvariant.sh mstats -DVR_MARCH_STATS; run on the GPU box); the ray order by
VRHIP_PIXEL_MAJOR."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["VRHIP_LIB_PATH"] = os.path.join(ROOT, "volumerenderercl_amd", "_variants", "libvrhip_mstats.so")
import torch
from volumerenderercl_amd import VolumeRenderCL, frontend, UCHAR
vr = VolumeRenderCL(); vr.initialize()
vr.synthVolume("shells", (2048,) * 3, UCHAR)
vr.setTransferFunction(frontend.tff_from_stops()); vr.setIllumination(1)
vr.updateView(frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0)))
vr.setRoundBudget(48); vr.setFrameTiming(False)
mt = frontend.Mt19937(); N = 32
out = torch.zeros((N, 1024, 1024, 4), dtype=torch.float32, device="cuda")
st = (C.c_ulonglong * 32)()
f = vr.lib.vrhip_debug_march_stats; f.argtypes = [C.c_void_p, C.c_int]
vr.render_batch(1024, 1024, [mt() for _ in range(N)], out.data_ptr()); torch.cuda.synchronize()
f(st, 1)
vr.render_batch(1024, 1024, [mt() for _ in range(N)], out.data_ptr()); torch.cuda.synchronize()
f(st, 1)
li = vr.lastLaunchInfo()
print("pixel_major", li["pixel_major"], "phase1_waves", li["phase1_waves"], "budget", li["round_budget"], "-- per frame of a 32-frame set")
names = ["wave-rounds", "live lanes x rounds", "DDA step executions", "  lanes in them", "lookahead executions", "  lanes in them",
         "evaluation batches", "  lanes in them", "refills", "valid samples evaluated"]
v = list(st)
for n, x in zip(names, v[16:26]):
    print("%-26s %12.0f" % (n, x / N))
r = v[16]
print("lanes alive per round %.1f, per lookahead %.1f, per evaluation batch %.1f; rounds with both blocks at most %.0f per frame" % (
    v[17] / r, v[21] / max(v[20], 1), v[23] / max(v[22], 1), (v[20] + v[22] - r) / N))
vr.close()
