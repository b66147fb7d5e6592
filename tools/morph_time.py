#!/usr/bin/env python3
"""tools/morph_time.py [OUT.json] -- what the volume morphology (vrhip_morph_volume) costs, on one GPU; prints one JSON
line and, with an argument, writes it there too (rewritten after every configuration, so that an interrupted run
leaves what it measured).
Scenes: tools/filter_time.py's two, 1024^3 FLOAT shells and the benchmark's headline volume (2048^3 UCHAR shells).  Per
scene: ERODE (one sweep), OPEN (two) and GRADIENT (one sweep, both extremes) with a BOX and a BALL of radius 1, 2 and 8
on every axis, from step 0 into step 1, with object-order ESS on / off.  In ms per vrhip_morph_volume call, a host
clock around the call (it ends in a synchronise), the median of 20 after 3 warm-ups (of 5 after one where a call takes
more than half a second: *_reps says which), with the spread (max - min) beside it as *_spread_ms.
In the same process, as the yardstick for the micro-brick staging: vrhip_filter_volume with a normalised Gaussian of
the same radius (three separable passes on single voxels staged lane by lane), timed the same way.
For ESS off also the bytes one sweep must move -- one read and one write of the volume, twice that for OPEN -- over the
time against the 8 TB/s HBM peak of DESIGN 5.2.  Also the share of blocks the cell grid skips per sweep.  Before
anything is timed the statistics of the ESS-on and ESS-off destinations are compared."""
import ctypes as C
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL, _lib, frontend

WARM, REPS = 3, 20
SLOW_MS, SLOW_REPS = 500.0, 5
HBM_PEAK = 8.0e12
OPS = (("erode", 1), ("open", 2), ("gradient", 1))   # name, sweeps
SHAPES = ("box", "ball")
RADII = (1, 2, 8)


def timed(fn):
    def one():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    first = one()
    slow = first > SLOW_MS   # (a call that long is timed SLOW_REPS times after one warm-up, and the key says so)
    for _ in range(0 if slow else WARM - 1):
        one()
    t = [one() for _ in range(SLOW_REPS if slow else REPS)]
    print("  %.3f ms (%d calls)" % (statistics.median(t), len(t)), file=sys.stderr, flush=True)
    return round(statistics.median(t), 4), round(max(t) - min(t), 4), len(t)


def save(out):
    line = json.dumps(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return line


out = {"tool": "morph_time", "reps": REPS, "warmups": WARM, "hbm_peak_bytes_per_s": HBM_PEAK}
for name, n, fmt, size in (("shells1024_float", 1024, FLOAT, 4), ("shells2048_uchar", 2048, UCHAR, 1)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    volume_bytes = n ** 3 * size
    out[name + "_bytes"] = volume_bytes

    def witness():
        vr.setTimestep(1)
        st, hist = vr.volume_statistics((256, 16), (0.0, 1.0, 0.25), moments=True)
        vr.setTimestep(0)
        return st, hist.tobytes()

    for radius in RADII:
        # the yardstick: the separable filter of the same radius, the parent's code
        fp = vr._filter_params("separable", frontend.gaussian_taps(0.5 + 0.3 * radius, radius), None)

        def run_filter():
            assert vr.lib.vrhip_filter_volume(vr.handle, C.byref(fp), 1) == _lib.OK, vr.lib.vrhip_last_error(vr.handle)

        for ess in (True, False):
            vr.setObjEss(ess)
            key = "%s_filter_gauss_r%d_%s" % (name, radius, "ess" if ess else "noess")
            print(key, file=sys.stderr, flush=True)
            out[key + "_ms"], out[key + "_spread_ms"], out[key + "_reps"] = timed(run_filter)
            if not ess:
                out[key + "_hbm_share"] = round(2 * volume_bytes / (out[key + "_ms"] * 1e-3) / HBM_PEAK, 4)
        save(out)
        for shape in SHAPES:
            for op, sweeps in OPS:
                p = frontend.morph_params(op, radius, shape)

                def run():
                    assert vr.lib.vrhip_morph_volume(vr.handle, C.byref(p), 1) == _lib.OK, vr.lib.vrhip_last_error(vr.handle)

                tag = "%s_%s_%s_r%d" % (name, op, shape, radius)
                # ESS on and off leave the same step: its statistics, table and moments, as the witness
                res = []
                for ess in (True, False):
                    vr.setObjEss(ess)
                    run()
                    res.append((witness(), vr.lastMorphInfo()))
                assert res[0][0] == res[1][0], tag
                on = res[0][1]
                out[tag + "_blocks_skipped_share"] = [round(on["blocks_skipped"][s] / on["blocks"][s], 4) for s in range(sweeps)]
                for ess in (True, False):
                    vr.setObjEss(ess)
                    key = "%s_%s" % (tag, "ess" if ess else "noess")
                    print(key, file=sys.stderr, flush=True)
                    out[key + "_ms"], out[key + "_spread_ms"], out[key + "_reps"] = timed(run)
                    if not ess:
                        out[key + "_hbm_share"] = round(sweeps * 2 * volume_bytes / (out[key + "_ms"] * 1e-3) / HBM_PEAK, 4)
                save(out)
    vr.close()
print(save(out))
