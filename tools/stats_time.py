#!/usr/bin/env python3
"""tools/stats_time.py [OUT.json] -- what the volume statistics (vrhip_volume_statistics) cost, on one GPU; prints one
JSON line and, with an argument, writes it there too.
Scenes: the benchmark's headline volume (2048^3 UCHAR shells) and 1024^3 FLOAT shells, the whole volume, window
[0, 1] x [0, 0.5).  Per scene, with object-order ESS on / off, bins (256,1), (256,64) and (256,256), with and without
moments, in ms per call into a host table, a host clock around the call (it ends in a synchronise), the median of 20
after 3 warm-ups (of 5 after one where a call takes more than half a second: *_reps says which), with the spread
(max - min) beside it as *_spread_ms; for ESS off also the volume's bytes
-- every voxel is read once -- over that time against the 8 TB/s HBM peak of DESIGN 5.2.
Also: the share of blocks the cell grid skips; (256,64) with the table forced to global memory (VRHIP_STATS_LDS_BINS=0)
against the default LDS path; and two baselines measured in the same run: vrhip_volume_histogram, the 1-D device
histogram of the ingest, on the same step, and once, at 1024^3, the host route -- vrhip_download_volume and
numpy.histogram.  Before anything is timed the ESS-on and ESS-off results are compared byte for byte."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL, _lib

WARM, REPS = 3, 20
SLOW_MS, SLOW_REPS = 500.0, 5
WINDOW = (0.0, 1.0, 0.5)
BINS = ((256, 1), (256, 64), (256, 256))
HBM_PEAK = 8.0e12


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


out = {"tool": "stats_time", "reps": REPS, "warmups": WARM, "window": WINDOW, "hbm_peak_bytes_per_s": HBM_PEAK}
for name, n, fmt, size in (("shells2048_uchar", 2048, UCHAR, 1), ("shells1024_float", 1024, FLOAT, 4)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    volume_bytes = n ** 3 * size
    out[name + "_bytes"] = volume_bytes
    for bins in BINS:
        for moments in (False, True):
            res = []
            for ess in (True, False):
                vr.setObjEss(ess)
                st, hist = vr.volume_statistics(bins, WINDOW, moments=moments)
                res.append((st, hist.tobytes(), vr.lastStatsInfo()))
            assert res[0][:2] == res[1][:2], (name, bins, moments)
            on = res[0][2]
            tag = "%s_%dx%d%s" % (name, bins[0], bins[1], "_moments" if moments else "")
            out[tag + "_blocks_skipped_share"] = round((on["blocks_skipped_constant"] + on["blocks_skipped_window"]) / on["blocks"], 4)
            out[tag + "_path"] = "lds" if on["hist_path"] == _lib.STATS_PATH_LDS else "global"
            out[tag + "_scratch_bytes"] = on["scratch_bytes"]
            for ess in (True, False):
                vr.setObjEss(ess)
                key = tag + ("_ess" if ess else "_noess")
                print(key, file=sys.stderr, flush=True)
                ms, sp, reps = timed(lambda: vr.volume_statistics(bins, WINDOW, moments=moments))
                out[key + "_ms"], out[key + "_spread_ms"], out[key + "_reps"] = ms, sp, reps
                if not ess:
                    out[key + "_hbm_share"] = round(volume_bytes / (ms * 1e-3) / HBM_PEAK, 4)
    # (256, 64): the table in LDS (the default) against atomics straight to global memory
    os.environ["VRHIP_STATS_LDS_BINS"] = "0"
    for ess in (True, False):
        vr.setObjEss(ess)
        ms, sp, reps = timed(lambda: vr.volume_statistics((256, 64), WINDOW))
        assert vr.lastStatsInfo()["hist_path"] == _lib.STATS_PATH_GLOBAL
        key = "%s_256x64_forced_global_%s" % (name, "ess" if ess else "noess")
        out[key + "_ms"], out[key + "_spread_ms"], out[key + "_reps"] = ms, sp, reps
    del os.environ["VRHIP_STATS_LDS_BINS"]
    # baseline (a): the ingest's 1-D device histogram of the same step
    ms, sp, _ = timed(lambda: vr.volumeHistogram(0))
    out[name + "_volume_histogram_ms"], out[name + "_volume_histogram_spread_ms"] = ms, sp
    if n == 1024:   # baseline (b), once: the host route
        t0 = time.perf_counter()
        host = vr.downloadVolume(0)
        t1 = time.perf_counter()
        h, _ = np.histogram(host, bins=256, range=(0.0, 1.0))
        t2 = time.perf_counter()
        out[name + "_host_route_download_ms"] = round((t1 - t0) * 1e3, 1)
        out[name + "_host_route_numpy_histogram_ms"] = round((t2 - t1) * 1e3, 1)
        vr.setObjEss(True)
        _, dev_hist = vr.volume_statistics((256, 1), WINDOW)
        assert int(h.sum()) == int(dev_hist.sum()), "host route and device disagree"   # (numpy bins in float64)
        del host
    vr.close()
line = json.dumps(out)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
