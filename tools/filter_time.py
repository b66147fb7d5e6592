#!/usr/bin/env python3
"""tools/filter_time.py [OUT.json] -- what the volume filters (vrhip_filter_volume) cost, on one GPU; prints one JSON
line and, with an argument, writes it there too (rewritten after every scene, so that an interrupted run leaves what
it measured).
Scenes: 1024^3 FLOAT shells and the benchmark's headline volume (2048^3 UCHAR shells).  Per scene: a normalised
Gaussian of radius 2 (sigma 1.0) and of radius 8 (sigma 3.0) on every axis, and the 3x3x3 median; with object-order
ESS on / off; from step 0 into step 1 ("new": the step exists after the first call) and in place.  In ms per
vrhip_filter_volume call, a host clock around the call (it ends in a synchronise), the median of 20 after 3 warm-ups
(of 5 after one where a call takes more than half a second: *_reps says which), with the spread (max - min) beside it
as *_spread_ms.  In place, step 0 is synthesised anew before every call and -- with ESS on -- its cell grid rebuilt,
both outside the clock; the allocation of the in-place scratch is inside it.
For ESS off also the bytes the call must move -- one read and one write of the volume -- over that time against the
8 TB/s HBM peak of DESIGN 5.2.  Also the share of blocks the cell grid skips, and once, at 1024^3, the host route the
call replaces: vrhip_download_volume, scipy.ndimage.gaussian_filter1d per axis (radius 2, clamped; a numpy separable
pass where scipy is missing) and the upload.  Before anything is timed the statistics of the ESS-on and ESS-off
destinations are compared."""
import ctypes as C
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL, _lib, frontend

WARM, REPS = 3, 20
SLOW_MS, SLOW_REPS = 500.0, 5
HBM_PEAK = 8.0e12
KINDS = (("gauss_r2", "separable", 1.0, 2), ("gauss_r8", "separable", 3.0, 8), ("median3", "median3", None, None))


def timed(fn, before=None):
    def one():
        if before:
            before()
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


out = {"tool": "filter_time", "reps": REPS, "warmups": WARM, "hbm_peak_bytes_per_s": HBM_PEAK}
for name, n, fmt, size in (("shells1024_float", 1024, FLOAT, 4), ("shells2048_uchar", 2048, UCHAR, 1)):
    vr = VolumeRenderCL(); vr.initialize()
    out["device"] = vr.getCurrentDeviceName()
    out["source_hash"] = vr.lib.vrhip_build_source_hash().decode()
    vr.synthVolume("shells", (n,) * 3, fmt)
    res3 = (C.c_uint32 * 3)(n, n, n)
    volume_bytes = n ** 3 * size
    out[name + "_bytes"] = volume_bytes

    def resynth(ess):
        # step 0 as it was, and -- what a first call after an upload would pay inside -- its cell grid
        assert vr.lib.vrhip_synth_volume(vr.handle, 1, res3, fmt, 0) == _lib.OK
        if ess:
            vr.volume_statistics((1, 1))

    for tag, kind, sigma, radius in KINDS:
        taps = frontend.gaussian_taps(sigma, radius) if sigma else None
        p = vr._filter_params(kind, taps, None)

        def run(dst):
            rc = vr.lib.vrhip_filter_volume(vr.handle, C.byref(p), dst)
            assert rc == _lib.OK, vr.lib.vrhip_last_error(vr.handle)

        # ESS on and off leave the same step: its statistics, table and moments, as the witness
        res = []
        for ess in (True, False):
            vr.setObjEss(ess)
            run(1)
            info = vr.lastFilterInfo()
            vr.setTimestep(1)
            st, hist = vr.volume_statistics((256, 16), (0.0, 1.0, 0.25), moments=True)
            vr.setTimestep(0)
            res.append((st, hist.tobytes(), info))
        assert res[0][:2] == res[1][:2], (name, tag)
        on = res[0][2]
        out["%s_%s_blocks_skipped_share" % (name, tag)] = round(on["blocks_skipped"] / on["blocks"], 4)
        for ess in (True, False):
            vr.setObjEss(ess)
            for where in ("new", "in_place"):
                key = "%s_%s_%s_%s" % (name, tag, "ess" if ess else "noess", where)
                print(key, file=sys.stderr, flush=True)
                if where == "new":
                    ms, sp, reps = timed(lambda: run(1))
                else:
                    ms, sp, reps = timed(lambda: run(0), before=lambda: resynth(ess))
                    out[key + "_scratch_bytes"] = vr.lastFilterInfo()["scratch_bytes"]
                    resynth(ess)
                out[key + "_ms"], out[key + "_spread_ms"], out[key + "_reps"] = ms, sp, reps
                if not ess:
                    out[key + "_hbm_share"] = round(2 * volume_bytes / (ms * 1e-3) / HBM_PEAK, 4)
        save(out)
    if n == 1024:   # once: the host route a radius-2 Gaussian replaces
        w = frontend.gaussian_taps(1.0, 2).astype(np.float32)
        t0 = time.perf_counter()
        host = vr.downloadVolume(0)
        t1 = time.perf_counter()
        try:
            from scipy import ndimage
            full = np.concatenate([w[:0:-1], w])
            for axis in range(3):
                host = ndimage.correlate1d(host, full, axis=axis, mode="nearest")
            out[name + "_host_route_filter"] = "scipy.ndimage.correlate1d"
        except ImportError:
            for axis in range(3):
                idx = np.arange(host.shape[axis])
                acc = w[0] * host
                for k in (1, 2):
                    acc += w[k] * (np.take(host, np.clip(idx - k, 0, None), axis=axis) +
                                   np.take(host, np.clip(idx + k, None, idx[-1]), axis=axis))
                host = acc
            out[name + "_host_route_filter"] = "numpy separable pass"
        t2 = time.perf_counter()
        vr.loadVolumeArrays([host], fmt)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        out[name + "_host_route_download_ms"] = round((t1 - t0) * 1e3, 1)
        out[name + "_host_route_filter_ms"] = round((t2 - t1) * 1e3, 1)
        out[name + "_host_route_upload_ms"] = round((t3 - t2) * 1e3, 1)
        del host
        save(out)
    vr.close()
print(save(out))
