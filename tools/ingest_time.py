"""Time to the first voxel in HBM, host loader against device-side ingest, on a 512^3 USHORT and a 512^3 FLOAT step.

  host path    DatRawReader (read + maximum + convert + histogram on one host thread), then vrhip_upload_volume
  device path  DatRawReader raw mode (file read only), then vrhip_ingest_raw; its time is split into the device
               part (vrhip_last_ingest_seconds: the maximum, re-tile and convert kernels) and the rest of the call
               (host-to-device copies and their waits)

Three loads each, medians.  The device part's bytes per second stand beside the brick build's
(vrhip_last_bricks_seconds) on the same volume: the brick build streams the same bytes once, the device part
reads them three times and writes them twice, so a third of the brick build's rate is its roof.  Prints one
JSON line per format.  For the convert kernel alone, run this tool under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volumerenderercl_amd import FLOAT, USHORT, _lib, datraw   # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def measure(lib, host, h, dat, res, fmt, loads):
    rows = {"host_loader": [], "host_upload": [], "raw_read": [], "ingest_call": [], "ingest_device": []}
    r3 = (C.c_uint32 * 3)(*res)
    for _ in range(loads):
        p = C.c_void_p()
        rc, dt = _timed(lambda: host.vrdr_load(dat.encode(), None, C.byref(p)))
        assert rc == 0
        rows["host_loader"].append(dt)
        rc, dt = _timed(lambda: lib.vrhip_upload_volume(h, host.vrdr_data(p, 0), r3, fmt, 0))
        assert rc == 0
        rows["host_upload"].append(dt)
        host.vrdr_free(p)
    info = datraw._Info()
    for _ in range(loads):
        p = C.c_void_p()
        rc, dt = _timed(lambda: host.vrdr_load_raw(dat.encode(), None, C.byref(p)))
        assert rc == 0
        rows["raw_read"].append(dt)
        host.vrdr_info(p, C.byref(info))
        hist, vmax = (C.c_double * 256)(), C.c_float()
        rc, dt = _timed(lambda: lib.vrhip_ingest_raw(h, host.vrdr_data(p, 0), info.bytes_per_timestep, r3, fmt, 1, 0, 0,
                                                     hist, C.byref(vmax)))
        assert rc == 0, lib.vrhip_last_error(h)
        rows["ingest_call"].append(dt)
        rows["ingest_device"].append(lib.vrhip_last_ingest_seconds(h))
        host.vrdr_free(p)
    med = {k: statistics.median(v) for k, v in rows.items()}
    assert lib.vrhip_build_bricks(h) == 0
    bricks = lib.vrhip_last_bricks_seconds(h)
    nbytes = res[0] * res[1] * res[2] * (2 if fmt == USHORT else 4)
    return {
        "format": "USHORT" if fmt == USHORT else "FLOAT", "res": list(res), "bytes": nbytes, "loads": loads,
        "host_path_s": med["host_loader"] + med["host_upload"], "host_loader_s": med["host_loader"],
        "host_upload_s": med["host_upload"],
        "device_path_s": med["raw_read"] + med["ingest_call"], "raw_read_s": med["raw_read"],
        "ingest_copies_s": med["ingest_call"] - med["ingest_device"], "ingest_device_s": med["ingest_device"],
        "ingest_device_GBps": nbytes / med["ingest_device"] / 1e9,
        "bricks_s": bricks, "bricks_GBps": nbytes / bricks / 1e9 if bricks else None,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--loads", type=int, default=3)
    args = ap.parse_args()
    lib = _lib.load()
    host = datraw._load()
    h = C.c_void_p()
    if lib.vrhip_create(0, C.byref(h)) != 0:
        raise SystemExit(lib.vrhip_last_error(None).decode())
    n = args.edge
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        for fmt, name in ((USHORT, "USHORT"), (FLOAT, "FLOAT")):
            v = rng.integers(0, 4096, n ** 3, dtype=np.uint16)
            v[: n ** 3 // 2] = 0                       # half the volume is empty space
            (v if fmt == USHORT else v.astype(np.float32)).tofile(os.path.join(tmp, "v.raw"))
            dat = os.path.join(tmp, "v.dat")
            with open(dat, "w") as f:
                f.write("ObjectFileName: v.raw\nResolution: %d %d %d\nSliceThickness: 1 1 1\nFormat: %s\n" % (n, n, n, name))
            print(json.dumps(measure(lib, host, h, dat, (n, n, n), fmt, args.loads)), flush=True)
    lib.vrhip_destroy(h)


if __name__ == "__main__":
    main()
