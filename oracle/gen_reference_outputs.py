#!/usr/bin/env python3
"""Generate tests/golden/reference_outputs.json: what the REFERENCE's own code, compiled under oracle/_ref by
`make -C oracle ref`, returns on the seeded random inputs of

  * tests/test_hdr_differential.py   -- libref_hdr.so (inc/hdr_loader.h): 48 .hdr files;
  * tests/test_loader_differential.py -- libref_datraw.so (src/io/datrawreader.cpp): 64 .dat/.raw data sets;
  * tests/test_oracle_golden.py      -- libref_rng.so (random.cl) and libref_kernel.so (volumeraycast.cl's
    builtin-free functions): sha256 of their output streams, and oracle/ref_kernel_free.py's analysis of
    ref_kernel.o.

The inputs come from the tests' own generators; the outputs are recorded as values where small and as sha256
of the exact bytes otherwise.  Runs only where the reference's sources were available to build oracle/_ref; the
file it writes is data and is committed, so those tests run everywhere.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(HERE, "_ref")
OUT = os.path.join(ROOT, "tests", "golden", "reference_outputs.json")
sys.path.insert(0, ROOT)

from oracle import ref_kernel_free  # noqa: E402
from tests import test_hdr_differential as thd  # noqa: E402
from tests import test_loader_differential as tld  # noqa: E402
from tests import test_oracle_golden as tog  # noqa: E402


def sha256(b):
    return hashlib.sha256(b).hexdigest()


def hdr_random():
    ref = C.CDLL(os.path.join(REF, "libref_hdr.so"))
    ref.refhdr_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    ref.refhdr_free.argtypes = [C.POINTER(C.c_float)]
    out = []
    for case in range(48):
        with tempfile.TemporaryDirectory() as d:
            path = thd.write_case(case, d)
            with open(path, "rb") as f:
                entry = {"input_sha256": sha256(f.read())}
            pix = C.POINTER(C.c_float)()
            rw, rh = C.c_uint(), C.c_uint()
            entry["ok"] = bool(ref.refhdr_load(path.encode(), C.byref(pix), C.byref(rw), C.byref(rh)))
            if entry["ok"]:
                px = np.ctypeslib.as_array(pix, shape=(rh.value, rw.value, 4)).astype(np.float32)
                ref.refhdr_free(pix)
                entry.update(shape=list(px.shape), pixels_sha256=sha256(px.tobytes()))
        out.append(entry)
    return out


class DatRawResult(C.Structure):
    _fields_ = [("res", C.c_uint * 4), ("thickness", C.c_double * 3), ("format", C.c_int),
                ("endianness", C.c_int), ("min_value", C.c_float), ("max_value", C.c_float),
                ("n_timesteps", C.c_ulonglong), ("bytes_per_timestep", C.c_ulonglong),
                ("channel_order", C.c_char * 16)]


def loader_random():
    ref = C.CDLL(os.path.join(REF, "libref_datraw.so"))
    ref.refdr_error.restype = C.c_char_p
    out = []
    for case in range(64):
        with tempfile.TemporaryDirectory() as d:
            dat = tld.write_case(case, d)
            entry = {"input_sha256": tld.input_sha256(d)}
            want = DatRawResult()
            entry["rc"] = rc = ref.refdr_load(dat.encode(), C.byref(want))
            if rc != 0:
                entry["error"] = ref.refdr_error().decode()
                out.append(entry)
                continue
            entry.update(res=list(want.res), thickness=list(want.thickness), format=want.format,
                         endianness=want.endianness, channel_order=want.channel_order.decode(),
                         min_max=[float(want.min_value), float(want.max_value)], n_timesteps=want.n_timesteps,
                         data_sha256=[], histogram_sha256=[])
            for t in range(want.n_timesteps):
                buf = (C.c_char * want.bytes_per_timestep)()
                assert ref.refdr_copy_data(t, buf, want.bytes_per_timestep) == 0
                entry["data_sha256"].append(sha256(bytes(buf)))
                h = (C.c_double * 256)()
                assert ref.refdr_copy_histogram(t, h) == 0
                entry["histogram_sha256"].append(sha256(np.asarray(list(h), dtype=np.float64).tobytes()))
        out.append(entry)
    return out


def rng():
    ref = C.CDLL(os.path.join(REF, "libref_rng.so"), mode=1)   # RTLD_LAZY
    ref.ParallelRNG.restype = C.c_uint32
    ref.ParallelRNG.argtypes = [C.c_uint32]
    ref.ParallelRNG3.restype = C.c_uint32
    ref.ParallelRNG3.argtypes = [C.c_uint32] * 3
    ref.mapUintFloat.restype = C.c_float
    ref.mapUintFloat.argtypes = [C.c_uint32]
    return tog.rng_streams(ref.ParallelRNG, ref.mapUintFloat, ref.ParallelRNG3)


def kernel_free():
    ref = C.CDLL(os.path.join(REF, "libref_kernel.so"), mode=1)   # RTLD_LAZY: 66 builtins stay undefined
    U4 = C.POINTER(C.c_uint32)
    ref.refk_hybrid_rand.restype = C.c_float
    ref.refk_hybrid_rand.argtypes = [U4]
    ref.refk_ui_rand_step.restype = C.c_uint32
    ref.refk_ui_rand_step.argtypes = [U4, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32]
    ref.refk_lcg_step.restype = C.c_uint32
    ref.refk_lcg_step.argtypes = [U4, C.c_uint32, C.c_uint32]
    ref.refk_check_bounding_box.restype = C.c_int
    ref.refk_check_bounding_box.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float]
    for name, n in (("ParallelRNG", 1), ("ParallelRNG3", 3)):   # the #include of random.cl, once more
        getattr(ref, name).restype = C.c_uint32
        getattr(ref, name).argtypes = [C.c_uint32] * n
    return tog.kernel_free_streams({"hybrid_rand": ref.refk_hybrid_rand, "ui_rand_step": ref.refk_ui_rand_step,
                                    "lcg_step": ref.refk_lcg_step, "parallel_rng": ref.ParallelRNG,
                                    "parallel_rng3": ref.ParallelRNG3,
                                    "check_bounding_box": ref.refk_check_bounding_box})


def main():
    out = {
        "_source": "outputs of the reference's own code compiled under oracle/_ref (make -C oracle ref) on the "
                   "seeded inputs of the tests that read this file; generated by oracle/gen_reference_outputs.py",
        "hdr_random": hdr_random(),
        "loader_random": loader_random(),
        "rng": rng(),
        "kernel_free": kernel_free(),
        "kernel_object_analysis": ref_kernel_free.analyse(os.path.join(REF, "ref_kernel.o")),
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
