"""The host side of the device-side ingest (no GPU needed): the loader's raw mode hands over the files' bytes
unchanged with the same parsed properties as the converting mode, and the libraries export the new entry
points with the signatures the Python bindings declare."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from volumerenderercl_amd import _lib, datraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "loader")
CASES = [c for c in json.load(open(os.path.join(GOLD, "expected.json")))["cases"] if c["rc"] == 0]


def _both(case):
    dat = os.path.join(GOLD, case["case"] + ".dat")
    conv, raw = datraw.DatRawReader(), datraw.DatRawReader()
    conv.read_files(datraw.Properties(dat))
    raw.read_files(datraw.Properties(dat), convert=False)
    return conv, raw


def _raw_files(case):
    """The raw file names of a case's .dat, as the loader resolves them (next to the .dat)."""
    conv = datraw.DatRawReader()
    dat = os.path.join(GOLD, case["case"] + ".dat")
    names = []
    for line in open(dat):
        tok = line.split()
        if tok and "ObjectFileName" in tok[0]:
            names = tok[1:]
    conv.read_files(datraw.Properties(dat))
    n = len(conv.data())
    if len(names) < n:   # a time series given as first name + count
        first = names[0]
        digits = [i for i, ch in enumerate(first) if ch.isdigit()]
        base, width, num = first[:digits[0]], digits[-1] - digits[0] + 1, int(first[digits[0]:digits[-1] + 1])
        names = [first] + ["%s%0*d" % (base, width, num + k) for k in range(1, n)]
    return [os.path.join(GOLD, x) for x in names]


@pytest.mark.parametrize("case", CASES, ids=[c["case"] for c in CASES])
def test_raw_mode_returns_the_files_bytes(case):
    _, raw = _both(case)
    files = _raw_files(case)
    assert len(raw.data()) == len(files)
    for t, f in enumerate(files):
        assert raw.data()[t].dtype == np.uint8
        assert raw.data()[t].tobytes() == open(f, "rb").read()
    assert raw.histograms() == []


@pytest.mark.parametrize("case", CASES, ids=[c["case"] for c in CASES])
def test_raw_mode_parses_like_the_converting_mode(case):
    conv, raw = _both(case)
    p, q = conv.properties(), raw.properties()
    assert q.volume_res == p.volume_res
    assert q.slice_thickness == p.slice_thickness
    assert q.format == p.format and q.endianness == p.endianness
    assert q.image_channel_order == p.image_channel_order
    assert len(raw.data()) == len(conv.data())
    for a, b in zip(raw.data(), conv.data()):
        assert a.nbytes == b.nbytes


def test_default_mode_is_the_converting_one():
    case = next(c for c in CASES if c["format"] == datraw.USHORT)
    dat = os.path.join(GOLD, case["case"] + ".dat")
    a, b = datraw.DatRawReader(), datraw.DatRawReader()
    a.read_files(datraw.Properties(dat))
    b.read_files(datraw.Properties(dat), convert=True)
    assert a.data()[0].tobytes() == b.data()[0].tobytes() and a.data()[0].dtype == np.uint16
    np.testing.assert_array_equal(a.histograms()[0], b.histograms()[0])


def test_libvrhip_exports_the_ingest_entry_points():
    lib = _lib.load()
    dbl, flt, u32 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    want = {
        "vrhip_ingest_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, u32, C.c_int, C.c_int, C.c_int,
                                       C.c_uint32, dbl, flt]),
        "vrhip_volume_histogram": (C.c_int, [C.c_void_p, C.c_uint32, dbl]),
        "vrhip_last_ingest_seconds": (C.c_double, [C.c_void_p]),
    }
    for name, (restype, argtypes) in want.items():
        assert _lib.SYMBOLS[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes
    # no renderer: an error code, not a crash (and 0 seconds)
    hist, vmax = (C.c_double * 256)(), C.c_float()
    assert lib.vrhip_ingest_raw(None, None, 0, None, 0, 1, 0, 0, hist, C.byref(vmax)) == _lib.ERR_INVALID
    assert lib.vrhip_volume_histogram(None, 0, hist) == _lib.ERR_INVALID
    assert lib.vrhip_last_ingest_seconds(None) == 0.0
    assert lib.vrhip_abi_version() == 1


def test_libvrhost_exports_the_raw_loader():
    datraw._load()
    host = C.CDLL(datraw.LIB_PATH)
    assert hasattr(host, "vrdr_load_raw")
    h = C.c_void_p()
    host.vrdr_load_raw.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    assert host.vrdr_load_raw(b"", None, C.byref(h)) == 1   # std::invalid_argument, like vrdr_load
    assert not h.value
