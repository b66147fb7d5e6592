"""The volume morphology's share of the C ABI on a GPU-less host: the 32- and 72-byte structures, the four symbols, the
enumerators as the header states them, a NULL renderer, every refusal that needs no device (vrhip_morph_params_check),
vrhip_morph_element against the restatement for every radius triple of a small grid, the host-only functions under the
host sanitizers in a program of their own, and the CLI's usage text and refusals (no compute calls here)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import morph_ref as mr
from volumerenderercl_amd import _lib, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")


def test_struct_sizes_and_offsets():
    assert C.sizeof(_lib.MorphParams) == 32 and C.sizeof(_lib.MorphInfo) == 72 and C.sizeof(_lib.MorphSweepInfo) == 24
    for name, off in (("op", 0), ("shape", 4), ("radius", 8), ("reserved", 20)):
        assert getattr(_lib.MorphParams, name).offset == off
    for name, off in (("sweep", 0), ("scratch_bytes", 48), ("sweeps", 56), ("empty_skip", 60), ("in_place", 64), ("reserved", 68)):
        assert getattr(_lib.MorphInfo, name).offset == off
    for name, off in (("blocks", 0), ("blocks_fetched", 8), ("blocks_skipped", 16)):
        assert getattr(_lib.MorphSweepInfo, name).offset == off
    assert C.sizeof(_lib.FilterParams) == 140 and C.sizeof(_lib.FilterInfo) == 40   # (the others keep their sizes)
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for struct, size in (("vrhip_morph_params", 32), ("vrhip_morph_sweep_info", 24), ("vrhip_morph_info", 72)):
        assert re.search(r"\} %s;\s*/\* %d bytes \*/" % (struct, size), text), struct


def test_symbols_load_and_refuse_a_null_renderer():
    lib = _lib.load()
    for name in ("vrhip_morph_volume", "vrhip_morph_params_check", "vrhip_morph_element", "vrhip_last_morph_info"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.vrhip_abi_version() == 1
    p = _lib.MorphParams()
    assert lib.vrhip_morph_volume(None, C.byref(p), 0) == _lib.ERR_INVALID
    assert lib.vrhip_last_morph_info(None, C.byref(_lib.MorphInfo())) == _lib.ERR_INVALID


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    m = re.search(r"#define VRHIP_MORPH_MAX_RADIUS (\d+)u", text)
    assert m and int(m.group(1)) == 8 == _lib.MORPH_MAX_RADIUS == mr.MAX_RADIUS
    names = ["ERODE", "DILATE", "OPEN", "CLOSE", "GRADIENT", "TOPHAT", "BLACKHAT"]
    for value, name in enumerate(names):
        m = re.search(r"\bVRHIP_MORPH_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == value == getattr(_lib, "MORPH_" + name) == getattr(mr, name), name
        assert frontend.MORPH_OPS[name.lower()] == value and mr.OP_NAMES[value] == name.lower()
    for name, value in (("BOX", 0), ("BALL", 1)):
        m = re.search(r"\bVRHIP_MORPH_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == value == getattr(_lib, "MORPH_" + name) == getattr(mr, name)
        assert frontend.MORPH_SHAPES[name.lower()] == value


def _params(op=0, shape=1, radius=(1, 1, 1), reserved=(0, 0, 0)):
    p = _lib.MorphParams()
    p.op, p.shape = op, shape
    p.radius[:] = radius
    p.reserved[:] = reserved
    return p


def test_refusals_that_need_no_device():
    check = _lib.load().vrhip_morph_params_check
    assert check(None) == _lib.ERR_INVALID
    good = [_params(op=op, shape=shape, radius=radius) for op in range(7) for shape in (0, 1)
            for radius in ((0, 0, 0), (1, 1, 1), (8, 8, 8), (4, 0, 2), (0, 8, 1))]
    for p in good:
        assert check(C.byref(p)) == _lib.OK, (p.op, p.shape, tuple(p.radius))
    bad = [_params(op=7), _params(op=0xffffffff), _params(shape=2), _params(shape=0xffffffff),
           _params(radius=(9, 0, 0)), _params(radius=(0, 9, 0)), _params(radius=(0, 0, 9)), _params(radius=(0, 0, 0xffffffff))]
    bad += [_params(reserved=tuple(int(i == k) for i in range(3))) for k in range(3)]
    for p in bad:
        assert check(C.byref(p)) == _lib.ERR_INVALID, (p.op, p.shape, tuple(p.radius), tuple(p.reserved))


def test_element_against_the_restatement():
    """Every radius triple of {0, 1, 2, 3, 5, 8}^3, both shapes: the library's list is the restatement's, row for row."""
    lib = _lib.load()
    for shape, name in ((mr.BOX, "box"), (mr.BALL, "ball")):
        for radius in itertools.product((0, 1, 2, 3, 5, 8), repeat=3):
            want = mr.element(shape, radius)
            got = frontend.morph_element(name, radius)
            assert got.dtype == np.int8 and np.array_equal(got, want), (name, radius)
    for radius, n in (((1, 1, 1), 7), ((2, 2, 2), 33), ((4, 4, 4), 257), ((8, 8, 8), 2109), ((2, 0, 3), 19)):
        assert len(frontend.morph_element("ball", radius)) == n
    # a capacity below the count: the count is reported, nothing is written, the call is refused
    p = _params(shape=_lib.MORPH_BALL, radius=(2, 2, 2))
    n = C.c_uint32(0)
    buf = (C.c_int8 * (3 * 32))(*([99] * 96))
    assert lib.vrhip_morph_element(C.byref(p), buf, 32, C.byref(n)) == _lib.ERR_INVALID and n.value == 33
    assert list(buf) == [99] * 96
    assert lib.vrhip_morph_element(C.byref(p), None, 0, C.byref(n)) == _lib.ERR_INVALID and n.value == 33
    assert lib.vrhip_morph_element(C.byref(p), None, 5, C.byref(n)) == _lib.ERR_INVALID
    assert lib.vrhip_morph_element(None, buf, 32, C.byref(n)) == _lib.ERR_INVALID
    assert lib.vrhip_morph_element(C.byref(p), buf, 32, None) == _lib.ERR_INVALID
    assert lib.vrhip_morph_element(C.byref(_params(radius=(9, 1, 1))), buf, 32, C.byref(n)) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        frontend.morph_element("ball", (9, 0, 0))
    with pytest.raises(ValueError):
        frontend.morph_element("sphere", 1)


def test_host_functions_under_the_host_sanitizers(tmp_path):
    """The host-only functions are plain C++: compiled here -- not loaded into python -- with AddressSanitizer and
    UBSan into a stand-alone program with its own main, which is run in the environment as it is."""
    exe = str(tmp_path / "morph_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-x", "c++", os.path.join(ROOT, "volumerenderercl_amd", "csrc", "vrhip_morph_host.hip"),
                           os.path.join(ROOT, "tests", "cxx", "morph_host_main.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("morph host functions: ok (1458 elements)")


def test_usage_text_names_morph():
    res = subprocess.run([EXE, "--morph"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render")
    assert "--morph OP box|ball RX RY RZ" in res.stderr and "--filter gauss SIGMA [RADIUS]" in res.stderr
    base = [EXE, "--synth", "shells", "32", "UCHAR", "--out", "x"]
    for args in (["--morph", "erode", "ball", "1", "1"],                 # a radius is missing
                 ["--morph", "shrink", "ball", "1", "1", "1"],           # a bad op
                 ["--morph", "erode", "sphere", "1", "1", "1"],          # a bad shape
                 ["--morph", "erode", "ball", "9", "1", "1"], ["--morph", "erode", "box", "1", "-1", "1"],
                 ["--morph", "open", "box", "1", "1", "x"], ["--morph", "open", "box", "1", "1.5", "1"],
                 ["--morph", "open", "box", "1", "1", "1", "--ranks", "2"]):
        res = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), args
