"""Technique 6's share of the C ABI on a GPU-less host (include/vrhip.h "technique == 6"): the four symbols, the
limits vrhip_tf2d_params_check accepts and refuses, vrhip_tf2d_lookup against the CPU restatement bit for bit,
vrhip_tf2d_build_ramp against a numpy formulation of the header's expression, the C++ caller against include/ alone,
the host-only functions under the host sanitizers in a stand-alone program, and the CLI's usage text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tf2d_ref
from volumerenderercl_amd import _lib, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")
INF, NAN = float("inf"), float("nan")


def test_symbols_constants_and_abi_version():
    lib = _lib.load()
    for name in ("vrhip_set_transfer_function_2d", "vrhip_tf2d_params_check", "vrhip_tf2d_lookup", "vrhip_tf2d_build_ramp"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.vrhip_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    assert re.search(r"#define VRHIP_ABI_VERSION 1\b", text)
    for name, value in (("TECHNIQUE_TF2D", _lib.TECH_TF2D), ("TF2D_MAX_NV", _lib.TF2D_MAX_NV), ("TF2D_MAX_NG", _lib.TF2D_MAX_NG),
                        ("TF2D_MAX_ENTRIES", _lib.TF2D_MAX_ENTRIES)):
        m = re.search(r"#define VRHIP_%s (\d+)u" % name, text)
        assert m and int(m.group(1)) == value, name
    assert _lib.TECH_TF2D == 6 and (_lib.TF2D_MAX_NV, _lib.TF2D_MAX_NG, _lib.TF2D_MAX_ENTRIES) == (4096, 256, 65536)
    # a NULL renderer is refused, not dereferenced
    one = np.zeros(4, np.uint8)
    assert lib.vrhip_set_transfer_function_2d(None, one.ctypes.data, 1, 1, 1.0) == _lib.ERR_INVALID


def test_params_check_limits():
    check = _lib.load().vrhip_tf2d_params_check
    for n_v, n_g, g_hi in ((1, 1, 1.0), (4096, 16, 0.25), (256, 256, 1e-30), (4096, 1, 3e38), (1, 256, 1e-45), (65536 // 256, 256, 1.0)):
        assert check(n_v, n_g, g_hi) == _lib.OK, (n_v, n_g, g_hi)
    for n_v, n_g, g_hi in ((0, 1, 1.0), (1, 0, 1.0), (4097, 1, 1.0), (1, 257, 1.0), (4096, 17, 1.0), (257, 256, 1.0),
                           (65537, 1, 1.0), (1, 1, 0.0), (1, 1, -0.0), (1, 1, -1.0), (1, 1, INF), (1, 1, -INF), (1, 1, NAN)):
        assert check(n_v, n_g, g_hi) == _lib.ERR_INVALID, (n_v, n_g, g_hi)
    # the product alone: 512 x 129 = 66048 > 65536 with both factors inside their own limits
    assert check(512, 128, 1.0) == _lib.OK and check(512, 129, 1.0) == _lib.ERR_INVALID


def _random_table(rng, n_v, n_g):
    t = rng.integers(0, 256, (n_g, n_v, 4), dtype=np.uint8)
    t[rng.random((n_g, n_v)) < 0.3, 3] = 0
    return t


def test_lookup_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    lookup = _lib.load().vrhip_tf2d_lookup
    special = [-INF, -2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 1.5, 2.0, 5.0, INF, NAN]
    for (n_v, n_g), g_hi in (((1, 1), 1.0), ((2, 1), 0.3), ((7, 5), 0.07), ((4096, 16), 0.25), ((256, 256), 3.0)):
        table = _random_table(rng, n_v, n_g)
        s = np.concatenate([rng.uniform(-0.2, 1.2, 300), special, special]).astype(np.float32)
        m = np.concatenate([rng.uniform(0.0, 1.5 * g_hi, 300), special, special[::-1]]).astype(np.float32)
        for sv, mv in zip(s, m):
            out = (C.c_float * 4)()
            assert lookup(table.ctypes.data, n_v, n_g, g_hi, float(sv), float(mv), out) == _lib.OK
            mine = np.array(out[:], np.float32)
            ref = tf2d_ref.lookup(table, g_hi, sv, mv)
            assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (n_v, n_g, sv, mv, mine, ref)
            assert np.array_equal(frontend.tf2d_lookup(table, g_hi, sv, mv).view(np.uint32), ref.view(np.uint32))
    # refusals: nothing is written
    out = (C.c_float * 4)(9, 9, 9, 9)
    t = np.zeros((1, 1, 4), np.uint8)
    assert lookup(None, 1, 1, 1.0, 0.0, 0.0, out) == _lib.ERR_INVALID
    assert lookup(t.ctypes.data, 1, 1, 0.0, 0.0, 0.0, out) == _lib.ERR_INVALID
    assert lookup(t.ctypes.data, 0, 1, 1.0, 0.0, 0.0, out) == _lib.ERR_INVALID
    assert lookup(t.ctypes.data, 1, 1, 1.0, 0.0, 0.0, None) == _lib.ERR_INVALID
    assert list(out) == [9, 9, 9, 9]


def _ramp_numpy(tff, n_g, g_hi, g0, g1):
    """include/vrhip.h's expression, one rounded fp32 operation each."""
    f = np.float32
    tff = np.asarray(tff, np.uint8).reshape(-1, 4)
    out = np.repeat(tff[None], n_g, axis=0).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        gj = ((np.arange(n_g, dtype=np.float32) + f(0.5)) * f(g_hi)) / f(n_g)
        w = (gj - f(g0)) / (f(g1) - f(g0))
        wj = np.where(w < 0, f(0), np.where(w > 1, f(1), w)).astype(np.float32)
        x = tff[None, :, 3].astype(np.float32) * wj[:, None]
        q = np.floor(x)
        out[:, :, 3] = (q + np.where(x - q >= f(0.5), f(1), f(0))).astype(np.uint8)
    return out


def test_build_ramp_equals_the_header_expression():
    rng = np.random.default_rng(5)
    for n_v, n_g, g_hi, g0, g1 in ((1, 1, 1.0, 0.0, 1.0), (256, 8, 0.25, 0.02, 0.1), (7, 5, 0.07, 0.0, 0.07), (4096, 16, 0.3, 0.1, 0.1000001),
                                   (64, 256, 2.0, 0.5, 1.5), (1024, 64, 0.5, 0.0, 0.25)):
        tff = rng.integers(0, 256, (n_v, 4), dtype=np.uint8)
        tff[:4, 3] = [0, 1, 254, 255][:min(4, n_v)]
        mine = frontend.tf2d_ramp(tff, n_g, g_hi, g0, g1)
        ref = _ramp_numpy(tff, n_g, g_hi, g0, g1)
        assert mine.shape == (n_g, n_v, 4) and np.array_equal(mine, ref), (n_v, n_g)
        assert np.array_equal(mine[..., :3], np.broadcast_to(tff[None, :, :3], mine.shape[:2] + (3,)))   # rgb is copied
        assert np.all(np.diff(mine[..., 3].astype(int), axis=0) >= 0)                                     # the ramp rises
    # ties go away from zero: alpha 1 at weight exactly 0.5 becomes 1, alpha 3 at 0.5 becomes 2
    tff = np.array([[9, 9, 9, 1], [9, 9, 9, 3]], np.uint8)
    mine = frontend.tf2d_ramp(tff, 1, 1.0, 0.0, 1.0)   # g_0 = 0.5: w = 0.5
    assert mine[0, :, 3].tolist() == [1, 2]
    # below g0 transparent, from g1 on the table's own alpha
    mine = frontend.tf2d_ramp(np.full((3, 4), 200, np.uint8), 10, 1.0, 0.3, 0.6)
    assert np.all(mine[:3, :, 3] == 0) and np.all(mine[6:, :, 3] == 200) and np.all(mine[3, :, 3] > 0)
    assert np.array_equal(frontend.tf2d_from_1d(tff, 3), np.repeat(tff[None], 3, axis=0))
    for bad in (dict(g0=0.5, g1=0.5), dict(g0=-0.1, g1=0.5), dict(g0=0.0, g1=INF), dict(g0=NAN, g1=1.0), dict(g_hi=0.0), dict(n_g=257)):
        kw = dict(n_g=4, g_hi=1.0, g0=0.0, g1=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            frontend.tf2d_ramp(tff, **kw)


def test_caller_compiles_against_include_alone():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "caller_tf2d.cpp")])


def test_host_functions_under_the_host_sanitizers(tmp_path):
    """The host-only functions are plain C++: compiled here -- not loaded into python -- with AddressSanitizer and
    UBSan into a stand-alone program with its own main, which is run in the environment as it is.  The sanitizers'
    runtimes are linked statically: the program then does not care what else the process has loaded before it."""
    exe = str(tmp_path / "tf2d_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-x", "c++", os.path.join(ROOT, "volumerenderercl_amd", "csrc", "vrhip_tf2d_api.hip"),
                           os.path.join(ROOT, "tests", "cxx", "tf2d_host_main.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("tf2d host functions: ok")


def test_python_wrapper_and_mirror_header():
    from volumerenderercl_amd import TECH_TF2D, VolumeRenderCL
    assert TECH_TF2D == 6 and hasattr(VolumeRenderCL, "setTransferFunction2D")
    text = open(os.path.join(ROOT, "include", "volumerendercl.h")).read()
    assert "TECH_TF2D = 6" in text and "setTransferFunction2D(" in text and "rampTransferFunction2D(" in text
    out = subprocess.run(["nm", "-DC", os.path.join(ROOT, "volumerenderercl_amd", "libvrhost.so")], capture_output=True,
                         text=True, check=True).stdout
    for sym in ("VolumeRenderCL::setTransferFunction2D(", "VolumeRenderCL::rampTransferFunction2D("):
        assert any(" T " in l and sym in l for l in out.splitlines()), sym


def test_cli_usage_names_tf2d():
    res = subprocess.run([EXE, "--no-such-option"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render")
    for opt in ("--tf2d FILE NV NG GHI", "--tf2d-ramp NG GHI G0 G1"):
        assert opt in res.stderr
    base = [EXE, "--synth", "shells", "32", "UCHAR", "--out", "x"]
    for args in (["--tf2d-ramp", "8", "0.25", "0.1", "0.1"], ["--tf2d-ramp", "0", "0.25", "0.0", "0.1"], ["--tf2d-ramp", "8", "0", "0.0", "0.1"],
                 ["--tf2d-ramp", "8", "0.25", "0.0", "0.1", "--mip"], ["--tf2d-ramp", "8", "0.25", "0.0", "0.1", "--iso", "0.5"],
                 ["--tf2d-ramp", "8", "0.25", "0.0", "0.1", "--ranks", "2"], ["--tf2d-ramp", "8", "0.25", "0.0", "0.1", "--ao"],
                 ["--tf2d", "t.rgba", "4097", "1", "0.25"], ["--tf2d", "t.rgba", "512", "129", "0.25"],
                 ["--tf2d", "t.rgba", "8", "8", "0.25", "--tf2d-ramp", "8", "0.25", "0.0", "0.1"]):
        res = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), args
