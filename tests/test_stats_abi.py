"""The volume statistics' share of the C ABI on a GPU-less host: the 64-, 72- and 48-byte structures, the three symbols,
the constants as the header states them, a NULL renderer, every refusal that needs no device (vrhip_stats_params_check),
the CLI's usage text, and the known answers of frontend.mean_std and frontend.otsu_threshold (no compute calls here)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from volumerenderercl_amd import _lib, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")


def test_struct_sizes_and_offsets():
    assert C.sizeof(_lib.StatsParams) == 64 and C.sizeof(_lib.VolumeStats) == 72 and C.sizeof(_lib.StatsInfo) == 48
    for name, off in (("lo", 0), ("hi", 12), ("bins_v", 24), ("bins_g", 28), ("v_lo", 32), ("v_hi", 36), ("g_hi", 40),
                      ("flags", 44), ("reserved", 48)):
        assert getattr(_lib.StatsParams, name).offset == off
    for name, off in (("voxels", 0), ("nan", 8), ("below", 16), ("above", 24), ("gradient_nan", 32), ("binned", 40),
                      ("min", 48), ("max", 52), ("sum", 56), ("sum_sq", 64)):
        assert getattr(_lib.VolumeStats, name).offset == off
    for name, off in (("blocks", 0), ("blocks_fetched", 8), ("blocks_skipped_constant", 16), ("blocks_skipped_window", 24),
                      ("scratch_bytes", 32), ("empty_skip", 40), ("hist_path", 44)):
        assert getattr(_lib.StatsInfo, name).offset == off
    assert C.sizeof(_lib.MeshParams) == 48 and C.sizeof(_lib.LaunchInfo) == 128   # (the others keep their sizes)
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for struct, size in (("vrhip_stats_params", 64), ("vrhip_volume_stats", 72), ("vrhip_stats_info", 48)):
        assert re.search(r"\} %s;\s*/\* %d bytes \*/" % (struct, size), text), struct


def test_symbols_load_and_refuse_a_null_renderer():
    lib = _lib.load()
    for name in ("vrhip_volume_statistics", "vrhip_last_stats_info", "vrhip_stats_params_check"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.vrhip_abi_version() == 1
    st = _lib.VolumeStats()
    st.voxels = 7
    hist = np.full(4, 9, np.uint64)
    p = _lib.StatsParams()
    p.bins_v, p.bins_g, p.v_lo, p.v_hi = 4, 1, 0.0, 1.0
    assert lib.vrhip_volume_statistics(None, C.byref(p), C.byref(st), hist.ctypes.data_as(C.c_void_p), 0) == _lib.ERR_INVALID
    assert lib.vrhip_last_stats_info(None, C.byref(_lib.StatsInfo())) == _lib.ERR_INVALID
    assert st.voxels == 7 and (hist == 9).all()   # refused, not dereferenced


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for name, value in (("STATS_MOMENTS", _lib.STATS_MOMENTS), ("STATS_SUM_CHUNK", _lib.STATS_SUM_CHUNK),
                        ("STATS_MAX_BINS_V", 4096), ("STATS_MAX_BINS_G", 256), ("STATS_MAX_BINS", 65536)):
        m = re.search(r"#define VRHIP_%s (\d+)u" % name, text)
        assert m and int(m.group(1)) == value, name
    for name, value in (("STATS_PATH_LDS", 0), ("STATS_PATH_GLOBAL", 1)):
        m = re.search(r"\bVRHIP_%s = (\d+)" % name, text)
        assert m and int(m.group(1)) == value == getattr(_lib, name)
    from tests import stats_ref
    assert stats_ref.SUM_CHUNK == _lib.STATS_SUM_CHUNK and stats_ref.BLOCK == _lib.MESH_BLOCK


def _params(bins=(16, 4), window=(0.0, 1.0, 0.5), flags=0, reserved=(0, 0, 0, 0)):
    p = _lib.StatsParams()
    p.bins_v, p.bins_g = bins
    p.v_lo, p.v_hi, p.g_hi = window
    p.flags, p.reserved[:] = flags, reserved
    return p


def test_refusals_that_need_no_device():
    check = _lib.load().vrhip_stats_params_check
    inf, nan = float("inf"), float("nan")
    assert check(None) == _lib.ERR_INVALID
    good = [_params(), _params(bins=(1, 1)), _params(bins=(4096, 16)), _params(bins=(256, 256)), _params(flags=_lib.STATS_MOMENTS),
            _params(bins=(256, 1), window=(0.0, 1.0, nan)), _params(bins=(256, 1), window=(-1.0, 2.0, 0.0)),
            _params(window=(-1e38, 2e38, 3e38))]
    for p in good:
        assert check(C.byref(p)) == _lib.OK, (p.bins_v, p.bins_g, p.v_lo, p.v_hi, p.g_hi)
    bad = [_params(bins=(0, 1)), _params(bins=(4097, 1)), _params(bins=(4, 0)), _params(bins=(4, 257)), _params(bins=(4096, 17)),
           _params(bins=(512, 129)),
           _params(window=(nan, 1.0, 1.0)), _params(window=(0.0, nan, 1.0)), _params(window=(-inf, 1.0, 1.0)),
           _params(window=(0.0, inf, 1.0)), _params(window=(0.5, 0.5, 1.0)), _params(window=(0.75, 0.5, 1.0)),
           _params(window=(-3e38, 3e38, 1.0)), _params(window=(0.0, 1e-45, 1.0)),
           _params(window=(0.0, 1.0, 0.0)), _params(window=(0.0, 1.0, -1.0)), _params(window=(0.0, 1.0, inf)),
           _params(window=(0.0, 1.0, nan)), _params(window=(0.0, 1.0, 1e-45)),
           _params(flags=2), _params(flags=3), _params(flags=0x80000000)]
    bad += [_params(reserved=tuple(int(i == k) for i in range(4))) for k in range(4)]
    for p in bad:
        what = (p.bins_v, p.bins_g, p.v_lo, p.v_hi, p.g_hi, p.flags, tuple(p.reserved))
        assert check(C.byref(p)) == _lib.ERR_INVALID, what


def test_usage_text_names_stats():
    res = subprocess.run([EXE, "--stats-moments"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render")
    for opt in ("--stats FILE.json", "--stats-bins V G", "--stats-window LO HI GHI", "--stats-region X0 Y0 Z0 X1 Y1 Z1",
                "--stats-moments", "--stats-hist FILE.u64", "--timestep T"):
        assert opt in res.stderr
    for args in (["--stats-bins", "8", "2"], ["--stats-window", "0", "1", "1"], ["--stats-hist", "h.u64"], ["--timestep", "1"],
                 ["--stats-region", "0", "0", "0", "8", "8", "8"]):   # the other options need --stats
        res = subprocess.run([EXE, "--synth", "shells", "32", "UCHAR", "--out", "x"] + args, capture_output=True, text=True,
                             timeout=60)
        assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), args


def test_mean_std_known_answers():
    # the values 0.25 (3 voxels) and 0.75 (1 voxel), and a NaN that does not count
    st = dict(voxels=5, nan=1, sum=1.5, sum_sq=3 * 0.0625 + 0.5625)
    mean, std = frontend.mean_std(st)
    assert mean == 0.375 and std == math.sqrt(0.75 / 4 - 0.375 ** 2) == math.sqrt(0.046875)
    assert frontend.mean_std(dict(voxels=8, nan=0, sum=4.0, sum_sq=2.0)) == (0.5, 0.0)          # a constant
    assert frontend.mean_std(dict(voxels=4, nan=0, sum=2.0, sum_sq=math.nextafter(1.0, 0.0)))[1] == 0.0   # rounding below zero
    assert all(math.isnan(v) for v in frontend.mean_std(dict(voxels=4, nan=4, sum=0.0, sum_sq=0.0)))


def test_otsu_known_answers():
    # two equal spikes at bins 1 and 6 of 8 over [0, 1]: every boundary between them separates them equally well,
    # the middle one (k = 4) is reported
    h = np.zeros(8, np.uint64)
    h[1] = h[6] = 100
    assert frontend.otsu_threshold(h, 0.0, 1.0) == 0.5
    assert frontend.otsu_threshold(h, -1.0, 3.0) == 1.0        # the same bins over another window
    # adjacent modes: the one boundary between them
    h = np.array([0, 50, 0, 0], np.uint64)
    h[2] = 70
    assert frontend.otsu_threshold(h, 0.0, 1.0) == 0.5
    # 4 bins with counts 6 2 1 6: the between-class variance is w0 w1 (mu0 - mu1)^2 with centres .125 .375 .625 .875;
    # k = 1: 6 * 9 * (0.125 - 6.375 / 9)^2 = 18.375, k = 2: 8 * 7 * (1.5 / 8 - 5.875 / 7)^2 = 23.79..., k = 3:
    # 9 * 6 * (2.125 / 9 - 0.875)^2 = 22.04...: the boundary 0.5
    assert frontend.otsu_threshold([6, 2, 1, 6], 0.0, 1.0) == 0.5
    # fewer than two occupied bins: the window's centre
    assert frontend.otsu_threshold([0, 9, 0, 0], 0.0, 1.0) == 0.5 and frontend.otsu_threshold([3], 0.2, 0.4) == pytest.approx(0.3)
    assert frontend.otsu_threshold(np.zeros(16), 0.0, 2.0) == 1.0
    # a uint64 row of a 2-D table and its column sum are both accepted
    table = np.zeros((4, 8), np.uint64)
    table[0, 1], table[3, 6] = 10, 10
    assert frontend.otsu_threshold(table.sum(axis=0), 0.0, 1.0) == 0.5
