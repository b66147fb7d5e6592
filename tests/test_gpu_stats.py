"""Volume statistics (vrhip_volume_statistics, vr_stats.hip) against their CPU restatement (tests/ref/stats_ref.c,
pinned by tests/test_stats_ref.py): the 72 bytes of the counts and moments and every word of the table equal the
restatement's -- every voxel type, one voxel, a row, partial blocks on every axis, regions that cut blocks, the table in
LDS and in global memory, moments on and off, object-order ESS on and off (the skipping must not change a bit), a
constant non-zero slab and a NaN inside a constant cell, determinism, a device destination, a second time step, the
renderer's state around a call, every refusal of the contract, the C++ class and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import common, stats_ref
from volumerenderercl_amd import FLOAT, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, _lib, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")

BINS = [(1, 1), (256, 1), (64, 64), (256, 256)]
WINDOW = (0.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _random(res, fmt, seed=5):
    rng = np.random.default_rng(seed)
    shape = (res[2], res[1], res[0])
    if fmt == UCHAR:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if fmt == USHORT:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return (rng.random(shape, dtype=np.float32) * 1.5 - 0.25).astype(np.float32)   # some below 0, some above 1


def _load(vr, vols, fmt):
    vr.loadVolumeArrays(vols if isinstance(vols, list) else [vols], fmt)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)


def _gpu(vr, bins, window=WINDOW, region=None, moments=False):
    """The raw call: (the 72 bytes of vrhip_volume_stats, hist uint64 [bins_g, bins_v] behind guard words)."""
    p = vr._stats_params(bins, window, region, moments)
    st = _lib.VolumeStats()
    n = bins[0] * bins[1]
    hist = np.full(n + 8, 0xabcdef, dtype=np.uint64)
    rc = vr._lib.vrhip_volume_statistics(vr._h, C.byref(p), C.byref(st), hist.ctypes.data_as(C.c_void_p), 0)
    assert rc == _lib.OK, vr._lib.vrhip_last_error(vr._h)
    assert (hist[n:] == 0xabcdef).all()
    return bytes(st), hist[:n].reshape(bins[1], bins[0]).copy()


def _blocks(res, region=None):
    lo, hi = region if region else ((0, 0, 0), res)
    n = 1
    for a, b in zip(lo, hi):
        n *= ((b - 1) // 8 - a // 8 + 1) if b > a else 0
    return n


def _check(vr, vol, fmt, bins, what, window=WINDOW, region=None, moments=False):
    """ESS on and off: counts, moments and table equal the restatement's bytes, and so each other.  Returns the
    restatement's pair and the two info blocks."""
    rst, rhist = stats_ref.compute(vol, fmt, bins, window, region, moments)
    infos = []
    for ess in (True, False):
        vr.setObjEss(ess)
        st, hist = _gpu(vr, bins, window, region, moments)
        got = _lib.VolumeStats.from_buffer_copy(st).as_dict()
        assert st == bytes(rst), "%s, ESS %s: %s" % (what, ess, got)
        bad = hist != rhist
        assert not bad.any(), "%s, ESS %s: %d bins differ, first at %s" % (what, ess, bad.sum(), np.argwhere(bad)[0])
        assert got["voxels"] == got["nan"] + got["below"] + got["above"] + got["gradient_nan"] + got["binned"]
        assert got["binned"] == int(hist.sum())
        si = vr.lastStatsInfo()
        assert si["blocks"] == _blocks(vol.shape[::-1], region), (what, si)
        assert si["blocks_fetched"] + si["blocks_skipped_constant"] + si["blocks_skipped_window"] == si["blocks"]
        assert si["empty_skip"] == (int(ess) if si["blocks"] else 0)
        assert si["hist_path"] == (_lib.STATS_PATH_LDS if bins[0] * bins[1] <= 16384 else _lib.STATS_PATH_GLOBAL)
        if not ess:
            assert si["blocks_fetched"] == si["blocks"]
        if moments and si["blocks"]:
            assert si["scratch_bytes"] >= 88 + 24 * ((si["blocks"] + 255) // 256)
        infos.append(si)
    vr.setObjEss(True)
    return (rst, rhist), infos


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
@pytest.mark.parametrize("res", [(1, 1, 1), (64, 1, 1), (9, 10, 11), (17, 8, 8)], ids=lambda r: "x".join(map(str, r)))
def test_small_volumes(vr, res, fmt):
    """One voxel; a row of eight blocks; partial blocks on every axis; a ninth point along x alone.  Every bin layout,
    the table in LDS ((1,1) .. (64,64)) and in global memory ((256,256)), moments on and off."""
    vol = _random(res, fmt)
    _load(vr, vol, fmt)
    paths = set()
    for k, bins in enumerate(BINS):
        for moments in ((False, True) if k % 2 else (True, False)):
            _, infos = _check(vr, vol, fmt, bins, "%s %d %s %s" % (res, fmt, bins, moments), moments=moments)
            paths.add(infos[0]["hist_path"])
    assert paths == {_lib.STATS_PATH_LDS, _lib.STATS_PATH_GLOBAL}


@pytest.mark.parametrize("fmt", [UCHAR, FLOAT], ids=["uchar", "float"])
def test_regions(vr, fmt):
    """Regions that cut blocks, one voxel, a flat one, an empty one -- and two that tile the volume add up."""
    vol = _random((17, 10, 11), fmt, seed=7)
    _load(vr, vol, fmt)
    for region in (((3, 1, 2), (15, 9, 11)), ((9, 8, 8), (10, 9, 9)), ((0, 0, 0), (8, 8, 8)), ((7, 0, 7), (9, 10, 9)),
                   ((4, 4, 4), (17, 4, 11))):
        for bins in ((64, 64), (256, 256)):
            (rst, _), infos = _check(vr, vol, fmt, bins, str(region), region=region, moments=True)
            n = int(np.prod([b - a for a, b in zip(*region)]))
            assert rst.voxels == n and (infos[0]["blocks"] == 0) == (n == 0)
    _, whole = _gpu(vr, (64, 64))
    _, left = _gpu(vr, (64, 64), region=((0, 0, 0), (11, 10, 11)))
    _, right = _gpu(vr, (64, 64), region=((11, 0, 0), (17, 10, 11)))
    assert np.array_equal(left + right, whole)
    # the Python twin: a dict and the table
    st, hist = vr.volume_statistics((64, 64), WINDOW, ((3, 1, 2), (15, 9, 11)), moments=True)
    rst, rhist = stats_ref.compute(vol, fmt, (64, 64), WINDOW, ((3, 1, 2), (15, 9, 11)), True)
    assert np.array_equal(hist, rhist) and hist.dtype == np.uint64 and hist.shape == (64, 64)
    assert st == {k: getattr(rst, k) for k, _ in rst._fields_}
    mean, std = frontend.mean_std(st)
    s = vol[2:11, 1:9, 3:15].astype(np.float64) * (1.0 / 255.0 if fmt == UCHAR else 1.0)
    assert abs(mean - s.mean()) < 1e-6 and abs(std - s.std()) < 1e-6


def _shells(vr):
    """Synthetic shells, large enough for two cells per axis at the cell grid's shift: (voxels, shift)."""
    vr.synthVolume("shells", (64, 64, 64), UCHAR)
    _, shift = vr.downloadCells()
    n = max(64, 2 << shift)
    if n != 64:
        vr.synthVolume("shells", (n, n, n), UCHAR)
    cells, shift = vr.downloadCells()
    assert min(cells.shape[:3]) >= 2 and shift >= 3
    return vr.downloadVolume(0), shift


def test_shells_and_skipping(vr):
    """The flagship's field: ESS on skips blocks, ESS off none, and not a bit changes; both table paths."""
    vol, _ = _shells(vr)
    vr.setTransferFunction(frontend.tff_from_stops())
    for bins, moments in (((256, 1), False), ((64, 64), True), ((256, 256), False)):
        (rst, _), (on, off) = _check(vr, vol, UCHAR, bins, "shells %s" % (bins,), moments=moments)
        assert rst.binned == vol.size
        assert on["blocks"] == off["blocks"] == vol.size // 512
        assert on["blocks_skipped_constant"] + on["blocks_skipped_window"] > 0, on
    # a window above the background: blocks of it are skipped as out of window, without moments only
    (_, _), (on, _) = _check(vr, vol, UCHAR, (256, 16), "shells window", window=(0.25, 1.0, 0.5))
    assert on["blocks_skipped_window"] > 0
    (_, _), (on, _) = _check(vr, vol, UCHAR, (256, 16), "shells window, moments", window=(0.25, 1.0, 0.5), moments=True)
    assert on["blocks_skipped_window"] == 0
    # from the table to an iso value: Otsu's threshold separates the background from the shells
    _, hist = _gpu(vr, (256, 1))
    t = frontend.otsu_threshold(hist[0], 0.0, 1.0)
    assert 0.0 < t < 1.0


def test_constant_slab_and_nan(vr):
    """Three cells along z: a constant non-zero slab (with its rim), a mixed layer, zeros -- and one NaN in the middle of
    a cell of zeros.  Without moments the constant cells of both values are skipped; with them only the zeros; the NaN's
    cell proves nothing and is fetched; no bit changes."""
    vr.synthVolume("shells", (64, 64, 64), UCHAR)
    _, shift = vr.downloadCells()
    S = 1 << shift
    vol = np.zeros((3 * S, 2 * S, 2 * S), dtype=np.float32)
    vol[:S + 2] = 0.3          # (a cell answers for its voxels and a rim of up to two: [S c - 1, S (c + 1) + 1])
    nan_at = (2 * S + S // 2, S + S // 2, S + S // 2)
    vol[nan_at] = np.nan
    _load(vr, vol, FLOAT)
    cells, shift2 = vr.downloadCells()
    assert shift2 == shift and cells.shape[:3] == (3, 2, 2)
    per_cell = (S // 8) ** 3
    for bins in ((64, 64), (256, 256)):
        (rst, rhist), (on, _) = _check(vr, vol, FLOAT, bins, "slab %s" % (bins,))
        assert rst.nan == 1 and rst.gradient_nan == 6
        assert on["blocks_skipped_constant"] == 4 * per_cell + 3 * per_cell and on["blocks_skipped_window"] == 0
        (_, _), (on, _) = _check(vr, vol, FLOAT, bins, "slab, moments %s" % (bins,), moments=True)
        assert on["blocks_skipped_constant"] == 3 * per_cell      # the zeros; 0.3 is fetched
    (rst, _), (on, _) = _check(vr, vol, FLOAT, (64, 4), "slab, window", window=(0.1, 1.0, 0.5))
    assert on["blocks_skipped_window"] == 3 * per_cell and on["blocks_skipped_constant"] == 4 * per_cell
    assert rst.below == vol.size - 1 - 4 * per_cell * 512 - 8 * S * S


def test_two_calls_and_a_device_destination(vr):
    import torch
    vol = _random((40, 33, 21), USHORT, seed=3)
    _load(vr, vol, USHORT)
    region = ((1, 2, 3), (39, 33, 20))
    a = _gpu(vr, (64, 64), region=region, moments=True)
    b = _gpu(vr, (64, 64), region=region, moments=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    rst, rhist = stats_ref.compute(vol, USHORT, (64, 64), WINDOW, region, True)
    assert a[0] == bytes(rst) and np.array_equal(a[1], rhist)
    rs = torch.cuda.ExternalStream(vr.get_stream())
    for bins in ((64, 64), (256, 256)):
        n = bins[0] * bins[1]
        dev = torch.full((n + 16,), 77, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = vr.volume_statistics(bins, WINDOW, region, moments=True, out_dev_ptr=dev.data_ptr())
        rs.synchronize()
        torch.cuda.synchronize()
        host = dev.cpu().numpy().view(np.uint64)
        rst, rhist = stats_ref.compute(vol, USHORT, bins, WINDOW, region, True)
        assert np.array_equal(host[:n].reshape(bins[1], bins[0]), rhist) and (host[n:] == 77).all()
        assert st == {k: getattr(rst, k) for k, _ in rst._fields_}


def test_second_time_step(vr):
    a, b = _random((17, 10, 11), UCHAR, seed=1), _random((17, 10, 11), UCHAR, seed=2)
    _load(vr, [a, b], UCHAR)
    try:
        first = _gpu(vr, (64, 64), moments=True)
        vr.setTimestep(1)
        _check(vr, b, UCHAR, (64, 64), "step 1", moments=True)
        second = _gpu(vr, (64, 64), moments=True)
        vr.setTimestep(0)
        _check(vr, a, UCHAR, (64, 64), "step 0 again", moments=True)
        assert first[0] != second[0] and _gpu(vr, (64, 64), moments=True)[0] == first[0]
    finally:
        vr.setTimestep(0)


def _ball(n=40, centre=(19.3, 20.1, 19.6), radius=13.0):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return np.round(np.clip(1.0 - d / radius, 0.0, 1.0) * 255).astype(np.uint8)


def _frames(vr, w, h, tech, between=None):
    vr.setTechnique(tech)
    vr.setIteration(0)
    vr.updateOutputImg(w, h)
    out = []
    if tech == TECH_RAYCAST:
        for i in range(3):
            vr.setSeed(500 + i)
            out.append(vr.runRaycastNoGL(w, h))
            if i == 1 and between:
                between()
    else:
        out.append(vr.render_samples(w, h, [11, 12]))
        if between:
            between()
        out.append(vr.render_samples(w, h, [13, 14, 15]))
    vr.setIteration(0)
    return out


@pytest.mark.parametrize("tech", [TECH_RAYCAST, TECH_PATHTRACE], ids=["raycast", "pathtrace_samples"])
def test_state_neutral(vr, tech):
    """Progressive frames with statistics between them equal the uninterrupted sequence bit for bit; the mesh's info
    block is not touched."""
    vol = _ball()
    _load(vr, vol, UCHAR)
    vr.updateView(common.views()["rot30"])
    vr.setObjEss(True)
    vr.isosurface_count(0.2)

    def between():
        before, mesh_before = vr.lastLaunchInfo(), vr.lastMeshInfo()
        vr.volume_statistics((256, 1))
        vr.volume_statistics((256, 256), (0.1, 0.9, 0.3), ((3, 5, 2), (29, 30, 31)), moments=True)
        assert vr.lastLaunchInfo() == before and vr.lastMeshInfo() == mesh_before

    try:
        plain = _frames(vr, 72, 56, tech)
        mixed = _frames(vr, 72, 56, tech, between)
    finally:
        vr.setTechnique(TECH_RAYCAST)
    assert len(plain) == len(mixed) >= 2
    for i, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "frame %d differs" % i
    assert not np.array_equal(plain[0], plain[-1])


def _params(bins=(16, 4), window=WINDOW, lo=(0, 0, 0), hi=(0, 0, 0), flags=0, reserved=(0, 0, 0, 0)):
    p = _lib.StatsParams()
    p.bins_v, p.bins_g = bins
    p.v_lo, p.v_hi, p.g_hi = window
    p.lo[:], p.hi[:], p.reserved[:], p.flags = lo, hi, reserved, flags
    return p


def test_refusals(vr):
    vol = _ball()
    _load(vr, vol, UCHAR)
    good = _gpu(vr, (16, 4), moments=True)
    lib, h = vr._lib, vr._h
    st = _lib.VolumeStats()
    hist = np.zeros(65536, np.uint64)
    H = hist.ctypes.data_as(C.c_void_p)
    inf, nan = float("inf"), float("nan")
    bad = [_params(bins=(0, 1)), _params(bins=(4097, 1)), _params(bins=(4, 0)), _params(bins=(4, 257)), _params(bins=(4096, 17)),
           _params(window=(nan, 1.0, 1.0)), _params(window=(0.0, inf, 1.0)), _params(window=(0.5, 0.5, 1.0)),
           _params(window=(0.75, 0.5, 1.0)), _params(window=(-3e38, 3e38, 1.0)), _params(window=(0.0, 1.0, 0.0)),
           _params(window=(0.0, 1.0, -1.0)), _params(window=(0.0, 1.0, inf)), _params(window=(0.0, 1.0, nan)),
           _params(flags=2), _params(flags=0x80000001),
           _params(hi=(41, 40, 40)), _params(hi=(40, 40, 41)), _params(lo=(5, 0, 0), hi=(4, 40, 40)),
           _params(lo=(0, 0, 9), hi=(40, 40, 8)), _params(hi=(0, 40, 40)), _params(lo=(1, 0, 0)), _params(hi=(40, 0, 0))]
    bad += [_params(reserved=tuple(int(i == k) for i in range(4))) for k in range(4)]
    for p in bad:
        what = (p.bins_v, p.bins_g, p.v_lo, p.v_hi, p.g_hi, p.flags, tuple(p.lo), tuple(p.hi), tuple(p.reserved))
        assert lib.vrhip_volume_statistics(h, C.byref(p), C.byref(st), H, 0) == _lib.ERR_INVALID, what
    ok = _params()
    assert lib.vrhip_volume_statistics(h, None, C.byref(st), H, 0) == _lib.ERR_INVALID
    assert lib.vrhip_volume_statistics(h, C.byref(ok), None, H, 0) == _lib.ERR_INVALID
    assert lib.vrhip_volume_statistics(h, C.byref(ok), C.byref(st), None, 0) == _lib.ERR_INVALID
    assert lib.vrhip_volume_statistics(h, C.byref(ok), C.byref(st), C.c_void_p(hist.ctypes.data + 8), 1) == _lib.ERR_INVALID
    assert lib.vrhip_last_stats_info(h, None) == _lib.ERR_INVALID
    assert not hist.any()
    with pytest.raises(ValueError):
        vr.volume_statistics((0, 1))
    with pytest.raises(ValueError):
        vr.volume_statistics((16, 4), region=((0, 0, 0), (41, 40, 40)))
    # g_hi is not looked at with one gradient bin
    assert lib.vrhip_volume_statistics(h, C.byref(_params(bins=(16, 1), window=(0.0, 1.0, nan))), C.byref(st), H, 0) == _lib.OK
    again = _gpu(vr, (16, 4), moments=True)
    assert again[0] == good[0] and np.array_equal(again[1], good[1])

    r = VolumeRenderCL()
    r.initialize()
    try:
        si = _lib.StatsInfo()
        assert r._lib.vrhip_last_stats_info(r._h, C.byref(si)) == _lib.ERR_NODATA
        assert r._lib.vrhip_volume_statistics(r._h, C.byref(ok), C.byref(st), H, 0) == _lib.ERR_NODATA   # no volume
        assert r._lib.vrhip_last_stats_info(r._h, C.byref(si)) == _lib.ERR_NODATA
        rg = np.zeros((40, 40, 40, 2), np.uint8)
        rg[..., 0] = vol
        r.loadVolumeArrays([rg], UCHAR, channels=2)
        assert r._lib.vrhip_volume_statistics(r._h, C.byref(ok), C.byref(st), H, 0) == _lib.ERR_UNSUPPORTED
        # no transfer function, no camera: the statistics all the same
        r.loadVolumeArrays([vol], UCHAR)
        fresh = _gpu(r, (16, 4), moments=True)
        assert fresh[0] == good[0] and np.array_equal(fresh[1], good[1])
    finally:
        r.close()


# ---- C++ class and CLI

def _synth(vr, kind, n):
    vr.synthVolume(kind, (n, n, n), UCHAR)
    return vr.downloadVolume(0)


def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_stats")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_stats.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "stats.bin")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    raw = open(out, "rb").read()
    vol = _synth(vr, "shells", 32)
    at = 0
    for bins, window, region, moments in (((64, 16), (0.0, 1.0, 0.5), None, True),
                                          ((256, 1), (0.1, 0.9, 1.0), ((3, 5, 2), (29, 30, 31)), False)):
        rst, rhist = stats_ref.compute(vol, UCHAR, bins, window, region, moments)
        assert raw[at:at + 72] == bytes(rst), bins
        at += 72
        assert raw[at:at + rhist.nbytes] == rhist.tobytes(), bins
        at += rhist.nbytes
    assert at == len(raw)


def test_cli_writes_the_statistics(vr, tmp_path):
    path, hpath = str(tmp_path / "stats.json"), str(tmp_path / "hist.u64")
    args = [EXE, "--synth", "shells", "32", "UCHAR", "--stats", path, "--stats-bins", "32", "8", "--stats-window", "0.1", "0.9",
            "0.25", "--stats-region", "0", "0", "0", "30", "32", "17", "--stats-moments", "--stats-hist", hpath]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    line = json.loads(res.stdout.strip().splitlines()[-1])
    doc = json.load(open(path))
    vol = _synth(vr, "shells", 32)
    rst, rhist = stats_ref.compute(vol, UCHAR, (32, 8), (0.1, 0.9, 0.25), ((0, 0, 0), (30, 32, 17)), True)
    assert np.array_equal(np.fromfile(hpath, dtype="<u8").reshape(8, 32), rhist)
    assert np.array_equal(np.array(doc["hist"], dtype=np.uint64), rhist) and doc["bins"] == [32, 8]
    for k in ("voxels", "nan", "below", "above", "gradient_nan", "binned", "sum", "sum_sq"):
        assert doc[k] == getattr(rst, k), k
    assert np.float32(doc["min"]) == rst.min and np.float32(doc["max"]) == rst.max
    mean, std = frontend.mean_std({k: getattr(rst, k) for k, _ in rst._fields_})
    assert abs(doc["mean"] - mean) < 1e-12 and abs(doc["std"] - std) < 1e-9
    assert line["voxels"] == rst.voxels and line["binned"] == rst.binned and line["stats"] == path


@pytest.mark.parametrize("extra", [["--pathtrace"], ["--mip"], ["--iso", 0.4], ["--slice-axis", "Z", 0], ["--depth", "max"],
                                   ["--mesh", 0.5, "m.ply"], ["--ranks", 2], ["--frames", 2], ["--rgba8"],
                                   ["--stats-bins", 4096, 17], ["--stats-bins", 0, 1], ["--stats-window", 0.5, 0.5, 1],
                                   ["--stats-bins", 8, 2, "--stats-window", 0, 1, 0], ["--timestep", -1]])
def test_cli_does_not_combine(tmp_path, extra):
    path = str(tmp_path / "bad.json")
    args = ["--synth", "shells", 32, "UCHAR", "--stats", path] + extra
    res = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), res.stderr
    assert "--stats FILE.json" in res.stderr and not os.listdir(str(tmp_path))
