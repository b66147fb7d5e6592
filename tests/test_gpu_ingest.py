"""Device-side ingest (vrhip_ingest_raw, vr_ingest.hip) against the host loader on the same raw files: the
stored bytes, the 256 doubles of the histogram and max_value must be EQUAL -- the loader's per-voxel work is
an order-independent maximum, one correctly rounded fp32 operation and an integer count, so there is nothing
to tolerate.  The host loader itself is pinned to the compiled reference by tests/test_loader_golden.py and
tests/test_loader_differential.py.  Also: the histogram of volumes that were never on the host
(vrhip_volume_histogram), and a frame from an ingested volume."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import common, scenes
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL, datraw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "loader")
PKG = os.path.join(ROOT, "volumerenderercl_amd")
NP = {UCHAR: np.uint8, USHORT: np.uint16, FLOAT: np.float32}
NAME = {UCHAR: "UCHAR", USHORT: "USHORT", FLOAT: "FLOAT"}
FLT_MIN = float(np.finfo(np.float32).tiny)
SIZE_ERROR = "Volume size does not match size specified in dat file."


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


@pytest.fixture
def vr_small_slabs(monkeypatch):
    """A renderer whose ingest staging holds the minimum of four slices (the knob is read by vrhip_create)."""
    monkeypatch.setenv("VRHIP_INGEST_SLAB_BYTES", "1")
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _write(tmp_path, name, words, res, fmt, big=False, order=None, extra=b"", drop=0):
    """`words`: the values a reader of the file's endianness sees, x fastest; returns the .dat path."""
    a = np.ascontiguousarray(words, dtype=NP[fmt]).reshape(-1)
    data = (a.byteswap() if big and fmt != UCHAR else a).tobytes() + extra
    if drop:
        data = data[:-drop]
    (tmp_path / (name + ".raw")).write_bytes(data)
    text = "ObjectFileName: %s.raw\nResolution: %d %d %d\nFormat: %s\n" % ((name,) + tuple(res) + (NAME[fmt],))
    if big:
        text += "Endianness: BIG\n"
    if order:
        text += "ChannelOrder: %s\n" % order
    (tmp_path / (name + ".dat")).write_text(text)
    return str(tmp_path / (name + ".dat"))


def _host(dat):
    r = datraw.DatRawReader()
    r.read_files(datraw.Properties(dat))
    return r


def _check(vr, dat, channels=1):
    """Loads `dat` with the host loader and with device ingest; bytes, histogram and max_value must be equal.
    Returns (host reader, ingest histogram of step 0)."""
    host = _host(dat)
    hp = host.properties()
    n = vr.loadVolumeData(datraw.Properties(dat), ingest="device")
    assert n == len(host.data())
    vox = hp.volume_res[0] * hp.volume_res[1] * hp.volume_res[2]
    for t in range(n):
        want = host.data()[t][:vox * channels][0::channels]   # what is stored (channel 0), without excess words
        got = vr.downloadVolume(t)
        assert got.dtype == want.dtype
        assert got.tobytes() == want.tobytes()                # NaN payloads and -0.0 count
        hist = vr.getHistogram(t)
        assert hist.dtype == np.float64 and hist.shape == (256,)
        assert hist.tolist() == host.histograms()[t].tolist()
    assert vr._props.max_value == hp.max_value and vr._props.min_value == hp.min_value
    return host, vr.getHistogram(0)


def _rng_words(fmt, n, seed, top=4095):
    rng = np.random.default_rng(seed)
    if fmt == UCHAR:
        return rng.integers(0, 256, n).astype(np.uint8)
    if fmt == USHORT:
        w = rng.integers(0, top + 1, n).astype(np.uint16)
        w[n // 2] = top
        return w
    return (rng.random(n) * 700.0 - 100.0).astype(np.float32)


# ---- padding on every axis and none, every format and endianness

@pytest.mark.parametrize("big", [False, True], ids=["little", "big"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
@pytest.mark.parametrize("res", [(5, 7, 9), (13, 6, 3), (4, 4, 4)], ids=lambda r: "x".join(map(str, r)))
def test_small_shapes(vr, tmp_path, res, fmt, big):
    n = res[0] * res[1] * res[2]
    words = _rng_words(fmt, n, seed=n + fmt)
    if fmt == USHORT and big:
        # The reference takes the maximum of the words as a little-endian host reads them.  `words` is what a
        # big-endian reader sees; 0xff01 is read as 0x01ff = 511 by the host -- below the host-side maximum --
        # while its big-endian value, 65281, is above every other word: a swapped comparison changes the result.
        words = (words & 0x0fff).astype(np.uint16)
        words[1] = 0xff01
        host_side = words.byteswap()
        assert int(host_side.max()) != int(words.max()) and int(host_side[1]) == 0x01ff < int(host_side.max())
    host, hist = _check(vr, _write(tmp_path, "v", words, res, fmt, big))
    assert hist.sum() == n                                    # padding voxels are not counted
    if fmt == USHORT and big:
        assert host.properties().max_value == float(words.byteswap().max())


# ---- the maximum is carried across slabs

@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("fmt", [USHORT, FLOAT], ids=["ushort", "float"])
def test_maximum_across_slabs(vr_small_slabs, tmp_path, fmt, where):
    res = (64, 48, 40)                                        # ten slabs of four slices
    n = res[0] * res[1] * res[2]
    words = _rng_words(fmt, n, seed=5, top=999)
    words[words >= (999 if fmt == USHORT else 500.0)] = 1
    pos = 17 if where == "first" else n - 17
    words[pos] = 3000 if fmt == USHORT else 2500.5
    host, hist = _check(vr_small_slabs, _write(tmp_path, "v", words, res, fmt))
    assert host.properties().max_value == float(words[pos]) and hist.sum() == n


def test_slab_size_changes_no_stored_byte(vr, vr_small_slabs, tmp_path):
    res = (21, 10, 19)
    words = _rng_words(FLOAT, res[0] * res[1] * res[2], seed=3)
    dat = _write(tmp_path, "v", words, res, FLOAT, big=True)
    _check(vr, dat)
    _check(vr_small_slabs, dat)
    assert vr.downloadVolume(0).tobytes() == vr_small_slabs.downloadVolume(0).tobytes()


# ---- FLOAT: raw values of every kind

@pytest.mark.parametrize("big", [False, True], ids=["little", "big"])
@pytest.mark.parametrize("palette", scenes.FLOAT_PALETTES)
def test_float_palettes(vr, tmp_path, palette, big):
    res = (13, 10, 9)
    vol = scenes.float_volume(palette, res)
    host, hist = _check(vr, _write(tmp_path, "v", vol, res, FLOAT, big))
    if palette == "negative":
        assert host.properties().max_value == FLT_MIN         # nothing above FLT_MIN: the loader's start value
    if palette == "specials":
        assert np.isnan(vol).any() and np.isinf(vol).any() and host.properties().max_value == float("inf")
    assert hist.sum() == vol.size


def _half_quotients():
    """fp32 values v with fl(fl(v / 4) * 255) == k + 0.5 exactly, found with NumPy's fp32 arithmetic."""
    k = np.arange(255, dtype=np.float64) + 0.5
    v = (np.float32(4.0) * (k / 255.0).astype(np.float32)).astype(np.float32)   # (* 4 and / 4 are exact)
    q = (v / np.float32(4.0)).astype(np.float32)
    keep = (q * np.float32(255.0)).astype(np.float32) == k.astype(np.float32)
    return v[keep]


def test_float_ties_and_denormal_quotients(vr, tmp_path):
    halves = _half_quotients()
    assert halves.size >= 32                                  # the ties are present
    tiny = np.float32(2e-38)                                  # a normal number whose quotient by 4 is denormal
    assert tiny > np.float32(FLT_MIN) and 0 < float(tiny) / 4.0 < FLT_MIN
    special = np.array([4.0, tiny, -tiny, 1e-40, -1e-41, FLT_MIN, 4.0 * FLT_MIN, -0.0, 0.0, 3.9999998], np.float32)
    words = np.concatenate([halves, -halves, special])
    res = (words.size, 1, 1)
    for big in (False, True):
        host, hist = _check(vr, _write(tmp_path, "t%d" % big, words, res, FLOAT, big))
        assert host.properties().max_value == 4.0
        stored = vr.downloadVolume(0).reshape(-1)
        # round half away from zero: the tie k + 0.5 is counted in bin k + 1
        assert (stored[:halves.size] * np.float32(255.0) % 1 == 0.5).all()
        denorm = stored[2 * halves.size + 1]
        assert 0 < float(denorm) < FLT_MIN and denorm == np.float32(tiny) / np.float32(4.0)
        assert hist.sum() == words.size


# ---- USHORT: every product within one ulp of a tie

def _near_ties(top):
    stretch = np.float32(65535.0) / np.float32(top)
    v = np.arange(top + 1, dtype=np.float32)
    p = (v * stretch).astype(np.float32)
    tie = np.floor(p) + np.float32(0.5)
    near = np.abs(p.astype(np.float64) - tie.astype(np.float64)) <= np.spacing(p).astype(np.float64)
    return np.nonzero(near)[0].astype(np.uint16)


@pytest.mark.parametrize("big", [False, True], ids=["little", "big"])
@pytest.mark.parametrize("top", [1, 255, 1000, 4095, 43690, 65535])
def test_ushort_maxima_and_ties(vr, tmp_path, top, big):
    ties = _near_ties(top)
    fill = np.random.default_rng(top).integers(0, top + 1, 300).astype(np.uint16)
    host_side = np.concatenate([[top], ties, fill]).astype(np.uint16)   # the words the host reads
    res = (37, 5, -(-host_side.size // 185))
    host_side = np.concatenate([host_side, np.zeros(res[0] * res[1] * res[2] - host_side.size, np.uint16)])
    words = host_side.byteswap() if big else host_side        # _write swaps them back into the file
    host, hist = _check(vr, _write(tmp_path, "v", words, res, USHORT, big))
    assert host.properties().max_value == float(top) and hist.sum() == host_side.size


def test_ushort_all_zero_step_stays_zero(vr, tmp_path):
    """Not compared with the loader, whose 0 * inf -> NaN -> integer conversion is undefined (vrhip.h)."""
    res = (9, 6, 5)
    n = res[0] * res[1] * res[2]
    vr.loadVolumeData(datraw.Properties(_write(tmp_path, "z", np.zeros(n, np.uint16), res, USHORT)), ingest="device")
    assert not vr.downloadVolume(0).any()
    assert vr.getHistogram(0)[0] == n and vr.getHistogram(0).sum() == n
    assert vr._props.max_value == FLT_MIN


# ---- the histogram's paths: one bin per wave, many blocks

@pytest.mark.parametrize("fmt,value", [(UCHAR, 7), (USHORT, 300), (FLOAT, 2.5), (FLOAT, 0.0), (FLOAT, -1.0)],
                         ids=["uchar", "ushort", "float", "float-zero", "float-negative"])
def test_constant_volumes(vr, tmp_path, fmt, value):
    res = (516, 5, 3)                                         # a brick row fills every lane of every wave
    n = res[0] * res[1] * res[2]
    words = np.full(n, value, NP[fmt])
    if fmt == USHORT:
        words[-1] = 600                                       # (constant but for the maximum: stretch != 65535 / 300)
    host, hist = _check(vr, _write(tmp_path, "c", words, res, fmt))
    assert hist.sum() == n and np.count_nonzero(hist) == (2 if fmt == USHORT else 1)


def test_random_uchar_96(vr, tmp_path):
    res = (96, 96, 96)
    words = np.random.default_rng(96).integers(0, 256, 96 ** 3).astype(np.uint8)
    host, hist = _check(vr, _write(tmp_path, "r", words, res, UCHAR))
    assert hist.tolist() == np.bincount(words, minlength=256).astype(np.float64).tolist()


# ---- RG / RGBA: every scalar of every channel

def _frame(vr, fmt):
    vr.setTransferFunction(common.tffs()["default"])
    vr.setSeed(scenes.SEED)
    vr.setLinearInterpolation(fmt != UCHAR)
    vr.updateView(common.views()["rot30"])
    vr.setIteration(0)
    return vr.runRaycastNoGL(64, 48)


@pytest.mark.parametrize("big", [False, True], ids=["little", "big"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
@pytest.mark.parametrize("order,nch", [("RG", 2), ("RGBA", 4)])
def test_multichannel(vr, tmp_path, order, nch, fmt, big):
    res = (6, 5, 7)
    n = res[0] * res[1] * res[2]
    words = _rng_words(fmt, n * nch, seed=nch * 10 + fmt)
    if fmt == FLOAT:
        words = np.abs(words)
        words[3] = 900.0                                      # the maximum sits in channel 3 (or 1)
    dat = _write(tmp_path, "m", words, res, fmt, big, order=order)
    host, hist = _check(vr, dat, channels=nch)
    assert hist.sum() == n * nch
    # the planes behind channel 0 cannot be downloaded: their stored values through the resident-volume
    # histogram, and a frame (RGBA reads all four, RG two), against the host path's
    stored, frame = vr.volumeHistogram(0), _frame(vr, fmt)
    vr.loadVolumeData(datraw.Properties(dat))
    assert vr.volumeHistogram(0).tolist() == stored.tolist()
    assert _frame(vr, fmt).tobytes() == frame.tobytes()


# ---- files longer and shorter than the volume

@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_file_longer_than_the_volume(vr, tmp_path, fmt):
    res = (5, 7, 9)
    n = res[0] * res[1] * res[2]
    words = _rng_words(fmt, n, seed=37)
    # 37 more bytes: the loader's loops run over them too -- they hold the maximum (and an odd byte at the end)
    extra = {UCHAR: bytes([255]) * 37, USHORT: np.full(18, 5000, np.uint16).tobytes() + b"\x01",
             FLOAT: np.full(9, 1e6, np.float32).tobytes() + b"\x01"}[fmt]
    assert len(extra) == 37
    host, hist = _check(vr, _write(tmp_path, "l", words, res, fmt, extra=extra))
    whole = n + 37 // np.dtype(NP[fmt]).itemsize
    assert hist.sum() == whole and host.data()[0].size == whole
    if fmt != UCHAR:
        assert host.properties().max_value == (5000.0 if fmt == USHORT else 1e6)
    # the resident-volume histogram sees the stored voxels only
    assert vr.volumeHistogram(0).sum() == n


@pytest.mark.parametrize("fmt", [UCHAR, FLOAT], ids=["uchar", "float"])
def test_file_shorter_than_the_volume(vr, tmp_path, fmt):
    res = (5, 7, 9)
    words = _rng_words(fmt, res[0] * res[1] * res[2], seed=1)
    dat = _write(tmp_path, "s", words, res, fmt, drop=3)
    with pytest.raises(RuntimeError) as e:
        vr.loadVolumeData(datraw.Properties(dat), ingest="device")
    assert str(e.value) == SIZE_ERROR
    with pytest.raises(RuntimeError) as e:
        vr.loadVolumeData(datraw.Properties(dat))
    assert str(e.value) == SIZE_ERROR


# ---- the reference's own loader cases

GOLDEN = [c for c in json.load(open(os.path.join(GOLD, "expected.json")))["cases"] if c["rc"] == 0]


@pytest.mark.parametrize("case", GOLDEN, ids=[c["case"] for c in GOLDEN])
def test_golden_loader_cases(vr, case):
    host, _ = _check(vr, os.path.join(GOLD, case["case"] + ".dat"))
    if case["case"] == "c12":   # (no Format key: the reference reads nothing)
        return
    vox = case["res"][0] * case["res"][1] * case["res"][2]
    for t in range(case["n_timesteps"]):
        want = base64.b64decode(case["data"][t])
        assert vr.downloadVolume(t).tobytes() == want[:vox * vr.downloadVolume(t).itemsize]
        assert {str(i): v for i, v in enumerate(vr.getHistogram(t)) if v} == case["histogram"][t]
    assert vr._props.max_value == case["max_value"]


# ---- histogram of resident volumes

def _bins(vol):
    """The loader's binning of stored values, with NumPy."""
    v = vol.reshape(-1)
    if v.dtype == np.uint8:
        b = v.astype(np.int64)
    elif v.dtype == np.uint16:
        b = (v >> 8).astype(np.int64)
    else:
        with np.errstate(all="ignore"):
            m = (v * np.float32(255.0)).astype(np.float64)
            rb = np.sign(m) * np.floor(np.abs(m) + 0.5)       # round half away from zero
            b = np.where((rb >= 0) & (rb <= 255), rb, 255).astype(np.int64)
    return np.bincount(b, minlength=256).astype(np.float64)


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
@pytest.mark.parametrize("kind", ["sphere", "shells"])
def test_synthetic_volume_has_a_histogram(vr, kind, fmt):
    res = (33, 20, 17)
    vr.synthVolume(kind, res, fmt)
    hist = vr.getHistogram(0)
    assert hist.tolist() == _bins(vr.downloadVolume(0)).tolist()
    assert hist.sum() == res[0] * res[1] * res[2] and np.count_nonzero(hist) > 1


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_device_uploaded_volume_has_a_histogram(vr, fmt):
    import torch
    res = (33, 20, 17)
    vol = scenes.float_volume("specials", res) if fmt == FLOAT else common.noise_volume(res, fmt, seed=4, smooth=False)
    dev = torch.from_numpy(vol.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    vr._check(vr.lib.vrhip_clear_volumes(vr.handle))
    vr._check(vr.lib.vrhip_upload_volume_device(vr.handle, C.c_void_p(dev.data_ptr()), (C.c_uint32 * 3)(*res), fmt, 0))
    hist = vr.volumeHistogram(0)
    assert hist.tolist() == _bins(vol).tolist() and hist.sum() == vol.size


def test_ingested_histogram_is_the_resident_one(vr, tmp_path):
    """Little-endian data: what ingest returned is the binning of what it stored."""
    res = (13, 6, 3)
    for fmt in (UCHAR, USHORT, FLOAT):
        words = _rng_words(fmt, res[0] * res[1] * res[2], seed=fmt)
        vr.loadVolumeData(datraw.Properties(_write(tmp_path, "h%d" % fmt, words, res, fmt)), ingest="device")
        assert vr.getHistogram(0).tolist() == vr.volumeHistogram(0).tolist()
        assert vr.lastIngestSeconds() > 0.0


# ---- the C++ class and a frame

def test_cpp_caller_frames_are_bit_identical(tmp_path):
    exe = str(tmp_path / "caller_ingest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_ingest.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    vol = common.noise_volume((40, 36, 33), USHORT, seed=2, smooth=False) >> 3
    dat = _write(tmp_path, "v", vol, (40, 36, 33), USHORT, big=True)
    out = subprocess.run([exe, dat], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "12288 floats identical, histogram total 47520, synthetic total 13824" in out.stdout


def test_parity_frame_from_an_ingested_volume(vr, tmp_path):
    """scenes.CASES[12] (USHORT 48^3, 80 x 64, rot30): the frame from the device-ingested .dat is the frame from
    the host-loaded one."""
    fmt, res, (W, H), view, tff, kw = scenes.CASES[12]
    assert fmt == USHORT
    vol = common.noise_volume(res, fmt, seed=1, smooth=False) >> 2   # (maximum below 65535: the stretch does something)
    dat = _write(tmp_path, "p", vol, res, fmt)
    frames = []
    for ingest in ("host", "device"):
        vr.loadVolumeData(datraw.Properties(dat), ingest=ingest)
        vr.setTransferFunction(common.tffs()[tff])
        vr.setSeed(scenes.SEED)
        vr.setIllumination(kw.get("illum", 1))
        vr.setLinearInterpolation(True)
        vr.updateView(common.views()[view])
        vr.setIteration(0)
        frames.append(vr.runRaycastNoGL(W, H))
    assert float(np.abs(frames[0] - frames[1]).max()) == 0.0 and frames[0].tobytes() == frames[1].tobytes()
    assert np.unique(frames[0].reshape(-1, 4), axis=0).shape[0] > 100   # (a picture, not a background)
