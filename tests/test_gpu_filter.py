"""Volume filters (vrhip_filter_volume, vr_filter.hip) against their CPU restatement (tests/ref/filter_ref.c, pinned by
tests/test_filter_ref.py): the downloaded destination equals the restatement byte for byte -- every voxel type, shapes
that are no multiple of the block or of a micro-brick, axes shorter than the radius, exactly one block, two tiles per
axis, every radius class with random signed and with Gaussian taps, the median, special floats, object-order ESS on and
off (the skipping must not change a byte) --, the three destinations, the refusals, the skip counts on a built
volume, what goes stale and what does not, the C++ class and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import filter_ref as fr
from volumerenderercl_amd import FLOAT, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, _lib, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")

F32 = np.float32
# (x, y, z): no multiple of the block (8) or a micro-brick (4); axes shorter than the radius, so that both clamps hit
# inside one tap sum; a multiple of both; exactly one block; the kernel's tile is the block: more than two per axis
SHAPES = [(37, 21, 13), (5, 70, 9), (64, 40, 24), (8, 8, 8), (17, 18, 19)]
RADII = [(0, 0, 0), (1, 1, 1), (8, 8, 8), (4, 0, 2), (0, 8, 1)]
FMTS = [UCHAR, USHORT, FLOAT]
FMT_IDS = ["uchar", "ushort", "float"]


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _random(res, fmt, seed=5, special=True):
    rng = np.random.default_rng(seed)
    shape = (res[2], res[1], res[0])
    if fmt == UCHAR:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if fmt == USHORT:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    v = (rng.random(shape, dtype=np.float32) * 4.0 - 1.5).astype(F32)   # values outside [0, 1]
    if special:
        flat = v.reshape(-1)
        idx = rng.choice(flat.size, 14, replace=False)
        flat[idx[:3]] = np.nan
        flat[idx[3]] = np.array([0xffc00123], np.uint32).view(F32)[0]   # a NaN with the sign set and a payload
        flat[idx[4:6]] = np.inf
        flat[idx[6:8]] = -np.inf
        flat[idx[8:11]] = -0.0
        flat[idx[11:]] = 0.0
    return v


def _bits(a):
    return a.view(np.uint32) if a.dtype == F32 else a


def _load(vr, vols, fmt, tff=False):
    vr.loadVolumeArrays(vols if isinstance(vols, list) else [vols], fmt)
    if tff:
        vr.setTransferFunction(frontend.tff_from_stops())
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)
    vr.setObjEss(True)


def _filter(vr, kind, radius=None, taps=None, dst=None):
    if kind == fr.MEDIAN3:
        return vr.filter_volume("median3", dst=dst)
    return vr.filter_volume("separable", taps=taps, radius=radius, dst=dst)


def _assert_equal(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d voxels differ, first at (z, y, x) %s: %s, restatement %s" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _blocks(res):
    return ((res[0] + 7) // 8) * ((res[1] + 7) // 8) * ((res[2] + 7) // 8)


def _check(vr, vol, fmt, kind, radius, taps, what):
    """Into step 1, ESS on and off: the bytes equal the restatement's.  The source (step 0, current) stays."""
    want = fr.compute(vol, fmt, kind, radius or (0, 0, 0), taps)
    infos = []
    for ess in (True, False):
        vr.setObjEss(ess)
        _filter(vr, kind, radius, taps, dst=1)
        _assert_equal(vr.downloadVolume(1), want, "%s, ESS %s" % (what, ess))
        fi = vr.lastFilterInfo()
        assert fi["blocks"] == _blocks(vol.shape[::-1]) == fi["blocks_fetched"] + fi["blocks_skipped"], (what, fi)
        assert fi["empty_skip"] == int(ess) and fi["in_place"] == 0 and fi["scratch_bytes"] == 16, (what, fi)
        if not ess:
            assert fi["blocks_skipped"] == 0
        infos.append(fi)
    vr.setObjEss(True)
    return want, infos


def _taps_random(radius, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.7, 0.9, r + 1).astype(F32) for r in radius]


def _taps_gauss(radius):
    return [fr.gaussian_taps(0.6 + 0.4 * r, r)[:r + 1] for r in radius]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("res", SHAPES, ids=lambda r: "x".join(map(str, r)))
def test_parity(vr, res, fmt):
    vol = _random(res, fmt, seed=sum(res) + fmt)
    _load(vr, vol, fmt)
    for k, radius in enumerate(RADII):
        for name, taps in (("random", _taps_random(radius, 31 * k + fmt)), ("gauss", _taps_gauss(radius))):
            _check(vr, vol, fmt, fr.SEPARABLE, radius, taps, "%s %s radius %s %s taps" % (res, FMT_IDS[fmt], radius, name))
    _check(vr, vol, fmt, fr.MEDIAN3, None, None, "%s %s median" % (res, FMT_IDS[fmt]))
    _assert_equal(vr.downloadVolume(0), vol, "the source")


@pytest.mark.parametrize("fmt", [UCHAR, USHORT], ids=["uchar", "ushort"])
def test_identity_and_saturation(vr, fmt):
    """Identity taps give the volume back; taps that overshoot clamp to the type's range on both sides."""
    res = (19, 9, 10)
    vol = _random(res, fmt, seed=3)
    _load(vr, vol, fmt)
    one = [np.ones(1, F32)] * 3
    want, _ = _check(vr, vol, fmt, fr.SEPARABLE, (0, 0, 0), one, "identity")
    assert np.array_equal(want, vol)
    for w0 in (3.0, -2.0):
        taps = [np.array([w0, 0.5], F32), np.ones(1, F32), np.ones(1, F32)]
        want, _ = _check(vr, vol, fmt, fr.SEPARABLE, (1, 0, 0), taps, "w0 = %g" % w0)
        assert (want == (np.iinfo(vol.dtype).max if w0 > 0 else 0)).mean() > 0.3


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_destinations(vr, fmt):
    """Appended, existing and in place give the same bytes; the source changes only in place; the info block says
    which; a destination above the number of steps is refused and the volumes stay."""
    res = (21, 13, 10)
    v0, v1 = _random(res, fmt, seed=8), _random(res, fmt, seed=9)
    _load(vr, [v0, v1], fmt)
    radius, taps = (2, 1, 3), _taps_random((2, 1, 3), 4)
    want = fr.compute(v0, fmt, fr.SEPARABLE, radius, taps)
    with pytest.raises(ValueError):
        _filter(vr, fr.SEPARABLE, radius, taps, dst=3)
    assert vr.getResolution()[3] == 2
    _assert_equal(vr.downloadVolume(0), v0, "step 0 after a refusal")
    _assert_equal(vr.downloadVolume(1), v1, "step 1 after a refusal")
    assert _filter(vr, fr.SEPARABLE, radius, taps, dst=2) == 2 and vr.getResolution()[3] == 3   # appended
    _assert_equal(vr.downloadVolume(2), want, "appended")
    assert vr.lastFilterInfo()["in_place"] == 0
    _filter(vr, fr.SEPARABLE, radius, taps, dst=1)                                             # existing
    _assert_equal(vr.downloadVolume(1), want, "existing")
    _assert_equal(vr.downloadVolume(0), v0, "the source")
    assert _filter(vr, fr.SEPARABLE, radius, taps) == 0                                        # in place
    _assert_equal(vr.downloadVolume(0), want, "in place")
    fi = vr.lastFilterInfo()
    nb = [(r + 3) // 4 for r in res]
    assert fi["in_place"] == 1 and fi["scratch_bytes"] == 16 + nb[0] * nb[1] * nb[2] * 64 * v0.itemsize, fi
    _assert_equal(vr.downloadVolume(2), want, "the appended step afterwards")
    # the median of the (now filtered) step 0, in place
    want2 = fr.compute(want, fmt, fr.MEDIAN3)
    _filter(vr, fr.MEDIAN3)
    _assert_equal(vr.downloadVolume(0), want2, "median in place")


def test_sharing_renderers(vr):
    """A renderer that borrows its volumes is refused before anything is touched; the owner filters in place under a
    sharer, which sees the new voxels at the address it holds."""
    res = (20, 12, 9)
    vol = _random(res, UCHAR, seed=12)
    _load(vr, vol, UCHAR, tff=True)
    twin = vr.shareVolumes()
    try:
        with pytest.raises(RuntimeError, match="belong to another renderer"):
            twin.filter_volume("median3")
        with pytest.raises(RuntimeError, match="belong to another renderer"):
            twin.filter_volume("median3", dst=1)
        _assert_equal(twin.downloadVolume(0), vol, "the sharer's view")
        _assert_equal(vr.downloadVolume(0), vol, "the owner's volume")
        want = fr.compute(vol, UCHAR, fr.MEDIAN3)
        vr.filter_volume("median3")
        assert vr.lastFilterInfo()["in_place"] == 1
        _assert_equal(vr.downloadVolume(0), want, "the owner, in place under a sharer")
        _assert_equal(twin.downloadVolume(0), want, "the sharer afterwards")
    finally:
        twin.close()


def test_unsupported_and_nodata():
    r = VolumeRenderCL()
    r.initialize()
    try:
        p = _lib.FilterParams()
        p.kind = _lib.FILTER_MEDIAN3
        assert r._lib.vrhip_last_filter_info(r._h, C.byref(_lib.FilterInfo())) == _lib.ERR_NODATA
        assert r._lib.vrhip_filter_volume(r._h, C.byref(p), 0) == _lib.ERR_NODATA
        assert r._lib.vrhip_filter_volume(r._h, None, 0) == _lib.ERR_INVALID
        rg = np.zeros((6, 5, 4, 2), np.uint8)
        r.loadVolumeArrays([rg], UCHAR)
        assert r._lib.vrhip_filter_volume(r._h, C.byref(p), 0) == _lib.ERR_UNSUPPORTED
        assert r._lib.vrhip_last_filter_info(r._h, C.byref(_lib.FilterInfo())) == _lib.ERR_NODATA
    finally:
        r.close()


@pytest.mark.parametrize("fmt", [UCHAR, FLOAT], ids=["uchar", "float"])
def test_ess_skips(vr, fmt):
    """Cells along z: two of a constant non-zero slab, one of noise, three of zeros (half the volume).  ESS on and off
    give the same bytes; off skips nothing; on, the median skips both constants and the smoothing only the zeros; the
    layer of blocks whose dilated extent reaches a noisy cell is fetched."""
    _load(vr, np.zeros((64, 64, 64), fr.NP_DTYPE[fmt]), fmt)
    _, shift = vr.downloadCells()
    S = 1 << shift
    assert shift >= 3
    rng = np.random.default_rng(2)
    vol = np.zeros((6 * S, 2 * S, 2 * S), fr.NP_DTYPE[fmt])
    c = 77 if fmt == UCHAR else F32(0.3)
    vol[:2 * S + 2] = c            # (a cell answers for its voxels and a rim of up to two)
    noise = vol[2 * S + 2:3 * S - 2]
    noise[...] = rng.integers(1, 256, noise.shape) if fmt == UCHAR else rng.random(noise.shape, dtype=F32) + F32(0.5)
    if fmt == FLOAT:
        vol[3 * S:4 * S:2] = -0.0   # zeros of either sign are zeros to the cells
    _load(vr, vol, fmt)
    cells, shift2 = vr.downloadCells()
    assert shift2 == shift and cells.shape[:3] == (6, 2, 2)
    assert (cells[:2] == c).all() and (cells[3:] == 0).all() and (cells[2, ..., 0] < cells[2, ..., 1]).all()
    layer = (2 * S // 8) ** 2      # blocks per layer of blocks
    n_slab, n_zero = 2 * S // 8, 3 * S // 8
    # the median: dilated by one voxel, the slab's last layer and the zeros' first reach the noise
    _, (on, off) = _check(vr, vol, fmt, fr.MEDIAN3, None, None, "median")
    assert on["blocks_skipped"] == (n_slab - 1 + n_zero - 1) * layer and off["blocks_skipped"] == 0
    # the smoothing: only the zeros; with a radius along z the first layer is fetched, with none it is not
    for radius, first in (((1, 1, 2), 1), ((8, 8, 8), 1), ((2, 3, 0), 0)):
        _, (on, off) = _check(vr, vol, fmt, fr.SEPARABLE, radius, _taps_random(radius, 6), "radius %s" % (radius,))
        assert on["blocks_skipped"] == (n_zero - first) * layer and off["blocks_skipped"] == 0, (radius, on)
    # a NaN in the zeros: its cell proves nothing any more
    if fmt == FLOAT:
        vol[5 * S + S // 2, S // 2, S // 2] = np.nan
        _load(vr, vol, fmt)
        _, (on, _) = _check(vr, vol, fmt, fr.MEDIAN3, None, None, "median with a NaN")
        per_cell = (S // 8) ** 3
        assert on["blocks_skipped"] < (n_slab - 1 + n_zero - 1) * layer - per_cell + 1


def _frame(r, W=96, H=64):
    r.setIteration(0)
    return r.runRaycastNoGL(W, H).copy()


def test_invalidation(vr):
    """In place, then a technique-0 frame with ESS and a histogram: what a fresh renderer gives for the same voxels."""
    vol = _random((40, 33, 26), UCHAR, seed=21)
    vol[:, :, 20:] = 0
    _load(vr, vol, UCHAR, tff=True)
    vr.updateView(frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0)))
    vr.setSeed(frontend.MT19937_FIRST_SEEDS[0])
    before = _frame(vr)
    _, hist_before = vr.volume_statistics(bins=(64, 8), window=(0.0, 1.0, 0.5))
    taps = fr.gaussian_taps(1.2, 3)[:4]
    vr.filter_volume("separable", taps=taps)   # (rebuilds the bricks, as a load does)
    after = _frame(vr)
    _, hist_after = vr.volume_statistics(bins=(64, 8), window=(0.0, 1.0, 0.5))
    filtered = vr.downloadVolume(0)
    _assert_equal(filtered, fr.compute(vol, UCHAR, fr.SEPARABLE, (3, 3, 3), [taps] * 3), "in place")
    assert not np.array_equal(before, after) and not np.array_equal(hist_before, hist_after)
    fresh = VolumeRenderCL()
    fresh.initialize()
    try:
        _load(fresh, filtered, UCHAR, tff=True)
        fresh.updateView(frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0)))
        fresh.setSeed(frontend.MT19937_FIRST_SEEDS[0])
        assert np.array_equal(_frame(fresh).view(np.uint32), after.view(np.uint32))
        _, hist_fresh = fresh.volume_statistics(bins=(64, 8), window=(0.0, 1.0, 0.5))
        assert np.array_equal(hist_fresh, hist_after)
        assert np.array_equal(fresh.downloadBricks(0), vr.downloadBricks(0))
    finally:
        fresh.close()


def test_isolation(vr):
    """Three accumulated frames of the current step, a jitter seed each, with a filter into ANOTHER step between the
    second and the third: the uninterrupted sequence, bit for bit."""
    z, y, x = np.meshgrid(np.arange(21), np.arange(30), np.arange(33), indexing="ij")
    d = np.sqrt((x - 16.3) ** 2 + (y - 14.1) ** 2 + (z - 10.6) ** 2)
    v0 = np.round(np.clip(1.0 - d / 12.0, 0.0, 1.0) * 255).astype(np.uint8)
    v1 = _random((33, 30, 21), UCHAR, seed=31)
    _load(vr, [v0, v1], UCHAR, tff=True)
    vr.updateView(frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0)))
    W, H = 96, 64

    def run(interrupt):
        vr.setIteration(0)
        frames = []
        for k in range(3):
            if k == 2 and interrupt:
                vr.filter_volume("median3", dst=1)
            vr.setSeed(500 + k)
            frames.append(vr.runRaycastNoGL(W, H).copy())
        return frames

    plain = run(False)
    mixed = run(True)
    for k in range(3):
        assert np.array_equal(plain[k].view(np.uint32), mixed[k].view(np.uint32)), "frame %d" % k
    assert not np.array_equal(plain[0], plain[2])   # (the sequence does accumulate)
    _assert_equal(vr.downloadVolume(1), fr.compute(v0, UCHAR, fr.MEDIAN3), "the other step")
    _assert_equal(vr.downloadVolume(0), v0, "the current step")


def _python_route(vr, n):
    """shells n^3 UCHAR, Gaussian sigma 1.5 (radius 5), then the median, as the C++ class and the CLI apply them."""
    vr.synthVolume("shells", (n, n, n), UCHAR)
    vr.setObjEss(True)
    out = []
    vr.filter_volume("separable", taps=frontend.gaussian_taps(1.5))
    out.append((vr.volume_statistics(), vr.lastFilterInfo()))
    vr.filter_volume("median3")
    out.append((vr.volume_statistics(), vr.lastFilterInfo()))
    return out


def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_filter")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_filter.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "filter.bin")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    raw = open(out, "rb").read()
    rec = 256 * 8 + 4 * 8 + 2 * 4
    assert len(raw) == 3 * rec
    route = _python_route(vr, 32)
    taps = [np.array([0.5, 0.25], F32), np.ones(1, F32), np.array([0.5, 0.5, -0.25], F32)]
    vr.filter_volume("separable", taps=taps, dst=1)
    vr.setTimestep(1)
    route.append((vr.volume_statistics(), vr.lastFilterInfo()))
    vr.setTimestep(0)
    for k, ((st, hist), fi) in enumerate(route):
        part = raw[k * rec:(k + 1) * rec]
        assert np.array_equal(np.frombuffer(part[:2048], np.uint64), hist[0]), k
        words = np.frombuffer(part[2048:2080], np.uint64)
        flags = np.frombuffer(part[2080:], np.uint32)
        assert list(words) == [fi["blocks"], fi["blocks_fetched"], fi["blocks_skipped"], fi["scratch_bytes"]], k
        assert list(flags) == [fi["empty_skip"], fi["in_place"]] == [1, int(k < 2)], k


def test_cli_filters_before_the_statistics(vr, tmp_path):
    path = str(tmp_path / "stats.json")
    args = [EXE, "--synth", "shells", "32", "UCHAR", "--filter", "gauss", "1.5", "--filter", "median", "--stats", path]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    doc = json.load(open(path))
    (st, hist), _ = _python_route(vr, 32)[1]
    for key in ("voxels", "nan", "below", "above", "gradient_nan", "binned"):
        assert doc[key] == st[key], key
    assert np.array_equal(np.array(doc["hist"], np.uint64), hist)
    # ... and it is the filters that made them: the unfiltered volume counts differently
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    assert not np.array_equal(vr.volume_statistics()[1], hist)
    # explicit taps from a file, before a mesh
    tfile = str(tmp_path / "taps.txt")
    open(tfile, "w").write("# x, y, z\n0.5 0.25\n1\n0.25 0.25 0.125\n")
    mesh = str(tmp_path / "m.stl")
    res = subprocess.run([EXE, "--synth", "sphere", "32", "UCHAR", "--filter", "taps", tfile, "--mesh", "0.5", mesh],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    vr.synthVolume("sphere", (32, 32, 32), UCHAR)
    taps = [np.array([0.5, 0.25], F32), np.ones(1, F32), np.array([0.25, 0.25, 0.125], F32)]
    vr.filter_volume("separable", taps=taps)
    assert json.loads(res.stdout.strip().splitlines()[-1])["triangles"] == len(vr.extract_isosurface(0.5)[0])
