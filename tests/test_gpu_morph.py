"""Volume morphology (vrhip_morph_volume, vr_morph.hip) against its CPU restatement (tests/ref/morph_ref.c, pinned by
tests/test_morph_ref.py): the downloaded destination equals the restatement byte for byte -- every voxel type, shapes
that are no multiple of the block or of a micro-brick, axes shorter than the radius, exactly one block, both halo
classes and a zero-radius axis, both structuring elements, all seven ops, special floats, object-order ESS on and off
(the skipping must not change a byte) --, the info block, the three destinations, the scratch held, the refusals, the
skip counts of both sweeps on a built volume, what goes stale and what does not, the C++ class and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import morph_ref as mr
from volumerenderercl_amd import FLOAT, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, _lib, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")

F32 = np.float32
# (x, y, z), the filters' shapes: no multiple of the block (8) or a micro-brick (4); axes shorter than the radius; a
# multiple of both; exactly one block; more than two blocks per axis
SHAPES = [(37, 21, 13), (5, 70, 9), (64, 40, 24), (8, 8, 8), (17, 18, 19)]
# no halo; one ring of micro-bricks; two rings; a zero-radius axis with one ring; a zero-radius axis with two and one
RADII_ALL_OPS = [(1, 1, 1), (4, 0, 2)]
RADII_SOME_OPS = [(0, 0, 0), (8, 8, 8), (0, 8, 1)]
SOME_OPS = [mr.ERODE, mr.GRADIENT, mr.TOPHAT]
FMTS = [UCHAR, USHORT, FLOAT]
FMT_IDS = ["uchar", "ushort", "float"]
WS = 32   # the counters of two sweeps


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _random(res, fmt, seed=5, special=True):
    """tests/test_gpu_filter.py's volumes: FLOAT carries NaNs with payloads, infinities, zeros of both signs and values
    outside [0, 1]."""
    rng = np.random.default_rng(seed)
    shape = (res[2], res[1], res[0])
    if fmt == UCHAR:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if fmt == USHORT:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    v = (rng.random(shape, dtype=np.float32) * 4.0 - 1.5).astype(F32)
    if special:
        flat = v.reshape(-1)
        idx = rng.choice(flat.size, 14, replace=False)
        flat[idx[:3]] = np.nan
        flat[idx[3]] = np.array([0xffc00123], np.uint32).view(F32)[0]
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


def _morph(vr, op, shape, radius, dst=None):
    return vr.morph_volume(mr.OP_NAMES[op], radius, mr.SHAPE_NAMES[shape], dst=dst)


def _assert_equal(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d voxels differ, first at (z, y, x) %s: %s, restatement %s" % (
        what, bad.sum(), np.argwhere(bad)[0], _bits(got)[bad][0], _bits(want)[bad][0])


def _blocks(res):
    return ((res[0] + 7) // 8) * ((res[1] + 7) // 8) * ((res[2] + 7) // 8)


def _vol_bytes(res, itemsize):
    return ((res[0] + 3) // 4) * ((res[1] + 3) // 4) * ((res[2] + 3) // 4) * 64 * itemsize


def _check_info(mi, res, op, ess, what):
    sweeps = 1 if op in (mr.ERODE, mr.DILATE, mr.GRADIENT) else 2
    assert mi["sweeps"] == sweeps and mi["empty_skip"] == int(ess), (what, mi)
    for s in range(2):
        blocks = _blocks(res) if s < sweeps else 0
        assert mi["blocks"][s] == blocks == mi["blocks_fetched"][s] + mi["blocks_skipped"][s], (what, mi)
        if not ess:
            assert mi["blocks_skipped"][s] == 0, (what, mi)
    return sweeps


def _check(vr, vol, fmt, op, shape, radius, what):
    """Into step 1, ESS on and off: the bytes equal the restatement's; the info block adds up."""
    want = mr.compute(vol, fmt, op, shape, radius)
    res = vol.shape[::-1]
    infos = []
    for ess in (True, False):
        vr.setObjEss(ess)
        _morph(vr, op, shape, radius, dst=1)
        _assert_equal(vr.downloadVolume(1), want, "%s, ESS %s" % (what, ess))
        mi = vr.lastMorphInfo()
        sweeps = _check_info(mi, res, op, ess, what)
        assert mi["in_place"] == 0 and mi["scratch_bytes"] == WS + (sweeps - 1) * _vol_bytes(res, vol.itemsize), (what, mi)
        infos.append(mi)
    vr.setObjEss(True)
    return want, infos


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("res", SHAPES, ids=lambda r: "x".join(map(str, r)))
def test_parity(vr, res, fmt):
    vol = _random(res, fmt, seed=sum(res) + fmt)
    _load(vr, vol, fmt)
    for radii, ops in ((RADII_ALL_OPS, range(7)), (RADII_SOME_OPS, SOME_OPS)):
        for radius in radii:
            for shape in (mr.BOX, mr.BALL):
                for op in ops:
                    _check(vr, vol, fmt, op, shape, radius, "%s %s %s %s radius %s" % (
                        res, FMT_IDS[fmt], mr.OP_NAMES[op], mr.SHAPE_NAMES[shape], radius))
    _assert_equal(vr.downloadVolume(0), vol, "the source")


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_destinations_and_scratch(vr, fmt):
    """Appended, existing and in place give the same bytes; the source changes only in place; the info block says which
    and what was held; a destination above the number of steps is refused and the volumes stay."""
    res = (21, 13, 10)
    v0, v1 = _random(res, fmt, seed=8), _random(res, fmt, seed=9)
    vb = _vol_bytes(res, v0.itemsize)
    radius = (2, 1, 3)
    for op, shape in ((mr.ERODE, mr.BALL), (mr.GRADIENT, mr.BOX), (mr.OPEN, mr.BALL), (mr.CLOSE, mr.BOX), (mr.TOPHAT, mr.BOX),
                      (mr.BLACKHAT, mr.BALL)):
        what = "%s %s" % (mr.OP_NAMES[op], mr.SHAPE_NAMES[shape])
        _load(vr, [v0, v1], fmt)
        want = mr.compute(v0, fmt, op, shape, radius)
        with pytest.raises(ValueError):
            _morph(vr, op, shape, radius, dst=3)
        assert vr.getResolution()[3] == 2
        _assert_equal(vr.downloadVolume(0), v0, "step 0 after a refusal")
        _assert_equal(vr.downloadVolume(1), v1, "step 1 after a refusal")
        assert _morph(vr, op, shape, radius, dst=2) == 2 and vr.getResolution()[3] == 3       # appended
        _assert_equal(vr.downloadVolume(2), want, what + " appended")
        two = _check_info(vr.lastMorphInfo(), res, op, True, what) - 1
        assert vr.lastMorphInfo()["in_place"] == 0 and vr.lastMorphInfo()["scratch_bytes"] == WS + two * vb
        _morph(vr, op, shape, radius, dst=1)                                                   # existing
        _assert_equal(vr.downloadVolume(1), want, what + " existing")
        _assert_equal(vr.downloadVolume(0), v0, "the source")
        assert _morph(vr, op, shape, radius) == 0                                              # in place
        _assert_equal(vr.downloadVolume(0), want, what + " in place")
        mi = vr.lastMorphInfo()
        _check_info(mi, res, op, True, what)
        assert mi["in_place"] == 1, mi
        if two:
            assert WS + vb <= mi["scratch_bytes"] <= WS + 2 * vb and (mi["scratch_bytes"] - WS) % vb == 0, mi
        else:
            assert mi["scratch_bytes"] == WS + vb, mi
        _assert_equal(vr.downloadVolume(2), want, "the appended step afterwards")
        _assert_equal(vr.downloadVolume(1), want, "the existing step afterwards")


def test_sharing_renderers(vr):
    """A renderer that borrows its volumes is refused before anything is touched; the owner works in place under a
    sharer, which sees the new voxels at the address it holds."""
    res = (20, 12, 9)
    vol = _random(res, UCHAR, seed=12)
    for op in (mr.DILATE, mr.OPEN, mr.BLACKHAT):
        _load(vr, vol, UCHAR, tff=True)
        twin = vr.shareVolumes()
        try:
            with pytest.raises(RuntimeError, match="belong to another renderer"):
                twin.morph_volume("erode", 1)
            with pytest.raises(RuntimeError, match="belong to another renderer"):
                twin.morph_volume("open", 1, dst=1)
            _assert_equal(twin.downloadVolume(0), vol, "the sharer's view")
            _assert_equal(vr.downloadVolume(0), vol, "the owner's volume")
            want = mr.compute(vol, UCHAR, op, mr.BALL, (2, 2, 1))
            _morph(vr, op, mr.BALL, (2, 2, 1))
            assert vr.lastMorphInfo()["in_place"] == 1
            _assert_equal(vr.downloadVolume(0), want, "the owner, in place under a sharer")
            _assert_equal(twin.downloadVolume(0), want, "the sharer afterwards")
        finally:
            twin.close()


def test_unsupported_and_nodata():
    r = VolumeRenderCL()
    r.initialize()
    try:
        p = frontend.morph_params("open", 1)
        assert r._lib.vrhip_last_morph_info(r._h, C.byref(_lib.MorphInfo())) == _lib.ERR_NODATA
        assert r._lib.vrhip_morph_volume(r._h, C.byref(p), 0) == _lib.ERR_NODATA
        assert r._lib.vrhip_morph_volume(r._h, None, 0) == _lib.ERR_INVALID
        for channels in (2, 4):   # RG, RGBA
            r.loadVolumeArrays([np.zeros((6, 5, 4, channels), np.uint8)], UCHAR)
            assert r._lib.vrhip_morph_volume(r._h, C.byref(p), 0) == _lib.ERR_UNSUPPORTED
            assert r._lib.vrhip_morph_volume(r._h, C.byref(p), 1) == _lib.ERR_UNSUPPORTED
        assert r._lib.vrhip_last_morph_info(r._h, C.byref(_lib.MorphInfo())) == _lib.ERR_NODATA
        r.loadVolumeArrays([np.zeros((6, 5, 4), np.uint8)], UCHAR)
        for bad in (dict(op=7), dict(shape=2), dict(radius=9), dict(reserved=1)):
            q = frontend.morph_params("open", 1)
            if "radius" in bad:
                q.radius[1] = 9
            elif "reserved" in bad:
                q.reserved[2] = 1
            else:
                setattr(q, *list(bad.items())[0])
            assert r._lib.vrhip_morph_volume(r._h, C.byref(q), 0) == _lib.ERR_INVALID, bad
        assert r._lib.vrhip_morph_volume(r._h, C.byref(p), 2) == _lib.ERR_INVALID   # above the number of steps
        assert r._lib.vrhip_last_morph_info(r._h, C.byref(_lib.MorphInfo())) == _lib.ERR_NODATA
        assert not r.downloadVolume(0).any()
    finally:
        r.close()


@pytest.mark.parametrize("fmt", [UCHAR, FLOAT], ids=["uchar", "float"])
def test_ess_skips(vr, fmt):
    """The filters' skip scene, a transfer function set and the bricks built: cells along z, two of a constant non-zero
    slab, one of noise, three of zeros (FLOAT: zeros of both signs), the boundaries off the block grid.  ESS on and
    off give the same bytes; off skips nothing; on, both sweeps skip blocks of both constants, the second fewer than
    the first (it asks for twice the margin); a NaN's cell proves nothing."""
    _load(vr, np.zeros((64, 64, 64), mr.NP_DTYPE[fmt]), fmt, tff=True)
    _, shift = vr.downloadCells()
    S = 1 << shift
    assert shift >= 3
    rng = np.random.default_rng(2)
    vol = np.zeros((6 * S, 2 * S, 2 * S), mr.NP_DTYPE[fmt])
    c = 77 if fmt == UCHAR else F32(0.3)
    vol[:2 * S + 2] = c            # (a cell answers for its voxels and a rim of up to two)
    noise = vol[2 * S + 2:3 * S - 2]
    noise[...] = rng.integers(1, 256, noise.shape) if fmt == UCHAR else rng.random(noise.shape, dtype=F32) + F32(0.5)
    if fmt == FLOAT:
        vol[3 * S:4 * S:2] = -0.0   # zeros of either sign are zeros to the cells
    _load(vr, vol, fmt, tff=True)
    cells, shift2 = vr.downloadCells()
    assert shift2 == shift and cells.shape[:3] == (6, 2, 2)
    assert (cells[:2] == c).all() and (cells[3:] == 0).all() and (cells[2, ..., 0] < cells[2, ..., 1]).all()
    layer = (2 * S // 8) ** 2      # blocks per layer of blocks
    n_slab, n_zero = 2 * S // 8, 3 * S // 8
    for op, shape, radius in ((mr.ERODE, mr.BALL, (1, 1, 2)), (mr.GRADIENT, mr.BOX, (2, 3, 0)), (mr.OPEN, mr.BOX, (1, 1, 2)),
                              (mr.CLOSE, mr.BALL, (2, 0, 1)), (mr.TOPHAT, mr.BALL, (1, 1, 2)), (mr.BLACKHAT, mr.BOX, (3, 3, 3))):
        what = "%s %s radius %s" % (mr.OP_NAMES[op], mr.SHAPE_NAMES[shape], radius)
        want, (on, off) = _check(vr, vol, fmt, op, shape, radius, what)
        # a layer of blocks next to the noisy cell is fetched when the dilated block reaches it: 8 voxels cover a
        # margin of 1 .. 8, and a margin of 0 reaches nothing
        for s in range(on["sweeps"]):
            first = 1 if (s + 1) * radius[2] else 0
            assert on["blocks_skipped"][s] == (n_slab - first + n_zero - first) * layer, (what, s, on)
        assert off["blocks_skipped"] == [0, 0]
        if op in (mr.GRADIENT, mr.TOPHAT, mr.BLACKHAT):   # the constants' differences are zeros
            assert not _bits(want[:2 * S - 8]).any() and not _bits(want[3 * S + 8:]).any()
    if fmt == FLOAT:   # a NaN in the zeros: its cell proves nothing any more
        vol[5 * S + S // 2, S // 2, S // 2] = np.nan
        _load(vr, vol, fmt, tff=True)
        _, (on, _) = _check(vr, vol, fmt, mr.OPEN, mr.BALL, (1, 1, 1), "open with a NaN")
        per_cell = (S // 8) ** 3
        for s in range(2):
            assert 0 < on["blocks_skipped"][s] < (n_slab - 1 + n_zero - 1) * layer - per_cell + 1


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
    vr.morph_volume("close", (2, 2, 1))   # (rebuilds the bricks, as a load does)
    after = _frame(vr)
    _, hist_after = vr.volume_statistics(bins=(64, 8), window=(0.0, 1.0, 0.5))
    closed = vr.downloadVolume(0)
    _assert_equal(closed, mr.compute(vol, UCHAR, mr.CLOSE, mr.BALL, (2, 2, 1)), "in place")
    assert not np.array_equal(before, after) and not np.array_equal(hist_before, hist_after)
    fresh = VolumeRenderCL()
    fresh.initialize()
    try:
        _load(fresh, closed, UCHAR, tff=True)
        fresh.updateView(frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0)))
        fresh.setSeed(frontend.MT19937_FIRST_SEEDS[0])
        assert np.array_equal(_frame(fresh).view(np.uint32), after.view(np.uint32))
        _, hist_fresh = fresh.volume_statistics(bins=(64, 8), window=(0.0, 1.0, 0.5))
        assert np.array_equal(hist_fresh, hist_after)
        assert np.array_equal(fresh.downloadBricks(0), vr.downloadBricks(0))
    finally:
        fresh.close()


def test_isolation(vr):
    """Three accumulated frames of the current step, a jitter seed each, with a two-sweep op into ANOTHER step between
    the second and the third: the uninterrupted sequence, bit for bit."""
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
                vr.morph_volume("tophat", 2, "ball", dst=1)
            vr.setSeed(500 + k)
            frames.append(vr.runRaycastNoGL(W, H).copy())
        return frames

    plain = run(False)
    mixed = run(True)
    for k in range(3):
        assert np.array_equal(plain[k].view(np.uint32), mixed[k].view(np.uint32)), "frame %d" % k
    assert not np.array_equal(plain[0], plain[2])   # (the sequence does accumulate)
    _assert_equal(vr.downloadVolume(1), mr.compute(v0, UCHAR, mr.TOPHAT, mr.BALL, (2, 2, 2)), "the other step")
    _assert_equal(vr.downloadVolume(0), v0, "the current step")


def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_morph")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_morph.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out = str(tmp_path / "morph.bin")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    raw = open(out, "rb").read()
    rec = 256 * 8 + 7 * 8 + 3 * 4
    assert len(raw) == 3 * rec
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    vr.setObjEss(True)
    route = []
    vr.morph_volume("open", 2)
    route.append((vr.volume_statistics(), vr.lastMorphInfo()))
    vr.morph_volume("close", 1, "box")
    route.append((vr.volume_statistics(), vr.lastMorphInfo()))
    vr.morph_volume("gradient", (3, 0, 1), "ball", dst=1)
    vr.setTimestep(1)
    route.append((vr.volume_statistics(), vr.lastMorphInfo()))
    vr.setTimestep(0)
    for k, ((st, hist), mi) in enumerate(route):
        part = raw[k * rec:(k + 1) * rec]
        assert np.array_equal(np.frombuffer(part[:2048], np.uint64), hist[0]), k
        words = np.frombuffer(part[2048:2104], np.uint64)
        flags = np.frombuffer(part[2104:], np.uint32)
        assert list(words) == [mi["blocks"][0], mi["blocks_fetched"][0], mi["blocks_skipped"][0], mi["blocks"][1],
                               mi["blocks_fetched"][1], mi["blocks_skipped"][1], mi["scratch_bytes"]], k
        assert list(flags) == [mi["sweeps"], mi["empty_skip"], mi["in_place"]] == [2 if k < 2 else 1, 1, int(k < 2)], k


def test_cli_morph_after_filter(vr, tmp_path):
    """--morph after --filter: the statistics of the two Python calls in that order -- and not of the other order."""
    path = str(tmp_path / "stats.json")
    args = [EXE, "--synth", "shells", "32", "UCHAR", "--filter", "median", "--morph", "tophat", "ball", "2", "1", "2", "--stats", path]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    doc = json.load(open(path))
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    vr.setObjEss(True)
    vr.filter_volume("median3")
    vr.morph_volume("tophat", (2, 1, 2), "ball")
    st, hist = vr.volume_statistics()
    for key in ("voxels", "nan", "below", "above", "gradient_nan", "binned"):
        assert doc[key] == st[key], key
    assert np.array_equal(np.array(doc["hist"], np.uint64), hist)
    vr.synthVolume("shells", (32, 32, 32), UCHAR)
    vr.morph_volume("tophat", (2, 1, 2), "ball")
    vr.filter_volume("median3")
    assert not np.array_equal(vr.volume_statistics()[1], hist)
