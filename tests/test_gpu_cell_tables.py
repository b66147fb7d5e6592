"""The tables vr_cells.hip derives from the cell grids and the transfer function -- per-cell opacity bound, empty bit,
macro-cell bound, the seven levels of leap radii -- downloaded (vrhip_download_cell_tables) and checked against the
plain reference of tests/cell_tables_ref.py: sound (never below what a sample can read), tight (never above the
widest window a correct kernel can read), exact where they are exact; at transfer functions of 1 .. 4096 entries,
on volumes whose extrema sit on the entries' edges, and on a volume long enough for every leap radius.  Then frames
at the same table sizes against the oracle.  tests/test_cell_tables_ref.py proves the assertions without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import cell_tables_ref as ctr
from tests import common, scenes, test_gpu_mip
from tests.test_gpu_parity import SEED, _compare, _setup
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu

FMT_IDS = {UCHAR: "uchar", USHORT: "ushort", FLOAT: "float"}
VIEWS = common.views()


def _renderer(env=()):
    """A renderer created under the environment switches `env` (they are read when it is created)."""
    with pytest.MonkeyPatch.context() as mp:
        for k in env:
            mp.setenv(k, "1" if k != "VRHIP_CELL_SHIFT" else "3")
        r = VolumeRenderCL()
        r.initialize()
    return r


@pytest.fixture(scope="module")
def vr():
    r = _renderer()
    yield r
    r.close()


@pytest.fixture(scope="module")
def vr_skip():
    r = _renderer(["VRHIP_EMPTY_SKIP"])
    yield r
    r.close()


@pytest.fixture(scope="module")
def vr_noskip():
    r = _renderer(["VRHIP_EMPTY_SKIP", "VRHIP_NO_EMPTY_SKIP"])
    yield r
    r.close()


@pytest.fixture(scope="module")
def vr_nocull():
    r = _renderer(["VRHIP_PT_NO_CULL"])
    yield r
    r.close()


@pytest.fixture(scope="module")
def vr_noleap():
    r = _renderer(["VRHIP_PT_NO_LEAP"])
    yield r
    r.close()


@pytest.fixture(params=[2, 3], ids=["cells4", "one_grid"])
def shifted(request, vr, monkeypatch):
    """The module's renderer with the default cell shifts, or with VRHIP_CELL_SHIFT=3: one grid for bounds and bits
    (the shifts are read whenever the tables are built)."""
    if request.param == 3:
        monkeypatch.setenv("VRHIP_CELL_SHIFT", "3")
    return vr, request.param


def _check_tables(r, fmt, tff, eshift, what):
    """Every assertion on the tables of the volume and transfer function loaded into r."""
    coarse, shift = r.downloadCells()
    fine, es = r.downloadCells(fine=True)
    t = r.downloadCellTables()
    assert (shift, es, t["shift"], t["eshift"]) == (3, eshift, 3, eshift)
    assert t["bound"].shape == coarse.shape[:3] and t["fine_dims"] == fine.shape[:3]
    assert t["macro"].shape == tuple(-(-s // 4) for s in coarse.shape[:3]) and t["leap"].shape[1:] == t["macro"].shape
    if eshift == 3:
        np.testing.assert_array_equal(fine, coarse)
    finite, A, E = ctr.check_bounds(t["bound"], coarse, fmt, tff, what)
    bits, ffinite, fA, fE = ctr.check_empty(t["empty"], fine, fmt, tff, what)
    ctr.check_macro_and_leaps(t["bound"], t["macro"], t["leap"], what)
    return t, (finite, A, E), (bits, ffinite, fA, fE)


# ---- the tables

@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=FMT_IDS.values())
def test_tables_at_every_transfer_function_size(shifted, fmt):
    r, eshift = shifted
    vol = common.noise_volume(ctr.NOISE_RES, fmt, seed=40 + fmt, smooth=False)
    r.loadVolumeArrays([vol], fmt)
    tight = 0
    for n in ctr.TF_SIZES:
        tff = ctr.sized_tff(n)
        r.setTransferFunction(tff)
        t, (finite, A, E), (bits, _, _, fE) = _check_tables(r, fmt, tff, eshift, "n %d" % n)
        assert finite.all()
        tight += int((E == 0).sum()) + int(bits.sum())
    assert tight > 0      # cells that read nothing exist: the empty bits and the zero bounds were put to the test


@pytest.mark.parametrize("fmt,n,seed,table", ctr.KNIFE_CASES,
                         ids=["%s-%d-%s" % (FMT_IDS[c[0]], c[1], c[3]) for c in ctr.KNIFE_CASES])
def test_tables_with_extrema_on_the_entries_edges(shifted, fmt, n, seed, table):
    r, eshift = shifted
    vol, tff = ctr.knife_case(fmt, n, seed, table)
    r.loadVolumeArrays([vol], fmt)
    r.setTransferFunction(tff)
    _, (finite, A, E), (bits, _, fA, fE) = _check_tables(r, fmt, tff, eshift, "%s n %d" % (table, n))
    assert ((A > 0) & (A < E)).any()
    if table == "comb":
        assert (E == 0).mean() >= 0.05 and (fE == 0).mean() >= 0.05
        assert bits.mean() >= 0.05


@pytest.mark.parametrize("palette", scenes.FLOAT_PALETTES)
def test_tables_of_float_volumes_outside_the_unit_range(shifted, palette):
    """Values outside [0, 1] read TF[0] or TF[n-1]; a cell that can sample NaN, +-inf or a value beyond FLT_MAX / 2 has
    bound 2 and no empty bit, whatever the transfer function."""
    r, eshift = shifted
    vol = scenes.float_volume(palette, (40, 33, 30), seed=17)
    r.loadVolumeArrays([vol], FLOAT)
    for n, first in ((1024, False), (257, True), (3, False), (4096, True)):
        tff = ctr.edge_tff(n, only_first=first)
        r.setTransferFunction(tff)
        t, (finite, _, _), (bits, ffinite, _, _) = _check_tables(r, FLOAT, tff, eshift, "%s n %d" % (palette, n))
        assert finite.all() == (palette != "specials")
        if palette == "specials":
            assert (~finite).sum() > 10 and (t["bound"].ravel()[~finite] == 2).all() and not bits[~ffinite].any()
            assert not t["leap"][:, t["macro"] == 2].any()


@pytest.mark.parametrize("axis", ["x", "y"])
def test_leap_radii_on_a_long_volume(vr, axis):
    """33 macro cells along one axis: every erosion pass decides something, and the saturated radius occurs."""
    vol, tff = ctr.blob_volume(axis), ctr.blob_tff()
    vr.loadVolumeArrays([vol], UCHAR)
    vr.setTransferFunction(tff)
    coarse, _ = vr.downloadCells()
    t = vr.downloadCellTables()
    assert sorted(t["macro"].shape) == [2, 3, 33]
    ctr.check_bounds(t["bound"], coarse, UCHAR, tff, axis)
    want = ctr.check_macro_and_leaps(t["bound"], t["macro"], t["leap"], axis)
    assert set(np.unique(want)) >= {0, 1, 2, 7, 14, 15, 16}
    assert len({want[j].tobytes() for j in range(7)}) >= 3
    bits, _ = ctr.unpack_bits(t["empty"], int(np.prod(t["fine_dims"])))
    assert bits.mean() > 0.9


@pytest.mark.parametrize("res,count", ctr.WORD_CASES, ids=[str(c[1] % 64) for c in ctr.WORD_CASES])
def test_empty_words_end_with_the_last_cell(vr, res, count):
    """Fine-grid cell counts of 0, 1, 31, 32, 33 and 63 mod 64 (a wave ballots 64 cells into two words)."""
    vol = np.zeros(res[::-1], np.uint8)
    vol[res[2] // 2, res[1] // 2, res[0] // 3] = 200
    tff = ctr.sized_tff(1000)
    vr.loadVolumeArrays([vol], UCHAR)
    vr.setTransferFunction(tff)
    fine, _ = vr.downloadCells(fine=True)
    t = vr.downloadCellTables()
    assert int(np.prod(t["fine_dims"])) == count and t["empty"].size == (count + 31) // 32
    bits, _, _, _ = ctr.check_empty(t["empty"], fine, UCHAR, tff, str(res))
    assert bits[-1] and 0 < (~bits).sum() <= 27


def test_download_is_refused_without_its_inputs():
    r = VolumeRenderCL()
    r.initialize()
    try:
        fn = r._lib.vrhip_download_cell_tables
        dims = (C.c_uint32 * 9)()
        assert fn(r._h, None, 0, None, 0, None, 0, None, 0, dims, None) == 3      # VRHIP_ERR_NODATA: no volume
        r.loadVolumeArrays([np.zeros((16, 16, 16), np.uint8)], UCHAR)
        assert fn(r._h, None, 0, None, 0, None, 0, None, 0, dims, None) == 3      # ... no transfer function
        r.setTransferFunction(ctr.sized_tff(3))
        assert fn(r._h, None, 0, None, 0, None, 0, None, 0, dims, None) == 0
        assert list(dims) == [2, 2, 2, 1, 1, 1, 4, 4, 4]
        buf = np.zeros(64, np.float32)
        assert fn(r._h, buf.ctypes.data_as(C.c_void_p), 7, None, 0, None, 0, None, 0, None, None) == 1   # VRHIP_ERR_INVALID: size mismatch
        assert fn(r._h, buf.ctypes.data_as(C.c_void_p), 8, None, 0, None, 0, None, 0, None, None) == 0
    finally:
        r.close()


# ---- frames at the same table sizes

FRAME_SIZES = (1, 2, 3, 255, 257, 1000, 4095)
FRAME_RES = {UCHAR: (56, 44, 40), USHORT: (41, 60, 47), FLOAT: (50, 38, 61)}


def _holes(fmt, res, seed):
    vol = common.noise_volume(res, fmt, seed=seed, smooth=False)
    vol[vol < vol.max() * 0.3] = 0       # exactly empty regions next to structure
    return vol


@pytest.mark.parametrize("n", FRAME_SIZES)
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=FMT_IDS.values())
def test_raycast_frames_at_every_transfer_function_size(vr_skip, fmt, n):
    """Empty-run skipping forced on, ESS on: instrumented and production kernels against the oracle, image and counters."""
    vol = _holes(fmt, FRAME_RES[fmt], 50 + fmt)
    tff = ctr.sized_tff(n)
    for illum in (0, 1):
        _setup(vr_skip, vol, fmt, tff, VIEWS["rot30"], illum=illum)
        _, _, st = _compare(vr_skip, vol, fmt, tff, 96 if illum else 93, 80)
        assert st["rays_hit"] > 0


@pytest.mark.parametrize("what", ["prefix_longer", "prefix_shorter", "nearest", "gradient_tff"])
def test_raycast_frames_rarer_reads_of_the_table(vr_skip, what):
    fmt = USHORT
    vol = _holes(fmt, FRAME_RES[fmt], 61)
    n = {"prefix_longer": 256, "prefix_shorter": 1024}.get(what, 257)
    tff = ctr.sized_tff(n)
    kw = {"nearest": {"linear": False}, "gradient_tff": {"illum": 2}}.get(what, {})
    _setup(vr_skip, vol, fmt, tff, VIEWS["close"], **kw)
    prefix = None
    if what.startswith("prefix"):
        m = 1024 if what == "prefix_longer" else 256
        alpha = np.repeat(tff[:, 3], m // n) if m > n else tff[:: n // m, 3]
        prefix = np.cumsum(alpha.astype(np.uint64)).astype(np.uint32)
        assert prefix.size == m
        vr_skip.setTffPrefixSum(prefix)
    W, H = 95, 80
    vr_skip.setStatsEnabled(True)
    got = vr_skip.runRaycastNoGL(W, H)
    gstats = vr_skip.getStats()
    vr_skip.setIteration(0)
    ref, rstats, _ = common.oracle_frame(vr_skip, vol, fmt, tff, W, H, prefix=prefix)
    np.testing.assert_array_equal(got, ref)
    assert gstats == rstats and gstats["rays_hit"] > 0
    vr_skip.setStatsEnabled(False)
    prod = vr_skip.runRaycastNoGL(W, H)
    vr_skip.setIteration(0)
    np.testing.assert_array_equal(prod, ref)


@pytest.mark.parametrize("fmt,n,seed,table", ctr.KNIFE_CASES,
                         ids=["%s-%d-%s" % (FMT_IDS[c[0]], c[1], c[3]) for c in ctr.KNIFE_CASES])
def test_empty_skipping_is_exact_on_the_entries_edges(vr_skip, vr_noskip, fmt, n, seed, table):
    """With and without empty runs: the same image and counters, equal to the oracle without ESS."""
    vol, tff = ctr.knife_case(fmt, n, seed, table)
    W, H = 96, 79
    outs = []
    for r in (vr_skip, vr_noskip):
        _setup(r, vol, fmt, tff, VIEWS["rot30"], ess=False)
        r.setStatsEnabled(True)
        outs.append((r.runRaycastNoGL(W, H).copy(), r.getStats()))
        r.setStatsEnabled(False)
        r.setIteration(0)
        outs.append((r.runRaycastNoGL(W, H).copy(), None))
        r.setIteration(0)
    ref, rstats, _ = common.oracle_frame(vr_skip, vol, fmt, tff, W, H, use_ess=False)
    for img, st in outs:
        np.testing.assert_array_equal(img, ref)
        assert st is None or st == rstats
    assert rstats["rays_hit"] > 0


def _accumulate(r, vol, fmt, tff, W, H, iterations=3, stats=False):
    mt = frontend.Mt19937()
    frames, st = [], []
    r.setStatsEnabled(stats)
    for it in range(iterations):
        r.setSeed(mt())
        r.setIteration(it)
        frames.append(r.runRaycastNoGL(W, H).copy())
        st.append(r.getStats() if stats else None)
    r.setStatsEnabled(False)
    return frames, st


def _pathtrace_all_ways(vr, vr_nocull, vr_noleap, vol, fmt, tff, W, H):
    """Three accumulated samples: the oracle's, and the same with culling off and with leaps off.  Returns the stats
    of the default renderer's iterations."""
    _setup(vr, vol, fmt, tff, VIEWS["rot30"], technique=1, ext=60.0)
    mt = frontend.Mt19937()
    ref, refs = None, []
    for it in range(3):
        vr.setSeed(mt())
        vr.setIteration(it)
        ref, _, _ = common.oracle_frame(vr, vol, fmt, tff, W, H, in_accum=ref)
        refs.append(ref)
    stats = None
    try:
        for r in (vr, vr_nocull, vr_noleap):
            _setup(r, vol, fmt, tff, VIEWS["rot30"], technique=1, ext=60.0)
            frames, st = _accumulate(r, vol, fmt, tff, W, H, stats=r is vr)
            for a, b in zip(frames, refs):
                np.testing.assert_array_equal(a, b)
            if r is vr:
                stats = st
                plain, _ = _accumulate(r, vol, fmt, tff, W, H)      # the production kernels
                for a, b in zip(plain, refs):
                    np.testing.assert_array_equal(a, b)
    finally:
        for r in (vr, vr_nocull, vr_noleap):
            r.setTechnique(0)
            r.setIteration(0)
            r.setSeed(SEED)
    return stats


@pytest.mark.parametrize("n", [3, 257, 1000, 4095])
def test_pathtrace_frames_at_every_transfer_function_size(vr, vr_nocull, vr_noleap, n):
    fmt = [FLOAT, UCHAR, USHORT, FLOAT][[3, 257, 1000, 4095].index(n)]
    vol = _holes(fmt, FRAME_RES[fmt], 70)
    stats = _pathtrace_all_ways(vr, vr_nocull, vr_noleap, vol, fmt, ctr.sized_tff(n), 96, 77)
    assert stats[0]["rays_hit"] > 0 and stats[0]["bricks_skipped"] > 0


def test_pathtrace_leaps_over_several_macro_cells(vr, vr_nocull, vr_noleap):
    """352 x 40 x 36 voxels, 11 macro cells along x, empty between a few blobs: walks leap, and change nothing."""
    zz, yy, xx = np.meshgrid(np.arange(36), np.arange(40), np.arange(352), indexing="ij")
    vol = np.zeros((36, 40, 352), np.float32)
    for cx, cy, cz, rad in ((20, 20, 18, 9.0), (335, 28, 14, 8.0)):
        d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2)
        vol = np.maximum(vol, np.clip(1.0 - d / rad, 0, 1).astype(np.float32))
    tff = ctr.sized_tff(1000)
    vr.loadVolumeArrays([vol], FLOAT)
    vr.setTransferFunction(tff)
    leap = vr.downloadCellTables()["leap"]
    assert leap.shape[1:] == (2, 2, 11) and leap.max() >= 4      # free cubes of radius 3 and more exist
    stats = _pathtrace_all_ways(vr, vr_nocull, vr_noleap, vol, FLOAT, tff, 160, 48)
    assert stats[0]["samples_nominal"] > 0, stats[0]            # steps taken in leaps


@pytest.mark.parametrize("n", [1, 3, 1000, 4095])
def test_mip_frames_at_every_transfer_function_size(vr, n):
    fmt = [UCHAR, USHORT, FLOAT, UCHAR][[1, 3, 1000, 4095].index(n)]
    vol = common.noise_volume(FRAME_RES[fmt], fmt, seed=80, smooth=False)
    tff = ctr.sized_tff(n)
    try:
        test_gpu_mip._load(vr, vol, fmt, tff)
        test_gpu_mip._both_ess(vr, vol, fmt, tff, 96, 79, "n %d" % n)
    finally:
        vr.setTechnique(0)
        vr.setObjEss(True)
        vr.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
