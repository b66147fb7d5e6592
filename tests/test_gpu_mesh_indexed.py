"""Indexed isosurface extraction (vrhip_isosurface_count_indexed / _extract_indexed, vr_mesh.hip) against its CPU
restatement (tests/ref/mesh_indexed_ref.c, pinned by tests/test_mesh_indexed_ref.py): counts, vertices, normals and
indices equal the restatement's raw bytes with object-order ESS on and off -- every voxel type, one and two point
blocks per cube block, vertices owned by every kind of neighbouring block, thin volumes, regions, a second time step,
grid values equal to isoValue, non-finite values, capacities and guard words, device destinations, determinism, the
renderer's state around a call, every refusal of the contract, the C++ class and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import common, mesh_ref
from tests import mesh_indexed_ref as ref
from volumerenderercl_amd import FLOAT, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, _lib, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")
BALL_REGION = ((3, 5, 2), (29, 30, 31))


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _load(vr, vols, fmt):
    vr.loadVolumeArrays(vols if isinstance(vols, list) else [vols], fmt)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if want is None:
        return
    assert got.shape == want.shape and got.dtype == want.dtype and got.dtype.itemsize == 4, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d words differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _blocks(res, region=None):
    lo = region[0] if region else (0, 0, 0)
    hi = [min(h, r - 1) for h, r in zip(region[1] if region else res, res)]
    n = 1
    for a, b in zip(lo, hi):
        n *= ((b - 1) // 8 - a // 8 + 1) if b > a else 0
    return n


def _check(vr, vol, fmt, iso, what, normals=False, region=None):
    """ESS on and off: the counts, vertices, normals and indices equal the restatement's bytes, and so each other."""
    want = ref.extract(vol, fmt, iso, normals=normals, region=region)
    m, n = want[0].shape[0], want[2].shape[0]
    infos = []
    for ess in (True, False):
        vr.setObjEss(ess)
        assert vr.isosurface_count_indexed(iso, region) == (m, n), (what, ess)
        vtx, nrm, idx = vr.extract_isosurface_indexed(iso, normals, region)
        _same(vtx, want[0], "%s, vertices, ESS %s" % (what, ess))
        _same(nrm, want[1], "%s, normals, ESS %s" % (what, ess))
        _same(idx, want[2], "%s, indices, ESS %s" % (what, ess))
        mi = vr.lastIndexedMeshInfo()
        assert (mi["vertices"], mi["triangles"]) == (m, n), (what, mi)
        assert mi["point_blocks"] == want[3] and mi["blocks"] == _blocks(vol.shape[::-1], region), (what, mi, want[3])
        assert mi["empty_skip"] == (int(ess) if mi["blocks"] else 0)
        assert mi["point_blocks_skipped"] <= mi["point_blocks"] and mi["blocks_skipped"] <= mi["blocks"]
        assert (mi["scratch_bytes"] > 0) == (mi["blocks"] > 0)
        if not ess:
            assert mi["point_blocks_skipped"] == 0 and mi["blocks_skipped"] == 0
        infos.append(mi)
    vr.setObjEss(True)
    return want, infos


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_voxel_types_on_partial_blocks(vr, fmt, normals):
    vol = ref.noise((17, 10, 9), fmt)
    _load(vr, vol, fmt)
    (vtx, _, idx, _), _ = _check(vr, vol, fmt, 0.5, "17x10x9 %d" % fmt, normals=normals)
    assert idx.shape[0] > 200 and vtx.shape[0] > 100
    _same(vtx[idx], mesh_ref.extract(vol, fmt, 0.5)[0], "vertices[indices] against the soup")


@pytest.mark.parametrize("res", [(9, 9, 9), (8, 8, 8), (16, 16, 16), (17, 17, 17), (33, 2, 5), (5, 1, 5)],
                         ids=lambda r: "x".join(map(str, r)))
def test_small_volumes(vr, res):
    """9^3: two point blocks per axis over one cube block; 8^3: one and one; 16^3 and 17^3: vertices owned by the +x,
    +y, +z, edge and corner neighbours of a cube block; one cube thick; an axis of length 1: nothing, VRHIP_OK."""
    vol = ref.noise(res, UCHAR, seed=9)
    _load(vr, vol, UCHAR)
    (vtx, _, idx, blocks), infos = _check(vr, vol, UCHAR, 0.5, str(res), normals=True)
    if 1 in res:
        assert vtx.shape[0] == 0 and idx.shape[0] == 0 and blocks == 0 and infos[0]["blocks"] == 0
    else:
        assert vtx.shape[0] > 0 and idx.shape[0] > 0
    if res == (9, 9, 9):
        assert blocks == 7 and infos[0]["blocks"] == 1
    if res in ((16, 16, 16), (17, 17, 17)):
        # every one of the seven neighbouring point blocks of block (0, 0, 0) owns vertices (its cubes name them)
        g = (vtx.astype(np.float64) + 1.0) * 0.5 * res[0] - 0.5
        owner = np.minimum(np.floor(g + 1e-4).astype(np.int64) // 8, 1)   # (of P; a vertex at t = 0 lies on P itself)
        for nb in range(1, 8):
            assert ((owner[:, 0] == (nb & 1)) & (owner[:, 1] == ((nb >> 1) & 1)) & (owner[:, 2] == (nb >> 2))).any(), nb


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
def test_ball_and_skipping(vr, normals):
    vol = ref.ball()
    _load(vr, vol, UCHAR)
    (vtx, _, idx, _), (on, off) = _check(vr, vol, UCHAR, 0.2, "ball", normals=normals)
    assert idx.shape[0] > 5000 and vtx.shape[0] > 2500
    assert on["point_blocks"] == off["point_blocks"] == 125 and on["point_blocks_skipped"] > 0 and off["point_blocks_skipped"] == 0
    assert on["blocks_skipped"] > 8 and on["scratch_bytes"] > 0 and off["scratch_bytes"] == on["scratch_bytes"]


def test_regions(vr):
    vol = ref.ball()
    _load(vr, vol, UCHAR)
    lo, hi = BALL_REGION
    (part, _, pidx, _), _ = _check(vr, vol, UCHAR, 0.2, "region", normals=True, region=BALL_REGION)
    whole = ref.extract(vol, UCHAR, 0.2)[0]
    assert 0 < part.shape[0] < whole.shape[0]
    # the region's vertices are vertices of the whole surface; those on its faces are there, none lies beyond them
    have = {v.tobytes() for v in whole}
    assert all(v.tobytes() in have for v in part)
    g = (part.astype(np.float64) + 1.0) * 0.5 * 40.0 - 0.5
    for ax in range(3):
        assert g[:, ax].min() > lo[ax] - 1e-4 and g[:, ax].max() < hi[ax] + 1e-4
    assert (np.abs(g[:, 0] - hi[0]) < 1e-4).any()   # (the ball, radius 10.4 about x = 19.3, passes through x = 29 only)
    gw = (whole.astype(np.float64) + 1.0) * 0.5 * 40.0 - 0.5
    assert (gw[:, 0] > hi[0] + 0.5).any()   # (interior vertices of the whole surface beyond the region: absent above)
    for region, some in ((((29, 20, 19), (30, 21, 20)), True), (((20, 20, 20), (40, 40, 40)), True),
                         (((8, 8, 8), (16, 24, 32)), True), (((4, 4, 4), (20, 4, 20)), False),
                         (((39, 0, 0), (40, 40, 40)), False)):
        (vtx, _, idx, _), infos = _check(vr, vol, UCHAR, 0.2, str(region), region=region)
        assert (vtx.shape[0] > 0) == some and (idx.shape[0] > 0) == some, region
        if not some:
            assert infos[0]["blocks"] == 0 and infos[0]["point_blocks"] == 0


def test_second_time_step(vr):
    a, b = ref.ball(), ref.ball(centre=(17.2, 22.4, 18.9), radius=11.0)
    _load(vr, [a, b], UCHAR)
    try:
        (first, _, _, _), _ = _check(vr, a, UCHAR, 0.2, "step 0")
        vr.setTimestep(1)
        (second, _, _, _), _ = _check(vr, b, UCHAR, 0.2, "step 1", normals=True)
        vr.setTimestep(0)
        (again, _, _, _), _ = _check(vr, a, UCHAR, 0.2, "step 0 again")
        assert first.shape != second.shape and again.tobytes() == first.tobytes()
    finally:
        vr.setTimestep(0)


def test_values_equal_to_iso_keep_their_duplicates(vr):
    vol = ref.exact_iso_volume()
    _load(vr, vol, FLOAT)
    (vtx, _, idx, _), _ = _check(vr, vol, FLOAT, 0.5, "exact isoValue", normals=True)
    pos = mesh_ref.extract(vol, FLOAT, 0.5)[0]
    assert vtx.shape[0] > frontend.weld_mesh(pos)[0].shape[0]
    assert vtx.shape[0] == ref.crossed_edges(vol, FLOAT, 0.5)
    _same(vtx[idx], pos, "vertices[indices] against the soup")


def test_non_finite_values(vr):
    vol = ref.noise((17, 10, 9), FLOAT, seed=21)
    flat = vol.reshape(-1)
    flat[7::97] = np.nan
    flat[11::89] = np.inf
    flat[13::83] = -np.inf
    _load(vr, vol, FLOAT)
    (vtx, nrm, _, _), _ = _check(vr, vol, FLOAT, 0.5, "non-finite", normals=True)
    assert vtx.shape[0] > 100 and np.isfinite(vtx).all() and np.isfinite(nrm).all()


GUARD_F, GUARD_I, PAD = -7.25, 0xDEADBEEF, 64


def _guarded(n_words, value, dtype):
    import torch
    return torch.full((PAD + n_words + PAD,), value, dtype=dtype, device="cuda")


def test_capacities_guards_and_device_destinations(vr):
    import torch
    vol = ref.ball()
    _load(vr, vol, UCHAR)
    want = ref.extract(vol, UCHAR, 0.2, normals=True)
    m, n = want[0].shape[0], want[2].shape[0]
    rs = torch.cuda.ExternalStream(vr.get_stream())
    p = vr._mesh_params(0.2, True, None)
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    vtx, nrm = _guarded(3 * m, GUARD_F, torch.float32), _guarded(3 * m, GUARD_F, torch.float32)
    idx = _guarded(3 * n, GUARD_I - (1 << 32), torch.int32)
    ptrs = [t.data_ptr() + 4 * PAD for t in (vtx, nrm, idx)]
    assert all(a % 16 == 0 for a in ptrs)
    torch.cuda.synchronize()

    def call(cap_v, cap_t, index_ptr=ptrs[2]):
        rc = vr._lib.vrhip_isosurface_extract_indexed(vr._h, C.byref(p), C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]),
                                                      C.c_void_p(index_ptr), cap_v, cap_t, C.byref(nv), C.byref(nt), 1)
        rs.synchronize()
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((vtx == GUARD_F).all()) and bool((nrm == GUARD_F).all()) and bool((idx == GUARD_I - (1 << 32)).all())

    # one short in vertices, one short in triangles: refused, both numbers reported, nothing written anywhere
    for cap_v, cap_t in ((m - 1, n), (m, n - 1), (0, 0)):
        nv.value = nt.value = 0
        assert call(cap_v, cap_t) == _lib.ERR_INVALID and (nv.value, nt.value) == (m, n), (cap_v, cap_t)
        assert untouched(), (cap_v, cap_t)
    assert "vertices" in vr._lib.vrhip_last_error(vr._h).decode()
    with pytest.raises(ValueError):
        vr.extract_isosurface_indexed(0.2, True, out_dev_ptrs=(ptrs[0], ptrs[1], ptrs[2], m - 1, n))
    # a misaligned index destination: refused before anything runs
    assert call(m, n, ptrs[2] + 4) == _lib.ERR_INVALID and untouched()
    # exact capacities: the restatement's bytes, the guard words before and behind them untouched
    assert vr.extract_isosurface_indexed(0.2, True, out_dev_ptrs=(ptrs[0], ptrs[1], ptrs[2], m, n)) == (m, n)
    rs.synchronize()
    torch.cuda.synchronize()
    hv, hn, hi = vtx.cpu().numpy(), nrm.cpu().numpy(), idx.cpu().numpy().view(np.uint32)
    _same(hv[PAD:PAD + 3 * m].reshape(m, 3), want[0], "device vertices")
    _same(hn[PAD:PAD + 3 * m].reshape(m, 3), want[1], "device normals")
    _same(hi[PAD:PAD + 3 * n].reshape(n, 3), want[2], "device indices")
    for h, g, k in ((hv, np.float32(GUARD_F), 3 * m), (hn, np.float32(GUARD_F), 3 * m), (hi, np.uint32(GUARD_I), 3 * n)):
        assert (h[:PAD] == g).all() and (h[PAD + k:] == g).all()
    # host memory with guard words around it
    hvtx, hidx = np.full(3 * m + 2 * PAD, GUARD_F, np.float32), np.full(3 * n + 2 * PAD, GUARD_I, np.uint32)
    p2 = vr._mesh_params(0.2, False, None)
    args = (C.c_void_p(hvtx.ctypes.data + 4 * PAD), None, C.c_void_p(hidx.ctypes.data + 4 * PAD))
    assert vr._lib.vrhip_isosurface_extract_indexed(vr._h, C.byref(p2), *args, m, n - 1, C.byref(nv), C.byref(nt), 0) == _lib.ERR_INVALID
    assert (hvtx == np.float32(GUARD_F)).all() and (hidx == GUARD_I).all() and (nv.value, nt.value) == (m, n)
    assert vr._lib.vrhip_isosurface_extract_indexed(vr._h, C.byref(p2), *args, m, n, C.byref(nv), C.byref(nt), 0) == _lib.OK
    _same(hvtx[PAD:PAD + 3 * m].reshape(m, 3), want[0], "host vertices")
    _same(hidx[PAD:PAD + 3 * n].reshape(n, 3), want[2], "host indices")
    assert (hvtx[:PAD] == np.float32(GUARD_F)).all() and (hvtx[PAD + 3 * m:] == np.float32(GUARD_F)).all()
    assert (hidx[:PAD] == GUARD_I).all() and (hidx[PAD + 3 * n:] == GUARD_I).all()


def test_two_calls_give_the_same_bytes(vr):
    vol = ref.noise((40, 33, 21), USHORT, seed=3)
    _load(vr, vol, USHORT)
    a = vr.extract_isosurface_indexed(0.5, True)
    b = vr.extract_isosurface_indexed(0.5, True)
    assert a[2].shape[0] > 1000 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    want = ref.extract(vol, USHORT, 0.5, normals=True)
    for got, w, what in zip(a, want, ("vertices", "normals", "indices")):
        _same(got, w, "40x33x21 " + what)


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
    """Progressive frames with an indexed extraction between them equal the uninterrupted sequence bit for bit."""
    vol = ref.ball()
    _load(vr, vol, UCHAR)
    vr.updateView(common.views()["rot30"])
    vr.setObjEss(True)

    def between():
        before = vr.lastLaunchInfo()
        vr.isosurface_count_indexed(0.2)
        vr.extract_isosurface_indexed(0.3, True, region=BALL_REGION)
        assert vr.lastLaunchInfo() == before

    try:
        plain = _frames(vr, 72, 56, tech)
        mixed = _frames(vr, 72, 56, tech, between)
    finally:
        vr.setTechnique(TECH_RAYCAST)
    assert len(plain) == len(mixed) >= 2
    for i, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "frame %d differs" % i
    assert not np.array_equal(plain[0], plain[-1])


def test_soup_and_indexed_calls_leave_each_other_alone(vr):
    vol = ref.ball()
    _load(vr, vol, UCHAR)
    soup = mesh_ref.extract(vol, UCHAR, 0.2, normals=True)
    pos, nrm = vr.extract_isosurface(0.2, True)
    info = vr.lastMeshInfo()
    vtx, _, idx = vr.extract_isosurface_indexed(0.3, False, region=BALL_REGION)
    assert vr.isosurface_count_indexed(0.25)[1] != info["triangles"]
    assert vr.lastMeshInfo() == info
    _same(pos, soup[0], "soup before")
    pos2, nrm2 = vr.extract_isosurface(0.2, True)
    _same(pos2, soup[0], "soup positions after an indexed call")
    _same(nrm2, soup[1], "soup normals after an indexed call")
    before = vr.lastIndexedMeshInfo()
    vr.isosurface_count(0.4)
    assert vr.lastIndexedMeshInfo() == before
    _same(vtx[idx], mesh_ref.extract(vol, UCHAR, 0.3, region=BALL_REGION)[0], "indexed between two soup calls")


def _params(iso=0.2, normals=0, lo=(0, 0, 0), hi=(0, 0, 0), reserved=(0, 0, 0, 0)):
    p = _lib.MeshParams()
    p.isoValue, p.normals = iso, normals
    p.lo[:], p.hi[:], p.reserved[:] = lo, hi, reserved
    return p


def test_refusals(vr):
    vol = ref.ball()
    _load(vr, vol, UCHAR)
    good = vr.extract_isosurface_indexed(0.2)
    m, n = good[0].shape[0], good[2].shape[0]
    lib, h = vr._lib, vr._h
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    vbuf, nbuf, ibuf = np.zeros(3 * m, np.float32), np.zeros(3 * m, np.float32), np.zeros(3 * n, np.uint32)
    V, NB, I = (b.ctypes.data_as(C.c_void_p) for b in (vbuf, nbuf, ibuf))
    cnt = (C.byref(nv), C.byref(nt))
    inf, nan = float("inf"), float("nan")
    bad = [_params(normals=2), _params(iso=nan), _params(iso=inf), _params(iso=-inf),
           _params(lo=(0, 0, 0), hi=(41, 40, 40)), _params(lo=(0, 0, 0), hi=(40, 40, 41)),
           _params(lo=(5, 0, 0), hi=(4, 40, 40)), _params(lo=(0, 0, 9), hi=(40, 40, 8)),
           _params(lo=(0, 0, 0), hi=(0, 40, 40)), _params(lo=(1, 0, 0), hi=(0, 0, 0)),
           _params(lo=(0, 0, 0), hi=(40, 0, 0))]
    bad += [_params(reserved=tuple(int(i == k) for i in range(4))) for k in range(4)]
    for p in bad:
        what = (p.isoValue, p.normals, tuple(p.lo), tuple(p.hi), tuple(p.reserved))
        assert lib.vrhip_isosurface_count_indexed(h, C.byref(p), *cnt) == _lib.ERR_INVALID, what
        assert lib.vrhip_isosurface_extract_indexed(h, C.byref(p), V, None, I, m, n, *cnt, 0) == _lib.ERR_INVALID, what
    ok = _params()
    assert lib.vrhip_isosurface_count_indexed(h, None, *cnt) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_count_indexed(h, C.byref(ok), None, cnt[1]) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_count_indexed(h, C.byref(ok), cnt[0], None) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(h, None, V, None, I, m, n, *cnt, 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(h, C.byref(ok), V, None, I, m, n, None, cnt[1], 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(h, C.byref(ok), V, None, I, m, n, cnt[0], None, 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(h, C.byref(ok), None, None, I, m, n, *cnt, 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(h, C.byref(ok), V, None, None, m, n, *cnt, 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract_indexed(h, C.byref(ok), V, NB, I, m, n, *cnt, 0) == _lib.ERR_INVALID        # normals == 0
    assert lib.vrhip_isosurface_extract_indexed(h, C.byref(_params(normals=1)), V, None, I, m, n, *cnt, 0) == _lib.ERR_INVALID
    for off in ((4, 0), (0, 4)):   # a device destination that is not 16-byte aligned
        assert lib.vrhip_isosurface_extract_indexed(h, C.byref(ok), C.c_void_p(vbuf.ctypes.data + off[0]), None,
                                                    C.c_void_p(ibuf.ctypes.data + off[1]), m, n, *cnt, 1) == _lib.ERR_INVALID
    assert lib.vrhip_last_indexed_mesh_info(h, None) == _lib.ERR_INVALID
    assert (vbuf == 0).all() and (ibuf == 0).all()
    with pytest.raises(ValueError):
        vr.isosurface_count_indexed(nan)
    again = vr.extract_isosurface_indexed(0.2)
    _same(again[0], good[0], "vertices after the refusals")
    _same(again[2], good[2], "indices after the refusals")

    r = VolumeRenderCL()
    r.initialize()
    try:
        mi = _lib.IndexedMeshInfo()
        assert r._lib.vrhip_last_indexed_mesh_info(r._h, C.byref(mi)) == _lib.ERR_NODATA
        assert r._lib.vrhip_isosurface_count_indexed(r._h, C.byref(ok), *cnt) == _lib.ERR_NODATA   # no volume
        assert r._lib.vrhip_isosurface_extract_indexed(r._h, C.byref(ok), V, None, I, m, n, *cnt, 0) == _lib.ERR_NODATA
        assert r._lib.vrhip_last_indexed_mesh_info(r._h, C.byref(mi)) == _lib.ERR_NODATA
        rg = np.zeros((40, 40, 40, 2), np.uint8)
        rg[..., 0] = vol
        r.loadVolumeArrays([rg], UCHAR, channels=2)
        assert r._lib.vrhip_isosurface_count_indexed(r._h, C.byref(ok), *cnt) == _lib.ERR_UNSUPPORTED
        assert r._lib.vrhip_isosurface_extract_indexed(r._h, C.byref(ok), V, None, I, m, n, *cnt, 0) == _lib.ERR_UNSUPPORTED
        # a soup call does not stand in for an indexed one
        r.loadVolumeArrays([vol], UCHAR)
        r.isosurface_count(0.2)
        assert r._lib.vrhip_last_indexed_mesh_info(r._h, C.byref(mi)) == _lib.ERR_NODATA
        fresh = r.extract_isosurface_indexed(0.2)
        _same(fresh[0], good[0], "a fresh renderer, vertices")
        _same(fresh[2], good[2], "a fresh renderer, indices")
    finally:
        r.close()


# ---- C++ class and CLI

def _synth(vr, kind, n):
    vr.synthVolume(kind, (n, n, n), UCHAR)
    return vr.downloadVolume(0)


def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_mesh_indexed")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_mesh_indexed.cpp"), "-o", exe,
                           "-L", PKG, "-lvrhost", "-lvrhip", "-Wl,-rpath," + PKG])
    out, files = str(tmp_path / "mesh.bin"), str(tmp_path / "sphere")
    res = subprocess.run([exe, out, files], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, *shape):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape)), offset=at).reshape(shape)
        at += a.nbytes
        return a

    _synth(vr, "sphere", 32)
    vtx, nrm, idx = vr.extract_isosurface_indexed(np.float32(0.4), True)
    m, n = int(take(np.uint64, 1)[0]), int(take(np.uint64, 1)[0])
    assert (m, n) == (vtx.shape[0], idx.shape[0]) and n > 100
    _same(take(np.float32, m, 3), vtx, "C++ vertices")
    _same(take(np.float32, m, 3), nrm, "C++ normals")
    _same(take(np.uint32, n, 3), idx, "C++ indices")
    pv, _, pidx = vr.extract_isosurface_indexed(np.float32(0.4), False, BALL_REGION)
    assert (int(take(np.uint64, 1)[0]), int(take(np.uint64, 1)[0])) == (pv.shape[0], pidx.shape[0])
    _same(take(np.float32, pv.shape[0], 3), pv, "C++ region vertices")
    _same(take(np.uint32, pidx.shape[0], 3), pidx, "C++ region indices")
    assert at == len(raw)
    fv, fn, fidx = frontend.read_ply(files + ".ply")
    _same(fv, vtx, "writePly vertices")
    _same(fn, nrm, "writePly normals")
    _same(fidx.astype(np.uint32), idx, "writePly indices")


@pytest.mark.parametrize("normals,region", [(True, True), (False, True), (True, False)],
                         ids=["normals_region", "plain_region", "normals_whole"])
def test_cli_indexed_ply_is_the_python_mesh(vr, tmp_path, normals, region):
    path = str(tmp_path / "shells.ply")
    args = [EXE, "--synth", "shells", "32", "UCHAR", "--mesh", "0.5", path, "--mesh-indexed"]
    args += ["--mesh-region", "0", "0", "0", "30", "32", "17"] if region else []
    res = subprocess.run(args + (["--mesh-normals"] if normals else []), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    _synth(vr, "shells", 32)
    vtx, nrm, idx = vr.extract_isosurface_indexed(0.5, normals, ((0, 0, 0), (30, 32, 17)) if region else None)
    assert info["triangles"] == idx.shape[0] > 100 and info["vertices"] == vtx.shape[0] and info["indexed"] is True
    fv, fn, fidx = frontend.read_ply(path)
    _same(fv, vtx, "vertices")
    _same(fn, nrm, "normals")
    _same(fidx.astype(np.uint32), idx, "indices")


def test_cli_without_the_flag_still_welds(vr, tmp_path):
    path = str(tmp_path / "shells.ply")
    args = [EXE, "--synth", "shells", "32", "UCHAR", "--mesh", "0.5", path, "--mesh-normals"]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    _synth(vr, "shells", 32)
    v, vn, idx = frontend.weld_mesh(*vr.extract_isosurface(0.5, True))
    fv, fn, fidx = frontend.read_ply(path)
    assert info["vertices"] == v.shape[0] and "indexed" not in info
    _same(fv, v, "vertices")
    _same(fn, vn, "normals")
    assert np.array_equal(fidx, idx)


@pytest.mark.parametrize("args", [["--mesh", 0.5, "out.stl", "--mesh-indexed"], ["--mesh-indexed"],
                                  ["--out", "frame", "--mesh-indexed"]])
def test_cli_usage_errors(tmp_path, args):
    full = ["--synth", "shells", 32, "UCHAR"] + args
    res = subprocess.run([EXE] + [str(a) for a in full], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), res.stderr
    assert "[--mesh-indexed]" in res.stderr and not os.listdir(str(tmp_path))
