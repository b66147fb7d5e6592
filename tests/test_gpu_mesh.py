"""Isosurface extraction (vrhip_isosurface_count / _extract, vr_mesh.hip) against its CPU restatement
(tests/ref/mesh_ref.c, pinned by tests/test_mesh_ref.py): the raw bytes of the triangle list equal the restatement's
and `count` equals its length -- every voxel type, partial blocks on every axis, small and thin volumes, normals,
object-order ESS on and off (the skipping must not change a byte), regions, a second time step, capacities and guard
words, determinism, the renderer's state around a call, every refusal of the contract, the C++ class and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import common, mesh_ref
from volumerenderercl_amd import FLOAT, TECH_PATHTRACE, TECH_RAYCAST, UCHAR, USHORT, VolumeRenderCL, _lib, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "volumerenderercl_amd")
EXE = os.path.join(PKG, "vrhip_render")


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _quantise(f, fmt):
    if fmt == UCHAR:
        return np.round(f * 255).astype(np.uint8)
    if fmt == USHORT:
        return np.round(f * 65535).astype(np.uint16)
    return f.astype(np.float32)


def _noise(res, fmt, seed=5):
    """Seeded noise, smoothed once along every axis: values in [0, 1] with structure down to a voxel, whatever the shape."""
    f = np.random.default_rng(seed).random((res[2] + 2, res[1] + 2, res[0] + 2))
    for ax in range(3):
        f = (np.take(f, range(0, f.shape[ax] - 2), ax) + np.take(f, range(1, f.shape[ax] - 1), ax) +
             np.take(f, range(2, f.shape[ax]), ax)) / 3.0
    return _quantise(f.astype(np.float32), fmt)


def _ball(n=40, fmt=UCHAR, centre=(19.3, 20.1, 19.6), radius=13.0):
    """1 at the centre, falling to exactly 0 at `radius` and beyond: whole cells of the grid are all 0, others all high."""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return _quantise(np.clip(1.0 - d / radius, 0.0, 1.0).astype(np.float32), fmt)


def _load(vr, vols, fmt):
    vr.loadVolumeArrays(vols if isinstance(vols, list) else [vols], fmt)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.setStatsEnabled(False)
    vr.setTechnique(TECH_RAYCAST)
    vr.setIteration(0)


def _same(got, ref, what):
    assert (got is None) == (ref is None), what
    if ref is None:
        return
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d words differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])


def _blocks(res, region=None):
    lo = region[0] if region else (0, 0, 0)
    hi = [min(h, r - 1) for h, r in zip(region[1] if region else res, res)]
    n = 1
    for a, b in zip(lo, hi):
        n *= ((b - 1) // 8 - a // 8 + 1) if b > a else 0
    return n


def _check(vr, vol, fmt, iso, what, normals=False, region=None):
    """ESS on and off: count, positions and normals equal the restatement's bytes, and so each other."""
    ref = mesh_ref.extract(vol, fmt, iso, normals=normals, region=region)
    res = vol.shape[::-1]
    infos = []
    for ess in (True, False):
        vr.setObjEss(ess)
        assert vr.isosurface_count(iso, region) == ref[0].shape[0], (what, ess)
        pos, nrm = vr.extract_isosurface(iso, normals, region)
        _same(pos, ref[0], "%s, positions, ESS %s" % (what, ess))
        _same(nrm, ref[1], "%s, normals, ESS %s" % (what, ess))
        mi = vr.lastMeshInfo()
        assert mi["triangles"] == ref[0].shape[0] and mi["blocks"] == _blocks(res, region), (what, mi)
        assert mi["empty_skip"] == (int(ess) if mi["blocks"] else 0) and mi["blocks_skipped"] <= mi["blocks"]
        if not ess:
            assert mi["blocks_skipped"] == 0
        infos.append(mi)
    vr.setObjEss(True)
    return ref, infos


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_voxel_types_on_partial_blocks(vr, fmt, normals):
    """17 x 10 x 9: two blocks with a partial one along x, partial blocks along y and z."""
    vol = _noise((17, 10, 9), fmt)
    _load(vr, vol, fmt)
    (pos, _), _ = _check(vr, vol, fmt, 0.5, "17x10x9 %d" % fmt, normals=normals)
    assert pos.shape[0] > 200


@pytest.mark.parametrize("res", [(9, 9, 9), (8, 8, 8), (33, 2, 5), (5, 1, 5)], ids=lambda r: "x".join(map(str, r)))
def test_small_volumes(vr, res):
    """One block with (9^3: the ninth point is the volume's last) and without (8^3) a neighbour's points, one cube thick,
    and an axis of length 1: zero triangles, VRHIP_OK."""
    vol = _noise(res, UCHAR, seed=9)
    _load(vr, vol, UCHAR)
    (pos, _), infos = _check(vr, vol, UCHAR, 0.5, str(res), normals=True)
    if 1 in res:
        assert pos.shape[0] == 0 and infos[0]["blocks"] == 0
    else:
        assert pos.shape[0] > 0


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
def test_ball_and_skipping(vr, normals):
    """A 40^3 ball: ESS on skips blocks (all outside at the corners, all inside at the centre), ESS off none, and not a
    byte changes."""
    vol = _ball()
    _load(vr, vol, UCHAR)
    (pos, _), (on, off) = _check(vr, vol, UCHAR, 0.2, "ball", normals=normals)
    assert pos.shape[0] > 5000
    assert on["blocks"] == off["blocks"] == 125 and on["blocks_skipped"] > 8 and off["blocks_skipped"] == 0


def test_region_is_the_filtered_whole_list(vr):
    vol = _ball()
    _load(vr, vol, UCHAR)
    lo, hi = (3, 5, 2), (29, 30, 31)
    (part, pn), _ = _check(vr, vol, UCHAR, 0.2, "region", normals=True, region=(lo, hi))
    whole, wn, _, cubes = mesh_ref.extract(vol, UCHAR, 0.2, normals=True, debug=True)
    keep = np.all((cubes >= np.array(lo)) & (cubes + 1 <= np.array(hi)), axis=1)
    assert 0 < keep.sum() < keep.size
    _same(part, whole[keep], "region against the filtered whole list")
    _same(pn, wn[keep], "region normals against the filtered whole list")
    # a region of one cube, one that ends at the volume's last point, and a flat one
    for region, some in ((((29, 20, 19), (30, 21, 20)), True), (((20, 20, 20), (40, 40, 40)), True),
                         (((4, 4, 4), (20, 4, 20)), False)):
        (pos, _), _ = _check(vr, vol, UCHAR, 0.2, str(region), region=region)
        assert (pos.shape[0] > 0) == some, region


def test_second_time_step(vr):
    a, b = _ball(), _ball(centre=(17.2, 22.4, 18.9), radius=11.0)
    _load(vr, [a, b], UCHAR)
    try:
        (first, _), _ = _check(vr, a, UCHAR, 0.2, "step 0")
        vr.setTimestep(1)
        (second, _), _ = _check(vr, b, UCHAR, 0.2, "step 1", normals=True)
        vr.setTimestep(0)
        (again, _), _ = _check(vr, a, UCHAR, 0.2, "step 0 again")
        assert first.shape != second.shape and again.tobytes() == first.tobytes()
    finally:
        vr.setTimestep(0)


GUARD = -7.25


def test_capacity_and_guards(vr):
    import torch
    vol = _ball()
    _load(vr, vol, UCHAR)
    ref, rn = mesh_ref.extract(vol, UCHAR, 0.2, normals=True)
    n = ref.shape[0]
    rs = torch.cuda.ExternalStream(vr.get_stream())
    p = vr._mesh_params(0.2, True, None)
    got = C.c_uint64(0)
    # capacity n - 1: refused, the number needed reported, nothing written
    pos = torch.full((n * 9 + 64,), GUARD, dtype=torch.float32, device="cuda")
    nrm = torch.full((n * 9 + 64,), GUARD, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = vr._lib.vrhip_isosurface_extract(vr._h, C.byref(p), C.c_void_p(pos.data_ptr()), C.c_void_p(nrm.data_ptr()), n - 1,
                                          C.byref(got), 1)
    rs.synchronize()
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and got.value == n
    assert bool((pos == GUARD).all()) and bool((nrm == GUARD).all())
    with pytest.raises(ValueError):
        vr.extract_isosurface(0.2, True, out_dev_ptrs=(pos.data_ptr(), nrm.data_ptr(), n - 1))
    # capacity n: the list, and the words behind it untouched
    assert vr.extract_isosurface(0.2, True, out_dev_ptrs=(pos.data_ptr(), nrm.data_ptr(), n)) == n
    rs.synchronize()
    torch.cuda.synchronize()
    hp, hn = pos.cpu().numpy(), nrm.cpu().numpy()
    _same(hp[:n * 9].reshape(n, 3, 3), ref, "device positions")
    _same(hn[:n * 9].reshape(n, 3, 3), rn, "device normals")
    assert (hp[n * 9:] == GUARD).all() and (hn[n * 9:] == GUARD).all()
    # host memory with guard words behind it
    hpos = np.full(n * 9 + 64, GUARD, np.float32)
    p2 = vr._mesh_params(0.2, False, None)
    assert vr._lib.vrhip_isosurface_extract(vr._h, C.byref(p2), hpos.ctypes.data_as(C.c_void_p), None, n, C.byref(got), 0) == _lib.OK
    _same(hpos[:n * 9].reshape(n, 3, 3), ref, "host positions")
    assert (hpos[n * 9:] == GUARD).all()
    assert vr._lib.vrhip_isosurface_extract(vr._h, C.byref(p2), hpos.ctypes.data_as(C.c_void_p), None, 0, C.byref(got), 0) == _lib.ERR_INVALID
    assert got.value == n and "triangles" in vr._lib.vrhip_last_error(vr._h).decode()


def test_two_calls_give_the_same_bytes(vr):
    vol = _noise((40, 33, 21), USHORT, seed=3)
    _load(vr, vol, USHORT)
    a = vr.extract_isosurface(0.5, True)
    b = vr.extract_isosurface(0.5, True)
    assert a[0].shape[0] > 1000 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _same(a[0], mesh_ref.extract(vol, USHORT, 0.5)[0], "40x33x21")


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
    """Progressive frames with an extraction between them equal the uninterrupted sequence bit for bit."""
    vol = _ball()
    _load(vr, vol, UCHAR)
    vr.updateView(common.views()["rot30"])
    vr.setObjEss(True)

    def between():
        before = vr.lastLaunchInfo()
        vr.isosurface_count(0.2)
        vr.extract_isosurface(0.3, True, region=((3, 5, 2), (29, 30, 31)))
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


def _params(iso=0.2, normals=0, lo=(0, 0, 0), hi=(0, 0, 0), reserved=(0, 0, 0, 0)):
    p = _lib.MeshParams()
    p.isoValue, p.normals = iso, normals
    p.lo[:], p.hi[:], p.reserved[:] = lo, hi, reserved
    return p


def test_refusals(vr):
    vol = _ball()
    _load(vr, vol, UCHAR)
    good = vr.extract_isosurface(0.2)[0]
    n = good.shape[0]
    lib, h = vr._lib, vr._h
    cnt = C.c_uint64(0)
    buf = np.zeros(n * 9, np.float32)
    nbuf = np.zeros(n * 9, np.float32)
    P, NB = buf.ctypes.data_as(C.c_void_p), nbuf.ctypes.data_as(C.c_void_p)
    inf, nan = float("inf"), float("nan")
    bad = [_params(normals=2), _params(iso=nan), _params(iso=inf), _params(iso=-inf),
           _params(lo=(0, 0, 0), hi=(41, 40, 40)), _params(lo=(0, 0, 0), hi=(40, 40, 41)),
           _params(lo=(5, 0, 0), hi=(4, 40, 40)), _params(lo=(0, 0, 9), hi=(40, 40, 8)),
           _params(lo=(0, 0, 0), hi=(0, 40, 40)), _params(lo=(1, 0, 0), hi=(0, 0, 0)),
           _params(lo=(0, 0, 0), hi=(40, 0, 0))]
    bad += [_params(reserved=tuple(int(i == k) for i in range(4))) for k in range(4)]
    for p in bad:
        what = (p.isoValue, p.normals, tuple(p.lo), tuple(p.hi), tuple(p.reserved))
        assert lib.vrhip_isosurface_count(h, C.byref(p), C.byref(cnt)) == _lib.ERR_INVALID, what
        assert lib.vrhip_isosurface_extract(h, C.byref(p), P, None, n, C.byref(cnt), 0) == _lib.ERR_INVALID, what
    ok = _params()
    assert lib.vrhip_isosurface_count(h, None, C.byref(cnt)) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_count(h, C.byref(ok), None) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract(h, None, P, None, n, C.byref(cnt), 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract(h, C.byref(ok), P, None, n, None, 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract(h, C.byref(ok), None, None, n, C.byref(cnt), 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract(h, C.byref(ok), P, NB, n, C.byref(cnt), 0) == _lib.ERR_INVALID        # normals == 0
    assert lib.vrhip_isosurface_extract(h, C.byref(_params(normals=1)), P, None, n, C.byref(cnt), 0) == _lib.ERR_INVALID
    assert lib.vrhip_isosurface_extract(h, C.byref(ok), C.c_void_p(buf.ctypes.data + 4), None, n, C.byref(cnt), 1) == _lib.ERR_INVALID
    assert lib.vrhip_last_mesh_info(h, None) == _lib.ERR_INVALID
    assert (buf == 0).all()
    with pytest.raises(ValueError):
        vr.isosurface_count(nan)
    _same(vr.extract_isosurface(0.2)[0], good, "after the refusals")

    r = VolumeRenderCL()
    r.initialize()
    try:
        mi = _lib.MeshInfo()
        assert r._lib.vrhip_last_mesh_info(r._h, C.byref(mi)) == _lib.ERR_NODATA
        assert r._lib.vrhip_isosurface_count(r._h, C.byref(ok), C.byref(cnt)) == _lib.ERR_NODATA   # no volume
        assert r._lib.vrhip_isosurface_extract(r._h, C.byref(ok), P, None, n, C.byref(cnt), 0) == _lib.ERR_NODATA
        assert r._lib.vrhip_last_mesh_info(r._h, C.byref(mi)) == _lib.ERR_NODATA
        rg = np.zeros((40, 40, 40, 2), np.uint8)
        rg[..., 0] = vol
        r.loadVolumeArrays([rg], UCHAR, channels=2)
        assert r._lib.vrhip_isosurface_count(r._h, C.byref(ok), C.byref(cnt)) == _lib.ERR_UNSUPPORTED
        assert r._lib.vrhip_isosurface_extract(r._h, C.byref(ok), P, None, n, C.byref(cnt), 0) == _lib.ERR_UNSUPPORTED
        # no transfer function, no camera: the surface all the same
        r.loadVolumeArrays([vol], UCHAR)
        _same(r.extract_isosurface(0.2)[0], good, "a fresh renderer")
    finally:
        r.close()


# ---- C++ class and CLI

def _synth(vr, kind, n):
    vr.synthVolume(kind, (n, n, n), UCHAR)
    return vr.downloadVolume(0)


def test_cpp_caller(vr, tmp_path):
    exe = str(tmp_path / "caller_mesh")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "caller_mesh.cpp"), "-o", exe,
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

    vol = _synth(vr, "sphere", 32)
    ref, rn = mesh_ref.extract(vol, UCHAR, np.float32(0.4), normals=True)
    n = int(take(np.uint64, 1)[0])
    assert n == ref.shape[0] > 100
    _same(take(np.float32, n, 3, 3), ref, "C++ positions")
    _same(take(np.float32, n, 3, 3), rn, "C++ normals")
    part = mesh_ref.extract(vol, UCHAR, np.float32(0.4), region=((3, 5, 2), (29, 30, 31)))[0]
    assert int(take(np.uint64, 1)[0]) == part.shape[0]
    _same(take(np.float32, part.shape[0], 3, 3), part, "C++ region")
    v, vn, idx = frontend.weld_mesh(ref, rn)
    nv = int(take(np.uint64, 1)[0])
    assert nv == v.shape[0]
    _same(take(np.float32, nv, 3), v, "weldMesh vertices")
    _same(take(np.float32, nv, 3), vn, "weldMesh normals")
    assert np.array_equal(take(np.uint32, n, 3), idx) and at == len(raw)
    pv, pn, pidx = frontend.read_ply(files + ".ply")
    _same(pv, v, "writePly vertices")
    _same(pn, vn, "writePly normals")
    assert np.array_equal(pidx, idx)
    sn, sp = frontend.read_stl(files + ".stl")
    _same(sp, ref, "writeStl positions")
    assert np.allclose(sn, frontend.facet_normals(ref), atol=1e-6)


@pytest.mark.parametrize("ext,normals", [("ply", True), ("ply", False), ("stl", False)])
def test_cli_files_reproduce_the_python_soup(vr, tmp_path, ext, normals):
    path = str(tmp_path / ("shells." + ext))
    args = [EXE, "--synth", "shells", "32", "UCHAR", "--mesh", "0.5", path, "--mesh-region", "0", "0", "0", "30", "32", "17"]
    res = subprocess.run(args + (["--mesh-normals"] if normals else []), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    vol = _synth(vr, "shells", 32)
    region = ((0, 0, 0), (30, 32, 17))
    pos, nrm = vr.extract_isosurface(0.5, normals, region)
    _same(pos, mesh_ref.extract(vol, UCHAR, 0.5, region=region)[0], "python")
    assert info["triangles"] == pos.shape[0] > 100
    v, vn, idx = frontend.weld_mesh(pos, nrm)
    if ext == "ply":
        fv, fn, fidx = frontend.read_ply(path)
        assert info["vertices"] == v.shape[0] == fv.shape[0]
        _same(fv, v, "vertices")
        _same(fn, vn, "normals")
        assert np.array_equal(fidx, idx)
        _same(fv[fidx], pos, "the welded vertices and indices reproduce the soup")
    else:
        sn, sp = frontend.read_stl(path)
        _same(sp, pos, "stl")
        assert np.allclose(sn, frontend.facet_normals(pos), atol=1e-6) and "vertices" not in info


@pytest.mark.parametrize("extra", [["--pathtrace"], ["--mip"], ["--iso", 0.4], ["--slice-axis", "Z", 0], ["--depth", "max"],
                                   ["--ranks", 2], ["--frames", 2], ["--rgba8"], ["--orbit", 0, 1, 0, 4],
                                   ["--frames-per-launch", 4], ["--img-ess"]])
def test_cli_does_not_combine(tmp_path, extra):
    path = str(tmp_path / "bad.ply")
    args = ["--synth", "shells", 32, "UCHAR", "--mesh", 0.5, path] + extra
    res = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), res.stderr
    assert "--mesh V FILE.stl|.ply" in res.stderr and not os.path.exists(path)


@pytest.mark.parametrize("args", [["--mesh", 0.5, "out.obj"], ["--mesh", 0.5, "out"], ["--mesh-normals"],
                                  ["--mesh-region", 0, 0, 0, 8, 8, 8], ["--timestep", 1], ["--mesh", "nan", "out.ply"]])
def test_cli_usage_errors(tmp_path, args):
    full = ["--synth", "shells", 32, "UCHAR", "--out", str(tmp_path / "bad")] + args
    res = subprocess.run([EXE] + [str(a) for a in full], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render"), res.stderr
    assert not os.listdir(str(tmp_path))
