"""The CPU restatement of the isosurface extraction (tests/ref/mesh_ref.c) against the contract of include/vrhip.h
"isosurface extraction", without a GPU: winding, closedness and topology of closed surfaces, the enclosed volume
between two counts of cubes, the edge vertex formula in plain numpy float32, non-finite and exactly-equal values, and
the list of a region as the filtered whole list.  tests/test_gpu_mesh.py then holds the kernels to the restatement."""
import numpy as np
import pytest

from tests import mesh_ref
from tests.mesh_ref import FLOAT, UCHAR, USHORT
from volumerenderercl_amd import frontend

N = 24


def _grid(n=N):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)


def _ball(n=N, centre=(11.3, 12.1, 11.7), radius=7.37):
    x, y, z = _grid(n)
    return (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def _two_balls():
    return np.maximum(_ball(centre=(6.2, 7.1, 6.6), radius=4.21), _ball(centre=(16.4, 15.8, 16.9), radius=4.63))


def _torus():
    """|(|xy| - R, z)| = r around the z axis through (11.6, 11.4, 11.8): R = 6.9, r = 2.83, inside positive."""
    x, y, z = _grid()
    q = np.sqrt((x - 11.6) ** 2 + (y - 11.4) ** 2) - 6.9
    return (2.83 - np.sqrt(q ** 2 + (z - 11.8) ** 2)).astype(np.float32)


FIELDS = {"ball": (_ball, 2), "two_balls": (_two_balls, 4), "torus": (_torus, 0)}
ISO = 0.013   # (asserted below: no voxel of the three fields equals it)


def _to_voxels(pos, res):
    """Box-space positions as voxel-centre coordinates, float64: the inverse of (g + 0.5) / res * 2 - 1."""
    return (np.asarray(pos, np.float64) + 1.0) * 0.5 * np.asarray(res, np.float64) - 0.5


@pytest.fixture(scope="module", params=sorted(FIELDS))
def surface(request):
    make, euler = FIELDS[request.param]
    vol = make()
    assert not (vol == np.float32(ISO)).any()
    # strictly inside the volume: the outermost layer of points is outside
    inside = vol >= np.float32(ISO)
    assert inside.any() and not (inside[0].any() or inside[-1].any() or inside[:, 0].any() or inside[:, -1].any()
                                 or inside[:, :, 0].any() or inside[:, :, -1].any())
    pos, _, dirs, cubes = mesh_ref.extract(vol, FLOAT, ISO, debug=True)
    return request.param, vol, euler, pos, dirs, cubes


def test_winding_points_outside(surface):
    """6a: the float64 right-hand normal of every non-degenerate triangle has a positive dot product with the mean of
    the outside vertices minus the mean of the inside vertices of its tetrahedron."""
    name, vol, _, pos, dirs, _ = surface
    p = _to_voxels(pos, (N, N, N))
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    live = np.linalg.norm(nrm, axis=1) > 0
    assert live.sum() > 100, name
    dots = np.einsum("ij,ij->i", nrm[live], dirs[live])
    assert (dots > 0).all(), "%s: %d triangles wound inwards" % (name, (dots <= 0).sum())


def test_closed_and_topology(surface):
    """6a: welded by bit-equal positions, every undirected edge belongs to exactly two triangles with opposite
    directions; V - E + F is 2, 4 and 0."""
    name, _, euler, pos, _, _ = surface
    verts, _, idx = frontend.weld_mesh(pos)
    # (no triangle is degenerate here: no voxel equals ISO, so every t lies strictly inside (0, 1))
    assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 1] != idx[:, 2]).all() and (idx[:, 0] != idx[:, 2]).all()
    a = idx[:, [0, 1, 2]].reshape(-1).astype(np.int64)
    b = idx[:, [1, 2, 0]].reshape(-1).astype(np.int64)
    nv = verts.shape[0]
    directed = a * nv + b
    assert np.unique(directed).size == directed.size, "%s: a directed edge is used twice" % name
    undirected, counts = np.unique(np.minimum(a, b) * nv + np.maximum(a, b), return_counts=True)
    assert (counts == 2).all(), "%s: %d edges are not shared by exactly two triangles" % (name, (counts != 2).sum())
    assert np.isin(b * nv + a, directed).all(), "%s: an edge lacks its opposite direction" % name
    assert nv - undirected.size + idx.shape[0] == euler, name


def test_ball_encloses_its_cubes():
    """6a: the single ball's enclosed volume (divergence theorem, float64, voxel units) lies between the number of
    cubes with all eight corners inside and that number plus the number of cubes the surface crosses: the surface
    passes through crossed cubes only, so the solid holds every all-inside cube and no all-outside one."""
    vol = _ball()
    pos, _ = mesh_ref.extract(vol, FLOAT, ISO)
    p = _to_voxels(pos, (N, N, N))
    volume = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0
    inside = vol >= np.float32(ISO)
    corners = sum(inside[dz:N - 1 + dz, dy:N - 1 + dy, dx:N - 1 + dx].astype(np.int32)
                  for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    full, crossed = int((corners == 8).sum()), int(((corners > 0) & (corners < 8)).sum())
    assert full > 500 and crossed > 500
    assert full <= volume <= full + crossed, (full, volume, full + crossed)


def _np_edge_vertex(sp, sq, iso, p, q, res):
    """The header's edge vertex, one np.float32 operation at a time."""
    f = np.float32
    with np.errstate(all="ignore"):
        t = (f(iso) - f(sp)) / (f(sq) - f(sp))
    if not t >= f(0):
        t = f(0)
    if t > f(1):
        t = f(1)
    out = []
    for ax in range(3):
        g = f(p[ax]) + f(q[ax] - p[ax]) * t
        out.append((g + f(0.5)) / f(res[ax]) * f(2) - f(1))
    return np.array(out, dtype=np.float32)


TET_CORNER = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def _corner_xyz(j):
    return np.array([j & 1, (j >> 1) & 1, j >> 2])


def _expected_vertices(vol, fmt, iso):
    """All edge vertices of a 2 x 2 x 2 volume's one cube by the formula: {bit pattern: True}, and the triangle count
    the masks dictate."""
    inv = {UCHAR: np.float32(1.0) / np.float32(255.0), USHORT: np.float32(1.0) / np.float32(65535.0), FLOAT: np.float32(1.0)}[fmt]
    with np.errstate(all="ignore"):
        s = [np.float32(vol[j >> 2, (j >> 1) & 1, j & 1]) * inv for j in range(8)]
    verts, count = set(), 0
    for tv in TET_CORNER:
        ins = [bool(s[c] >= np.float32(iso)) for c in tv]
        count += {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(ins)]
        for i in range(4):
            for j in range(i + 1, 4):
                if ins[i] != ins[j]:
                    v = _np_edge_vertex(s[tv[i]], s[tv[j]], iso, _corner_xyz(tv[i]), _corner_xyz(tv[j]), (2, 2, 2))
                    verts.add(v.tobytes())
    return verts, count


@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=["uchar", "ushort", "float"])
def test_edge_vertices_against_numpy(fmt):
    """200 seeded random cubes per voxel type: the positions are the formula's, evaluated in np.float32."""
    rng = np.random.default_rng(1234 + fmt)
    seen = 0
    for _ in range(200):
        if fmt == UCHAR:
            vol, iso = rng.integers(0, 256, (2, 2, 2)).astype(np.uint8), float(rng.uniform(0.2, 0.8))
        elif fmt == USHORT:
            vol, iso = rng.integers(0, 65536, (2, 2, 2)).astype(np.uint16), float(rng.uniform(0.2, 0.8))
        else:
            vol, iso = rng.normal(0, 3, (2, 2, 2)).astype(np.float32), float(rng.normal(0, 1))
        iso = float(np.float32(iso))
        pos, _ = mesh_ref.extract(vol, fmt, iso)
        expect, count = _expected_vertices(vol, fmt, iso)
        assert pos.shape[0] == count
        got = {v.tobytes() for v in pos.reshape(-1, 3)}
        assert got == expect
        seen += len(got)
    assert seen > 1000


@pytest.mark.parametrize("odd", [np.nan, np.inf, -np.inf, "equal"])
def test_odd_values(odd):
    """A NaN, +-inf and a corner exactly equal to isoValue: finite positions, the counts the masks dictate (a NaN is
    outside, an equal corner inside), the vertices the formula gives."""
    iso = 0.25
    rng = np.random.default_rng(7)
    for corner in range(8):
        vol = rng.uniform(-1, 1, (2, 2, 2)).astype(np.float32)
        vol[corner >> 2, (corner >> 1) & 1, corner & 1] = np.float32(iso) if odd == "equal" else odd
        pos, nrm = mesh_ref.extract(vol, FLOAT, iso, normals=True)
        expect, count = _expected_vertices(vol, FLOAT, iso)
        assert pos.shape[0] == count and count > 0
        assert np.isfinite(pos).all() and np.isfinite(nrm).all()
        assert {v.tobytes() for v in pos.reshape(-1, 3)} == expect


def test_axis_of_length_one_has_no_cubes():
    vol = np.random.default_rng(3).uniform(0, 1, (5, 1, 5)).astype(np.float32)
    pos, _ = mesh_ref.extract(vol, FLOAT, 0.5)
    assert pos.shape == (0, 3, 3)


def test_region_is_the_filtered_whole_list():
    """A region not aligned to the blocks: its list is the whole list with the cubes outside it removed, in order."""
    vol = _ball()
    whole, wn, _, cubes = mesh_ref.extract(vol, FLOAT, ISO, normals=True, debug=True)
    lo, hi = (3, 5, 2), (17, 20, 13)
    part, pn, _, pcubes = mesh_ref.extract(vol, FLOAT, ISO, normals=True, region=(lo, hi), debug=True)
    keep = np.all((cubes >= np.array(lo)) & (cubes + 1 <= np.array(hi)), axis=1)
    assert 0 < keep.sum() < keep.size
    assert part.tobytes() == whole[keep].tobytes() and pn.tobytes() == wn[keep].tobytes()
    assert (pcubes == cubes[keep]).all()
    # the order of the list: blocks x fastest, then cubes x fastest
    b = cubes.astype(np.int64) // mesh_ref.BLOCK
    c = cubes.astype(np.int64) % mesh_ref.BLOCK
    key = (((b[:, 2] * 8 + b[:, 1]) * 8 + b[:, 0]) * 512) + (c[:, 2] * 8 + c[:, 1]) * 8 + c[:, 0]
    assert (np.diff(key) >= 0).all()


def test_normals_are_technique_4s_or_zero():
    """Unit length where the gradient is not zero; (0, 0, 0) in a constant neighbourhood."""
    vol = _ball()
    _, nrm = mesh_ref.extract(vol, FLOAT, ISO, normals=True)
    ln = np.linalg.norm(nrm.reshape(-1, 3).astype(np.float64), axis=1)
    assert np.allclose(ln, 1.0, atol=1e-5)
    # +inf and -inf next to each other: inf - inf taps, a NaN gradient -- written as (0, 0, 0)
    vol2 = np.full((2, 2, 2), -np.inf, np.float32)
    vol2[0, 0, 0] = np.inf
    _, nrm2 = mesh_ref.extract(vol2, FLOAT, 0.5, normals=True)
    assert nrm2.shape[0] == 6 and (nrm2.view(np.uint32) == 0).all()
