"""The CPU restatement of the indexed isosurface extraction (tests/ref/mesh_indexed_ref.c) against the contract of
include/vrhip.h "indexed isosurface extraction", without a GPU: vertices[indices] is the soup of tests/mesh_ref.py bit
for bit, the vertex count is an independent count of eligible crossed edges, every vertex is used, the closed ball is
a closed surface by its indices alone, and identity is the edge -- grid values equal to isoValue keep the duplicates a
weld by bit-equality merges.  tests/test_gpu_mesh_indexed.py then holds the kernels to the restatement."""
import numpy as np
import pytest

from tests import mesh_indexed_ref as ref
from tests import mesh_ref
from tests.mesh_ref import FLOAT, UCHAR, USHORT
from volumerenderercl_amd import frontend

BALL_REGION = ((3, 5, 2), (29, 30, 31))
CASES = {
    "noise_uchar": (lambda: ref.noise((17, 10, 9), UCHAR), UCHAR, 0.5, None),
    "noise_ushort": (lambda: ref.noise((17, 10, 9), USHORT), USHORT, 0.5, None),
    "noise_float": (lambda: ref.noise((17, 10, 9), FLOAT), FLOAT, 0.5, None),
    "9x9x9": (lambda: ref.noise((9, 9, 9), UCHAR, seed=9), UCHAR, 0.5, None),
    "8x8x8": (lambda: ref.noise((8, 8, 8), UCHAR, seed=9), UCHAR, 0.5, None),
    "33x2x5": (lambda: ref.noise((33, 2, 5), UCHAR, seed=9), UCHAR, 0.5, None),
    "5x1x5": (lambda: ref.noise((5, 1, 5), UCHAR, seed=9), UCHAR, 0.5, None),
    "ball": (ref.ball, UCHAR, 0.2, None),
    "ball_region": (ref.ball, UCHAR, 0.2, BALL_REGION),
    "exact_iso": (ref.exact_iso_volume, FLOAT, 0.5, None),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    make, fmt, iso, region = CASES[request.param]
    vol = make()
    soup = mesh_ref.extract(vol, fmt, iso, normals=True, region=region)
    mesh = ref.extract(vol, fmt, iso, normals=True, region=region)
    return request.param, vol, fmt, iso, region, soup, mesh


def test_indices_reproduce_the_soup(case):
    name, _, _, _, _, (pos, nrm), (vtx, vn, idx, _) = case
    assert idx.shape == (pos.shape[0], 3) and vtx.shape == vn.shape
    if name == "5x1x5":
        assert vtx.shape[0] == 0 and idx.shape[0] == 0
        return
    assert idx.shape[0] > 0 and idx.max() < vtx.shape[0]
    assert vtx[idx].tobytes() == pos.tobytes(), name
    assert vn[idx].tobytes() == nrm.tobytes(), name


def test_vertex_count_is_the_crossed_edge_count(case):
    name, vol, fmt, iso, region, _, (vtx, _, _, _) = case
    assert vtx.shape[0] == ref.crossed_edges(vol, fmt, iso, region), name


def test_every_vertex_is_used(case):
    name, _, _, _, _, _, (vtx, _, idx, _) = case
    used = np.zeros(vtx.shape[0], bool)
    used[idx.reshape(-1)] = True
    assert used.all(), "%s: %d vertices belong to no triangle" % (name, (~used).sum())


def test_plain_and_normals_agree(case):
    name, vol, fmt, iso, region, _, (vtx, _, idx, blocks) = case
    v2, n2, i2, b2 = ref.extract(vol, fmt, iso, normals=False, region=region)
    assert n2 is None and v2.tobytes() == vtx.tobytes() and i2.tobytes() == idx.tobytes() and b2 == blocks, name


def test_vertex_order_and_positions_against_numpy():
    """The vertex list, written out in plain Python: point blocks x fastest, points x fastest, d ascending, every
    eligible crossed edge's vertex by the header's formula, one np.float32 operation at a time."""
    f = np.float32
    res = (17, 10, 9)
    vol = ref.noise(res, FLOAT)
    inside = vol >= f(0.5)
    expect = []
    for bz, by, bx in np.ndindex(2, 2, 3):
        for lz, ly, lx in np.ndindex(8, 8, 8):
            P = (8 * bx + lx, 8 * by + ly, 8 * bz + lz)
            for d in range(1, 8):
                Q = tuple(P[ax] + ((d >> ax) & 1) for ax in range(3))
                if any(Q[ax] > res[ax] - 1 for ax in range(3)):   # (the whole volume: eligible = Q is a point of it)
                    continue
                if inside[P[2], P[1], P[0]] == inside[Q[2], Q[1], Q[0]]:
                    continue
                sp, sq = vol[P[2], P[1], P[0]], vol[Q[2], Q[1], Q[0]]
                t = min(max((f(0.5) - sp) / (sq - sp), f(0)), f(1))
                expect.append([(f(P[ax]) + f(Q[ax] - P[ax]) * t + f(0.5)) / f(res[ax]) * f(2) - f(1) for ax in range(3)])
    vtx = ref.extract(vol, FLOAT, 0.5)[0]
    assert vtx.shape[0] > 2000 and vtx.tobytes() == np.array(expect, dtype=np.float32).tobytes()


def test_closed_ball_from_the_indices_alone():
    """Euler characteristic 2, and every undirected edge in exactly two triangles, with opposite directions: no weld."""
    vol = ref.ball()
    vtx, _, idx, _ = ref.extract(vol, UCHAR, 0.2)
    nv = vtx.shape[0]
    a = idx[:, [0, 1, 2]].reshape(-1).astype(np.int64)
    b = idx[:, [1, 2, 0]].reshape(-1).astype(np.int64)
    assert (a != b).all()
    directed = a * nv + b
    assert np.unique(directed).size == directed.size
    undirected, counts = np.unique(np.minimum(a, b) * nv + np.maximum(a, b), return_counts=True)
    assert (counts == 2).all(), "%d edges are not shared by exactly two triangles" % (counts != 2).sum()
    assert np.isin(b * nv + a, directed).all()
    assert nv - undirected.size + idx.shape[0] == 2


def test_values_equal_to_iso_keep_their_duplicates():
    """Identity is the edge: a point equal to isoValue puts t = 0 on all of its crossed edges -- several vertices, one
    position -- and a weld by bit-equality ends with strictly fewer."""
    vol = ref.exact_iso_volume()
    assert (vol == np.float32(0.5)).sum() > 5
    pos, _ = mesh_ref.extract(vol, FLOAT, 0.5)
    vtx, _, idx, _ = ref.extract(vol, FLOAT, 0.5)
    welded = frontend.weld_mesh(pos)[0]
    assert vtx.shape[0] > welded.shape[0]
    assert vtx.shape[0] == ref.crossed_edges(vol, FLOAT, 0.5)
    assert np.unique(vtx.view(np.uint32), axis=0).shape[0] == welded.shape[0]
    assert vtx[idx].tobytes() == pos.tobytes()


@pytest.mark.parametrize("fmt", [UCHAR, FLOAT], ids=["uchar", "float"])
def test_no_value_equal_to_iso_gives_the_weld(fmt):
    vol = ref.noise((17, 10, 9), fmt)
    iso = 0.5 if fmt == FLOAT else 0.501   # (127.755 / 255: no 8-bit value)
    assert not (ref.normalised(vol, fmt) == np.float32(iso)).any()
    pos, _ = mesh_ref.extract(vol, fmt, iso)
    vtx, _, idx, _ = ref.extract(vol, fmt, iso)
    wv, _, widx = frontend.weld_mesh(pos)
    assert vtx.shape[0] == wv.shape[0] > 100
    assert vtx[idx].tobytes() == wv[widx].tobytes()


def test_region_without_a_cube_and_refusals():
    vol = ref.ball()
    for region in (((4, 4, 4), (20, 4, 20)), ((39, 0, 0), (40, 40, 40))):
        vtx, _, idx, blocks = ref.extract(vol, UCHAR, 0.2, region=region)
        assert vtx.shape[0] == 0 and idx.shape[0] == 0 and blocks == 0
    with pytest.raises(ValueError):
        ref.extract(vol, UCHAR, 0.2, region=((0, 0, 0), (41, 40, 40)))
    with pytest.raises(ValueError):
        ref.extract(vol, UCHAR, float("nan"))


def test_point_blocks():
    """9^3: two point blocks per axis, of which (1, 1, 1) owns only the point (8, 8, 8) and no eligible edge; 8^3: one."""
    assert ref.extract(ref.noise((9, 9, 9), UCHAR, seed=9), UCHAR, 0.5)[3] == 7
    assert ref.extract(ref.noise((8, 8, 8), UCHAR, seed=9), UCHAR, 0.5)[3] == 1
    assert ref.extract(ref.noise((17, 10, 9), UCHAR), UCHAR, 0.5)[3] == 3 * 2 * 2 - 0
    assert ref.extract(ref.ball(), UCHAR, 0.2, region=BALL_REGION)[3] == 4 * 4 * 4
