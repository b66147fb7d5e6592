"""The pixel-major ray index of a launch set, checked directly: the pre-pass's notes, its ray records and the index
vr_regroup_kernel makes of them are downloaded (vrhip_download_ray_order) and held to the plain restatement of
tests/ray_order_ref.py.  Integers throughout, no tolerance.  Frames cannot see what is checked here: an index that
names every ray once renders the same pixels in any order, with any padding, and a ray named twice writes its pixel
twice with the same value.

The scene: "shells" at 48^3 UCHAR, ESS on, seen under the rotation of view "rot30" from a camera moved so that the
object leaves the frame at its right and bottom edges -- with "rot30" itself the object sits in the middle of a 36 x 28
frame and no patch is cut, full or live in some frames only.  View and order of the seeds were chosen with the oracle
on the CPU; the guard (_guard) asserts, with the oracle, that every set still has what it was chosen for."""
import ctypes as C

import numpy as np
import pytest

from oracle import vro
from tests import common
from tests import ray_order_ref as ror
from volumerenderercl_amd import UCHAR, VolumeRenderCL, frontend, tiles

pytestmark = pytest.mark.gpu

RES = (48, 48, 48)
VIEW = frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0), (-0.55, 0.45, 1.3))
_mt = frontend.Mt19937(4357)
_S = [_mt() for _ in range(256)]
# the sixth seed of the sequence second: with it the first two frames already have a patch that is live in one of them
# and dead in the other (36 x 28; 64 x 48: the first three)
SEEDS = [_S[0], _S[5]] + _S[1:5] + _S[6:]
SMALL, LARGE = (36, 28), (64, 48)
# set sizes on both sides of 64 % sf == 0, of sf == 64 and of sf > 64 (64 / sf == 0), the smallest and the largest
SET_SIZES = (2, 3, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 255, 256)
CASES = [(SMALL, sf, 64) for sf in SET_SIZES] + [(LARGE, sf, 64) for sf in (3, 9, 33, 64)] + \
        [(SMALL, sf, g) for g in (1, 32) for sf in (3, 9, 65)] + [(LARGE, 9, 1), (LARGE, 9, 32)]


def _configure(r):
    r.loadVolumeArrays([vro.synth_volume("shells", list(RES), vro.UCHAR)], UCHAR)
    r.setTransferFunction(common.tffs()["default"])
    r.setIllumination(1)
    r.setLinearInterpolation(True)
    r.setCamOrtho(False)
    r.setObjEss(True)
    r.updateSamplingRate(1.5)
    r.setBBox(-1, -1, -1, 1, 1, 1)
    r.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    r.setStatsEnabled(False)
    r.updateView(VIEW)
    r.setIteration(0)


class Scene:
    """The renderers (one per VRHIP_PM_GROUP, created on demand) and the oracle's answers, shared by the tests."""

    def __init__(self):
        self.vol = vro.synth_volume("shells", list(RES), vro.UCHAR)
        self.tff = common.tffs()["default"]
        self.bricks = vro.generate_bricks(self.vol, vro.UCHAR)
        self.prefix = vro.prefix_sum(np.ascontiguousarray(self.tff, dtype=np.uint8).reshape(-1))
        self._vr, self._taken = {}, {}

    def vr(self, group=64, env=()):
        key = (group,) + tuple(env)
        if key not in self._vr:
            with pytest.MonkeyPatch.context() as mp:
                if group != 64:
                    mp.setenv("VRHIP_PM_GROUP", str(group))
                for k, v in env:
                    mp.setenv(k, v)
                r = VolumeRenderCL()
                r.initialize()
            _configure(r)
            self._vr[key] = r
        return self._vr[key]

    def close(self):
        for r in self._vr.values():
            r.close()

    def taken(self, W, H, seed, tile):
        """The oracle's samples_taken over the rays of `tile` (x0, y0, w, h) of the frame of `seed`."""
        key = (W, H, seed, tile)
        if key not in self._taken:
            cam, rp, rc, pt = common.to_oracle_params(*self.vr().params())
            rp.seed, rp.iteration = seed, 0
            self._taken[key] = vro.render_tile(self.vol, vro.UCHAR, self.tff, cam, rp, rc, pt, use_ess=True, W=W, H=H,
                                               tile=tile, bricks=self.bricks, prefix=self.prefix,
                                               threads=1)[1]["samples_taken"]
        return self._taken[key]

    def patch_taken(self, W, H, seed, col, row):
        return self.taken(W, H, seed, (8 * col, 8 * row, min(8, W - 8 * col), min(8, H - 8 * row)))

    def ray_live(self, W, H, seed, gx, gy):
        return self.taken(W, H, seed, (gx, gy, 1, 1)) > 0


@pytest.fixture(scope="module")
def scene():
    s = Scene()
    yield s
    s.close()


def _render(r, W, H, seeds, **kw):
    import torch
    ids = kw.get("tile_ids")
    shape = (len(seeds), H, W, 4) if ids is None else (len(seeds), len(ids), kw["tile_h"], kw["tile_w"], 4)
    out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
    r.render_batch(W, H, seeds, out.data_ptr(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _guard(s, W, H, seeds, patches):
    """The vacuity guard, on the inputs alone (the oracle, on the CPU): among `patches` (column, row) the set has a
    patch dead in every frame, one with all 64 pixels live in every frame, one live in some frames only and -- where
    the frame's edges cut patches at all (36 x 28; 64 x 48 is whole patches) -- one cut by the edge with live rays."""
    live = {p: [s.patch_taken(W, H, sd, *p) > 0 for sd in seeds] for p in patches}
    assert any(not any(v) for v in live.values()), "no patch is dead in every frame"
    assert any(any(v) and not all(v) for v in live.values()), "no patch is live in some frames only: choose other seeds"
    whole = lambda p: 8 * p[0] + 8 <= W and 8 * p[1] + 8 <= H
    if W % 8 or H % 8:
        assert any(not whole(p) and any(v) for p, v in live.items()), "no patch cut by the frame edge has a live ray"

    def full(p):
        return all(s.ray_live(W, H, sd, 8 * p[0] + x, 8 * p[1] + y) for sd in seeds for y in range(8) for x in range(8))
    assert any(whole(p) and all(v) and full(p) for p, v in live.items()), "no patch has all 64 pixels live in every frame"


def _check_order(ro, W, H, sf, group, want_patches=None):
    """Assertions 1-4 of the module on one downloaded ray order; returns {(gx, gy, frame)} of the live rays."""
    n, cap, icap = ro["n_items"], ro["live_list_cap"], ro["pm_list_cap"]
    assert ro["set_frames"] == sf and ro["group"] == group and n % sf == 0
    assert cap == ror.live_list_cap(n) and icap == ror.pm_list_cap(n, sf)
    items, ballot, first = ro["items"], ro["ballot"], ro["first"]
    n_patches = n // sf
    # the queue: item q = patch * sf + frame, every patch of the frame (or of the tiles asked for) once
    assert np.array_equal(items[:, 2], np.tile(np.arange(sf), n_patches))
    patch_of = items[::sf, :2]
    assert np.array_equal(items[:, :2], np.repeat(patch_of, sf, axis=0))
    patches = [tuple(int(v) for v in p) for p in patch_of]
    assert len(set(patches)) == n_patches
    if want_patches is None:
        want_patches = {(c, r) for c in range((W + 7) // 8) for r in range((H + 7) // 8)}
    assert set(patches) == set(want_patches)

    # ---- 1. records against notes
    for k in range(ror.LISTS):
        assert ro["ray_counts"][k] <= cap and len(ro["records"][k]) == ro["ray_counts"][k], k
        assert np.array_equal(ro["records"][k][:, 3], k * cap + np.arange(ro["ray_counts"][k]))
    recs = np.concatenate(ro["records"])
    rec_at = np.full(ror.LISTS * cap, -1, dtype=np.int64)
    rec_at[recs[:, 3]] = np.arange(len(recs))
    pops = np.array([ror.popcount(b) for b in ballot], dtype=np.int64)
    assert sum(ro["ray_counts"]) == int(pops.sum()) == len(recs)
    for k in range(ror.LISTS):   # (list q % 8 takes item q's records)
        assert ro["ray_counts"][k] == int(pops[k::ror.LISTS].sum()), k
    bits = np.arange(64)
    live_rays = set()
    for q in range(n):
        if not pops[q]:
            continue
        col, row, f = (int(v) for v in items[q])
        px = bits[[(int(ballot[q]) >> int(b)) & 1 == 1 for b in bits]]
        # the pre-pass's lane px handles pixel (8 col + (px & 7), 8 row + (px >> 3)): ror.pixel_of_bit
        gx, gy = 8 * col + (px & 7), 8 * row + (px >> 3)
        assert (gx < W).all() and (gy < H).all(), "item %d: a ballot bit outside the frame" % q
        at = int(first[q])
        assert at // cap == q % ror.LISTS and (at + pops[q] - 1) // cap == q % ror.LISTS, q
        assert (rec_at[at:at + pops[q]] >= 0).all(), q
        got = recs[rec_at[at:at + pops[q]]]
        want = np.stack([gx, gy, np.full(len(px), f), at + np.arange(len(px))], axis=1)
        assert np.array_equal(got, want), "item %d (patch %d %d, frame %d): records\n%s\nwant\n%s" % (q, col, row, f, got, want)
        live_rays.update((int(x), int(y), f) for x, y in zip(gx, gy))
    assert len(live_rays) == len(recs)

    # ---- 2. the index against the restatement
    runs = ror.expected_runs(sf, ballot, first, group)
    assert set(runs) == {p for p in range(n_patches) if pops[p * sf:(p + 1) * sf].any()}
    named = []
    for k in range(ror.LISTS):
        mine = {p: r for p, r in runs.items() if p % ror.LISTS == k}
        entries = ro["index"][k]
        assert ro["index_counts"][k] <= icap, "index list %d: counter %d beyond pm_list_cap %d" % (k, ro["index_counts"][k], icap)
        assert len(entries) == ro["index_counts"][k] == sum(len(r) for r in mine.values()), \
            "index list %d: counter %d, the padded runs of its patches have %d entries" % (
                k, ro["index_counts"][k], sum(len(r) for r in mine.values()))
        order = ror.split_runs(entries, mine)
        assert sorted(order) == sorted(mine), "index list %d: runs of patches %s, live patches %s" % (k, order, sorted(mine))
        # (padding only at a run's end and up to a multiple of the group: that is the restatement's run)
        at = 0
        for p in order:
            run = entries[at:at + len(mine[p])]
            at += len(run)
            assert len(run) % group == 0
            real = run[run != ror.PM_NONE]
            assert (run[:len(real)] != ror.PM_NONE).all() and len(run) - len(real) < group
            # ---- 4. pixel-major within the run: (pixel, frame) strictly increasing, pixel first
            assert (rec_at[real] >= 0).all()
            r = recs[rec_at[real]]
            col, row = patches[p]
            key = ((r[:, 1] - 8 * row) * 8 + (r[:, 0] - 8 * col)) * sf + r[:, 2]
            assert ((r[:, 0] >> 3) == col).all() and ((r[:, 1] >> 3) == row).all(), "patch %d: a run mixes patches" % p
            assert (np.diff(key) > 0).all(), "patch %d: the run is not in pixel-major order" % p
            named.append(real)
    # ---- 3. permutation: the index names every live record exactly once
    named = np.concatenate(named) if named else np.zeros(0, np.uint32)
    assert len(named) == len(recs) and np.array_equal(np.sort(named.astype(np.int64)), np.sort(recs[:, 3]))
    return live_rays


@pytest.mark.parametrize("size,sf,group", CASES)
def test_ray_order_of_a_set(scene, size, sf, group):
    s = scene
    (W, H), seeds = size, SEEDS[:sf]
    r = s.vr(group)
    _guard(s, W, H, seeds, [(c, q) for c in range((W + 7) // 8) for q in range((H + 7) // 8)])
    _render(r, W, H, seeds)
    li = r.lastLaunchInfo()
    assert li["pixel_major"] == 1 and li["ray_list"] == 1 and li["frames"] == sf, li
    ro = r.downloadRayOrder()
    again = r.downloadRayOrder()                                       # (the download changes nothing)
    assert np.array_equal(ro["notes"], again["notes"]) and ro["index_counts"] == again["index_counts"]
    _check_order(ro, W, H, sf, group)


def test_ray_order_of_a_tile_subset(scene):
    """A rank's share of the frame: the queue holds the patches of the listed tiles only (16 x 16 tiles of the 36 x 28
    frame: three by two; the right column and the bottom row are cut)."""
    s = scene
    (W, H), sf, T = SMALL, 5, 16
    seeds = SEEDS[:sf]
    ids = np.array([5, 1, 2, 4], dtype=np.uint32)
    split = tiles.TileSplit(W, H, T, T, 1, 0)
    patches = set()
    for t in ids:
        x0, y0, w, h = split.tile_rect(int(t))
        patches |= {(c, q) for c in range(x0 // 8, (x0 + w + 7) // 8) for q in range(y0 // 8, (y0 + h + 7) // 8)}
    assert len(patches) < ((W + 7) // 8) * ((H + 7) // 8)
    _guard(s, W, H, seeds, sorted(patches))
    r = s.vr()
    _render(r, W, H, seeds, tile_w=T, tile_h=T, tile_ids=ids)
    assert r.lastLaunchInfo()["pixel_major"] == 1
    _check_order(r.downloadRayOrder(), W, H, sf, 64, want_patches=patches)


def test_liveness_against_the_oracle(scene):
    """A ray is in the lists exactly when the oracle, rendering that pixel alone with that seed, takes a sample: the
    pre-pass keeps a ray that reaches a brick the ESS bitmap does not skip, and such a brick's segment is at least one
    step long (dda_step clamps its end to t + stepSize), so the oracle's inner loop runs at least once there."""
    s = scene
    (W, H), sf = SMALL, 5
    seeds = SEEDS[:sf]
    r = s.vr()
    _render(r, W, H, seeds)
    live = _check_order(r.downloadRayOrder(), W, H, sf, 64)
    want = {(x, y, f) for f, sd in enumerate(seeds) for y in range(H) for x in range(W) if s.ray_live(W, H, sd, x, y)}
    assert want, "the oracle takes no sample at all"
    assert not want - live, "live by the oracle, missing from the ray lists: %s" % sorted(want - live)[:10]
    assert not live - want, "in the ray lists, no sample by the oracle: %s" % sorted(live - want)[:10]


def test_no_ray_order_without_a_pixel_major_set(scene, monkeypatch):
    s = scene
    (W, H), seeds = SMALL, SEEDS[:5]
    r = s.vr()

    def nodata(vr):
        rc = vr._lib.vrhip_download_ray_order(vr._h, (C.c_uint32 * 8)(), None, 0, None, 0, None, None, 0, None, 0)
        with pytest.raises(RuntimeError):
            vr.downloadRayOrder()
        return rc == 3                                                 # VRHIP_ERR_NODATA

    _render(r, W, H, seeds)
    r.downloadRayOrder()
    # a frame alone
    r.setSeed(seeds[0])
    r.setIteration(0)
    r.runRaycastNoGL(W, H)
    assert nodata(r)
    _render(r, W, H, seeds)
    r.downloadRayOrder()
    # a set of one frame
    _render(r, W, H, seeds[:1])
    assert r.lastLaunchInfo()["pixel_major"] == 0 and nodata(r)
    # a camera per frame
    _render(r, W, H, seeds, views=[VIEW] * len(seeds))
    assert r.lastLaunchInfo()["pixel_major"] == 0 and nodata(r)
    _render(r, W, H, seeds)
    r.downloadRayOrder()
    # the instrumented kernels have no ray list
    r.setStatsEnabled(True)
    try:
        _render(r, W, H, seeds)
        assert r.lastLaunchInfo()["pixel_major"] == 0 and nodata(r)
    finally:
        r.setStatsEnabled(False)
    # VRHIP_PIXEL_MAJOR=0, and a renderer that has rendered nothing
    off = s.vr(env=(("VRHIP_PIXEL_MAJOR", "0"),))
    assert nodata(off)
    _render(off, W, H, seeds)
    assert off.lastLaunchInfo()["pixel_major"] == 0 and nodata(off)
