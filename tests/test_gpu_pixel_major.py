"""Pixel-major ray order of a launch set (vrhip_render_batch, >= 2 frames of one camera): phase 1 draws the set's rays
pixel by pixel across its frames through an index behind the pre-pass (vr_regroup_kernel).  A schedule, not a result:
every frame of a set equals the frame of its seed rendered alone, bit for bit, and the oracle's; whole frames and tile
shares; the knob and the launch info say which order ran."""
import numpy as np
import pytest

from oracle import vro
from tests import common
from volumerenderercl_amd import UCHAR, VolumeRenderCL, frontend, tiles

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # the project's bound against the oracle
RES = (64, 64, 64)
FIELDS = ("sphere", "shells")
# set sizes around the eight index lists' turn (2, 5: below; 8: one turn; 9: above), the benchmark's 32, the largest set
CASES = [((128, 128), n) for n in (2, 5, 8, 9, 32)] + [((100, 76), n) for n in (2, 5, 8, 9, 32)] + [((64, 64), 256)]

_mt = frontend.Mt19937(4357)
SEEDS = [_mt() for _ in range(256)]


def _configure(r, kind):
    r.loadVolumeArrays([vro.synth_volume(kind, list(RES), vro.UCHAR)], UCHAR)
    r.setTransferFunction(common.tffs()["default"])
    r.setIllumination(1)
    r.setLinearInterpolation(True)
    r.setCamOrtho(False)
    r.setObjEss(True)
    r.updateSamplingRate(1.5)
    r.setBBox(-1, -1, -1, 1, 1, 1)
    r.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    r.setStatsEnabled(False)
    r.updateView(common.views()["rot30"])
    r.setIteration(0)


class Scene:
    """One renderer per field, with what the tests share: the frames of the seeds rendered alone and the oracle's."""

    def __init__(self, kind):
        self.kind = kind
        self.vol = vro.synth_volume(kind, list(RES), vro.UCHAR)
        self.tff = common.tffs()["default"]
        self.bricks = vro.generate_bricks(self.vol, vro.UCHAR)
        self.vr = VolumeRenderCL()
        self.vr.initialize()
        _configure(self.vr, kind)
        self._single, self._oracle = {}, {}

    def single(self, W, H, seed):
        key = (W, H, seed)
        if key not in self._single:
            self.vr.setStatsEnabled(False)
            self.vr.setSeed(seed)
            self.vr.setIteration(0)
            self._single[key] = self.vr.runRaycastNoGL(W, H).copy()
            assert self.vr.lastLaunchInfo()["pixel_major"] == 0   # a single frame keeps the pre-pass's order
        return self._single[key]

    def oracle(self, W, H, seed, tile=None):
        key = (W, H, seed, tile)
        if key not in self._oracle:
            cam, rp, rc, pt = common.to_oracle_params(*self.vr.params())
            rp.seed, rp.iteration = seed, 0
            img, stats, _ = vro.render_tile(self.vol, vro.UCHAR, self.tff, cam, rp, rc, pt, use_ess=True, W=W, H=H, tile=tile,
                                             bricks=self.bricks)
            self._oracle[key] = (img, stats)
        return self._oracle[key]

    def batch(self, W, H, seeds, vr=None, **kw):
        import torch
        vr = vr or self.vr
        ids = kw.get("tile_ids")
        shape = (len(seeds), H, W, 4) if ids is None else (len(seeds), len(ids), kw["tile_h"], kw["tile_w"], 4)
        out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
        vr.render_batch(W, H, seeds, out.data_ptr(), **kw)
        torch.cuda.synchronize()
        return out.cpu().numpy()


_scenes = {}


@pytest.fixture(scope="module")
def scene():
    def get(kind):
        if kind not in _scenes:
            _scenes[kind] = Scene(kind)
        return _scenes[kind]
    yield get
    for s in _scenes.values():
        s.vr.close()
    _scenes.clear()


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("size,n", CASES)
def test_every_frame_of_a_set_equals_its_seed_alone_and_the_oracle(scene, kind, size, n):
    s = scene(kind)
    (W, H), seeds = size, SEEDS[:n]
    singles = [s.single(W, H, sd) for sd in seeds]
    got = s.batch(W, H, seeds)
    li = s.vr.lastLaunchInfo()
    assert li["pixel_major"] == 1 and li["frames"] == n and li["ray_list"] == 1 and li["views"] == 0, li
    for f in range(n):
        d = float(np.abs(got[f] - singles[f]).max())
        assert d == 0.0, "frame %d of %d: max abs difference %g" % (f, n, d)
    assert not np.array_equal(got[0], got[1])                       # (the seeds do move the rays)
    # the oracle, frame by frame, and the six work counters of the set through the instrumented path
    want = dict.fromkeys(s.vr.getStats(), 0)
    for f, sd in enumerate(seeds):
        ref, rstats = s.oracle(W, H, sd)
        assert float(np.abs(got[f] - ref).max()) <= TOL, "frame %d against the oracle" % f
        for k in want:
            want[k] += rstats[k]
    s.vr.setStatsEnabled(True)
    try:
        inst = s.batch(W, H, seeds)
        assert s.vr.lastLaunchInfo()["instrumented"] == 1
        assert s.vr.getStats() == want
    finally:
        s.vr.setStatsEnabled(False)
    for f in range(n):
        assert np.array_equal(inst[f], singles[f]), "frame %d (instrumented)" % f


def test_patch_live_in_some_frames_and_dead_in_others(scene):
    """The rim of the outer shell crosses patch edges: for some 8x8 patches the jitter decides whether any ray meets a
    brick to sample.  Such a patch leaves index entries for a part of the set's frames only.  The oracle says (on the
    CPU) that the chosen seeds have one -- a patch where it takes samples in some frames and none in others -- before
    the set is compared."""
    s = scene("shells")
    W = H = 128
    seeds = SEEDS[:9]
    taken = np.array([[[s.oracle(W, H, sd, tile=(px * 8, py * 8, 8, 8))[1]["samples_taken"] for px in range(W // 8)]
                       for py in range(H // 8)] for sd in seeds])                          # [frame, patch row, patch column]
    live = taken > 0
    mixed = [(int(px), int(py)) for py, px in zip(*np.nonzero(live.any(axis=0) & ~live.all(axis=0)))]
    assert mixed, "no patch is live in some frames of the set and dead in others: choose other seeds"
    got = s.batch(W, H, seeds)
    assert s.vr.lastLaunchInfo()["pixel_major"] == 1
    for f, sd in enumerate(seeds):
        assert np.array_equal(got[f], s.single(W, H, sd)), f
        for px, py in mixed:
            ref = s.oracle(W, H, sd, tile=(px * 8, py * 8, 8, 8))[0]
            assert float(np.abs(got[f][py * 8:py * 8 + 8, px * 8:px * 8 + 8] - ref).max()) <= TOL, (f, px, py)


def test_knob_and_launch_info(scene, monkeypatch):
    s = scene("shells")
    W, H, seeds = 100, 76, SEEDS[:5]
    on = s.batch(W, H, seeds)
    assert s.vr.lastLaunchInfo()["pixel_major"] == 1
    # a camera per frame: the same pixel is not the same ray
    views = [common.views()["rot30"]] * len(seeds)
    per_view = s.batch(W, H, seeds, views=views)
    li = s.vr.lastLaunchInfo()
    assert li["views"] == 1 and li["pixel_major"] == 0, li
    assert np.array_equal(per_view, on)
    # a set of one frame, and a frame alone
    one = s.batch(W, H, seeds[:1])
    assert s.vr.lastLaunchInfo()["pixel_major"] == 0
    assert np.array_equal(one[0], on[0])
    s.single(W, H, seeds[0])
    assert s.vr.lastLaunchInfo()["pixel_major"] == 0
    # the knob, read when a renderer is created
    for value, want in (("0", 0), ("1", 1)):
        monkeypatch.setenv("VRHIP_PIXEL_MAJOR", value)
        r = VolumeRenderCL()
        r.initialize()
        try:
            _configure(r, "shells")
            got = s.batch(W, H, seeds, vr=r)
            assert r.lastLaunchInfo()["pixel_major"] == want
            assert np.array_equal(got, on), "VRHIP_PIXEL_MAJOR=%s" % value
        finally:
            r.close()
    monkeypatch.delenv("VRHIP_PIXEL_MAJOR")
    # every group size the index can be padded to
    for group in ("1", "32"):
        monkeypatch.setenv("VRHIP_PM_GROUP", group)
        r = VolumeRenderCL()
        r.initialize()
        try:
            _configure(r, "shells")
            got = s.batch(W, H, seeds, vr=r)
            assert r.lastLaunchInfo()["pixel_major"] == 1
            assert np.array_equal(got, on), "VRHIP_PM_GROUP=%s" % group
        finally:
            r.close()


@pytest.mark.parametrize("kind", FIELDS)
def test_tile_shares_of_a_set(scene, kind):
    """Two ranks' tile shares of a 5-frame set, each rendered on this device (a subset of the patches in the queue):
    the tiles of the whole-frame set, bit for bit."""
    s = scene(kind)
    W, H, T, seeds = 100, 76, 16, SEEDS[:5]
    whole = s.batch(W, H, seeds)
    seen = 0
    for rank in range(2):
        split = tiles.TileSplit(W, H, T, T, 2, rank)
        ids = np.asarray(split.my_tiles, dtype=np.uint32)
        got = s.batch(W, H, seeds, tile_w=T, tile_h=T, tile_ids=ids)
        assert s.vr.lastLaunchInfo()["pixel_major"] == 1
        for f in range(len(seeds)):
            for k, t in enumerate(ids):
                x0, y0, w, h = split.tile_rect(t)
                assert np.array_equal(got[f, k, :h, :w], whole[f][y0:y0 + h, x0:x0 + w]), (rank, f, int(t))
        seen += len(ids)
    assert seen == split.n_tiles
