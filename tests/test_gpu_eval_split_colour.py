"""The evaluation batch of the production kernels looks the transfer function's alpha up in eval_front and the colour
only for the samples the wave gathers (eval_dense; eval_back reads it from the slot).  The instrumented kernels keep
the one-piece eval_batch with the full lookup per sample: they are the control.

Volumes 20x12x9 and 33^3 in the three voxel types, with the footprint volume and without, a frame alone and a set of
three, round budgets 1 and 3 (both phases evaluate), through the 4-wave and the 12-wave marching kernels.  At these
sizes the ESS bricks are too small for the empty-run lookahead, and a renderer then runs twelve waves with the
footprint volume for single frames and sets alike; VRHIP_EMPTY_SKIP=1 turns the lookahead on, and frames alone and sets
of three run four waves.  The launch info is asserted per case, and the last test asserts that both were met.

Transfer functions:
  comb    alpha 0 on two table entries in four, 1 / 255 on the other two, opaque above 0.4: within a batch of four
          consecutive samples, samples whose two taps are both 0 (alpha exactly 0: no slot) sit next to samples with
          the smallest alpha the table can hold, and both next to lit ones; every entry has a colour of its own
  sparse  alpha only on the entries the volume's top half per cent of voxels read: the bricks that hold one are
          marched, and most waves in them gather nothing at all (n_slots == 0)
  dense   alpha 3 / 255 everywhere: every valid sample of a wave is gathered -- up to 256 slots, the dense loop's
          second to fourth pass -- and no ray ends early

Every production frame equals the instrumented kernels' frame of its seed bit for bit; that frame is within the
project's 1e-4 of the oracle and its six work counters equal the oracle's."""
import numpy as np
import pytest

from oracle import vro
from tests import common, scenes
from tests.test_gpu_float_range import _same as _float_same, _tff as _float_tff
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # the project's bound against the oracle
W, H = 52, 44                   # (patches cut by the right and the lower edge)
FMT_NAME = {UCHAR: "uchar", USHORT: "ushort", FLOAT: "float"}
_mt = frontend.Mt19937(4357)
SEEDS = [_mt() for _ in range(3)]
ENVS = [(), (("VRHIP_NO_FOOTPRINT", "1"),), (("VRHIP_EMPTY_SKIP", "1"),)]
MET = set()                     # (voxel type, footprint, phase1_waves, phase2_waves) of the launches below
SHADED = []                     # samples_shaded of the control frames, in the order they were rendered


def _unit(vol, fmt):
    return vol.astype(np.float64) / {UCHAR: 255.0, USHORT: 65535.0, FLOAT: 1.0}[fmt]


def _tff(name, vol, fmt, n=256):
    i = np.arange(n)
    t = np.zeros((n, 4), np.uint8)
    t[:, 0] = 20 + (i * 37) % 200
    t[:, 1] = 230 - (i * 53) % 190
    t[:, 2] = 15 + (i * 101) % 225
    if name == "comb":
        t[:, 3] = np.where(i % 4 < 2, 0, 1)
        t[i > 0.4 * n, 3] = 140
    elif name == "sparse":
        first = int(np.floor(np.quantile(_unit(vol, fmt), 0.995) * n))
        t[min(first, n - 1):, 3] = 255
    elif name == "dense":
        t[:, 3] = 3
    else:
        raise KeyError(name)
    return t


def _configure(r, tff):
    r.setTransferFunction(tff)
    r.setIllumination(1)
    r.setLinearInterpolation(True)
    r.setCamOrtho(False)
    r.setUseGradient(False)
    r.setObjEss(True)
    r.updateSamplingRate(1.5)
    r.setBBox(-1, -1, -1, 1, 1, 1)
    r.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    r.updateView(common.views()["rot30"])
    r.setIteration(0)


class Renderers:
    def __init__(self):
        self._vr = {}

    def get(self, env):
        if env not in self._vr:
            with pytest.MonkeyPatch.context() as mp:   # (the switches are read when a renderer is created)
                for k, v in env:
                    mp.setenv(k, v)
                r = VolumeRenderCL()
                r.initialize()
            self._vr[env] = r
        return self._vr[env]

    def close(self):
        for r in self._vr.values():
            r.close()


@pytest.fixture(scope="module")
def renderers():
    rs = Renderers()
    yield rs
    rs.close()


def _single(r, seed):
    r.setSeed(seed)
    r.setIteration(0)
    return r.runRaycastNoGL(W, H).copy()


def _batch(r, seeds):
    import torch
    out = torch.full((len(seeds), H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    r.render_batch(W, H, seeds, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _control(r, vol, fmt, tff, nan=False):
    """The instrumented kernels' frames of SEEDS (stats on), each held to the oracle: image and work counters."""
    frames = []
    bricks = vro.generate_bricks(vol, fmt)
    for seed in SEEDS:
        r.setStatsEnabled(True)
        got = _single(r, seed)
        stats = r.getStats()
        assert r.lastLaunchInfo()["instrumented"] != 0
        r.setIteration(0)
        cam, rp, rc, pt = common.to_oracle_params(*r.params())
        rp.seed, rp.iteration = seed, 0
        ref, rstats, _ = vro.render_tile(vol, fmt, tff, cam, rp, rc, pt, use_ess=True, W=W, H=H, bricks=bricks)
        if nan:
            _float_same(got, ref, "instrumented kernels against the oracle")
        else:
            err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
            assert err <= TOL, "instrumented kernels against the oracle: %g" % err
        assert stats == rstats, (stats, rstats)
        assert stats["samples_taken"] > 0
        frames.append(got)
        SHADED.append(stats["samples_shaded"])
    r.setStatsEnabled(False)
    return frames


def _implied_waves(r, env, n):
    """phase1_waves of a frame alone or a set of n < 4 frames (fill_launch, launch_variant): twelve with the footprint
    volume where the lookahead is off, else four."""
    env = dict(env)
    lookahead = bool(env.get("VRHIP_EMPTY_SKIP")) or max(r.brickInfo()[2]) >= 16
    return 12 if not env.get("VRHIP_NO_FOOTPRINT") and not lookahead else 4


def _check_case(renderers, vol, fmt, tff, nan=False):
    def same(got, want, what):
        if nan:
            np.testing.assert_array_equal(got, want, err_msg=what)   # (NaN where NaN is)
        else:
            assert np.array_equal(got, want), "%s: max abs difference %g" % (what, float(np.abs(got - want).max()))

    control = None
    for env in ENVS:
        r = renderers.get(env)
        r.loadVolumeArrays([vol], fmt)
        _configure(r, tff)
        r.setStatsEnabled(False)
        if control is None:
            control = _control(r, vol, fmt, tff, nan=nan)
            assert not np.array_equal(control[0], control[1])   # (the seeds do move the rays)
        try:
            for budget in (1, 3):
                r.setRoundBudget(budget)
                for n in (1, 3):
                    what = "%s budget %d, %d frame(s)" % (dict(env), budget, n)
                    got = [_single(r, SEEDS[0])] if n == 1 else _batch(r, SEEDS)
                    li = r.lastLaunchInfo()
                    assert li["instrumented"] == 0 and li["extras"] == 0 and li["ray_list"] == 1, (what, li)
                    assert li["footprint"] == (0 if dict(env).get("VRHIP_NO_FOOTPRINT") else 1), (what, li)
                    assert li["phase1_waves"] == _implied_waves(r, env, n), (what, li)
                    assert li["round_budget"] == budget and li["phase2_waves"] != 0, (what, li)
                    assert li["pixel_major"] == (1 if n > 1 else 0), (what, li)
                    MET.add((FMT_NAME[fmt], li["footprint"], li["phase1_waves"], li["phase2_waves"]))
                    for f in range(n):
                        same(got[f], control[f], "%s, frame %d against the instrumented kernels" % (what, f))
        finally:
            r.setRoundBudget(10)
    return control


def _volume(res, fmt):
    return common.noise_volume(res, fmt, seed=11, smooth=False)


@pytest.mark.parametrize("tff_name", ["comb", "sparse", "dense"])
@pytest.mark.parametrize("fmt", [UCHAR, USHORT, FLOAT], ids=lambda f: FMT_NAME[f])
@pytest.mark.parametrize("res", [(20, 12, 9), (33, 33, 33)], ids=lambda r: "x".join(map(str, r)))
def test_colour_of_gathered_samples_only(renderers, res, fmt, tff_name):
    vol = _volume(res, fmt)
    tff = _tff(tff_name, vol, fmt)
    del SHADED[:]
    control = _check_case(renderers, vol, fmt, tff)
    assert (np.abs(control[0][..., :3] - 1.0).max(axis=-1) > 0).any()   # (some pixels differ from the background)
    # lit samples (alpha above 0.1: gradient and shading terms on the colour) in "comb" and "sparse", none in "dense"
    assert all(s > 0 for s in SHADED) if tff_name != "dense" else not any(SHADED), SHADED


def test_float_volume_with_inf_and_nan_voxels(renderers):
    """scenes.float_volume("specials"): values on both sides of [0, 1], 3 % of the voxels NaN, +-inf, -0.0, denormals
    and +-3e38, with opaque coloured table edges -- what those voxels read.  Compared to the same control."""
    vol = scenes.float_volume("specials", (33, 33, 33), seed=30)
    _check_case(renderers, vol, FLOAT, _float_tff(1024), nan=True)


def test_four_and_twelve_waves_were_met(renderers):
    """Every voxel type through the 4-wave and the 12-wave phase 1 with the footprint volume and the 4-wave one
    without it.  (The cases above have left their launch info in MET; run alone, this test renders one case each.)"""
    if not MET:
        for fmt in (UCHAR, USHORT, FLOAT):
            vol = _volume((20, 12, 9), fmt)
            _check_case(renderers, vol, fmt, _tff("comb", vol, fmt))
    met1 = {m[:3] for m in MET}
    want = {(name, fp, waves) for name in FMT_NAME.values() for fp, waves in ((1, 4), (1, 12), (0, 4))}
    assert want <= met1, sorted(want - met1)
    assert {m[3] for m in MET} >= {4, 12}, sorted(MET)
