"""Pixel-major launch sets through every instantiation of phase 1 on the ray list, vr_raycast_rays_kernel<VT, SKIP_LDS,
FP, WAVES>: the three voxel types, the skip bitmap in LDS or not, the footprint volume or not, four or twelve waves;
through schedules that suspend and partly refill waves whose lanes hold rays of different frames; through the inputs
the pre-pass and the ray set-up read (orthographic camera, clip box, gradient background, environment map, a later time
step); and through sequences that reuse the index block and the alternating control blocks.

Every frame of a set equals the frame of its seed rendered alone on a default renderer, bit for bit; its first and
last frame meet the oracle (TOL); and the launch info is asserted -- pixel_major, ray_list and the phase1_waves,
footprint and skip_in_lds the case implies --, so a case that falls back to another kernel fails."""
import numpy as np
import pytest

from oracle import vro
from tests import common, scenes
from tests.test_gpu_float_range import _same as _float_same, _tff as _float_tff
from tests.test_gpu_parity import _env_map
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # the project's bound against the oracle (tests/test_gpu_pixel_major.py)
FMT_NAME = {UCHAR: "uchar", USHORT: "ushort", FLOAT: "float"}
_mt = frontend.Mt19937(4357)
SEEDS = [_mt() for _ in range(9)]
SIZES = {9: (100, 76), 3: (72, 56), 5: (72, 56)}
SEEN = {}                       # case id -> launch info: the instantiations the sweep has met (the last test)


# ---- scenes: name -> (volumes, format, transfer function, view, _setup keywords, environment map, time step)
def _scene(name):
    tff = common.tffs()["default"]
    if name in FMT_NAME.values():
        fmt = {v: k for k, v in FMT_NAME.items()}[name]
        res = {UCHAR: (48, 48, 48), USHORT: (44, 40, 48), FLOAT: (40, 48, 44)}[fmt]
        return [vro.synth_volume("shells", list(res), fmt)], fmt, tff, "rot30", {}, None, 0
    if name in ("beyond_unit", "nan"):
        # tests/test_gpu_float_range.py: values on both sides of [0, 1] ("straddle"), and a field sprinkled with NaN,
        # +-inf and +-3e38 ("specials"), with that file's transfer function (opaque, coloured edges)
        vol = scenes.float_volume({"beyond_unit": "straddle", "nan": "specials"}[name], (44, 40, 48), seed=30)
        return [vol], FLOAT, _float_tff(1024), "rot30", {}, None, 0
    shells = vro.synth_volume("shells", [48, 48, 48], UCHAR)
    if name == "ortho":
        return [shells], UCHAR, tff, "rot30", {"ortho": True}, None, 0
    if name == "clip":
        return [shells], UCHAR, tff, "rot30", {"bbox": (-0.6, -0.7, -0.5, 0.5, 0.8, 0.7)}, None, 0
    if name == "gradient":
        return [shells], UCHAR, tff, "rot30", {"gradient_bg": True, "background": (0.2, 0.5, 0.9, 1.0)}, None, 0
    if name == "envmap":
        return [shells], UCHAR, tff, "rot30", {}, _env_map(), 0
    if name == "step1":
        return [vro.synth_volume("sphere", [48, 48, 48], UCHAR), shells], UCHAR, tff, "rot30", {}, None, 1
    if name == "haze":
        return [shells], UCHAR, common.tffs()["haze"], "rot30", {}, None, 0
    raise KeyError(name)


class Sweep:
    """Renderers by environment (the switches are read when one is created), the scene each of them holds, the frames
    of the seeds rendered alone on the default renderer and the oracle's frames."""

    def __init__(self):
        self._vr, self._held, self._scenes, self._single, self._oracle, self._bricks = {}, {}, {}, {}, {}, {}

    def scene(self, name):
        if name not in self._scenes:
            self._scenes[name] = _scene(name)
        return self._scenes[name]

    def vr(self, env=()):
        if env not in self._vr:
            with pytest.MonkeyPatch.context() as mp:
                for k, v in env:
                    mp.setenv(k, v)
                r = VolumeRenderCL()
                r.initialize()
            self._vr[env] = r
        return self._vr[env]

    def hold(self, env, name):
        """The renderer of `env`, with scene `name` loaded."""
        r = self.vr(env)
        if self._held.get(env) != name:
            vols, fmt, tff, view, kw, envmap, step = self.scene(name)
            r.loadVolumeArrays(vols, fmt)
            _configure(r, tff, common.views()[view], kw)
            r.setEnvironmentMap(envmap)
            r.setTimestep(step)
            r.setStatsEnabled(False)
            r.setRoundBudget(10)
            self._held[env] = name
        return r

    def single(self, name, W, H, seed):
        key = (name, W, H, seed)
        if key not in self._single:
            r = self.hold((), name)
            r.setSeed(seed)
            r.setIteration(0)
            self._single[key] = r.runRaycastNoGL(W, H).copy()
            assert r.lastLaunchInfo()["pixel_major"] == 0
        return self._single[key]

    def oracle(self, name, W, H, seed):
        key = (name, W, H, seed)
        if key not in self._oracle:
            vols, fmt, tff, _, _, envmap, step = self.scene(name)
            if name not in self._bricks:
                self._bricks[name] = vro.generate_bricks(vols[step], fmt)
            cam, rp, rc, pt = common.to_oracle_params(*self.hold((), name).params())
            rp.seed, rp.iteration = seed, 0
            self._oracle[key] = vro.render_tile(vols[step], fmt, tff, cam, rp, rc, pt, use_ess=True, W=W, H=H,
                                                bricks=self._bricks[name], env=envmap)[0]
        return self._oracle[key]

    def close(self):
        for r in self._vr.values():
            r.close()


def _configure(r, tff, view, kw):
    """The state every case shares (tests/test_gpu_pixel_major.py), and what the scene's keywords change of it."""
    r.setTransferFunction(tff)
    r.setIllumination(1)
    r.setLinearInterpolation(True)
    r.setCamOrtho(kw.get("ortho", False))
    r.setUseGradient(kw.get("gradient_bg", False))
    r.setObjEss(True)
    r.updateSamplingRate(1.5)
    r.setBBox(*kw.get("bbox", (-1, -1, -1, 1, 1, 1)))
    if "background" in kw:
        r.setBackground(kw["background"])
    else:
        r.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    r.updateView(view)
    r.setIteration(0)


@pytest.fixture(scope="module")
def sweep():
    s = Sweep()
    yield s
    s.close()


def _batch(r, W, H, seeds):
    import torch
    out = torch.full((len(seeds), H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    r.render_batch(W, H, seeds, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _implied(r, env, n):
    """(phase1_waves, footprint, skip_in_lds) a set of n frames implies under `env` (fill_launch, launch_variant): the
    footprint volume unless switched off; twelve waves with it where VRHIP_OCC says so, else for sets of four frames and
    more and for volumes whose bricks are too small for the empty-run lookahead (edge below 16 voxels, as at these
    sizes: VRHIP_EMPTY_SKIP=1 turns the lookahead on all the same, and the three-frame set then runs four waves)."""
    env = dict(env)
    fp = 0 if env.get("VRHIP_NO_FOOTPRINT") else 1
    lookahead = bool(env.get("VRHIP_EMPTY_SKIP")) or max(r.brickInfo()[2]) >= 16
    three = int(env["VRHIP_OCC"]) == 3 if "VRHIP_OCC" in env else (n >= 4 or not lookahead)
    return (12 if fp and three else 4), fp, 0 if env.get("VRHIP_SKIP_GLOBAL") else 1


def _check_set(sweep, case_id, name, env, n, budget=None, nan=False):
    W, H = SIZES[n]
    seeds = SEEDS[:n]
    singles = [sweep.single(name, W, H, sd) for sd in seeds]
    r = sweep.hold(env, name)
    if budget is not None:
        r.setRoundBudget(budget)
    try:
        with pytest.MonkeyPatch.context() as mp:   # (VRHIP_SKIP_GLOBAL is read at every launch, the others at creation)
            for k, v in env:
                mp.setenv(k, v)
            got = _batch(r, W, H, seeds)
    finally:
        r.setRoundBudget(10)
    li = r.lastLaunchInfo()
    SEEN[case_id] = (FMT_NAME[sweep.scene(name)[1]], li)
    waves, fp, lds = _implied(r, env, n)
    assert li["pixel_major"] == 1 and li["ray_list"] == 1 and li["frames"] == n and li["views"] == 0, li
    assert (li["phase1_waves"], li["footprint"], li["skip_in_lds"]) == (waves, fp, lds), li
    assert li["empty_skip"] == (1 if dict(env).get("VRHIP_EMPTY_SKIP") else 0), li
    if budget is not None:
        assert li["round_budget"] == budget, li
    for f in range(n):
        if nan:
            np.testing.assert_array_equal(got[f], singles[f], err_msg="frame %d of %d" % (f, n))   # (NaN where NaN is)
        else:
            assert np.array_equal(got[f], singles[f]), "frame %d of %d: max abs difference %g" % (
                f, n, float(np.abs(got[f] - singles[f]).max()))
    assert not np.array_equal(got[0], got[1])                          # (the seeds do move the rays)
    for f in (0, n - 1):
        ref = sweep.oracle(name, W, H, seeds[f])
        if nan:
            _float_same(got[f], ref, "frame %d against the oracle" % f)
        else:
            assert float(np.abs(got[f] - ref).max()) <= TOL, "frame %d against the oracle" % f
    return got


INSTANTIATIONS = [
    ((), 3), ((), 9),
    ((("VRHIP_NO_FOOTPRINT", "1"),), 9),
    ((("VRHIP_SKIP_GLOBAL", "1"),), 3), ((("VRHIP_SKIP_GLOBAL", "1"),), 9),
    ((("VRHIP_NO_FOOTPRINT", "1"), ("VRHIP_SKIP_GLOBAL", "1")), 3),
    ((("VRHIP_OCC", "2"),), 9), ((("VRHIP_OCC", "3"),), 3),
    ((("VRHIP_OCC", "2"), ("VRHIP_SKIP_GLOBAL", "1")), 9),
    ((("VRHIP_EMPTY_SKIP", "1"),), 3), ((("VRHIP_EMPTY_SKIP", "1"),), 9),
]


def _env_id(env):
    return "+".join("%s=%s" % (k[6:].lower(), v) for k, v in env) or "default"


@pytest.mark.parametrize("env,n", INSTANTIATIONS, ids=lambda v: _env_id(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("name", ["uchar", "ushort", "float"])
def test_voxel_types_through_every_instantiation(sweep, name, env, n):
    _check_set(sweep, "%s %s n=%d" % (name, _env_id(env), n), name, env, n)


@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("name", ["beyond_unit", "nan"])
def test_float_values_beyond_unit_and_non_finite(sweep, name, n):
    got = _check_set(sweep, "%s n=%d" % (name, n), name, (), n, nan=True)
    if name == "nan":
        assert np.isnan(got).any()                                     # (the palette does reach the pixels)


SCHEDULES = [((), 1), ((), 3), ((("VRHIP_REFILL_MIN", "1"),), None), ((("VRHIP_REFILL_MIN", "5"),), None),
             ((("VRHIP_REFILL_MIN", "1"),), 3), ((("VRHIP_NO_SORT", "1"),), 3)]


@pytest.mark.parametrize("env,budget", SCHEDULES,
                         ids=["budget1", "budget3", "refill1", "refill5", "refill1+budget3", "nosort+budget3"])
@pytest.mark.parametrize("name", ["uchar", "float"])
@pytest.mark.parametrize("n", [3, 9])
def test_schedules_that_suspend_and_partly_refill(sweep, n, name, env, budget):
    """A round budget of 1 or 3 suspends most rays to phase 2 from waves whose neighbouring lanes hold the same pixel in
    different frames; VRHIP_REFILL_MIN 1 / 5 refills 4 / 20 idle lanes at a time instead of whole waves, so a wave draws
    index entries that start and end inside a patch's run."""
    _check_set(sweep, "%s %s budget=%s n=%d" % (name, _env_id(env), budget, n), name, env, n, budget=budget)
    if budget is not None:
        assert SEEN["%s %s budget=%s n=%d" % (name, _env_id(env), budget, n)][1]["phase2_waves"] != 0


@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("name", ["ortho", "clip", "gradient", "envmap", "step1"])
def test_inputs_of_the_prepass_and_the_ray_setup(sweep, name, n):
    got = _check_set(sweep, "%s n=%d" % (name, n), name, (), n)
    if name in ("gradient", "envmap"):
        # the dead pixels' colour is the pre-pass's to write and depends on the pixel: not one colour
        assert len(np.unique(got[0][0, :, :3], axis=0)) > 1


def test_sequences_on_one_renderer(sweep):
    """9 frames, 3, one alone, 9 again; then the same set after a new transfer function and after a viewport change:
    the index block and the two control blocks are reused, grown and shrunk."""
    r = sweep.hold((), "uchar")
    (W, H), (w, h) = SIZES[9], SIZES[3]

    def same(name, W, H, n):
        got = _batch(sweep.hold((), name), W, H, SEEDS[:n])
        assert r.lastLaunchInfo()["pixel_major"] == (1 if n > 1 else 0)
        for f in range(n):
            assert np.array_equal(got[f], sweep.single(name, W, H, SEEDS[f])), (name, W, H, n, f)
        return got

    first = same("uchar", W, H, 9)
    same("uchar", W, H, 3)
    r.setSeed(SEEDS[4])
    r.setIteration(0)
    assert np.array_equal(r.runRaycastNoGL(W, H), first[4])
    again = same("uchar", W, H, 9)
    assert np.array_equal(again, first)
    singles = [sweep.single("haze", W, H, sd) for sd in SEEDS[:9]]     # (on the same renderer: it holds "haze" now ...)
    sweep.hold((), "uchar")
    r.setTransferFunction(sweep.scene("haze")[2])                      # (... and here by a new transfer function alone)
    sweep._held[()] = "haze"
    hazy = same("haze", W, H, 9)
    assert all(np.array_equal(a, b) for a, b in zip(hazy, singles))
    assert not np.array_equal(hazy, first)
    same("haze", w, h, 9)
    same("haze", W, H, 9)
    assert np.array_equal(same("uchar", W, H, 9), first)


def test_rgba8_set_equals_the_quantised_float_set(sweep):
    import torch
    r = sweep.hold((), "uchar")
    W, H = SIZES[5]
    seeds = SEEDS[:5]
    want = frontend.quantise_rgba8(_batch(r, W, H, seeds))
    assert r.lastLaunchInfo()["pixel_major"] == 1
    out = torch.zeros((5, H, W, 4), dtype=torch.uint8, device="cuda")
    got = r.render_batch(W, H, seeds, rgba8=True, out=out)
    torch.cuda.synchronize()
    assert r.lastLaunchInfo()["pixel_major"] == 1 and r.lastLaunchInfo()["frames"] == 5
    assert np.array_equal(got.cpu().numpy(), want)


def test_every_instantiation_was_met(sweep, capsys):
    """Each voxel type with the footprint volume at four and at twelve waves and without it at four, each with the skip
    bitmap in LDS and not -- all with pixel_major == 1.  (The cases above have left their launch info in SEEN; run alone,
    this test renders them itself.)"""
    for name in ("uchar", "ushort", "float"):
        for env, n in INSTANTIATIONS:
            case_id = "%s %s n=%d" % (name, _env_id(env), n)
            if case_id not in SEEN:
                _check_set(sweep, case_id, name, env, n)
    met = {(fmt, li["skip_in_lds"], li["footprint"], li["phase1_waves"]) for fmt, li in SEEN.values() if li["pixel_major"] == 1}
    with capsys.disabled():
        for case_id, (fmt, li) in sorted(SEEN.items()):
            print("\n%-40s VT=%-6s SKIP_LDS=%d FP=%d WAVES=%-2d pixel_major=%d ray_list=%d round_budget=%d phase2_waves=%d" % (
                case_id, fmt, li["skip_in_lds"], li["footprint"], li["phase1_waves"], li["pixel_major"], li["ray_list"],
                li["round_budget"], li["phase2_waves"]), end="")
    want = {(fmt, lds, fp, waves) for fmt in FMT_NAME.values() for lds in (0, 1) for fp, waves in ((1, 4), (1, 12), (0, 4))}
    assert want <= met, sorted(want - met)
