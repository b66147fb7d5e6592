"""Which ray-cast kernels a render call launches (vr_launch_raycast: format, ESS, statistics, the XS shading modes,
the footprint volume, per-frame cameras): every combination renders a tiny frame that equals the oracle's bit for
bit, and vrhip_last_launch_info names the variant the inputs imply."""
import itertools

import numpy as np
import pytest

from oracle import vro
from tests import common
from volumerenderercl_amd import FLOAT, UCHAR, USHORT, VolumeRenderCL

pytestmark = pytest.mark.gpu

RES = (16, 16, 16)
W, H = 32, 24
SEEDS = [3499211612, 581869302]
VIEWS = ["rot30", "close"]

# format x ESS x statistics x illumination (1: default shading, 2: an XS mode) x (one camera | two per-frame cameras),
# and one default frame of a renderer created with the footprint volume disabled
COMBOS = [c + (False,) for c in itertools.product((UCHAR, USHORT, FLOAT), (True, False), (False, True), (1, 2),
                                                   (False, True))]
COMBOS.append((UCHAR, True, False, 1, False, True))

_refs = {}


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


def _setup(r, vol, fmt, ess, stats, illum):
    r.loadVolumeArrays([vol], fmt)
    r.setTransferFunction(common.tffs()["default"])
    r.setIllumination(illum)
    r.setLinearInterpolation(True)
    r.setCamOrtho(False)
    r.setUseGradient(False)
    r.setContours(False)
    r.setAerial(False)
    r.setObjEss(ess)
    r.updateSamplingRate(1.5)
    r.setAmbientOcclusion(False)
    r.setTechnique(0)
    r.setBBox(-1, -1, -1, 1, 1, 1)
    r.setShowESS(False)
    r.setImgEss(False)
    r.params()[1].backgroundColor[:] = [1.0, 1.0, 1.0, 1.0]
    r.setStatsEnabled(stats)
    r.setSeed(SEEDS[0])
    r.updateView(common.views()[VIEWS[0]])
    r.setIteration(0)


def _oracle_frames(r, vol, fmt, ess, illum):
    """The oracle's frames of (VIEWS[f], SEEDS[f]), computed once per format, ESS and illumination."""
    key = (fmt, ess, illum)
    if key not in _refs:
        cam, rp, rc, pt = common.to_oracle_params(*r.params())
        frames = []
        for name, seed in zip(VIEWS, SEEDS):
            cam.viewMat[:] = common.views()[name]
            rp.seed, rp.iteration = seed, 0
            ref, _, _ = vro.render_tile(vol, fmt, common.tffs()["default"], cam, rp, rc, pt, use_ess=ess, W=W, H=H)
            ref.setflags(write=False)
            frames.append(ref)
        _refs[key] = frames
    return _refs[key]


def _render(r, views):
    if not views:
        return [r.runRaycastNoGL(W, H)]
    import torch
    out = torch.full((2, H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    r.render_batch(W, H, SEEDS, out.data_ptr(), views=[common.views()[n] for n in VIEWS])
    torch.cuda.synchronize()
    return list(out.cpu().numpy())


@pytest.mark.parametrize("fmt,ess,stats,illum,views,no_fp", COMBOS)
def test_launch_info_names_the_variant_the_inputs_imply(vr, monkeypatch, fmt, ess, stats, illum, views, no_fp):
    vol = vro.synth_volume("sphere", list(RES), fmt)
    r = vr
    if no_fp:
        monkeypatch.setenv("VRHIP_NO_FOOTPRINT", "1")
        r = VolumeRenderCL()
        r.initialize()
    try:
        _setup(r, vol, fmt, ess, stats, illum)
        refs = _oracle_frames(r, vol, fmt, ess, illum)
        got = _render(r, views)
        li = r.lastLaunchInfo()
    finally:
        if no_fp:
            r.close()
    assert np.ptp(refs[0][..., :3]) > 0.05   # the sphere is in the frame
    for f, frame in enumerate(got):
        assert np.array_equal(frame, refs[f]), "frame %d: max abs diff %.3g" % (f, np.abs(frame - refs[f]).max())
    # launch_typed: illumination 2 is one of the XS modes; the footprint volume serves the default kernels only
    # (no XS mode, no statistics)
    xs = illum >= 2
    fp = not xs and not stats and not no_fp
    # launch_variant: the DDA pre-pass runs with ESS in the un-instrumented kernels, its ray list feeds phase 1 of
    # the default ones; three waves per SIMD (12 per workgroup) with ESS on the footprint volume -- the ESS bricks of
    # a 16^3 volume are too small for the empty-run lookahead, so the renderer asks for them in both phases
    prepass = ess and not stats
    wide = ess and fp
    want = {"instrumented": int(stats), "extras": int(xs), "footprint": int(fp),
            "prepass": int(prepass), "ray_list": int(prepass and not xs),
            "phase1_waves": 12 if wide else 4, "phase2_waves": 12 if wide else 4}
    assert {k: li[k] for k in want} == want, li
