"""One long-lived renderer walks through every cause that invalidates derived host state (voxels of a
step written, volumes cleared, volumes shared, time step changed, transfer function changed, bricks
built, plus viewport, technique and ESS switches).  After each step its frame is compared with the
frame of a FRESH renderer put directly into that state.  The same kernels render both frames, so they
are equal bit for bit (np.array_equal) unless stale state -- a skip bitmap, cell bounds, empty bits, a
footprint volume, patch classes of an earlier state -- leaks through.

Sizes are small and no multiple of 4 or 8, so brick, cell and patch rims are present.  Stats are off:
these are the production kernels, and the footprint volume is used with stats off only.
"""
import ctypes

import numpy as np
import pytest

from tests import common
from volumerenderercl_amd import FLOAT, UCHAR, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu

SEED = 3499211612
BIG, TALL = (72, 56), (40, 88)
RES_U, RES_F = (40, 36, 44), (24, 50, 33)

VOLS = {
    "u0": common.noise_volume(RES_U, UCHAR, seed=71, smooth=False),
    "u1": common.noise_volume(RES_U, UCHAR, seed=72, smooth=True),
    "u2": (common.noise_volume(RES_U, UCHAR, seed=73, smooth=False)[::-1, :, ::-1] // 2).copy(),
    "f0": common.noise_volume(RES_F, FLOAT, seed=74, smooth=False),
}
FMT = {"u0": UCHAR, "u1": UCHAR, "u2": UCHAR, "f0": FLOAT}
RES = {"u0": RES_U, "u1": RES_U, "u2": RES_U, "f0": RES_F}
TFFS = {
    "tf1": frontend.opaque_ramp_tff(),            # transparent below 0.25
    "tf2": frontend.haze_tff(),                   # transparent below 0.05
    "tf1_256": frontend.opaque_ramp_tff(n=256),   # another number of entries
    "tf3": frontend.tff_from_stops(),
}

_FRESH = {}   # state -> the fresh renderer's frame (many steps of the walk return to a state)


def _configure(r):
    for name, val in (("setIllumination", 1), ("setAmbientOcclusion", False), ("setShowESS", False),
                      ("setImgEss", False), ("setContours", False), ("setAerial", False), ("setCamOrtho", False),
                      ("setUseGradient", False), ("setLinearInterpolation", True)):
        getattr(r, name)(val)
    r.updateSamplingRate(1.5)
    r.setExtinction(100.0)
    r.updateView(common.views()["rot30"])
    r.setStatsEnabled(False)


def _frame(r, size):
    r.setSeed(SEED)
    r.setIteration(0)
    return r.runRaycastNoGL(*size)


def _upload_in_place(r, name, step):
    """Other voxels into an existing time step (no clear), then the bricks again."""
    v = np.ascontiguousarray(VOLS[name])
    r._check(r.lib.vrhip_upload_volume(r.handle, v.ctypes.data_as(ctypes.c_void_p),
                                       (ctypes.c_uint32 * 3)(*RES[name]), FMT[name], step))
    r._generate_bricks()


def _upload_other_size(r, name):
    """A volume of another size and format over the loaded ones, without clearing them first."""
    v = np.ascontiguousarray(VOLS[name])
    r._check(r.lib.vrhip_upload_volume(r.handle, v.ctypes.data_as(ctypes.c_void_p),
                                       (ctypes.c_uint32 * 3)(*RES[name]), FMT[name], 0))
    r._timestep = 0
    r._finish_load(RES[name], 1, FMT[name], (1.0, 1.0, 1.0))


class State:
    def __init__(self, vols, tff="tf1", step=0, tech=0, ess=True, size=BIG):
        self.vols, self.tff, self.step, self.tech, self.ess, self.size = tuple(vols), tff, step, tech, ess, size

    def key(self, forced):
        return (self.vols, self.tff, self.step, self.tech, self.ess, self.size, forced)


def _fresh_frame(st, forced):
    """The frame of a new renderer put directly into state `st` (created under the environment of the caller)."""
    key = st.key(forced)
    if key not in _FRESH:
        r = VolumeRenderCL()
        r.initialize()
        try:
            r.loadVolumeArrays([VOLS[n] for n in st.vols], FMT[st.vols[0]])
            _configure(r)
            r.setTransferFunction(TFFS[st.tff])
            r.setTechnique(st.tech)
            r.setObjEss(st.ess)
            r.setTimestep(st.step)
            _FRESH[key] = _frame(r, st.size)
        finally:
            r.close()
    return _FRESH[key]


class Walk:
    """A renderer and the state it is meant to be in."""

    def __init__(self, vols, forced=False):
        self.forced = forced
        self.r = VolumeRenderCL()
        self.r.initialize()
        self.st = State(vols)
        self.r.loadVolumeArrays([VOLS[n] for n in vols], FMT[vols[0]])
        _configure(self.r)
        self.r.setTransferFunction(TFFS["tf1"])     # (uploads the TF, builds the bricks, sets the prefix sum)
        self.r.setTechnique(0)
        self.r.setObjEss(True)
        self.seen = []

    def close(self):
        self.r.close()

    def check(self, label, frames=1):
        """`frames` frames in the current state; the last one equals the fresh renderer's."""
        for _ in range(frames):
            got = _frame(self.r, self.st.size)
        want = _fresh_frame(self.st, self.forced)
        assert np.isfinite(got).all(), label
        assert np.array_equal(got, want), "%s: max |walked - fresh| = %g" % (label, np.abs(got - want).max())
        self.seen.append(want)
        return got

    def tff(self, name):
        self.r.setTransferFunction(TFFS[name])
        self.st.tff = name

    def step(self, t):
        self.r.setTimestep(t)
        self.st.step = t

    def overwrite(self, t, name):
        _upload_in_place(self.r, name, t)
        v = list(self.st.vols)
        v[t] = name
        self.st.vols = tuple(v)

    def technique(self, tech):
        self.r.setTechnique(tech)
        self.st.tech = tech

    def ess(self, on):
        self.r.setObjEss(on)
        self.st.ess = on

    def size(self, s):
        self.st.size = s

    def ess_off_and_on(self):
        """Step 6: without ESS bricks the cells' empty bits carry the skipping (ray_skip_empty)."""
        self.ess(False)
        self.check("ESS off")
        self.tff("tf2")
        self.check("ESS off, TF edit")
        self.tff("tf1")
        self.check("ESS off, TF back")
        self.ess(True)
        self.check("ESS on again")


def test_one_renderer_walks_through_every_cause_of_invalidation():
    w = Walk(["u0", "u1"])
    try:
        # 1. a frame; three frames in a row on one step of a time series build the footprint volume and use it
        w.check("first frame")
        w.check("footprint volume of step 0", frames=3)
        w.check("with the footprint volume")
        # 2. the other time step: plain layout first, its own footprint volume after three frames
        w.step(1)
        w.check("step 1, first frame")
        w.check("step 1, footprint volume", frames=3)
        w.step(0)
        w.check("back on step 0")
        # 3. transfer functions: another transparent range, another number of entries and back
        w.tff("tf2")
        w.check("TF 2")
        w.tff("tf1_256")
        w.check("TF of 256 entries")
        w.tff("tf1")
        w.check("TF of 1024 entries")
        # 4. step 1 overwritten in place while step 0 is shown, bricks rebuilt
        w.overwrite(1, "u2")
        w.step(1)
        w.check("step 1 overwritten")
        w.step(0)
        w.check("step 0 after the overwrite")
        # 5. path tracer (opacity bounds of the cells), a TF edit under it, and back
        w.technique(1)
        w.check("path tracer")
        w.tff("tf3")
        w.check("path tracer, TF edit")
        w.technique(0)
        w.check("ray caster again")
        w.tff("tf1")
        # 6. ESS off: the empty bits
        w.ess_off_and_on()
        # 7. viewport
        w.size(TALL)
        w.check("viewport 40x88")
        w.size(BIG)
        w.check("viewport 72x56 again")
        # 8. a volume of the other size and format over the loaded ones
        _upload_other_size(w.r, "f0")
        w.st.vols, w.st.step = ("f0",), 0
        w.tff("tf2")
        w.check("FLOAT volume of another size")
        w.technique(1)
        w.check("FLOAT volume, path tracer")
        w.technique(0)
        # 10. clear, upload again
        w.r.loadVolumeArrays([VOLS["u1"], VOLS["u0"]], UCHAR)
        w.st.vols = ("u1", "u0")
        w.tff("tf1")
        w.step(1)
        w.check("after clear and upload")
        w.ess(False)
        w.check("after clear and upload, ESS off")
        # the walk has been through states whose frames differ (else it would prove nothing)
        assert len({f.tobytes() for f in w.seen}) >= 12
    finally:
        w.close()


def test_empty_bits_forced_on_follow_transfer_function_and_voxels(monkeypatch):
    """Step 6 on a renderer created with VRHIP_EMPTY_SKIP=1 (the fresh ones too): the empty bits are used with
    ESS bricks of any size, next to the skip bitmap."""
    monkeypatch.setenv("VRHIP_EMPTY_SKIP", "1")
    w = Walk(["u0", "u1"], forced=True)
    try:
        w.check("forced, first frame")
        w.tff("tf2")
        w.check("forced, TF edit with ESS")
        w.tff("tf1")
        w.ess_off_and_on()
        w.step(1)
        w.check("forced, step 1")
        w.overwrite(1, "u2")
        w.check("forced, step 1 overwritten")
    finally:
        w.close()


def test_twin_renderers_walk():
    """Step 9: a second renderer on the first one's voxels."""
    w = Walk(["u0", "u1"])
    twin = None
    try:
        a = w.check("owner")
        twin = w.r.shareVolumes()
        ts = State(w.st.vols)

        def twin_check(label):
            got = _frame(twin, ts.size)
            want = _fresh_frame(ts, False)
            assert np.array_equal(got, want), "twin, %s: max diff %g" % (label, np.abs(got - want).max())
            return got

        assert np.array_equal(twin_check("shared"), a)
        # the owner overwrites the step both show; the twin takes the rebuilt bricks (its own vrhip_build_bricks,
        # without which it reports that they are not built) and derives everything else anew
        w.overwrite(0, "u2")
        ts.vols = w.st.vols
        twin._generate_bricks()
        b = twin_check("owner overwrote step 0")
        assert not np.array_equal(a, b)
        w.check("owner after its overwrite")
        # the owner's TF is the owner's
        w.tff("tf2")
        assert np.array_equal(twin_check("owner edited its TF"), b)
        w.check("owner with TF 2")
        # the twin's time step is the twin's
        twin.setTimestep(1)
        ts.step = 1
        twin_check("its own time step")
        w.check("owner still on step 0")
        # a volume of another size: the twin is detached
        _upload_other_size(w.r, "f0")
        w.st.vols, w.st.step = ("f0",), 0
        w.tff("tf2")
        with pytest.raises(RuntimeError, match="No volume data is loaded."):
            _frame(twin, ts.size)
        w.check("owner with the FLOAT volume")
    finally:
        if twin is not None:
            twin.close()
        w.close()
