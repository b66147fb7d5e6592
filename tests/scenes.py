"""The parity scenes, shared by the GPU tests (HIP path vs oracle, tests/test_gpu_parity.py) and
the CPU tests (literal vs parity-definition oracle, tests/test_oracle_literal.py), and a
renderer-free builder of the four kernel-argument structs for them."""
import numpy as np

from oracle import vro
from tests import common
from volumerenderercl_amd import frontend

UCHAR, USHORT, FLOAT = 0, 1, 2
SEED = 3499211612


CASES = [
    # fmt, res, (W, H), view, tff, kwargs
    (UCHAR, (48, 48, 48), (96, 80), "default", "default", {}),
    (UCHAR, (48, 48, 48), (96, 80), "rot30", "default", {"ess": False}),
    (UCHAR, (64, 40, 52), (120, 72), "rot30", "opaque", {"gradient_bg": True}),
    (UCHAR, (33, 47, 29), (64, 64), "close", "haze", {"illum": 0}),
    (UCHAR, (48, 48, 48), (64, 64), "inside", "default", {}),
    (UCHAR, (48, 48, 48), (72, 56), "rot30", "default", {"linear": False}),
    (UCHAR, (48, 48, 48), (72, 56), "rot30", "default", {"ortho": True}),
    (UCHAR, (48, 48, 48), (64, 64), "default", "default",
     {"bbox": (-0.5, -0.8, -1.0, 0.7, 0.6, 0.2)}),
    (UCHAR, (40, 40, 40), (64, 48), "rot30", "haze", {"contours": True, "aerial": True}),
    (UCHAR, (40, 40, 40), (64, 48), "close", "opaque", {"illum": 0, "contours": True}),
    (UCHAR, (32, 32, 80), (64, 64), "rot30", "default", {"thickness": (1.0, 1.0, 2.5)}),
    (UCHAR, (128, 128, 128), (128, 128), "rot30", "default", {"rate": 0.7}),
    (USHORT, (48, 48, 48), (80, 64), "rot30", "default", {}),
    (USHORT, (40, 56, 36), (64, 64), "close", "opaque", {"ess": False}),
    (FLOAT, (48, 48, 48), (80, 64), "rot30", "default", {}),
    (FLOAT, (36, 36, 36), (64, 64), "default", "haze", {"illum": 0}),
    # shading modes 2-5: TF-opacity gradient, Sobel, gradient-magnitude TF, cel
    (UCHAR, (48, 48, 48), (80, 64), "rot30", "default", {"illum": 2}),
    (UCHAR, (40, 44, 36), (64, 64), "rot30", "opaque", {"illum": 3, "contours": True}),
    (UCHAR, (40, 40, 40), (64, 64), "close", "default", {"illum": 4}),
    (USHORT, (40, 40, 40), (64, 64), "rot30", "opaque", {"illum": 4, "ess": False}),
    (FLOAT, (40, 40, 40), (72, 56), "rot30", "default", {"illum": 5}),
    (FLOAT, (32, 32, 32), (64, 48), "default", "opaque", {"illum": 3, "ess": False}),
    (UCHAR, (40, 40, 40), (64, 48), "inside", "default", {"illum": 5, "aerial": True}),
    # ambient occlusion at early ray termination (calcAO, volumeraycast.cl:368-392, :870-876)
    (UCHAR, (48, 48, 48), (80, 64), "rot30", "opaque", {"ao": True}),
    (FLOAT, (40, 40, 40), (64, 64), "close", "opaque", {"ao": True, "ess": False, "illum": 0}),
    (USHORT, (40, 44, 36), (64, 56), "rot30", "opaque", {"ao": True, "illum": 3}),
    # showEss (:888-896): rays without a sample and rays ending next to a box edge are marked
    (UCHAR, (48, 48, 48), (96, 80), "rot30", "default",
     {"show_ess": True, "background": (0.25, 0.5, 1.0, 1.0)}),
    (USHORT, (40, 44, 36), (64, 56), "default", "haze", {"show_ess": True, "ess": False}),
    (FLOAT, (40, 40, 40), (64, 64), "close", "opaque", {"show_ess": True, "illum": 0}),
]


PT_CASES = [
    # fmt, res, (W, H), view, tff, smooth, kwargs -- technique 1 (Woodcock-tracking path tracer)
    (FLOAT, (48, 48, 48), (96, 80), "rot30", "default", True, {}),
    (FLOAT, (48, 48, 48), (64, 64), "default", "haze", False, {"ext": 30.0}),
    (UCHAR, (64, 40, 52), (72, 56), "rot30", "opaque", True, {"ext": 250.0, "gradient_bg": True}),
    (USHORT, (40, 56, 36), (64, 64), "close", "default", True, {"ext": 60.0}),
    (FLOAT, (48, 48, 48), (64, 64), "inside", "default", True, {}),
    (UCHAR, (48, 48, 48), (64, 64), "default", "default", False,
     {"bbox": (-0.5, -0.8, -1.0, 0.7, 0.6, 0.2), "ortho": True}),
]


MC_CASES = [
    # fmt, channels, res, view, kwargs -- CL_RGBA / CL_RG volumes (volumeraycast.cl:838-855)
    (UCHAR, 4, (40, 40, 40), "rot30", {}),
    (FLOAT, 4, (36, 40, 32), "close", {"ess": False, "linear": False}),
    (USHORT, 2, (40, 36, 44), "rot30", {"aerial": True}),
    (UCHAR, 2, (40, 40, 40), "default", {"ess": False, "illum": 0}),
    (UCHAR, 4, (40, 40, 40), "rot30", {"illum": 4}),               # gradient magnitude of .x
    (FLOAT, 4, (32, 32, 32), "inside", {"ao": True, "show_ess": True}),
]


FP_CASES = [
    # fmt, res, (W, H), view, tff, kwargs -- frames the default kernels render from the footprint
    # volume (un-instrumented, volume not much wider than the viewport)
    (UCHAR, (48, 48, 48), (96, 80), "rot30", "default", {}),
    (UCHAR, (33, 47, 29), (64, 64), "close", "haze", {"illum": 0}),
    (UCHAR, (48, 48, 48), (64, 64), "inside", "default", {}),        # edge-clamped fetches
    (USHORT, (40, 56, 36), (64, 64), "close", "opaque", {"ess": False}),
    (USHORT, (45, 45, 45), (80, 64), "rot30", "default", {"contours": True}),
    (FLOAT, (48, 48, 48), (80, 64), "rot30", "default", {}),
    (FLOAT, (37, 37, 37), (64, 64), "inside", "haze", {"ess": False}),
]


def oracle_params(res, view, kw, seed=SEED):
    """(cam, rp, rc, pt) for a scene, built the way VolumeRenderCL builds them
    (volumerendercl.cpp:347-362 calcScaling, :620-631 brickRes, the setters of :922-1047) --
    tests/test_gpu_parity.py checks them byte for byte against the product's own structs.
    view: a name of common.views() or the 16 floats of a row-major view matrix."""
    cam = vro.CameraParams()
    cam.viewMat[:] = common.views()[view] if isinstance(view, str) else [float(x) for x in view]
    bb = kw.get("bbox", (-1, -1, -1, 1, 1, 1))
    cam.bbox_bl[:] = [bb[0], bb[1], bb[2], 0]
    cam.bbox_tr[:] = [bb[3], bb[4], bb[5], 0]
    cam.ortho = 1 if kw.get("ortho", False) else 0
    rp = vro.RenderingParams()
    bg = kw.get("background")
    rp.backgroundColor[:] = [bg[0], bg[1], bg[2], 0.0] if bg is not None else [1.0, 1.0, 1.0, 1.0]
    rp.modelScale[:] = vro.calc_scaling(list(res), list(kw.get("thickness", (1.0, 1.0, 1.0)))) + [0]
    rp.illumType = kw.get("illum", 1)
    rp.imgEss = 1 if kw.get("img_ess", False) else 0
    rp.showEss = 1 if kw.get("show_ess", False) else 0
    rp.useLinear = 1 if kw.get("linear", True) else 0
    rp.useGradient = 1 if kw.get("gradient_bg", False) else 0
    rp.technique = kw.get("technique", 0)
    rp.seed = seed
    rp.iteration = 0
    rc = vro.RaycastParams()
    rc.samplingRate = kw.get("rate", 1.5)
    rc.useAO = 1 if kw.get("ao", False) else 0
    rc.contours = 1 if kw.get("contours", False) else 0
    rc.aerial = 1 if kw.get("aerial", False) else 0
    _, brf, _ = vro.brick_layout(list(res))
    rc.brickRes[:] = brf + [0]
    pt = vro.PathtraceParams(kw.get("ext", 100.0))
    return cam, rp, rc, pt


FLOAT_PALETTES = ("hu", "straddle", "huge", "negative", "specials")


def float_volume(palette, res, seed=7, nch=1):
    """A FLOAT volume [z, y, x] (or [z, y, x, nch]) of raw values outside [0, 1], from the unit noise field v:
    hu        v * 4095 - 1024                   CT Hounsfield units
    straddle  v * 2 - 0.5                       both sides of [0, 1]
    huge      v * 3e7 + 1                       x * n far above 2^31 for every table size
    negative  -(v * 1000) - 0.5                 all below 0
    specials  straddle, 3 % of the voxels replaced by NaN, +-inf, -0.0, denormals and +-3e38"""
    planes = []
    for c in range(nch):
        v = common.noise_volume(res, FLOAT, seed=seed + c, smooth=False).astype(np.float64)
        if palette == "hu":
            f = v * 4095.0 - 1024.0
        elif palette in ("straddle", "specials"):
            f = v * 2.0 - 0.5
        elif palette == "huge":
            f = v * 3e7 + 1.0
        elif palette == "negative":
            f = -(v * 1000.0) - 0.5
        else:
            raise ValueError(palette)
        f = f.astype(np.float32)
        if palette == "specials":
            rng = np.random.default_rng(seed + 100 + c)
            special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-41, 3e38, -3e38], np.float32)
            pick = rng.random(f.shape) < 0.03
            f[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
        planes.append(f)
    return planes[0] if nch == 1 else np.stack(planes, axis=-1)


def multichannel_volume(fmt, nch, res):
    planes = [common.noise_volume(res, fmt, seed=20 + c, smooth=False) for c in range(nch)]
    vol = np.stack(planes, axis=-1)
    if nch == 4:   # keep the opacity channel moderate so that rays are not cut at once
        vol[..., 3] = (vol[..., 3] * 0.2).astype(vol.dtype)
    return vol


# ---- seeded random scenes (tests/test_gpu_parity.py's five randomised tests, tests/test_gpu_random_techniques.py and
# its CPU companion tests/test_random_scenes_ref.py)

def random_view(rng):
    """A view matrix with a random rotation and the eye inside (z 0.2 .. 0.9) or outside (1.2 .. 4) the box."""
    q = frontend.quat_from_axis_angle(tuple(rng.normal(size=3)), float(rng.uniform(0, 360)))
    z = float(rng.choice([rng.uniform(0.2, 0.9), rng.uniform(1.2, 4.0)]))
    return frontend.view_matrix(q, (float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), z))


def random_scene(rng):
    """A scene drawn from the parameter space the reference's GUI can reach: voxel type, odd non-cubic resolution,
    anisotropic slice thickness, empty halves, transfer-function stops, camera inside / outside / orthographic,
    clip box, sampling rate, shading, ESS, filtering, jitter seed, odd viewports.
    Returns (vol, fmt, tff, view, kw, W, H); kw holds keys of oracle_params (and "ess", "seed")."""
    fmt = [UCHAR, USHORT, FLOAT][int(rng.integers(3))]
    res = tuple(int(v) for v in rng.integers(17, 70, size=3))
    vol = common.noise_volume(res, fmt, seed=int(rng.integers(1 << 30)), smooth=bool(rng.integers(2)))
    if rng.random() < 0.5:   # a slab of nothing: bricks to skip, cells to step over
        ax, cut = int(rng.integers(3)), float(rng.uniform(0.2, 0.6))
        sl = [slice(None)] * 3
        n = vol.shape[ax]
        sl[ax] = slice(0, int(n * cut)) if rng.random() < 0.5 else slice(int(n * (1 - cut)), n)
        vol[tuple(sl)] = 0
    pos = np.sort(rng.uniform(0.02, 0.98, size=int(rng.integers(1, 4))))
    stops = [(0.0, (0, 0, 0, 0))]
    for p in pos:
        stops.append((float(p), tuple(int(v) for v in rng.integers(0, 256, size=3)) +
                      (int(rng.integers(0, 256)) if rng.random() < 0.7 else 0,)))
    stops.append((1.0, tuple(int(v) for v in rng.integers(0, 256, size=3)) + (int(rng.integers(0, 256)),)))
    tff = frontend.tff_from_stops(stops)
    view = random_view(rng)
    kw = {"illum": int(rng.integers(2)), "ess": bool(rng.random() < 0.75), "linear": bool(rng.random() < 0.85),
          "ortho": bool(rng.random() < 0.2), "rate": float(rng.choice([0.5, 1.0, 1.5, 2.0, 3.1])),
          "gradient_bg": bool(rng.random() < 0.3), "seed": int(rng.integers(1, 1 << 32))}
    if rng.random() < 0.3:
        lo = rng.uniform(-1.0, -0.2, size=3)
        hi = rng.uniform(0.2, 1.0, size=3)
        kw["bbox"] = tuple(float(v) for v in lo) + tuple(float(v) for v in hi)
    if rng.random() < 0.3:
        kw["thickness"] = tuple(float(v) for v in rng.choice([0.5, 1.0, 1.0, 2.0, 3.3], size=3))
    if rng.random() < 0.25:
        kw["background"] = tuple(float(v) for v in rng.uniform(0, 1, size=3)) + (1.0,)
    W, H = int(rng.integers(33, 150)), int(rng.integers(33, 120))
    return vol, fmt, tff, view, kw, W, H


DEPTH_MODES = ("iso", "max", "opacity")
_MAXV = {UCHAR: 255.0, USHORT: 65535.0, FLOAT: 1.0}


def value_range(vol, fmt):
    """(lo, hi) of the volume's values in the transfer function's coordinate (normalised; FLOAT: raw)."""
    return float(vol.min()) / _MAXV[fmt], float(vol.max()) / _MAXV[fmt]


def random_tf2d_table(rng, tff, n_g, n_v):
    """A 2-D table uint8 [n_g, n_v, 4] made from the 1-D table in numpy alone: column i is the 1-D entry under the
    centre of value bin i; row j's alpha is scaled by a weight of its own, some rows by 0 (never all of them); some
    value columns -- a run from column 0 upwards, as in a table that hides the low values, and single ones -- are
    transparent in every row: what technique 6's search stage and cell bound step over."""
    tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1, 4)
    n = tff.shape[0]
    src = np.minimum(((np.arange(n_v) + 0.5) / n_v * n).astype(np.int64), n - 1)
    cols = tff[src].astype(np.float64)
    weight = rng.uniform(0.3, 1.0, size=n_g)
    clear_rows = rng.random(n_g) < 0.15
    clear_rows[int(rng.integers(n_g))] = False
    weight[clear_rows] = 0.0
    low = rng.random() < 0.6
    run = max(1, int(n_v * rng.uniform(0.08, 0.3)))
    clear_cols = rng.random(n_v) < 0.1
    if low:
        clear_cols[:run] = True
    table = np.empty((n_g, n_v, 4), np.uint8)
    table[:, :, :3] = cols[None, :, :3]
    table[:, :, 3] = np.round(cols[None, :, 3] * weight[:, None])
    table[:, clear_cols, 3] = 0
    return table


def random_extras(rng, vol, fmt, tff, depth_mode=None):
    """What techniques 4 and 6 and the depth images need on top of a random_scene, drawn after it from the same rng:
    iso (inside the volume's value range), refine (0, 1 or 4), depth_mode (drawn, or the one asked for) with its
    depth_threshold (iso: a value inside the range; opacity: 0.05 .. 0.5; max: 0, not read), g_hi and table, the
    2-D transfer function [n_g, n_v, 4] of random_tf2d_table."""
    lo, hi = value_range(vol, fmt)
    ex = {"iso": float(np.float32(lo + (hi - lo) * rng.uniform(0.1, 0.55))),
          "refine": int(rng.choice([0, 1, 4]))}
    drawn = DEPTH_MODES[int(rng.integers(3))]
    thresholds = {"iso": float(np.float32(lo + (hi - lo) * rng.uniform(0.1, 0.55))), "max": 0.0,
                  "opacity": float(np.float32(rng.uniform(0.05, 0.5)))}
    ex["depth_mode"] = drawn if depth_mode is None else depth_mode
    ex["depth_threshold"] = thresholds[ex["depth_mode"]]
    ex["g_hi"] = float(rng.choice([0.05, 0.12, 0.3]))
    n_g, n_v = int(rng.choice([1, 2, 5, 8, 16])), int(rng.choice([7, 64, 256]))
    ex["table"] = random_tf2d_table(rng, tff, n_g, n_v)
    return ex


def technique_case(seed_base, case, depth_mode=None):
    """Case `case` of a randomised technique test: (vol, fmt, tff, view, kw, W, H, extras, rng) -- the rng is handed
    back for whatever the test draws after the extras (batch views, rectangles)."""
    rng = np.random.default_rng(seed_base + case)
    vol, fmt, tff, view, kw, W, H = random_scene(rng)
    ex = random_extras(rng, vol, fmt, tff, depth_mode)
    return vol, fmt, tff, view, kw, W, H, ex, rng
