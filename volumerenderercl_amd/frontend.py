"""Front-end formulas that feed the hot path: the 16-float view
matrix and the 1024-entry RGBA8 transfer-function table the reference's Qt widget hands to
`VolumeRenderCL::updateView` / `setTransferFunction`.

Restated from Qt 5 semantics (QMatrix4x4 / QPropertyAnimation); Qt is not available here,
so these two are PARITY UNPINNED -- the pinned contract of the hot path is its numeric
inputs (16 floats, 4096 bytes), which every test feeds identically to oracle and GPU.
"""
import math

import numpy as np

# resetCam, volumerenderwidget.cpp:91-92,1069-1074
DEFAULT_ROTATION = (1.0, 0.0, 0.0, 0.0)     # quaternion w, x, y, z
DEFAULT_TRANSLATION = (0.0, 0.0, 2.0)

# TransferFunctionWidget::resetTransferFunction, transferfunctionwidget.cpp:338-346
DEFAULT_STOPS = [(0.00, (0, 0, 0, 0)), (0.10, (125, 125, 125, 0)), (1.00, (0, 0, 0, 255))]

# first outputs of a default-seeded std::mt19937 (reference frame seeds)
MT19937_FIRST_SEEDS = (3499211612, 581869302, 3890346734)


class Mt19937:
    """std::mt19937 (32-bit Mersenne twister, init_genrand seeding); default seed 5489.
    The reference draws one output per frame as the jitter seed (volumerendercl.cpp:212)."""

    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.idx = 624

    def __call__(self):
        if self.idx >= 624:
            mt = self.mt
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.idx = 0
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def quat_from_axis_angle(axis, degrees):
    """QQuaternion::fromAxisAndAngle (axis normalised)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    s = math.sin(h)
    return (math.cos(h), a[0] * s, a[1] * s, a[2] * s)


def quat_mul(p, q):
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return (pw * qw - px * qx - py * qy - pz * qz,
            pw * qx + px * qw + py * qz - pz * qy,
            pw * qy - px * qz + py * qw + pz * qx,
            pw * qz + px * qy - py * qx + pz * qw)


def rotation_matrix(q):
    w, x, y, z = q
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def view_matrix(rotation=DEFAULT_ROTATION, translation=DEFAULT_TRANSLATION):
    """updateViewMatrix, volumerenderwidget.cpp:1079-1098: M = R(q) * T(t) * S(t.z), handed
    over row-major.  Upper 3x3 = t.z * R, last column = R * t."""
    R = rotation_matrix(rotation)
    t = np.asarray(translation, dtype=np.float64)
    M = np.eye(4)
    M[:3, :3] = R * t[2]
    M[:3, 3] = R @ t
    return [float(np.float32(v)) for v in M.reshape(-1)]


def _ease(kind, t):
    """QEasingCurve::valueForProgress for the curves the GUI offers (mainwindow.cpp:945-957), with the
    operation order of Qt's src/3rdparty/easing/easing.cpp (easeNone, easeInOutQuad, easeInOutCubic)."""
    t = min(1.0, max(0.0, t))
    if kind == "linear":
        return t
    if kind == "quad":     # QEasingCurve::InOutQuad
        t *= 2.0
        if t < 1:
            return t * t / 2.0
        t -= 1
        return -0.5 * (t * (t - 2) - 1)
    if kind == "cubic":    # QEasingCurve::InOutCubic
        t *= 2.0
        if t < 1:
            return 0.5 * t * t * t
        t -= 2.0
        return 0.5 * (t * t * t + 2)
    raise ValueError(kind)


def tff_from_stops(stops=DEFAULT_STOPS, n=1024, easing="linear"):
    """updateTransferFunction, volumerenderwidget.cpp:916-938: entry i samples the key-value
    animation at time qRound(i/n*8192) of 8192; QVariantAnimation interpolates QColor per channel as
    qBound(0, int(f + (t - f) * localProgress), 255) (_q_interpolate<int> truncates) with
    localProgress = (progress - start) / (end - start) in double; then max(0, c - 3).
    setKeyValueAt replaces an earlier key at the same position; missing end stops (the GUI always
    has them) repeat the nearest stop's colour.  Known answers derived by hand from these semantics:
    tests/test_frontend_files.py."""
    dedup = []
    for s in sorted(stops, key=lambda s: s[0]):     # (stable)
        if dedup and dedup[-1][0] == s[0]:
            dedup[-1] = s
        else:
            dedup.append(s)
    stops = dedup
    if stops[0][0] > 0.0:
        stops = [(0.0, stops[0][1])] + stops
    if stops[-1][0] < 1.0:
        stops = stops + [(1.0, stops[-1][1])]
    out = np.zeros((n, 4), dtype=np.uint8)
    for i in range(n):
        time = int(math.floor(i / n * 8192.0 + 0.5))
        p = _ease(easing, time / 8192.0)
        k = 0
        while k + 2 < len(stops) and p >= stops[k + 1][0]:
            k += 1
        (p0, c0), (p1, c1) = stops[k], stops[k + 1]
        lp = 0.0 if p1 == p0 else (p - p0) / (p1 - p0)
        for c in range(4):
            v = int(c0[c] + (c1[c] - c0[c]) * lp)
            v = min(255, max(0, v))
            out[i, c] = max(0, v - 3)
    return out


def opaque_ramp_tff(n=1024):
    """ERT stress table of SURVEY 8(d): alpha = clamp(4*(x - 0.25)), grey ramp colour."""
    x = (np.arange(n) + 0.5) / n
    out = np.zeros((n, 4), dtype=np.uint8)
    out[:, 3] = np.clip(np.round(255 * np.clip(4 * (x - 0.25), 0, 1)), 0, 255)
    out[:, 0] = np.round(255 * x)
    out[:, 1] = np.round(255 * (1 - x))
    out[:, 2] = 128
    return out


def haze_tff(n=1024, alpha=12):
    """Semi-transparent table (no ERT, every sample shaded or not by `alpha`): keeps rays
    alive through the whole volume -- the dense-sampling regime of SURVEY 7."""
    x = (np.arange(n) + 0.5) / n
    out = np.zeros((n, 4), dtype=np.uint8)
    out[:, 0] = np.round(255 * x)
    out[:, 1] = np.round(200 * (1 - x))
    out[:, 2] = 90
    out[:, 3] = np.where(x > 0.05, alpha, 0)
    return out


def prefix_sum(tff):
    """volumerendercl.cpp:879-884."""
    tff = np.asarray(tff, dtype=np.uint8).reshape(-1, 4)
    return np.cumsum(tff[:, 3].astype(np.uint64)).astype(np.uint32)


def quantise_rgba8(frame_f32):
    """The 8-bit frame of float pixels, per channel: 0 for a NaN, else rint(clip(f * 255.0f, 0, 255)) in float32
    -- one rounded fp32 multiply, a clamp, round-half-to-even: OpenCL's convert_uchar_sat_rte(f * 255.0f), what
    write_imagef does on the reference's CL_UNORM_INT8 output image (volumerendercl.cpp:468-478).  The numpy
    statement of what the library's kernels compute (vr_rgba8.hip); same shape, dtype uint8."""
    f = np.asarray(frame_f32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(np.clip(f * np.float32(255.0), np.float32(0.0), np.float32(255.0)))
    return np.where(np.isnan(f), np.float32(0.0), q).astype(np.uint8)


# ---- the reference GUI's saved files: camera state, transfer functions ----------

def read_tff_stops(path):
    """`.tff` gradient-stop file (MainWindow::readTff / saveTff, mainwindow.cpp:583-657): one
    stop per line, `position r g b a`; lines with fewer than 5 fields are skipped."""
    stops = []
    with open(path) as f:
        for line in f:
            p = line.split()
            if len(p) < 5:
                continue
            stops.append((float(p[0]), tuple(int(float(v)) for v in p[1:5])))
    if not stops:
        raise ValueError("Empty transfer function file.")
    return stops


def write_tff_stops(path, stops):
    with open(path, "w") as f:
        for pos, c in stops:
            f.write("%s %d %d %d %d\n" % (repr(float(pos)), c[0], c[1], c[2], c[3]))


def read_raw_tff(path):
    """Raw transfer function text file (MainWindow::loadRawTff / saveRawTff, mainwindow.cpp:
    662-727): whitespace-separated numbers, each cast to unsigned char; RGBA8 table."""
    import numpy as np
    with open(path) as f:
        vals = [float(v) for v in f.read().split()]
    tff = np.array([int(v) & 0xFF for v in vals], dtype=np.uint8)
    if tff.size == 0 or tff.size % 4:
        raise ValueError("Invalid raw transfer function file " + path)
    return tff


def write_raw_tff(path, tff):
    import numpy as np
    with open(path, "w") as f:
        f.write("".join("%d " % int(c) for c in np.asarray(tff, dtype=np.uint8).reshape(-1)))


def read_cam_state(path):
    """JSON state file (MainWindow::loadCamState, mainwindow.cpp:374-410 and
    VolumeRenderWidget::read, volumerenderwidget.cpp:1457-1480).  Returns a dict with the keys
    present in the file: rotation (w, x, y, z), translation (x, y, z), imgResFactor, rayStepSize,
    useLerp, useAO, showContours, useAerial, showBox, useOrtho."""
    import json
    with open(path) as f:
        js = json.load(f)
    out = {}
    if "camRotation" in js:
        p = str(js["camRotation"]).split(" ")
        if len(p) >= 4:
            out["rotation"] = tuple(float(v) for v in p[:4])
    if "camTranslation" in js:
        p = str(js["camTranslation"]).split(" ")
        if len(p) >= 3:
            out["translation"] = tuple(float(v) for v in p[:3])
    for k in ("imgResFactor", "rayStepSize"):
        if isinstance(js.get(k), (int, float)) and not isinstance(js.get(k), bool):
            out[k] = float(js[k])
    for k in ("useLerp", "useAO", "showContours", "useAerial", "showBox", "useOrtho"):
        if isinstance(js.get(k), bool):
            out[k] = js[k]
    return out


def write_cam_state(path, rotation=DEFAULT_ROTATION, translation=DEFAULT_TRANSLATION, **flags):
    """MainWindow::saveCamState + VolumeRenderWidget::write (mainwindow.cpp:415-452,
    volumerenderwidget.cpp:1496-1505): floats go through double as QString::number does."""
    import json
    import numpy as np
    js = {"imgResFactor": float(flags.get("imgResFactor", 1.0)),
          "rayStepSize": float(flags.get("rayStepSize", 1.5))}
    for k, d in (("useLerp", True), ("useAO", False), ("showContours", False), ("useAerial", False),
                 ("showBox", False), ("useOrtho", False)):
        js[k] = bool(flags.get(k, d))
    js["camRotation"] = " ".join("%.6g" % float(np.float32(v)) for v in rotation)
    js["camTranslation"] = " ".join("%.6g" % float(np.float32(v)) for v in translation)
    with open(path, "w") as f:
        json.dump(js, f, indent=4)


def apply_cam_state(vr, state):
    """Apply a state read by read_cam_state to a VolumeRenderCL (what the GUI's widgets forward)."""
    vr.updateView(view_matrix(state.get("rotation", DEFAULT_ROTATION),
                              state.get("translation", DEFAULT_TRANSLATION)))
    if "rayStepSize" in state:
        vr.updateSamplingRate(state["rayStepSize"])
    if "useLerp" in state:
        vr.setLinearInterpolation(state["useLerp"])
    if "showContours" in state:
        vr.setContours(state["showContours"])
    if "useAerial" in state:
        vr.setAerial(state["useAerial"])
    if "useOrtho" in state:
        vr.setCamOrtho(state["useOrtho"])
    if "useAO" in state:
        vr.setAmbientOcclusion(state["useAO"])
    if state.get("showBox"):
        vr.setShowESS(True)


# ---- camera paths recorded by the GUI, replayed headless (one frame per camera entry)

def _f32(text):
    """QString::toFloat: the recorded numbers are read back as floats."""
    return float(np.float32(float(text)))


def _split_entries(path):
    with open(path) as f:
        return [e.split() for e in f.read().split(";") if e.strip()]


def read_view_record(prefix):
    """recordViewConfig (volumerenderwidget.cpp:1030-1048): `<prefix>_quat.txt` holds `w x y z; ` and
    `<prefix>_trans.txt` `x y z; ` per recorded view, appended to one line.  Returns the view matrices
    (16 floats each, view_matrix), in recording order."""
    quats, trans = _split_entries(prefix + "_quat.txt"), _split_entries(prefix + "_trans.txt")
    if len(quats) != len(trans):
        raise ValueError("view record %s: %d rotations but %d translations" % (prefix, len(quats), len(trans)))
    views = []
    for q, t in zip(quats, trans):
        if len(q) != 4 or len(t) != 3:
            raise ValueError("view record %s: malformed entry %r / %r" % (prefix, " ".join(q), " ".join(t)))
        views.append(view_matrix(tuple(_f32(v) for v in q), tuple(_f32(v) for v in t)))
    if not views:
        raise ValueError("view record %s: no views" % prefix)
    return views


def read_interaction_log(path):
    """Interaction log (toggleInteractionLogging / logInteraction, volumerenderwidget.cpp:313-358), parsed
    as setSequenceStep (:364-408) does -- the payload follows the last `;`.  Returns the events in order:
    ("camera", 16-float view matrix) for `<ms>; camera; w x y z, tx ty tz`, ("transferFunction", uint8
    RGBA8 table), ("timestep", int).  `tffInterpolation` lines are parsed and dropped: the tables in the log
    are already sampled.  A line of none of these kinds, or one whose payload does not parse, is an error."""
    events = []
    with open(path) as f:
        lines = f.read().splitlines()
    for n, line in enumerate(lines, 1):
        if not line.strip():
            continue
        pos = line.rfind(";")
        payload = line[pos + 2:] if pos >= 0 else ""
        try:
            if pos < 0:
                raise ValueError("no ';'")
            if "camera" in line:
                v = [_f32(x) for x in payload.replace(",", "").split()]
                if len(v) != 7:
                    raise ValueError("a camera entry is 7 numbers")
                events.append(("camera", view_matrix(tuple(v[:4]), tuple(v[4:]))))
            elif "timestep" in line:
                events.append(("timestep", int(payload.strip())))
            elif "transferFunction" in line:
                vals = [int(x) & 0xFF for x in payload.split()]
                if not vals or len(vals) % 4:
                    raise ValueError("a transfer function is RGBA8 entries")
                events.append(("transferFunction", np.array(vals, dtype=np.uint8)))
            elif "tffInterpolation" in line:
                if payload.strip() not in ("linear", "quad", "cubic"):
                    raise ValueError("unknown interpolation")
            else:
                raise ValueError("unknown event")
        except ValueError as e:
            raise ValueError("interaction log %s, line %d: %s" % (path, n, e))
    if not any(k == "camera" for k, _ in events):
        raise ValueError("interaction log %s: no camera entries" % path)
    return events


def orbit_views(axis, n, rotation=DEFAULT_ROTATION, translation=DEFAULT_TRANSLATION):
    """A turntable: n views evenly spaced over 360 degrees about `axis`, each step composed onto the start
    rotation the way the GUI's mouse rotation is (_rotQuat * step, volumerenderwidget.cpp:1115); the
    translation stays."""
    if int(n) < 1:
        raise ValueError("orbit_views: n >= 1")
    return [view_matrix(quat_mul(rotation, quat_from_axis_angle(axis, 360.0 * k / int(n))), translation)
            for k in range(int(n))]


# ---- depth images (include/vrhip.h "depth images and picking"; VolumeRenderCL.render_depth / pick)

def box_to_voxel(pos, res):
    """Box-space positions ([-1, 1]^3, the last axis x, y, z) as continuous voxel coordinates: (pos * 0.5 + 0.5) * res,
    in float64 -- the voxel whose cell holds the point is floor() of it."""
    return (np.asarray(pos, dtype=np.float64) * 0.5 + 0.5) * np.asarray(res, dtype=np.float64)[:3]


def depth_grey(xyzt, kind):
    """A depth image as grey bytes [h, w], the picture `vrhip_render --depth` writes: hits between white (the
    smallest t) and black (the largest), everything else black."""
    t = np.asarray(xyzt, dtype=np.float32)[..., 3]
    hit = np.asarray(kind) == 2
    out = np.zeros(t.shape, dtype=np.uint8)
    if hit.any():
        lo, hi = t[hit].min(), t[hit].max()
        g = 1.0 - (t[hit] - lo) / (hi - lo) if hi > lo else np.ones(int(hit.sum()), np.float32)
        out[hit] = np.round(np.clip(g, 0.0, 1.0) * 255.0).astype(np.uint8)
    return out


# ---- meshes (include/vrhip.h "isosurface extraction"; VolumeRenderCL.extract_isosurface)

def weld_mesh(positions, normals=None):
    """A triangle list [n, 3, 3] as an indexed mesh: (vertices float32 [m, 3], normals float32 [m, 3] or None, indices
    uint32 [n, 3]).  Vertices are unique by bit-equal position; the first occurrence keeps its index order and its
    normal."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    keys = pos.view(np.uint32).reshape(-1, 3)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # unique vertices by first occurrence
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    idx = rank[np.asarray(inverse).reshape(-1)].astype(np.uint32).reshape(-1, 3)
    sel = first[order]
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)[sel].copy()
    return pos[sel].copy(), nrm, idx


def facet_normals(positions):
    """The unit right-hand normal of every triangle of a list [n, 3, 3], float32 [n, 3]; (0, 0, 0) for a degenerate one."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1)
    out = np.zeros_like(n)
    ok = ln > 0
    out[ok] = n[ok] / ln[ok, None]
    return out.astype(np.float32)


def write_stl(path, positions):
    """A triangle list [n, 3, 3] as binary STL: the soup as it is, each facet's normal from its winding."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3, 3)
    rec = np.zeros(pos.shape[0], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    rec["n"] = facet_normals(pos)
    rec["v"] = pos
    with open(path, "wb") as f:
        f.write(b"vrhip isosurface".ljust(80, b" "))
        f.write(np.uint32(pos.shape[0]).astype("<u4").tobytes())
        f.write(rec.tobytes())


def read_stl(path):
    """A binary STL as (facet normals float32 [n, 3], positions float32 [n, 3, 3])."""
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0])
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), count=n, offset=84)
    return rec["n"].copy(), rec["v"].copy()


def write_ply(path, positions, normals=None):
    """A triangle list as binary_little_endian PLY, welded (weld_mesh): x y z, nx ny nz when normals are given, and
    the faces as uchar-counted lists of uint indices.  Returns (vertices, faces) written."""
    v, nrm, idx = weld_mesh(positions, normals)
    head = ["ply", "format binary_little_endian 1.0", "comment vrhip isosurface", "element vertex %d" % v.shape[0],
            "property float x", "property float y", "property float z"]
    if nrm is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    head += ["element face %d" % idx.shape[0], "property list uchar uint vertex_indices", "end_header"]
    vert = np.hstack([v, nrm]) if nrm is not None else v
    face = np.zeros(idx.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<u4", 3)]))
    face["n"] = 3
    face["i"] = idx
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(vert, dtype="<f4").tobytes())
        f.write(face.tobytes())
    return v.shape[0], idx.shape[0]


def read_ply(path):
    """A PLY as write_ply (or `vrhip_render --mesh`) writes it: (vertices float32 [m, 3], normals float32 [m, 3] or
    None, indices uint32 [n, 3])."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "format binary_little_endian 1.0" not in lines:
        raise ValueError("read_ply: not a binary little-endian PLY")
    nv = nf = 0
    props = []
    for ln in lines:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:2] == ["property", "float"]:
            props.append(w[2])
    if props not in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"]):
        raise ValueError("read_ply: unexpected vertex properties %r" % (props,))
    vert = np.frombuffer(raw, dtype="<f4", count=nv * len(props), offset=end).reshape(nv, len(props))
    face = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("i", "<u4", 3)]), count=nf, offset=end + vert.nbytes)
    if nf and not np.all(face["n"] == 3):
        raise ValueError("read_ply: not a triangle mesh")
    return (vert[:, :3].copy(), vert[:, 3:].copy() if len(props) == 6 else None, face["i"].astype(np.uint32))


# ---- volume statistics (include/vrhip.h "volume statistics"; VolumeRenderCL.volume_statistics): from its result to a
# mean and an isoValue.  Host arithmetic in float64.

def mean_std(stats):
    """(mean, standard deviation) of the normalised value over the non-NaN voxels of a volume_statistics(...,
    moments=True) result: sum / n and sqrt(sum_sq / n - mean^2) (population, clamped at 0), n = voxels - nan.
    No such voxel: (nan, nan)."""
    n = int(stats["voxels"]) - int(stats["nan"])
    if n <= 0:
        return float("nan"), float("nan")
    mean = float(stats["sum"]) / n
    return mean, float(np.sqrt(max(float(stats["sum_sq"]) / n - mean * mean, 0.0)))


def otsu_threshold(hist_row, v_lo, v_hi):
    """Otsu's threshold of a 1-D histogram over [v_lo, v_hi] (a row of volume_statistics' table, or its column sum
    hist.sum(axis=0)): the bin boundary v_lo + k * (v_hi - v_lo) / bins, 1 <= k < bins, that maximises the
    between-class variance w0 * w1 * (mu0 - mu1)^2 of the bins below and from k on, every bin at its centre; of equal
    maxima the middle one (a plateau between two separated modes).  An isoValue for setIsoParams / extract_isosurface.
    Fewer than two occupied bins: the window's centre."""
    h = np.asarray(hist_row, dtype=np.float64).ravel()
    bins = h.size
    width = (float(v_hi) - float(v_lo)) / bins
    if bins < 2 or np.count_nonzero(h) < 2:
        return 0.5 * (float(v_lo) + float(v_hi))
    centres = float(v_lo) + (np.arange(bins) + 0.5) * width
    w0 = np.cumsum(h)[:-1]                 # the bins below boundary k = 1 .. bins - 1
    w1 = h.sum() - w0
    m0 = np.cumsum(h * centres)[:-1]
    m1 = (h * centres).sum() - m0
    ok = (w0 > 0) & (w1 > 0)
    var = np.zeros(bins - 1)
    var[ok] = w0[ok] * w1[ok] * (m0[ok] / w0[ok] - m1[ok] / w1[ok]) ** 2
    best = np.flatnonzero(var >= var.max() * (1.0 - 1e-12))
    k = int(best[(best.size - 1) // 2]) + 1
    return float(v_lo) + k * width


# ---- 2-D transfer functions (include/vrhip.h "technique == 6"; VolumeRenderCL.setTransferFunction2D): tables of shape
# (n_g, n_v, 4) uint8, row j = gradient bin j of volume_statistics(..., bins_g=n_g, g_hi=g_hi), value fastest.

def _tf1d(tff):
    tff = np.ascontiguousarray(tff, dtype=np.uint8).reshape(-1, 4)
    if tff.shape[0] < 1:
        raise ValueError("empty transfer function")
    return tff


def tf2d_from_1d(tff, n_g):
    """n_g rows, each the 1-D table: TF2(s, m) = TF(s) whatever the gradient -- technique 6 then renders technique
    0's image (object-order ESS off)."""
    return np.ascontiguousarray(np.broadcast_to(_tf1d(tff)[None], (int(n_g),) + _tf1d(tff).shape))


def tf2d_ramp(tff, n_g, g_hi, g0, g1):
    """Boundary emphasis: n_g rows of the 1-D table, their alpha scaled by a ramp over the gradient magnitude that is
    0 up to g0 and 1 from g1 on (vrhip_tf2d_build_ramp: the expression is in include/vrhip.h)."""
    from . import _lib
    tff = _tf1d(tff)
    out = np.zeros((int(n_g), tff.shape[0], 4), np.uint8)
    rc = _lib.load().vrhip_tf2d_build_ramp(tff.ctypes.data, tff.shape[0], int(n_g), float(g_hi), float(g0), float(g1),
                                           out.ctypes.data)
    if rc != _lib.OK:
        raise ValueError("tf2d_ramp: table sizes 1..4096 x 1..256 (at most 65536 entries), g_hi finite and > 0, "
                         "0 <= g0 < g1 finite")
    return out


def tf2d_lookup(table, g_hi, s, m):
    """Technique 6's lookup of the table at value s and gradient magnitude m (vrhip_tf2d_lookup): float32 RGBA."""
    import ctypes as C
    from . import _lib
    table = np.ascontiguousarray(table, dtype=np.uint8)
    if table.ndim != 3 or table.shape[2] != 4:
        raise ValueError("the 2-D transfer function must have shape (n_g, n_v, 4)")
    out = (C.c_float * 4)()
    rc = _lib.load().vrhip_tf2d_lookup(table.ctypes.data, table.shape[1], table.shape[0], float(g_hi), float(s), float(m), out)
    if rc != _lib.OK:
        raise ValueError("tf2d_lookup: invalid table size or g_hi")
    return np.array(out[:], dtype=np.float32)


# ---- pre-integrated classification (include/vrhip.h "technique == 8")

def preint_slab(tff, sf, sb, raw=False):
    """Technique 8's classification of the slab between the sample values sf (front) and sb (back) with the 1-D table
    tff (uint8 [n, 4], as setTransferFunction takes it): float32 (Cbar.rgb, abar), the opacity-weighted mean colour and
    the mean opacity of the transfer function over the values in between (vrhip_preint_slab: host only, the device's
    result bit for bit).  raw: the values are a FLOAT volume's (any float); otherwise normalised ones in [-1, 2]."""
    import ctypes as C
    from . import _lib
    entries = (_tf1d(tff).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    out = (C.c_float * 4)()
    rc = _lib.load().vrhip_preint_slab(entries.ctypes.data, entries.shape[0], 1 if raw else 0, float(sf), float(sb), out)
    if rc != _lib.OK:
        raise ValueError("preint_slab: tables of 1..4096 entries; values that are not raw must lie in [-1, 2]")
    return np.array(out[:], dtype=np.float32)


# ---- volume filters (include/vrhip.h "volume filters"; VolumeRenderCL.filter_volume)

def gaussian_taps(sigma, radius=None):
    """The weights w[0 .. radius] of a normalised Gaussian for filter_volume(kind="separable"), float32, as
    vrhip_filter_gaussian_taps computes them, in float64: t_k = exp(-k^2 / (2 sigma^2)), S = t_0 + 2 (t_1 + ... +
    t_R) added in ascending order, w_k = t_k / S.  radius None: ceil(3 sigma), at most 8."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError("gaussian_taps: sigma must be finite and positive")
    if radius is None:
        radius = min(int(math.ceil(3.0 * sigma)), 8)
    radius = int(radius)
    if not 0 <= radius <= 8:
        raise ValueError("gaussian_taps: radius must be 0..8")
    t = [math.exp(-(float(k) * float(k)) / (2.0 * sigma * sigma)) for k in range(radius + 1)]
    tail = 0.0
    for k in range(1, radius + 1):
        tail = tail + t[k]
    total = t[0] + 2.0 * tail
    return np.array([v / total for v in t], dtype=np.float32)


# ---- volume morphology (include/vrhip.h "volume morphology"; VolumeRenderCL.morph_volume)

MORPH_OPS = {"erode": 0, "dilate": 1, "open": 2, "close": 3, "gradient": 4, "tophat": 5, "blackhat": 6}   # VRHIP_MORPH_*
MORPH_SHAPES = {"box": 0, "ball": 1}


def morph_params(op, radius, shape="ball"):
    """A MorphParams from names: op one of MORPH_OPS, shape "box" or "ball", radius 0..8, one for all axes or (x, y, z)."""
    from . import _lib
    if op not in MORPH_OPS:
        raise ValueError("morph: op must be one of %s" % ", ".join(MORPH_OPS))
    if shape not in MORPH_SHAPES:
        raise ValueError("morph: shape must be 'box' or 'ball'")
    radius = [radius] * 3 if np.isscalar(radius) else list(radius)
    if len(radius) != 3 or any(not 0 <= int(v) <= _lib.MORPH_MAX_RADIUS or int(v) != v for v in radius):
        raise ValueError("morph: a radius is an integer 0..8, one for all axes or one per axis")
    p = _lib.MorphParams()
    p.op = MORPH_OPS[op]
    p.shape = MORPH_SHAPES[shape]
    p.radius[:] = [int(v) for v in radius]
    return p


def morph_element(shape, radius):
    """The offsets (dx, dy, dz) of the structuring element (vrhip_morph_element), int8 [n, 3], z, y, x ascending."""
    import ctypes as C
    from . import _lib
    p = morph_params("erode", radius, shape)
    n = C.c_uint32(0)
    lib = _lib.load()
    lib.vrhip_morph_element(C.byref(p), None, 0, C.byref(n))   # (the count; refused for its capacity)
    out = np.zeros((n.value, 3), np.int8)
    if lib.vrhip_morph_element(C.byref(p), out.ctypes.data_as(C.POINTER(C.c_int8)), n.value, C.byref(n)) != _lib.OK:
        raise ValueError("morph_element: the library refuses the arguments")
    return out


# ---- slice views (include/vrhip.h "slice views"; VolumeRenderCL.render_slices).  The contract is the 80-byte
# vrhip_slice_params block; the helpers below compute in float64 and store float32.

_SLICE_MODES = {"max": 0, "min": 1, "mean": 2}
_SLICE_OUTPUTS = {"tf": 0, "value": 1}


def make_slice(origin, u, v, w=(0.0, 0.0, 0.0), samples=1, mode="max", output="tf"):
    """A SliceParams from its vectors in box space (the volume is [-1, 1]^3): origin = image centre, u = centre ->
    centre of the right edge, v = centre -> centre of the top edge, w = the slab from its first to its last face
    (zeros: a thin slice).  mode "max" | "min" | "mean" over `samples` planes; output "tf" (transfer function over
    the background) or "value" (the filtered value itself in r, g, b; alpha 1)."""
    from ._lib import SliceParams
    if mode not in _SLICE_MODES:
        raise ValueError("slice mode must be 'max', 'min' or 'mean'")
    if output not in _SLICE_OUTPUTS:
        raise ValueError("slice output must be 'tf' or 'value'")
    if not 1 <= int(samples) <= 256:
        raise ValueError("slice samples must be 1 .. 256")
    s = SliceParams()
    for name, vec in (("origin", origin), ("u", u), ("v", v), ("w", w)):
        vec = np.asarray(vec, dtype=np.float64).reshape(-1)
        if vec.size != 3 or not np.all(np.isfinite(vec)):
            raise ValueError("slice %s must be three finite numbers" % name)
        getattr(s, name)[:] = [float(np.float32(x)) for x in vec] + [0.0]
    s.samples, s.mode, s.output, s.reserved = int(samples), _SLICE_MODES[mode], _SLICE_OUTPUTS[output], 0
    return s


def axis_slice(axis, position, thickness=0.0, samples=1, mode="max", output="tf"):
    """The full cross-section of the box perpendicular to `axis` ("x", "y", "z" or 0, 1, 2) at `position` in [-1, 1]
    along it; thickness (box units, along +axis, centred on position) and samples make it a slab.
    Orientation, for a volume array vol[z, y, x] (row 0 of an image is its top):
      axis z (axial):    right = +x, up = +y    image[r, c] ~ vol[iz, ny - 1 - r, c]
      axis y (coronal):  right = -x, up = +z    image[r, c] ~ vol[nz - 1 - r, iy, nx - 1 - c]
      axis x (sagittal): right = +y, up = +z    image[r, c] ~ vol[nz - 1 - r, c, ix]
    i.e. each is seen from the positive side of its axis: u x v points along +axis, at the viewer, and slice_stack
    steps from -1 towards +1.
    The image always spans the whole box, whatever its size in pixels: the caller picks width : height from the
    model scale (VolumeRenderCL.params()[1].modelScale; the box's physical extent along an axis is 2 / modelScale)
    -- or width, height = the resolution along right and up for one pixel per voxel."""
    a = {"x": 0, "y": 1, "z": 2}.get(axis.lower(), None) if isinstance(axis, str) else int(axis)
    if a not in (0, 1, 2):
        raise ValueError("slice axis must be 'x', 'y' or 'z'")
    right, up = ((1, 2), (0, 2), (0, 1))[a]
    origin, u, v, w = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
    origin[a] = float(position)
    u[right] = -1.0 if a == 1 else 1.0
    v[up] = 1.0
    w[a] = float(thickness)
    return make_slice(origin, u, v, w, samples, mode, output)


def plane_slice(origin, normal, up, half_width, half_height, thickness=0.0, samples=1, mode="max", output="tf"):
    """An oblique plane through `origin` (box space) perpendicular to `normal`: v = half_height * the unit vector of
    `up` made orthogonal to the normal, u = half_width * (v^ x n^) -- seen from the side the normal points to, right
    is to the right (normal +z, up +y: right = +x) -- and w = thickness * n^."""
    n = np.asarray(normal, dtype=np.float64).reshape(-1)
    upv = np.asarray(up, dtype=np.float64).reshape(-1)
    if n.size != 3 or upv.size != 3 or not np.all(np.isfinite(n)) or not np.all(np.isfinite(upv)):
        raise ValueError("plane_slice: normal and up must be three finite numbers")
    ln = np.linalg.norm(n)
    if not ln > 0:
        raise ValueError("plane_slice: the normal must not be zero")
    n = n / ln
    vv = upv - n * np.dot(upv, n)
    lv = np.linalg.norm(vv)
    if not lv > 1e-12 * max(1.0, np.linalg.norm(upv)):
        raise ValueError("plane_slice: up must not be parallel to the normal")
    vv = vv / lv
    uu = np.cross(vv, n)
    return make_slice(origin, uu * float(half_width), vv * float(half_height), n * float(thickness), samples, mode, output)


def slice_normal(s):
    """The unit normal of a SliceParams (float64): along w for a slab, else u x v."""
    w = np.array(s.w[:3], dtype=np.float64)
    if not np.any(w != 0):
        w = np.cross(np.array(s.u[:3], dtype=np.float64), np.array(s.v[:3], dtype=np.float64))
    ln = np.linalg.norm(w)
    if not ln > 0:
        raise ValueError("slice has no normal (u x v and w are zero)")
    return w / ln


def slice_stack(s, n, span):
    """n parallel copies of slice `s` stepped along its normal over `span` box units centred on s.origin: copy k
    sits at origin + ((k + 0.5) / n - 0.5) * span * normal, k = 0 .. n - 1 (span 2 and n = the resolution along an
    axis: one axis_slice through every voxel centre, from -1 towards +1)."""
    from ._lib import SliceParams
    import ctypes as C
    if int(n) < 1:
        raise ValueError("slice_stack: n >= 1")
    nrm = slice_normal(s)
    o = np.array(s.origin[:3], dtype=np.float64)
    out = []
    for k in range(int(n)):
        c = SliceParams()
        C.memmove(C.byref(c), C.byref(s), C.sizeof(SliceParams))
        p = o + ((k + 0.5) / int(n) - 0.5) * float(span) * nrm
        c.origin[:] = [float(np.float32(x)) for x in p] + [0.0]
        out.append(c)
    return out
