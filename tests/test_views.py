"""Camera paths the reference GUI records (recordViewConfig, the interaction log) and turntables, parsed into
the 16-float views the per-frame-camera batch renders: the Python front end, the headless C++ host's twin of it
(vrhip_render --dump-views, no GPU involved) float for float, and a C++ caller of the renderFrames overload."""
import os
import subprocess

import numpy as np
import pytest

from volumerenderercl_amd import frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")

# (rotation, translation) the way QTextStream writes floats: 6 significant digits
QUATS = [(1, 0, 0, 0), (0.965926, 0.258819, 0, 0), (0.707107, 0, 0.707107, 0), (0.5, 0.5, -0.5, 0.5)]
TRANS = [(0, 0, 2), (0, 0, 2), (0.1, -0.05, 1.2), (0, 0, 0.4)]


def _qt(v):
    return "%g" % float(np.float32(v))


def _write_record(prefix, quats=QUATS, trans=TRANS):
    # recordViewConfig appends one `w x y z; ` / `x y z; ` per view: every entry on one line
    with open(prefix + "_quat.txt", "w") as f:
        f.write("".join(" ".join(_qt(v) for v in q) + "; " for q in quats))
    with open(prefix + "_trans.txt", "w") as f:
        f.write("".join(" ".join(_qt(v) for v in t) + "; " for t in trans))


def _expected(q, t):
    return frontend.view_matrix(tuple(float(np.float32(v)) for v in q), tuple(float(np.float32(v)) for v in t))


def _tff_line(ms, tff):
    return "%d; transferFunction; %s\n" % (ms, "".join("%d " % int(c) for c in np.asarray(tff).reshape(-1)))


def _camera_line(ms, q, t):
    return "%d; camera; %s, %s\n" % (ms, " ".join(_qt(v) for v in q), " ".join(_qt(v) for v in t))


def _write_log(path, tff2):
    # toggleInteractionLogging's initial block, then interactions (logInteraction appends lines)
    s = "0; tffInterpolation; linear\n" + _tff_line(0, frontend.tff_from_stops())
    s += _camera_line(0, QUATS[0], TRANS[0]) + "0; timestep; 0\n"
    s += _camera_line(120, QUATS[1], TRANS[1])
    s += "250; tffInterpolation; quad\n" + _tff_line(250, tff2)
    s += _camera_line(300, QUATS[2], TRANS[2]) + _camera_line(420, QUATS[3], TRANS[3])
    with open(path, "w") as f:
        f.write(s)


def test_read_view_record(tmp_path):
    prefix = str(tmp_path / "path")
    _write_record(prefix)
    views = frontend.read_view_record(prefix)
    assert len(views) == len(QUATS)
    for v, q, t in zip(views, QUATS, TRANS):
        assert v == _expected(q, t)
        assert np.allclose(v, frontend.view_matrix(q, t), atol=1e-5)
    # the second view is the project's "rot30"-style rotation about x by 30 degrees
    assert np.allclose(views[1], frontend.view_matrix(frontend.quat_from_axis_angle((1, 0, 0), 30.0)), atol=1e-5)


def test_read_interaction_log(tmp_path):
    tff2 = frontend.haze_tff()
    path = str(tmp_path / "log.txt")
    _write_log(path, tff2)
    ev = frontend.read_interaction_log(path)
    assert [k for k, _ in ev] == ["transferFunction", "camera", "timestep", "camera", "transferFunction",
                                  "camera", "camera"]
    np.testing.assert_array_equal(ev[0][1], np.asarray(frontend.tff_from_stops()).reshape(-1))
    np.testing.assert_array_equal(ev[4][1], np.asarray(tff2).reshape(-1))
    assert ev[2][1] == 0
    cams = [v for k, v in ev if k == "camera"]
    for v, q, t in zip(cams, QUATS, TRANS):
        assert v == _expected(q, t)


def test_bad_input_raises(tmp_path):
    prefix = str(tmp_path / "bad")
    _write_record(prefix, QUATS, TRANS[:3])
    with pytest.raises(ValueError):
        frontend.read_view_record(prefix)
    path = str(tmp_path / "bad.txt")
    with open(path, "w") as f:
        f.write("0; camera; 1 0 0 0, 0 0\n")    # 6 numbers
    with pytest.raises(ValueError):
        frontend.read_interaction_log(path)
    with open(path, "w") as f:
        f.write("0; camera; 1 0 0 0, 0 0 2\n0; zoom; 3\n")
    with pytest.raises(ValueError):
        frontend.read_interaction_log(path)


def test_orbit_views_quarter_steps():
    start = frontend.quat_from_axis_angle((1, 1, 0), 30.0)
    views = frontend.orbit_views((0, 1, 0), 4, start, (0.0, 0.0, 2.0))
    assert len(views) == 4
    for k, v in enumerate(views):
        want = frontend.view_matrix(frontend.quat_mul(start, frontend.quat_from_axis_angle((0, 1, 0), 90.0 * k)),
                                    (0.0, 0.0, 2.0))
        assert v == want
    assert views[0] == frontend.view_matrix(start, (0.0, 0.0, 2.0))
    assert len(set(tuple(v) for v in views)) == 4


def _dump(tmp_path, *args):
    out = tmp_path / "views.f32"
    r = subprocess.run([EXE, "--dump-views", str(out)] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    return np.fromfile(str(out), dtype=np.float32).reshape(-1, 16)


def test_cli_dump_views_equals_python(tmp_path):
    prefix = str(tmp_path / "path")
    _write_record(prefix)
    np.testing.assert_array_equal(_dump(tmp_path, "--camera-path", prefix),
                                  np.array(frontend.read_view_record(prefix), dtype=np.float32))
    log = str(tmp_path / "log.txt")
    _write_log(log, frontend.haze_tff())
    want = [v for k, v in frontend.read_interaction_log(log) if k == "camera"]
    np.testing.assert_array_equal(_dump(tmp_path, "--camera-path", log), np.array(want, dtype=np.float32))
    got = _dump(tmp_path, "--orbit", 0, 1, 0, 64, "--rotate", 1, 1, 0, 30)
    want = frontend.orbit_views((0, 1, 0), 64, frontend.quat_from_axis_angle((1, 1, 0), 30.0))
    np.testing.assert_array_equal(got, np.array(want, dtype=np.float32))
    got = _dump(tmp_path, "--orbit", 1, 0, 0, 7, "--translate", 0.1, -0.05, 1.2)
    want = frontend.orbit_views((1, 0, 0), 7, frontend.DEFAULT_ROTATION, (0.1, -0.05, 1.2))
    np.testing.assert_array_equal(got, np.array(want, dtype=np.float32))


def test_cli_rejects_bad_paths(tmp_path):
    out = str(tmp_path / "v.f32")
    prefix = str(tmp_path / "bad")
    _write_record(prefix, QUATS, TRANS[:3])
    bad_log = str(tmp_path / "bad.txt")
    with open(bad_log, "w") as f:
        f.write("0; camera; 1 0 0 0, 0 0\n")
    for args, code in ((["--camera-path", ""], 2), (["--orbit", 0, 1, 0, 0], 2), (["--camera-path", prefix], 1),
                       (["--camera-path", bad_log], 1), (["--camera-path", str(tmp_path / "missing")], 1)):
        r = subprocess.run([EXE, "--dump-views", out] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == code, (args, r.returncode, r.stderr)


def test_views_caller_compiles_against_include_alone():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "caller_views.cpp")])
