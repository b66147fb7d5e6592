"""8-bit RGBA frames through the layers, as far as that can be checked without a GPU: the four entry points in the
header, the library and the binding, the C++ methods, the command line -- and the known answers of the one
conversion everything else is compared with (frontend.quantise_rgba8)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from volumerenderercl_amd import VolumeRenderCL, _lib, frontend, tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")

ENTRY_POINTS = {
    "vrhip_quantise_rgba8": ["r", "hip_stream", "src_dev", "rows", "row_pixels", "src_stride", "dst", "dst_is_device"],
    "vrhip_render_frame_rgba8": ["r", "width", "height", "out_rgba8", "out_is_device"],
    "vrhip_frame_rgba8": ["r", "width", "height", "out_rgba8", "out_is_device"],
    "vrhip_pack_tiles_rgba8": ["r", "hip_stream", "tiles_dev", "n_slots", "tile_pixels", "scratch_dev", "msg_dev",
                               "count_dev"],
    "vrhip_assemble_batch_rgba8": ["r", "hip_stream", "msgs_dev", "world", "n_frames", "cap", "maxc", "pos_dev",
                                   "rank_slot_of_tile_dev", "width", "height", "tile_w", "tile_h", "frames_dev"],
}


def _header():
    with open(os.path.join(ROOT, "include", "vrhip.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_header_library_and_binding_agree(name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, _header())
    assert m, "include/vrhip.h does not declare %s" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ENTRY_POINTS[name]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is ctypes.c_int and len(argtypes) == len(ENTRY_POINTS[name])
    assert getattr(_lib.load(), name).argtypes == argtypes


def test_the_float_twins_take_the_same_arguments():
    """pack / assemble in 8-bit pixels take the arguments of their float counterparts."""
    for name in ("vrhip_pack_tiles", "vrhip_assemble_batch"):
        assert len(_lib.SYMBOLS[name][1]) == len(_lib.SYMBOLS[name + "_rgba8"][1])


def test_python_wrappers():
    sig = inspect.signature(VolumeRenderCL.render_frame_rgba8)
    assert list(sig.parameters) == ["self", "width", "height", "out"] and sig.parameters["out"].default is None
    sig = inspect.signature(VolumeRenderCL.quantise_rgba8)
    assert list(sig.parameters)[:3] == ["self", "frames", "out"] and sig.parameters["out"].default is None
    assert inspect.signature(VolumeRenderCL.render_batch).parameters["rgba8"].default is False
    assert inspect.signature(tiles.TileDriver.__init__).parameters["pixel_format"].default == "float"
    vr = VolumeRenderCL()            # not initialised: no GPU is touched, nothing is rendered
    assert vr.render_frame_rgba8(64, 48) is None
    assert vr.render_batch(64, 48, [1, 2], rgba8=True) is None
    with pytest.raises(ValueError):
        tiles.TileDriver(None, tiles.TileSplit(64, 64, 16, 16, 1, 0), "cpu", pixel_format="rgb565")


def test_rgba8_caller_compiles_against_include_alone():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "caller_rgba8.cpp")])


def test_host_library_defines_the_methods():
    out = subprocess.run(["nm", "-DC", os.path.join(ROOT, "volumerenderercl_amd", "libvrhost.so")], capture_output=True,
                         text=True, check=True).stdout
    defs = [l for l in out.splitlines() if " T " in l]
    assert len([l for l in defs if "VolumeRenderCL::runRaycastRGBA8(" in l]) == 1, defs
    assert len([l for l in defs if "VolumeRenderCL::frameRGBA8(" in l]) == 1, defs
    assert len([l for l in defs if "VolumeRenderCL::renderFramesRGBA8(" in l]) == 2, defs   # without / with views


def test_cli_usage_names_rgba8():
    r = subprocess.run([EXE, "--no-such-option"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--rgba8" in r.stderr


def test_cli_rejects_rgba8_with_ranks(tmp_path):
    r = subprocess.run([EXE, "--synth", "sphere", "32", "uchar", "--size", "40", "24", "--rgba8", "--ranks", "2",
                        "--out", str(tmp_path / "never_written")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2
    assert "--rgba8" in r.stderr and "--ranks" in r.stderr


# ---- the conversion's known answers

def _f32(x):
    return np.float32(x)


def _neighbours(x):
    return np.nextafter(_f32(x), _f32(-np.inf)), np.nextafter(_f32(x), _f32(np.inf))


def _product(x):
    """The correctly rounded fp32 product x * 255.0f: exact in float64 (24 + 8 significant bits), rounded once."""
    return np.float32(np.float64(x) * 255.0)


def tie_table():
    """For k in {0, 1, 2, 127, 253, 254}: a float x whose fp32 product with 255.0f is exactly k + 0.5 (found among
    the floats next to (k + 0.5) / 255) with its two fp32 neighbours, each with the byte expected from the
    product's side of the tie: below -> k, above -> k + 1, on it -> the even one of the two."""
    rows = []
    for k in (0, 1, 2, 127, 253, 254):
        x = _f32((k + 0.5) / 255.0)
        cand = [x]
        for _ in range(3):
            cand = [_neighbours(cand[0])[0]] + cand + [_neighbours(cand[-1])[1]]
        exact = [c for c in cand if _product(c) == _f32(k + 0.5)]
        if not exact:
            continue
        x = exact[0]
        for v in (_neighbours(x)[0], x, _neighbours(x)[1]):
            p = float(_product(v))
            want = k if p < k + 0.5 else k + 1 if p > k + 0.5 else (k if k % 2 == 0 else k + 1)
            rows.append((v, want))
    return rows


# computed by hand: 0.5 * 255 = 127.5, a tie, to the even 128; float32(1 / 255) * 255 = 1.00000006 -> 1;
# the smallest denormal times 255 is still far below 0.5; the clamp takes 2 and +inf to 255, -1 and -inf to 0
HAND_TABLE = [(0.0, 0), (-0.0, 0), (1.0, 255), (0.5, 128), (np.float32(1.0) / np.float32(255.0), 1), (2.0, 255),
              (-1.0, 0), (np.inf, 255), (-np.inf, 0), (np.nan, 0), (np.float32(1.4e-45), 0)]


def known_answers():
    rows = HAND_TABLE + tie_table()
    return np.array([r[0] for r in rows], dtype=np.float32), np.array([r[1] for r in rows], dtype=np.uint8)


def test_quantise_known_answers():
    x, want = known_answers()
    assert x[10] > 0 and x[10] == np.nextafter(np.float32(0), np.float32(1))      # the smallest denormal
    ties = tie_table()
    assert any(_product(v) == _f32(127.5) and w == 128 for v, w in ties)          # 0.5 itself: exists exactly
    assert len(ties) >= 3
    # ties go to the even value
    for v, w in ties:
        p = float(_product(v))
        if p == np.floor(p) + 0.5:
            assert w % 2 == 0, (v, p, w)
    got = frontend.quantise_rgba8(x)
    assert got.dtype == np.uint8 and got.shape == x.shape
    np.testing.assert_array_equal(got, want)
    # shape is kept, a pixel is the bytes R, G, B, A in memory order
    px = frontend.quantise_rgba8(np.array([[[1.0, 0.0, 0.5, 2.0 / 255.0]]], dtype=np.float32))
    assert px.shape == (1, 1, 4) and px.tobytes() == bytes([255, 0, 128, 2])
    assert int(px.view(np.uint32)[0, 0, 0]) == 255 | 0 << 8 | 128 << 16 | 2 << 24


def test_torch_statement_of_the_conversion_agrees():
    """The tile driver's torch path (CPU tensors, stand-in renderers) quantises like frontend.quantise_rgba8."""
    import torch
    x, want = known_answers()
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    allx = np.concatenate([x, bits])
    got = tiles.quantise_rgba8_torch(torch, torch.from_numpy(allx)).numpy()
    np.testing.assert_array_equal(got, frontend.quantise_rgba8(allx))
    np.testing.assert_array_equal(got[: len(want)], want)
