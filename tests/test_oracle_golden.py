"""Pins the CPU oracle: (1) against the reference itself where it builds with no stand-ins
(oracle/_ref: random.cl RNG), through the outputs recorded from it in tests/golden/reference_outputs.json
(oracle/gen_reference_outputs.py); (2) against the known-answer values the compiled reference produced
(tests/golden/survey_kats.json); (3) host-side sizing rules."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from oracle import vro

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "survey_kats.json")))


def recorded(section):
    """Outputs of the compiled reference (read when a test runs: oracle/gen_reference_outputs.py imports this module
    to write the file)."""
    with open(os.path.join(HERE, "golden", "reference_outputs.json")) as f:
        return json.load(f)[section]


def test_rng_kats():
    L = vro.lib()
    for x, out in KATS["ParallelRNG"].items():
        assert L.vro_parallel_rng(int(x)) == out
    for k in KATS["ParallelRNG3"]:
        assert L.vro_parallel_rng3(k["x"], k["y"], k["z"]) == k["out"]
    for v, out in KATS["mapUintFloat"].items():
        assert L.vro_map_uint_float(int(v)) == out
    from volumerenderercl_amd import frontend
    mt = frontend.Mt19937()
    assert [mt() for _ in range(3)] == KATS["mt19937_default_first3"]


def rng_streams(parallel_rng, map_uint_float, parallel_rng3):
    """sha256 of each function's outputs (uint32 / float32 bytes, in order) over 22003 arguments and 5728 triples."""
    h = {name: hashlib.sha256() for name in ("ParallelRNG", "mapUintFloat", "ParallelRNG3")}
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.arange(0, 2000), rng.integers(0, 2 ** 32, 20000),
                         [2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1]]).astype(np.uint64)
    for x in xs:
        x = int(x)
        h["ParallelRNG"].update(np.uint32(parallel_rng(x)).tobytes())
        h["mapUintFloat"].update(np.float32(map_uint_float(x)).tobytes())
    tr = rng.integers(0, 2 ** 32, (5000, 3))
    for a, b, c in tr:
        h["ParallelRNG3"].update(np.uint32(parallel_rng3(int(a), int(b), int(c))).tobytes())
    for gx in range(0, 1032, 37):
        for gy in range(0, 1032, 41):
            h["ParallelRNG3"].update(np.uint32(parallel_rng3(gx, gy, 3499211612)).tobytes())
    return {name: d.hexdigest() for name, d in h.items()}


def test_rng_bit_exact_vs_compiled_reference():
    """random.cl compiled from the reference's own source (no stand-ins, RTLD_LAZY): the oracle's outputs hash
    like the reference's on the same arguments."""
    L = vro.lib()
    assert rng_streams(L.vro_parallel_rng, L.vro_map_uint_float, L.vro_parallel_rng3) == recorded("rng")


def test_intersect_bbox_kat():
    k = KATS["intersectBBox"]
    f3 = lambda v: (C.c_float * 3)(*v)
    tn, tf = C.c_float(), C.c_float()
    hit = vro.lib().vro_intersect_bbox(f3(k["orig"]), f3(k["dir"]), f3(k["lower"]), f3(k["upper"]),
                                       C.byref(tn), C.byref(tf))
    assert hit == k["hit"]
    assert abs(tn.value - k["tnear"]) < 2e-7 and abs(tf.value - k["tfar"]) < 3e-7


def test_generate_bricks_kat():
    """8^3 volume, 2^3 brick image: last voxel plane excluded."""
    k = KATS["generateBricks_8cube"]
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    vol = ((x + 8 * y + 64 * z) % 256).astype(np.uint8)
    out = np.zeros((2, 2, 2, 2), dtype=np.uint8)
    u3 = lambda v: (C.c_uint32 * 3)(*v)
    rc = vro.lib().vro_generate_bricks(vol.ctypes.data_as(C.c_void_p), u3([8, 8, 8]), vro.UCHAR,
                                       u3(k["brick_image"]), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    np.testing.assert_array_equal(out[..., 0], np.array(k["min"]))
    np.testing.assert_array_equal(out[..., 1], np.array(k["max"]))


def test_background_pixels_kat():
    """volumeRender entry (volumeraycast.cl:589-683): RNG jitter, padded-grid NDC, view
    transform, modelScale, gradient background -- all rays miss the moved clip box."""
    k = KATS["volumeRender_background"]
    cam = vro.CameraParams()
    cam.viewMat[:] = k["viewMat"]
    cam.bbox_bl[:] = k["bbox_bl"] + [0]
    cam.bbox_tr[:] = k["bbox_tr"] + [0]
    cam.ortho = k["ortho"]
    rp = vro.RenderingParams()
    rp.backgroundColor[:] = k["background"]
    rp.modelScale[:] = k["modelScale"] + [0]
    rp.illumType, rp.useLinear, rp.useGradient, rp.seed = 1, 1, k["useGradient"], k["seed"]
    rc = vro.RaycastParams()
    rc.samplingRate = 1.5
    rc.brickRes[:] = [8, 8, 8, 0]
    vol = np.zeros((8, 8, 8), np.uint8)
    tff = np.zeros((1024, 4), np.uint8)
    img, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=True, W=k["W"], H=k["H"])
    assert st["rays_hit"] == 0
    np.testing.assert_allclose(img[0, 0], k["pixel_0_0"], atol=1.5e-7, rtol=0)
    np.testing.assert_allclose(img[11, 19], k["pixel_19_11"], atol=1.5e-7, rtol=0)


def test_round_pow2_and_brick_layout():
    L = vro.lib()
    # volumerendercl.cpp:39-54: nearest of the two surrounding powers of two
    expect = {0: 0, 1: 1, 2: 2, 3: 4, 4: 4, 5: 4, 6: 8, 7: 8, 8: 8, 11: 8, 12: 16, 16: 16, 32: 32}
    for n, e in expect.items():
        assert L.vro_round_pow2(n) == e, n
    assert vro.brick_layout([256, 256, 256]) == ([4, 4, 4], [64.0, 64.0, 64.0], [64, 64, 64])
    assert vro.brick_layout([1024] * 3) == ([16] * 3, [64.0] * 3, [64] * 3)
    assert vro.brick_layout([2048] * 3) == ([32] * 3, [64.0] * 3, [64] * 3)
    assert vro.brick_layout([250, 129, 30]) == ([4, 2, 1], [62.5, 64.5, 30.0], [63, 65, 30])
    assert L.vro_padded(512) == 520 and L.vro_padded(1024) == 1032 and L.vro_padded(20) == 24


def test_calc_scaling():
    assert vro.calc_scaling([256, 256, 128], [1.0, 1.0, 1.0]) == [1.0, 1.0, 2.0]
    assert vro.calc_scaling([100, 100, 50], [1.0, 1.0, 2.0]) == [1.0, 1.0, 1.0]
    ms = vro.calc_scaling([64, 32, 16], [0.5, 1.0, 3.0])
    np.testing.assert_allclose(ms, [96 / 64, 96 / 64, 1.0], rtol=1e-6)


def test_powr_definition():
    """Parity definition of native_powr: exact at the ends, accurate in between."""
    L = vro.lib()
    for y in (1 / 1.5, 40.0, 0.2, 3.0):
        assert L.vro_powr(1.0, y) == 1.0
        assert L.vro_powr(0.0, y) == 0.0
    xs = np.linspace(1e-4, 1.0, 4001, dtype=np.float32)
    for y, tol in ((np.float32(1 / 1.5), 6e-7), (np.float32(40.0), 2e-5)):
        got = np.array([L.vro_powr(float(x), float(y)) for x in xs], dtype=np.float64)
        ref = np.power(xs.astype(np.float64), float(y))
        m = ref > 1e-30
        assert np.max(np.abs(got[m] - ref[m]) / ref[m]) < tol


def test_prefix_sum():
    tff = np.zeros((1024, 4), np.uint8)
    tff[:, 3] = np.arange(1024) % 251
    np.testing.assert_array_equal(vro.prefix_sum(tff), np.cumsum(tff[:, 3].astype(np.uint32)))


# ---- the builtin-free functions of the reference's kernel file itself -----------------
KFREE = json.load(open(os.path.join(HERE, "golden", "kernel_free.json")))


def _u4(st):
    return (C.c_uint32 * 4)(*[int(v) for v in st])


def test_hybrid_rng_and_box_edges_match_the_committed_reference_outputs():
    """tests/golden/kernel_free.json: what volumeraycast.cl's own ui_randStep / lcgStep /
    hybridui_rand (:48-80, calcAO's generator) and checkBoundingBox (:323-343, showEss) returned when
    the compiled reference was run here (oracle/gen_kernel_golden.py)."""
    L = vro.lib()
    for ch in KFREE["hybridui_rand_chains"]:
        st = _u4(ch["state"])
        for want in ch["draws_hex"]:
            got = L.vro_hybrid_rand(st)
            assert float(np.float32(got)).hex() == want
        assert list(st) == ch["final_state"]
    for k in KFREE["steps"]:
        st = _u4(k["state"])
        r = L.vro_ui_rand_step(st, *k["args"]) if k["fn"] == "ui_randStep" else L.vro_lcg_step(st, *k["args"])
        assert r == k["ret"] and list(st) == k["after"], k
    f3 = lambda v: (C.c_float * 3)(*v)
    for k in KFREE["checkBoundingBox"]:
        assert L.vro_check_bounding_box(f3(k["pos"]), f3(k["voxLen"]), k["bound"][0], k["bound"][1]) == k["ret"], k


def kernel_free_streams(f):
    """sha256 of the outputs (and advanced states) of the kernel file's builtin-free functions over 10^5 generator
    states and 20000 positions around the unit box's edges.  f maps hybrid_rand, ui_rand_step, lcg_step, parallel_rng,
    parallel_rng3 and check_bounding_box to the oracle's functions or to the compiled reference's."""
    h = {name: hashlib.sha256() for name in ("hybridui_rand", "steps", "ParallelRNG", "checkBoundingBox")}
    rng = np.random.default_rng(7)
    states = rng.integers(0, 2 ** 32, (100000, 4), dtype=np.uint64)
    states[:64, :] = np.arange(64, dtype=np.uint64)[:, None]           # small states
    states[64:128, 1:] = 0xFFFFFFFF
    for i, st in enumerate(states):
        a = _u4(st)
        h["hybridui_rand"].update(np.float32(f["hybrid_rand"](a)).tobytes() + bytes(a))
        if i % 8 == 0:     # a second draw from the advanced state, and the single steps
            h["hybridui_rand"].update(np.float32(f["hybrid_rand"](a)).tobytes())
            for args in ((0, 13, 19, 12, 4294967294), (1, 2, 25, 4, 4294967288), (2, 3, 11, 17, 4294967280)):
                a = _u4(st)
                h["steps"].update(np.uint32(f["ui_rand_step"](a, *args)).tobytes() + bytes(a))
            a = _u4(st)
            h["steps"].update(np.uint32(f["lcg_step"](a, 1664525, 1013904223)).tobytes() + bytes(a))
            x, y, z = int(st[0]), int(st[1]), int(st[2])
            h["ParallelRNG"].update(np.uint32(f["parallel_rng"](x)).tobytes() +
                                    np.uint32(f["parallel_rng3"](x, y, z)).tobytes())
    f3 = lambda v: (C.c_float * 3)(*v)
    for _ in range(20000):
        vox = rng.choice([1 / 32, 1 / 48, 1 / 256, 1 / 100], 3).astype(np.float32)
        pos = (rng.choice([0.0, 1.0, 0.5], 3) + rng.normal(0, 1.5, 3) * vox).astype(np.float32)
        b0, b1 = float(np.float32(rng.random() * 0.3)), float(np.float32(0.7 + rng.random() * 0.3))
        h["checkBoundingBox"].update(np.int32(f["check_bounding_box"](f3(pos), f3(vox), b0, b1)).tobytes())
    return {name: d.hexdigest() for name, d in h.items()}


def test_hybrid_rng_bit_exact_vs_compiled_reference_kernel_file():
    """volumeraycast.cl compiled from the reference's own source (66 OpenCL builtins left undefined,
    RTLD_LAZY, nothing stands in for them): the functions that reach none of them, over 10^5 states --
    the oracle's outputs hash like the reference's (recorded in tests/golden/reference_outputs.json)."""
    L = vro.lib()
    got = kernel_free_streams({"hybrid_rand": L.vro_hybrid_rand, "ui_rand_step": L.vro_ui_rand_step,
                               "lcg_step": L.vro_lcg_step, "parallel_rng": L.vro_parallel_rng,
                               "parallel_rng3": L.vro_parallel_rng3, "check_bounding_box": L.vro_check_bounding_box})
    assert got == recorded("kernel_free")


def test_list_of_builtin_free_reference_functions():
    """What can be pinned is exactly what oracle/ref_kernel_free.py finds in the compiled object (its analysis,
    recorded in tests/golden/reference_outputs.json): nothing that needs an OpenCL builtin is executed, and nothing
    executable is left out."""
    res = recorded("kernel_object_analysis")
    free = sorted(f for f, undefined in res.items() if not undefined)
    assert free == sorted(["ParallelRNG", "ParallelRNG2", "ParallelRNG3", "map256", "mapUintFloat", "ui_randStep",
                           "lcgStep", "hybridui_rand", "getf4", "checkBoundingBox"])
    assert len(res["volumeRender"]) >= 50 and res["generateBricks"] and res["intersectBBox"]
