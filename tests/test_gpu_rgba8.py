"""8-bit RGBA frames on the GPU: the quantise kernel against the numpy statement of the conversion
(frontend.quantise_rgba8) on crafted tensors, and every way to an 8-bit frame -- vrhip_render_frame_rgba8,
render_batch(rgba8=True), the tile driver's 8-bit gather, the pack / assemble entry points, the C++ host -- against
that statement applied to the float frame the existing suite pins to the oracle.  Equality of bytes throughout."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import common
from tests.test_rgba8_abi import known_answers
from volumerenderercl_amd import UCHAR, VolumeRenderCL, frontend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "volumerenderercl_amd", "vrhip_render")
SEEDS = [3499211612, 581869302, 3890346734]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def vr():
    r = VolumeRenderCL()
    r.initialize()
    yield r
    r.close()


@pytest.fixture(scope="module")
def sphere(vr):
    """The 32^3 sphere, default transfer function, rot30 view."""
    from oracle import vro
    vr.loadVolumeArrays([vro.synth_volume("sphere", [32, 32, 32], vro.UCHAR)], UCHAR)
    vr.setTransferFunction(frontend.tff_from_stops())
    vr.updateView(common.views()["rot30"])
    return vr


def _crafted(n_pixels, seed):
    """n_pixels float4 pixels: the known-answer table, then random bit patterns reinterpreted as fp32 (NaNs,
    infinities, denormals among them)."""
    table, _ = known_answers()
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, size=4 * n_pixels, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    k = min(bits.size, table.size)
    bits[:k] = table[:k]
    return bits.reshape(n_pixels, 4)


def test_quantise_table_and_random_bit_patterns(vr):
    import torch
    table, want = known_answers()
    pad = (-table.size) % 4
    rng = np.random.default_rng(1)
    x = np.concatenate([table, np.zeros(pad, np.float32),
                        rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    assert np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[np.isfinite(x)]) < 1.2e-38).any()
    got = vr.quantise_rgba8(torch.from_numpy(x.reshape(-1, 4)).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(got[: want.size], want)
    np.testing.assert_array_equal(got, frontend.quantise_rgba8(x))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257])
def test_quantise_pixel_counts_to_host_and_device(vr, n):
    """Every pixel count around the per-lane and per-workgroup widths; the bytes behind the destination's end keep
    their sentinel."""
    import torch
    x = _crafted(n, seed=n)
    want = frontend.quantise_rgba8(x)
    src = torch.from_numpy(x).cuda()
    dst = torch.full((n + 64, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    vr.quantise_rgba8(src, dst[:n])
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[:n], want)
    assert (got[n:] == SENTINEL).all()
    host = np.full((n + 64, 4), SENTINEL, dtype=np.uint8)
    out = vr.quantise_rgba8(src, host[:n])
    assert np.shares_memory(out, host)
    np.testing.assert_array_equal(host[:n], want)
    assert (host[n:] == SENTINEL).all()


def test_quantise_strided_rows(vr):
    """rows = 3, row_pixels = 37, src_stride = 64 through the entry point itself: the rows dense in the destination,
    the source's gaps and the destination's tail untouched."""
    import torch
    rows, rp, stride = 3, 37, 64
    x = _crafted(rows * stride, seed=99).reshape(rows, stride, 4)
    gap = np.float32(-123.25)
    x[:, rp:] = gap
    src = torch.from_numpy(x).cuda()
    dst = torch.full((rows * rp + 64, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    vr._check(vr.lib.vrhip_quantise_rgba8(vr.handle, C.c_void_p(stream), C.c_void_p(src.data_ptr()), rows, rp, stride,
                                          C.c_void_p(dst.data_ptr()), 1))
    host = np.full((rows * rp + 64, 4), SENTINEL, dtype=np.uint8)
    vr._check(vr.lib.vrhip_quantise_rgba8(vr.handle, C.c_void_p(stream), C.c_void_p(src.data_ptr()), rows, rp, stride,
                                          host.ctypes.data_as(C.c_void_p), 0))
    torch.cuda.synchronize()
    want = frontend.quantise_rgba8(x[:, :rp]).reshape(rows * rp, 4)
    for got in (dst.cpu().numpy(), host):
        np.testing.assert_array_equal(got[: rows * rp], want)
        assert (got[rows * rp:] == SENTINEL).all()
    after = src.cpu().numpy()
    assert (after[:, rp:] == gap).all() and np.array_equal(after.view(np.uint32), x.view(np.uint32))


def test_quantise_argument_errors(vr):
    import torch
    src = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    dst = torch.zeros((8, 4), dtype=torch.uint8, device="cuda")
    f = vr.lib.vrhip_quantise_rgba8
    s, d = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    assert f(vr.handle, None, None, 1, 8, 8, d, 1) == 1              # VRHIP_ERR_INVALID: NULL source
    assert f(vr.handle, None, s, 1, 8, 8, None, 1) == 1              # NULL destination
    assert f(vr.handle, None, s, 1, 8, 7, d, 1) == 1                 # src_stride < row_pixels
    assert f(vr.handle, None, s, 1 << 16, 1 << 16, 1 << 16, d, 1) == 1   # rows x row_pixels overflows 32 bits
    assert vr.lib.vrhip_render_frame_rgba8(vr.handle, 8, 8, None, 0) == 1
    assert vr.lib.vrhip_pack_tiles_rgba8(vr.handle, None, s, 1, 256, None, d, d) == 1
    assert vr.lib.vrhip_assemble_batch_rgba8(vr.handle, None, None, 1, 1, 1, 4, d, d, 16, 16, 16, 16, d) == 1
    ptrs = (C.c_void_p * 1)(dst.data_ptr())
    assert vr.lib.vrhip_assemble_batch_rgba8(vr.handle, None, ptrs, 65, 1, 1, 4, d, d, 16, 16, 16, 16, d) == 1   # world > 64


@pytest.mark.parametrize("W,H", [(40, 24), (64, 64)])
def test_render_frame_rgba8_equals_quantised_float_frame(sphere, W, H):
    import torch
    vr = sphere
    vr.setSeed(SEEDS[0])
    vr.setIteration(0)
    f32 = vr.runRaycastNoGL(W, H)
    assert 0 < (f32 != f32[0, 0]).sum()          # not a blank frame
    want = frontend.quantise_rgba8(f32)
    vr.setIteration(0)
    got = vr.render_frame_rgba8(W, H)
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    np.testing.assert_array_equal(got, want)
    vr.setIteration(0)
    dev = torch.full((H + 1, W, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    vr.render_frame_rgba8(W, H, out=dev[:H])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev[:H].cpu().numpy(), want)
    assert (dev[H].cpu().numpy() == SENTINEL).all()


def test_render_frame_rgba8_keeps_the_float_accumulation(sphere):
    """Path tracer, iteration 0 then 1: the second 8-bit frame is the quantised second frame of the float
    sequence -- the frame buffer kept the unquantised first frame."""
    vr = sphere
    W, H = 40, 24
    vr.setTechnique(VolumeRenderCL.TECH_PATHTRACE)
    try:
        seq = []
        vr.setIteration(0)
        for k in range(2):
            vr.setSeed(SEEDS[k])
            seq.append(vr.runRaycastNoGL(W, H))
        assert not np.array_equal(seq[0], seq[1])
        vr.setIteration(0)
        got = []
        for k in range(2):
            vr.setSeed(SEEDS[k])
            got.append(vr.render_frame_rgba8(W, H))
        assert vr.params()[1].iteration == 2
        np.testing.assert_array_equal(got[0], frontend.quantise_rgba8(seq[0]))
        np.testing.assert_array_equal(got[1], frontend.quantise_rgba8(seq[1]))
    finally:
        vr.setTechnique(VolumeRenderCL.TECH_RAYCAST)


def test_render_batch_rgba8_frames_and_tiles(sphere):
    """Three frames with three views from one launch set: whole frames, and a tile subset with a partial tile at the
    frame's edge."""
    import torch
    vr = sphere
    W, H, T = 100, 76, 32
    v = common.views()
    views = [v["rot30"], v["default"], v["close"]]
    singles = []
    for view, seed in zip(views, SEEDS):
        vr.updateView(view)
        vr.setSeed(seed)
        vr.setIteration(0)
        singles.append(frontend.quantise_rgba8(vr.runRaycastNoGL(W, H)))
    vr.updateView(v["rot30"])
    got = vr.render_batch(W, H, SEEDS, views=views, rgba8=True)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W, 4)
    li = vr.lastLaunchInfo()
    assert li["frames"] == 3 and li["views"] == 1, li
    got = got.cpu().numpy()
    for f in range(3):
        np.testing.assert_array_equal(got[f], singles[f])
    tiles_x = (W + T - 1) // T
    ids = np.array([0, 3, 5, 11], dtype=np.uint32)      # 3: the right edge (4 columns), 11: the bottom right corner
    out = torch.full((3, len(ids), T, T, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    vr.render_batch(W, H, SEEDS, out=out, tile_w=T, tile_h=T, tile_ids=ids, views=views, rgba8=True)
    torch.cuda.synchronize()
    tl = out.cpu().numpy()
    for f in range(3):
        for k, t in enumerate(ids):
            x0, y0 = (int(t) % tiles_x) * T, (int(t) // tiles_x) * T
            w, h = min(T, W - x0), min(T, H - y0)
            np.testing.assert_array_equal(tl[f, k, :h, :w], singles[f][y0:y0 + h, x0:x0 + w])
    assert min(T, W - 3 * T) < T


def test_pack_and_assemble_synthetic_tiles(vr):
    """Three 16 x 16 tiles through vrhip_pack_tiles_rgba8 / vrhip_message_positions / vrhip_assemble_batch_rgba8: one
    constant, one constant only after quantisation (pixels less than 1/510 apart), one that differs in a single
    pixel's alpha -- one whole tile travels."""
    import torch
    T, S = 16, 3
    P = T * T
    tiles = np.zeros((S, P, 4), dtype=np.float32)
    tiles[0] = [0.25, 0.5, 0.75, 1.0]
    rng = np.random.default_rng(3)
    tiles[1] = np.float32(100.0 / 255.0) + (rng.random((P, 4)).astype(np.float32) - 0.5) * np.float32(1.0 / 600.0)
    tiles[2] = [0.1, 0.2, 0.3, 1.0]
    tiles[2, 77, 3] = 0.5
    q = frontend.quantise_rgba8(tiles)
    assert not (tiles[1] == tiles[1][0]).all() and (q[1] == 100).all()
    assert np.abs(tiles[1] - np.float32(100.0 / 255.0)).max() < 1.0 / 1020.0     # any two less than 1/510 apart
    src = torch.from_numpy(tiles).cuda()
    spad = (S + 3) // 4 * 4
    msg = torch.full((spad + S + S * P + 16,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(S, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vr._check(vr.lib.vrhip_pack_tiles_rgba8(vr.handle, stream, C.c_void_p(src.data_ptr()), S, P,
                                            C.c_void_p(scratch.data_ptr()), C.c_void_p(msg.data_ptr()),
                                            C.c_void_p(count.data_ptr())))
    torch.cuda.synchronize()
    assert int(count.item()) == 1
    m = msg.cpu().numpy()
    assert m[0] == 2                                                  # the slot list: tile 2
    words = q.reshape(S, P, 4).view(np.uint32).reshape(S, P)
    np.testing.assert_array_equal(m[spad: spad + S].view(np.uint32), words[:, 0])
    np.testing.assert_array_equal(m[spad + S: spad + S + P].view(np.uint32), words[2])
    assert (m[spad + S + S * P:] == -1).all()                         # nothing behind the worst case
    # the frame: the three tiles side by side, 48 x 16
    W, H = 3 * T, T
    pos = torch.zeros(S, dtype=torch.int32, device="cuda")
    ptrs = (C.c_void_p * 1)(msg.data_ptr())
    counts = (C.c_uint32 * 1)(1)
    vr._check(vr.lib.vrhip_message_positions(vr.handle, stream, ptrs, counts, 1, S, C.c_void_p(pos.data_ptr())))
    rank_slot = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    frame = torch.full((H + 1, W, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    vr._check(vr.lib.vrhip_assemble_batch_rgba8(vr.handle, stream, ptrs, 1, 1, S, spad, C.c_void_p(pos.data_ptr()),
                                                C.c_void_p(rank_slot.data_ptr()), W, H, T, T, C.c_void_p(frame.data_ptr())))
    torch.cuda.synchronize()
    assert pos.cpu().tolist() == [-1, -1, 0]
    got = frame.cpu().numpy()
    for s in range(S):
        np.testing.assert_array_equal(got[:H, s * T:(s + 1) * T], q[s].reshape(T, T, 4))
    assert (got[H] == SENTINEL).all()


def test_tile_driver_rgba8_over_a_world_of_one():
    """TileDriver(force_gather=True, pixel_format="rgba8") on a world-size-1 `nccl` group: sparse (the two new entry
    points), dense (the torch path with the library's quantiser) and the batched form; every frame equals the
    quantised full-frame render.  In a process of its own: the process group is global state."""
    code = r"""
import numpy as np, torch, torch.distributed as dist
from tests import common
from volumerenderercl_amd import UCHAR, VolumeRenderCL, frontend, tiles
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:PORT", rank=0, world_size=1, device_id=dev)
vr = VolumeRenderCL(); vr.initialize()
vol = common.noise_volume((56, 48, 40), UCHAR, seed=5, smooth=False)
vr.loadVolumeArrays([vol], UCHAR)
vr.setTransferFunction(common.tffs()["default"])
vr.updateView(common.views()["rot30"])
W, H, T = 200, 136, 32                     # ragged right / bottom tiles
seeds = [3499211612, 581869302, 3890346734]
full = []
for sd in seeds:
    vr.setSeed(sd); vr.setIteration(0); full.append(frontend.quantise_rgba8(vr.runRaycastNoGL(W, H)))
split = tiles.TileSplit(W, H, T, T, 1, 0)
frame = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
for sparse in (True, False):
    drv = tiles.TileDriver(vr, split, dev, force_gather=True, sparse=sparse, pixel_format="rgba8")
    assert drv._gpu_pack()
    vr.setSeed(seeds[0]); vr.setIteration(0)
    assert np.array_equal(drv.render_frame(frame).cpu().numpy(), full[0]), sparse
    if sparse:
        st = drv.gather_stats
        assert st["batches"] == 1 and 0 < st["sent_bytes"] < st["dense_bytes"] == 4 * split.cap * T * T, st
    drvb = tiles.TileDriver(vr, split, dev, batch=3, force_gather=True, sparse=sparse, pixel_format="rgba8")
    frames = torch.zeros((3, H, W, 4), dtype=torch.uint8, device=dev)
    drvb.submit_frames(seeds); drvb.collect_batch(frames); torch.cuda.synchronize()
    got = frames.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], full[i]), (sparse, i)
# the full-frame launch of a world of one that does not gather
drv1 = tiles.TileDriver(vr, split, dev, pixel_format="rgba8")
vr.setSeed(seeds[1]); vr.setIteration(0)
out = drv1.render_frame(frame); torch.cuda.synchronize()
assert np.array_equal(out.cpu().numpy(), full[1])
vr.close()
dist.destroy_process_group()
print("RGBA8_WORLD1_OK")
"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    p = subprocess.run([sys.executable, "-c", code.replace("PORT", str(port))], cwd=ROOT,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RGBA8_WORLD1_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


class _Hub:
    """One process plays every rank of a world: the collectives of TileDriver over tensors the ranks deposit."""

    def __init__(self, world):
        self.world, self.counts, self.msgs, self.outs = world, {}, {}, {}

    class Done:
        def wait(self):
            pass

    def for_rank(self, rank):
        hub = self

        class D:
            def all_gather(self, out_list, t, async_op=False):
                hub.counts[rank] = t.clone()
                hub.outs[rank] = out_list
                return hub.Done()

            def gather(self, t, gather_list, dst=0, async_op=False):
                hub.msgs[rank] = t
                if gather_list is not None:
                    for r in range(hub.world):
                        gather_list[r].copy_(hub.msgs[r])
                return hub.Done()
        return D()


@pytest.mark.parametrize("W,H,T,batch", [(96, 64, 32, 1), (80, 56, 16, 3)])
def test_sparse_rgba8_gather_of_two_ranks_with_an_odd_slot_count(sphere, W, H, T, batch):
    """A world of two rehearsed in one process, batch x cap not a multiple of 4 (3 and 3 x 10 = 30): rank 0 receives the
    messages as the rows of one block, and the second row has to be as well aligned as the first for
    vrhip_assemble_batch_rgba8."""
    import torch
    from volumerenderercl_amd import tiles
    vr = sphere
    dev = torch.device("cuda", 0)
    world = 2
    hub = _Hub(world)
    splits = [tiles.TileSplit(W, H, T, T, world, k) for k in range(world)]
    assert (batch * splits[0].cap) % 4 != 0
    drivers = [tiles.TileDriver(vr, splits[k], dev, dist=hub.for_rank(k), batch=batch, sparse=True, pixel_format="rgba8")
               for k in range(world)]
    seeds = SEEDS[:batch]
    vr.updateView(common.views()["rot30"])
    for k in (1, 0):
        assert drivers[k]._gpu_pack()
        drivers[k].submit_frames(seeds)
    for k in (1, 0):
        for r in range(world):
            hub.outs[k][r].copy_(hub.counts[r])
    drivers[1]._issue_payloads()
    frames = torch.full((batch, H, W, 4), SENTINEL, dtype=torch.uint8, device=dev)
    drivers[0].collect_batch(frames)
    torch.cuda.synchronize()
    assert drivers[0]._last_assembled["keep"] is not None          # the fused kernel assembled, not the torch path
    assert drivers[0]._recv[0][1].data_ptr() % 16 == 0
    got = frames.cpu().numpy()
    for i, seed in enumerate(seeds):
        vr.setSeed(seed)
        vr.setIteration(0)
        np.testing.assert_array_equal(got[i], frontend.quantise_rgba8(vr.runRaycastNoGL(W, H)), err_msg=str(i))
    vr.setSeed(None)


def test_cpp_host_methods_run(tmp_path):
    """VolumeRenderCL::runRaycastRGBA8 / frameRGBA8 / renderFramesRGBA8 executed (tests/cxx/run_rgba8.cpp, built here,
    in a child process): two accumulating path-tracer frames as bytes equal the conversion of the same two frames
    from runRaycastNoGL on a second renderer -- same seeds drawn, iteration advanced -- and a launch set's bytes equal
    the conversion of its floats."""
    exe = str(tmp_path / "run_rgba8")
    pkg = os.path.join(ROOT, "volumerenderercl_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cxx", "run_rgba8.cpp"), "-o", exe, "-L", pkg, "-lvrhost", "-lvrhip",
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    prefix = str(tmp_path / "o")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, prefix], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "iteration 2 2" in r.stdout, r.stdout
    W, H = 40, 24
    a = [np.fromfile("%s.a%d.f32" % (prefix, k), dtype=np.float32).reshape(H, W, 4) for k in range(2)]
    b = [np.fromfile("%s.b%d.u8" % (prefix, k), dtype=np.uint8).reshape(H, W, 4) for k in range(2)]
    assert not np.array_equal(a[0], a[1]) and (a[1] != a[1][0, 0]).any()
    for k in range(2):
        np.testing.assert_array_equal(b[k], frontend.quantise_rgba8(a[k]), err_msg="frame %d" % k)
    np.testing.assert_array_equal(np.fromfile(prefix + ".a1.u8", dtype=np.uint8).reshape(H, W, 4), b[1])
    s32 = np.fromfile(prefix + ".set.f32", dtype=np.float32).reshape(3, H, W, 4)
    s8 = np.fromfile(prefix + ".set.u8", dtype=np.uint8).reshape(3, H, W, 4)
    assert not np.array_equal(s32[0], s32[1])
    np.testing.assert_array_equal(s8, frontend.quantise_rgba8(s32))


def test_cli_rgba8(tmp_path):
    """vrhip_render --rgba8: PREFIX.rgba.u8 is the conversion of PREFIX.rgba.f32 from the same invocation, PREFIX.ppm
    carries its R, G, B bytes; frame by frame and in launch sets."""
    W, H = 40, 24
    prefix = str(tmp_path / "one")
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, "--synth", "sphere", "32", "uchar", "--size", str(W), str(H),
                        "--rgba8", "--out", prefix], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout, r.stderr)
    f32 = np.fromfile(prefix + ".rgba.f32", dtype=np.float32).reshape(H, W, 4)
    u8 = np.fromfile(prefix + ".rgba.u8", dtype=np.uint8).reshape(H, W, 4)
    assert (f32 != f32[0, 0]).any()
    np.testing.assert_array_equal(u8, frontend.quantise_rgba8(f32))
    with open(prefix + ".ppm", "rb") as f:
        ppm = f.read()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert ppm.startswith(head) and ppm[len(head):] == u8[:, :, :3].tobytes()
    assert not os.path.exists(prefix + ".frames.rgba.u8")
    # the progressive path tracer's image: the bytes of the accumulated frame
    prefix = str(tmp_path / "pt")
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, "--synth", "sphere", "32", "uchar", "--size", str(W), str(H),
                        "--pathtrace", "--frames", "4", "--rgba8", "--out", prefix], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout, r.stderr)
    f32 = np.fromfile(prefix + ".rgba.f32", dtype=np.float32).reshape(H, W, 4)
    np.testing.assert_array_equal(np.fromfile(prefix + ".rgba.u8", dtype=np.uint8).reshape(H, W, 4),
                                  frontend.quantise_rgba8(f32))
    # launch sets of an orbit: every frame
    prefix = str(tmp_path / "orbit")
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, "--synth", "sphere", "32", "uchar", "--size", str(W), str(H),
                        "--orbit", "0", "1", "0", "5", "--frames-per-launch", "2", "--rgba8", "--out", prefix],
                       capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout, r.stderr)
    f32 = np.fromfile(prefix + ".frames.rgba.f32", dtype=np.float32).reshape(5, H, W, 4)
    u8 = np.fromfile(prefix + ".frames.rgba.u8", dtype=np.uint8).reshape(5, H, W, 4)
    assert not np.array_equal(f32[0], f32[2])
    np.testing.assert_array_equal(u8, frontend.quantise_rgba8(f32))
    np.testing.assert_array_equal(np.fromfile(prefix + ".rgba.u8", dtype=np.uint8).reshape(H, W, 4), u8[4])
