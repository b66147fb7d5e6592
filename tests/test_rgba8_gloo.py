"""8-bit frames on the multi-GPU path, on CPU: `gloo` worlds of 2 and 3 ranks run the tile decomposition + gather
(tiles.TileDriver with pixel_format="rgba8", dense and sparse) with the oracle standing in for the per-tile
renderer.  The assembled uint8 frame must equal frontend.quantise_rgba8 of the single-rank float frame, byte for
byte, and the sparse gather must send exactly the bytes of its message layout."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import vro
from volumerenderercl_amd import frontend, tiles

SEEDS = [11, 22222]


def _scene():
    vol = vro.synth_volume("sphere", [32, 32, 32], vro.UCHAR)
    cam = vro.CameraParams()
    cam.viewMat[:] = frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30))
    cam.bbox_bl[:] = [-1, -1, -1, 0]
    cam.bbox_tr[:] = [1, 1, 1, 0]
    rp = vro.RenderingParams()
    rp.backgroundColor[:] = [1, 1, 1, 1]
    rp.modelScale[:] = [1, 1, 1, 0]
    rp.illumType, rp.useLinear, rp.seed = 1, 1, 581869302
    rc = vro.RaycastParams()
    rc.samplingRate = 1.5
    _, brf, _ = vro.brick_layout([32, 32, 32])
    rc.brickRes[:] = brf + [0]
    return vol, frontend.tff_from_stops(), cam, rp, rc


def _worker(rank, world, port, W, H, T, q, sparse):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vol, tff, cam, rp, rc = _scene()
    split = tiles.TileSplit(W, H, T, T, world, rank)

    def render_tiles(ids, out, seed=None):
        if seed is not None:
            rp.seed = seed
        for k, t in enumerate(ids):
            x0, y0, w, h = split.tile_rect(t)
            img, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H, tile=(x0, y0, w, h), threads=1)
            out[k, :h, :w] = torch.from_numpy(img)

    drv = tiles.TileDriver(None, split, torch.device("cpu"), render_tiles_fn=render_tiles, dist=dist, sparse=sparse,
                           pixel_format="rgba8")
    frame = torch.zeros((H, W, 4), dtype=torch.uint8) if rank == 0 else None
    for _ in range(2):   # two frames: buffers are reusable
        out = drv.render_frame(frame)
    first = out.numpy().copy() if rank == 0 else None
    # batched: the frames of two jitter seeds in one gather
    drvf = tiles.TileDriver(None, split, torch.device("cpu"), render_tiles_fn=render_tiles, dist=dist,
                            batch=len(SEEDS), sparse=sparse, pixel_format="rgba8")
    drvf.submit_frames(SEEDS)
    o = drvf.collect_batch(torch.zeros((len(SEEDS), H, W, 4), dtype=torch.uint8) if rank == 0 else None)
    if rank == 0:
        assert o.dtype == torch.uint8
        q.put((first, o.numpy().copy(), dict(drvf.gather_stats)))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _whole_tiles(split_of, world, frames8, T):
    """The largest number, over the ranks, of tiles of `frames8` (uint8 [n, H, W, 4]) whose pixels -- in the rank's
    tile buffer, zeroes beyond the frame's edge -- are not all equal."""
    counts = []
    for r in range(world):
        s, c = split_of(r), 0
        for f in range(frames8.shape[0]):
            for t in s.my_tiles:
                x0, y0, w, h = s.tile_rect(t)
                tile = np.zeros((T, T, 4), dtype=np.uint8)
                tile[:h, :w] = frames8[f, y0:y0 + h, x0:x0 + w]
                words = tile.view(np.uint32).reshape(-1)
                c += int((words != words[0]).any())
        counts.append(c)
    return max(counts)


@pytest.mark.parametrize("world,W,H,T,sparse", [(2, 96, 64, 32, False), (3, 80, 56, 16, False),
                                                 (2, 96, 64, 32, True), (3, 80, 56, 16, True),
                                                 (3, 160, 112, 16, True)])
def test_gloo_rgba8_gather_matches_quantised_single_rank(world, W, H, T, sparse):
    vol, tff, cam, rp, rc = _scene()
    ref, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, W, H, T, q, sparse)) for r in range(world)]
    for p in procs:
        p.start()
    got, batched, stats = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    np.testing.assert_array_equal(got, frontend.quantise_rgba8(ref))
    want = []
    for seed in SEEDS:
        rp.seed = seed
        f32, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H)
        want.append(frontend.quantise_rgba8(f32))
    want = np.stack(want)
    np.testing.assert_array_equal(batched, want)
    if not sparse:
        assert stats["batches"] == 0
        return
    # the message of the one batch: [spad slot numbers | S words | c whole tiles of P words], once per peer
    split_of = lambda r: tiles.TileSplit(W, H, T, T, world, r)
    S, P = len(SEEDS) * split_of(0).cap, T * T
    spad = (S + 3) // 4 * 4
    c = _whole_tiles(split_of, world, want, T)
    if W == 160:   # (at the smaller sizes every tile touches the silhouette; here whole ones lie outside it)
        assert 0 < c < S, (c, S)
    assert stats["batches"] == 1
    assert stats["sent_bytes"] == 4 * (spad + S + c * P) * (world - 1), (stats, spad, S, c, P)
    assert stats["dense_bytes"] == 4 * S * P * (world - 1), stats
