"""Per-frame cameras on the multi-GPU path, on CPU: `gloo` worlds of 2 and 3 ranks run the tile decomposition +
batched gather (tiles.TileDriver.submit_frames with views) with the oracle standing in for the per-tile renderer.
Every gathered frame must equal the oracle's frame of its own view and seed."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import vro
from volumerenderercl_amd import frontend, tiles

SEEDS = [11, 22222, 3333333, 44, 555]


def _views():
    return [frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30)),
            frontend.view_matrix(),
            frontend.view_matrix(frontend.quat_from_axis_angle((0.2, 1, 0.1), 75.0), (0.1, -0.05, 1.2)),
            frontend.view_matrix(frontend.quat_from_axis_angle((0, 1, 0), 20.0), (0.0, 0.0, 0.4)),
            frontend.view_matrix(frontend.DEFAULT_ROTATION, (6.0, 0.0, 2.0))]   # misses the box


def _scene():
    vol = vro.synth_volume("sphere", [32, 32, 32], vro.UCHAR)
    cam = vro.CameraParams()
    cam.viewMat[:] = frontend.view_matrix()
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

    def render_tiles(ids, out, seed=None, view=None):
        if seed is not None:
            rp.seed = seed
        if view is not None:
            cam.viewMat[:] = view
        for k, t in enumerate(ids):
            x0, y0, w, h = split.tile_rect(t)
            img, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H, tile=(x0, y0, w, h), threads=1)
            out[k, :h, :w] = torch.from_numpy(img)

    views = _views()
    drv = tiles.TileDriver(None, split, torch.device("cpu"), render_tiles_fn=render_tiles, dist=dist, batch=3,
                           sparse=sparse)
    frames = torch.zeros((3, H, W, 4)) if rank == 0 else None
    got = []
    drv.submit_frames(SEEDS[:3], views[:3])
    drv.submit_frames(SEEDS[3:], views[3:])   # (two gathers in flight)
    for n in (3, 2):
        o = drv.collect_batch(frames)
        if rank == 0:
            got += [o[i].numpy().copy() for i in range(n)]
    if rank == 0:
        q.put(got)
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world,W,H,T,sparse", [(2, 96, 64, 32, False), (3, 80, 56, 16, True)])
def test_gloo_submit_frames_views_match_oracle(world, W, H, T, sparse):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, W, H, T, q, sparse)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    vol, tff, cam, rp, rc = _scene()
    assert len(got) == len(SEEDS)
    for seed, view, frame in zip(SEEDS, _views(), got):
        rp.seed = seed
        cam.viewMat[:] = view
        want, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H)
        np.testing.assert_array_equal(frame, want)
    assert not np.array_equal(got[0], got[1])   # (the views differ)


def test_submit_frames_rejects_view_count():
    split = tiles.TileSplit(64, 64, 32, 32, 2, 0)
    drv = tiles.TileDriver(None, split, torch.device("cpu"), render_tiles_fn=lambda *a, **k: None, dist=dist,
                           batch=3)
    with pytest.raises(ValueError):
        drv.submit_frames([1, 2], [frontend.view_matrix()])
