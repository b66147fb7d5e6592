#!/usr/bin/env python3
"""tools/rgba8_time.py [VIEWPORT] -- what 8-bit frames cost and save, on one GPU; prints one JSON line.  Every time is
the median of 20 after 3 warm-ups.
  quantise_*      the quantise kernel alone (HIP events), against the 20 bytes per pixel it moves; the one-frame case
                  (20 MB) is small enough to stay in the 256 MiB Infinity Cache between repetitions (expected, not
                  measured here), the 32-frame case (671 MB) is not
  to_host_*       frames per second into pinned host memory for 32-frame launch sets of the 2048^3 shells headline:
                  render + (quantise +) copy, host clock around a synchronised set
  frame_*         vrhip_render_frame_rgba8 against vrhip_render_frame for one frame left on the device (host clock)
  gather_*        the sparse gather's sent bytes per frame for the 8-rank split of that frame, float against rgba8 --
                  a ONE-GPU REHEARSAL: one process renders and packs all eight shares, nothing travels"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from volumerenderercl_amd import VolumeRenderCL, frontend, tiles

V = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
F, T, WORLD, WARM, REPS = 32, 64, 8, 3, 20
dev = torch.device("cuda", 0)
vr = VolumeRenderCL(); vr.initialize()
vr.synthVolume("shells", (2048,) * 3, 0)
vr.setTransferFunction(frontend.tff_from_stops())
vr.updateView(frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30.0)))
vr.setRoundBudget(48)
vr.set_stream(torch.cuda.current_stream().cuda_stream)
mt = frontend.Mt19937()
seeds = [mt() for _ in range(F)]


def median_of(fn):
    for _ in range(WARM):
        fn()
    return statistics.median(fn() for _ in range(REPS))


def host_clock(fn):
    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    return timed


out = {"tool": "rgba8_time", "device": vr.getCurrentDeviceName(), "viewport": V, "frames_per_set": F,
       "source_hash": vr.lib.vrhip_build_source_hash().decode(), "reps": REPS, "warmups": WARM}

# ---- the kernel alone
frames = torch.zeros((F, V, V, 4), dtype=torch.float32, device=dev)
vr.render_batch(V, V, seeds, frames.data_ptr())
bytes8 = torch.empty((F, V, V, 4), dtype=torch.uint8, device=dev)
for n in (1, F):
    def kernel(n=n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); vr.quantise_rgba8(frames[:n], bytes8[:n]); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    t = median_of(kernel)
    out["quantise_%dx%d2_ms" % (n, V)] = round(t * 1e3, 5)
    out["quantise_%dx%d2_GBps" % (n, V)] = round(20.0 * n * V * V / t / 1e9, 1)

# ---- launch sets to host memory
host32 = torch.empty((F, V, V, 4), dtype=torch.float32).pin_memory()
host8 = torch.empty((F, V, V, 4), dtype=torch.uint8).pin_memory()


def set_float():
    vr.render_batch(V, V, seeds, frames.data_ptr())
    host32.copy_(frames, non_blocking=True)


def set_rgba8():
    vr.render_batch(V, V, seeds, out=bytes8, rgba8=True)
    host8.copy_(bytes8, non_blocking=True)


out["to_host_float_fps"] = round(F / median_of(host_clock(set_float)), 1)
out["to_host_rgba8_fps"] = round(F / median_of(host_clock(set_rgba8)), 1)
assert torch.equal(host8, torch.from_numpy(frontend.quantise_rgba8(host32.numpy())))

# ---- one frame
vr.setRoundBudget(10)
vr.setSeed(seeds[0])
one8 = torch.empty((V, V, 4), dtype=torch.uint8, device=dev)


def frame_float():
    vr.setIteration(0); vr.runRaycast(V, V)


def frame_rgba8():
    vr.setIteration(0); vr.render_frame_rgba8(V, V, out=one8)


out["frame_float_ms"] = round(median_of(host_clock(frame_float)) * 1e3, 4)
out["frame_rgba8_ms"] = round(median_of(host_clock(frame_rgba8)) * 1e3, 4)
vr.setRoundBudget(48)


# ---- the 8-rank sparse gather, rehearsed: one process plays all ranks (as tools/assemble_time.py)
class Hub:
    def __init__(self):
        self.counts, self.msgs, self.outs = {}, {}, {}

    class Done:
        def wait(self):
            pass

    def for_rank(self, rank):
        hub = self

        class D:
            def all_gather(self, out_list, t, async_op=False):
                hub.counts[rank] = t.clone(); hub.outs[rank] = out_list
                return hub.Done()

            def gather(self, t, gather_list, dst=0, async_op=False):
                hub.msgs[rank] = t
                if gather_list is not None:
                    for r in range(WORLD):
                        gather_list[r].copy_(hub.msgs[r])
                return hub.Done()
        return D()


del frames, bytes8, host32, host8
G = 4      # frames per gather of the rehearsal
for fmt in ("float", "rgba8"):
    hub = Hub()
    splits = [tiles.TileSplit(V, V, T, T, WORLD, k) for k in range(WORLD)]
    drivers = [tiles.TileDriver(vr, splits[k], dev, dist=hub.for_rank(k), batch=G, sparse=True, pixel_format=fmt)
               for k in range(WORLD)]
    order = list(range(1, WORLD)) + [0]
    for k in order:
        d = drivers[k]
        vr.render_batch(V, V, seeds[:G], d.local[0].data_ptr(), T, T, splits[k].my_tiles, frame_stride=splits[k].cap * T * T)
        d.next_buf = 1
        d._start_gather(0, G)
    for k in order:
        for r in range(WORLD):
            hub.outs[k][r].copy_(hub.counts[r])
    for k in order:
        drivers[k]._issue_payloads()
    torch.cuda.synchronize()
    st = drivers[1].gather_stats        # a peer: its message to rank 0, counted once per peer
    out["gather_%s_sent_bytes_per_frame" % fmt] = st["sent_bytes"] // G
    out["gather_%s_dense_bytes_per_frame" % fmt] = st["dense_bytes"] // G
    if fmt == "rgba8":
        got = torch.zeros((G, V, V, 4), dtype=torch.uint8, device=dev)
        assert drivers[0]._assemble_fused(drivers[0].pending[0], got)
        torch.cuda.synchronize()
        vr.setSeed(seeds[1]); vr.setIteration(0)
        assert (got[1].cpu().numpy() == frontend.quantise_rgba8(vr.runRaycastNoGL(V, V))).all()
    del drivers
out["gather_note"] = "one-GPU rehearsal of the 8-rank split, %d frames per gather, %d x %d tiles" % (G, T, T)
print(json.dumps(out))
