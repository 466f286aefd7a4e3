"""Per-wave timeline of one persistent depth-0 launch (development probe).

    python tools/persistent_trace.py [CONFIG] [N_VIEWS[,N_VIEWS...]] [BUILD]

BUILD (default "phase") is an _ab build made with
`tools/ablate.sh flags phase "-DRT_PHASE_TRACE"`. Lane 0 of every resident
wave of render_persistent0 records the 100 MHz real-time clock at kernel entry
(slot 0), after the staging barrier (13), at the start of its first chunk (1)
and of its first single tile (14) and when it leaves the loop (7); it counts its
refills (10), sums their time (11) and keeps the longest (12), and counts its
chunks (15) and tiles (9); slot 8 is HW_ID with XCC_ID above it (slots 2-6 are
the tile's own stamps). Prints the table DESIGN.md §3 has for the queued
launch: prologue, ramp, time in refills per wave, idle after a wave's last
tile (mean, by queue, by XCC and by SIMD) and the span, plus the wave-time per
tile the schedule model (tools/model/persistent_model.py) takes.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import openglraytracer_amd as rt  # noqa: E402
from oracle import scenes  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "config2"
counts = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "9,64,256").split(",")]
name = sys.argv[3] if len(sys.argv) > 3 else "phase"
L = C.CDLL(os.path.join(ROOT, "_ab", name, "libopenglraytracer_amd.so"))
vp, i = C.c_void_p, C.c_int
L.rt_create.argtypes = [i, vp]
L.rt_scene_create.argtypes = [vp, vp, i, vp, i, vp, i, vp]
L.rt_context_set.argtypes = [vp, i, i]
L.rt_render_batch.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, vp, vp]
L.rt_debug_phase_read.argtypes = [vp, C.c_size_t]
L.rt_debug_last_queued.argtypes = [vp]
L.rt_debug_persistent_queue.argtypes = [i, i, vp]


def queue_of(g):
    """the queue of each global wave of the grid (the kernel's own function)"""
    o = np.zeros(3, np.int32)
    res = []
    for x in g:
        assert L.rt_debug_persistent_queue(int(x), int(g.max()) + 1, o.ctypes.data) == 0
        res.append(int(o[0]))
    return np.array(res)


ctx = C.c_void_p()
assert L.rt_create(0, C.byref(ctx)) == 0
assert L.rt_context_set(ctx, rt.abi.RT_OPT_PERSISTENT0, 1 << 16) == 0  # forced: the whole resident grid
build, w, h, depth = scenes.CONFIGS[cfg]
assert depth == 0, "the probe reads the persistent depth-0 grid"
objs, mats, lights = build(), rt.reference_materials(), rt.reference_lights()
sc = C.c_void_p()
assert L.rt_scene_create(ctx, (rt.Object * len(objs))(*objs), len(objs), (rt.Material * len(mats))(*mats), len(mats),
                         (rt.Light * len(lights))(*lights), len(lights), C.byref(sc)) == 0
stream = torch.cuda.Stream()
slots = 8 * 4 * 256  # resident waves at 8 waves per SIMD (upper bound)
us = 0.01  # 100 MHz ticks
for n_views in counts:
    views = (rt.View * n_views)(*[rt.make_view(None, k / 60.0) for k in range(n_views)])
    out = torch.empty((n_views, h, w, 4), dtype=torch.float32, device="cuda")
    for _ in range(3):  # warm; the last launch's record is read
        assert L.rt_debug_phase_clear() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert L.rt_render_batch(ctx, sc, views, n_views, w, h, depth, 8, 1, 0, C.c_void_p(out.data_ptr()),
                                 C.c_void_p(stream.cuda_stream)) == 0
        e1.record(stream)
        torch.cuda.synchronize()
    assert L.rt_debug_last_queued(ctx) == 1, "the launch was tiled"
    buf = np.zeros(slots * 16, dtype=np.uint64)
    assert L.rt_debug_phase_read(buf.ctypes.data, buf.nbytes) == 0
    R = buf.reshape(slots, 16).astype(np.int64)
    live = R[:, 0] > 0
    g = np.nonzero(live)[0]
    R = R[live]
    t0 = R[:, 0].min()
    start, barrier, end = (R[:, 0] - t0) * us, (R[:, 13] - t0) * us, (R[:, 7] - t0) * us
    worked = R[:, 1] > 0  # waves that took a chunk
    first = np.where(worked, (R[:, 1] - t0) * us, end)
    n_refill, t_refill, max_refill = R[:, 10], R[:, 11] * us, R[:, 12] * us
    chunks, tiles = R[:, 15], R[:, 9]
    span = end.max()
    print(f"== {cfg}, {n_views} views of {w} x {h} in one persistent launch: {live.sum()} waves, "
          f"{tiles.sum()} tiles in {chunks.sum()} chunks; HIP events {e0.elapsed_time(e1) * 1e3:.1f} us, "
          f"first entry -> last leave {span:.1f} us")
    for q in (0, 1, 10, 50, 90, 99, 100):
        print(f"  p{q:<3d} entry {np.percentile(start, q):8.2f}  staged {np.percentile(barrier, q):8.2f}  "
              f"first tile {np.percentile(first, q):8.2f}  leave {np.percentile(end, q):8.2f} us")
    idle = span - end
    busy = end - first
    print(f"  ramp (mean entry) {start.mean():.2f} us; prologue (entry -> staged) mean {(barrier - start).mean():.2f} "
          f"max {(barrier - start).max():.2f} us; mean wave-time before its first tile {first.mean():.2f} us")
    print(f"  refills per wave: {n_refill.mean():.1f} x {t_refill.sum() / max(n_refill.sum(), 1):.2f} us = "
          f"{t_refill.mean():.1f} us ({t_refill.mean() / span * 100:.2f} % of the span), longest {max_refill.max():.1f} us")
    print(f"  idle after a wave's last tile: mean {idle.mean():.2f} us, p90 {np.percentile(idle, 90):.2f}, "
          f"max {idle.max():.2f} ({idle.mean() / span * 100:.2f} % of the span)")
    q = queue_of(g)
    qidle = np.array([idle[q == k].mean() for k in range(32)])
    qend = np.array([end[q == k].max() for k in range(32)])
    print(f"  by queue: mean idle min {qidle.min():.2f} median {np.median(qidle):.2f} max {qidle.max():.2f} us; "
          f"last leave min {qend.min():.1f} max {qend.max():.1f} us")
    print("  mean idle by queue (rows q / 4, columns q % 4): "
          + " | ".join(" ".join("%5.1f" % qidle[4 * a + b] for b in range(4)) for a in range(8)))
    xcc = (R[:, 8] >> 32) & 15
    simd = (R[:, 8] >> 4) & 3
    print("  by XCC: " + ", ".join("%d: %d waves, idle %.1f us, %.1f tiles per wave, last leave %.1f"
                                    % (x, (xcc == x).sum(), idle[xcc == x].mean(), tiles[xcc == x].mean(),
                                       end[xcc == x].max()) for x in np.unique(xcc)))
    print("  by SIMD: " + ", ".join("%d: idle %.1f us, %.1f tiles per wave" % (x, idle[simd == x].mean(),
                                                                           tiles[simd == x].mean())
                                     for x in np.unique(simd)))
    print("  XCC of work-group b: b % 8 in " + "%.3f of the waves" % np.mean(xcc == (g // 4) % 8))
    w_t = busy[worked] / np.maximum(tiles[worked], 1)
    print(f"  wave-time per tile (first tile -> leave, refills and dequeues included): mean {w_t.mean():.3f} us, "
          f"p10 {np.percentile(w_t, 10):.3f} p90 {np.percentile(w_t, 90):.3f}; tiles per wave min {tiles.min()} "
          f"mean {tiles.mean():.1f} max {tiles.max()}")
    single = R[:, 14] > 0
    if single.any():
        s1 = (R[single, 14] - t0) * us
        print(f"  first single tile: {single.sum()} waves, min {s1.min():.1f} median {np.median(s1):.1f} "
              f"max {s1.max():.1f} us ({span - s1.min():.1f} .. {span - s1.max():.1f} us before the end)")
    accounted = start.mean() + (first - start).mean() + t_refill.mean() + idle.mean()
    print(f"  of the span's {span:.1f} us per wave: entry {start.mean():.1f} + prologue and first dequeue "
          f"{(first - start).mean():.1f} + refills {t_refill.mean():.1f} + idle at the end {idle.mean():.1f} = "
          f"{accounted:.1f} us not in tiles ({accounted / span * 100:.2f} %); HIP events - span "
          f"{e0.elapsed_time(e1) * 1e3 - span:.1f} us", flush=True)
    del out
