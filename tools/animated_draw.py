"""The shipped workload's draw() with the scene moved on the host and on the
device (include/rt.h, rt_anim): 1280x720, depth 0, one process, three
interleaved repeats, medians.

  A  per frame: rt_scene_update(rt_reference_objects(t)) + one synchronous
     render (bench.py's draw_loop shape), wall clock;
  B  per frame: one synchronous rt_render_animated, wall clock
     (B' the same calls asynchronous on one stream, 4 frames in flight);
  C  256 frames in one call: rt_render_batch_scenes over 256 prebuilt scenes
     against rt_render_batch_animated (which also runs the animate kernel for
     the 256 frames), stream time between two events.

Run it under a time limit of its own, e.g.
  timeout -k 10 300 python tools/animated_draw.py | tee profiles/<name>.log
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import openglraytracer_amd as rt  # noqa: E402

W, H, DEPTH, N, BATCH = 1280, 720, 0, 200, 256


def frame_time(k):
    return k / 60.0


def main():
    ctx = rt.Context(0)
    print(rt.lib().rt_version().decode(), flush=True)
    base, anim = rt.reference_animation()
    live = rt.Scene(ctx, rt.reference_objects(0.0))
    an1 = rt.Anim(ctx, base, anim, max_frames=1)
    an4 = rt.Anim(ctx, base, anim, max_frames=4)
    anb = rt.Anim(ctx, base, anim, max_frames=BATCH)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    big = torch.empty((BATCH, H, W, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    times = [frame_time(k) for k in range(BATCH)]
    views = [rt.make_view(None, t) for t in times]
    scenes = [rt.Scene(ctx, rt.reference_objects(t)) for t in times]
    torch.cuda.synchronize()

    def draw_a(k):
        t = frame_time(k)
        live.update(rt.reference_objects(t))
        rt.render_batch(ctx, live, out.data_ptr(), W, H, DEPTH, [rt.make_view(None, t)])

    def draw_b(k):
        rt.render_animated_device(ctx, an1, out.data_ptr(), W, H, DEPTH, frame_time(k))

    def draw_b_async(k):
        rt.render_animated_device(ctx, an4, outs[k % 4].data_ptr(), W, H, DEPTH, frame_time(k), stream=stream.cuda_stream)

    # the two paths draw the same frame
    draw_a(77)
    want = out.cpu().numpy().copy()
    draw_b(77)
    assert np.array_equal(out.cpu().numpy(), want), "A and B differ"

    def wall(draw, drain=False):
        for k in range(5):
            draw(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(N):
            draw(k)
        if drain:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / N * 1e6

    def events(call):
        call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / BATCH * 1e3

    def batch_prebuilt():
        rt.render_batch_scenes(ctx, scenes, big.data_ptr(), W, H, DEPTH, views, stream=stream.cuda_stream)

    def batch_animated():
        rt.render_batch_animated(ctx, anb, big.data_ptr(), W, H, DEPTH, times, stream=stream.cuda_stream)

    batch_prebuilt()
    torch.cuda.synchronize()
    want = big[200].cpu().numpy().copy()
    big.zero_()
    batch_animated()
    torch.cuda.synchronize()
    assert np.array_equal(big[200].cpu().numpy(), want), "C: prebuilt and animated differ"

    ctx.set_timing(False)  # (no per-launch events: the loops time themselves)
    res = {k: [] for k in ("A", "B", "B_async", "C_prebuilt", "C_animated", "C_animated_host")}
    for rep in range(3):
        res["A"].append(wall(draw_a))
        res["B"].append(wall(draw_b))
        res["B_async"].append(wall(draw_b_async, drain=True))
        res["C_prebuilt"].append(events(batch_prebuilt))
        res["C_animated"].append(events(batch_animated))
        t0 = time.perf_counter()
        batch_animated()
        res["C_animated_host"].append((time.perf_counter() - t0) / BATCH * 1e6)
        torch.cuda.synchronize()
        print("repeat %d: " % rep + ", ".join("%s %.2f" % (k, v[-1]) for k, v in res.items()), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print("%dx%d depth %d, us per frame, medians of 3 interleaved repeats (%d frames each; C: %d frames per call)"
          % (W, H, DEPTH, N, BATCH))
    print("A  rt_scene_update + synchronous render      %8.2f" % med["A"])
    print("B  rt_render_animated, synchronous           %8.2f  (%.2fx of A)" % (med["B"], med["B"] / med["A"]))
    print("B' rt_render_animated, one stream, 4 slots   %8.2f" % med["B_async"])
    print("C  rt_render_batch_scenes, prebuilt scenes   %8.2f" % med["C_prebuilt"])
    print("C  rt_render_batch_animated                  %8.2f  (%.3fx of prebuilt; host %.2f us per frame of the call)"
          % (med["C_animated"], med["C_animated"] / med["C_prebuilt"], med["C_animated_host"]))
    for s in scenes:
        s.close()
    for a in (an1, an4, anb):
        a.close()
    live.close()
    ctx.close()


if __name__ == "__main__":
    main()
