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

--scene config2: the headline workload instead, 1920x1080, depth 0, the room
and 16 spheres, every sphere on SIN_OFFSET position channels and every third
one on a radius channel too (rt_anim_create2); A moves the scene with
rt_animate_objects2, and C gains a row for config 2's static 256-frame launch
(rt_render_batch of one scene: the persistent grid, which a batch of per-slot
blobs does not take).

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
CONFIG2 = sys.argv[1:] == ["--scene", "config2"]
assert CONFIG2 or not sys.argv[1:], "usage: animated_draw.py [--scene config2]"
if CONFIG2:
    W, H = 1920, 1080


def frame_time(k):
    return k / 60.0


def config2_animation():
    """Config 2's objects, every sphere moving about its place, every third breathing."""
    from openglraytracer_amd.abi import AnimChannel, ObjectAnim, RT_ANIM_SIN_OFFSET
    rng = np.random.default_rng(2)
    base = rt.bench_objects(16)
    anim, radius = [ObjectAnim() for _ in base], [AnimChannel() for _ in base]
    for i in range(1, len(base)):
        for k in range(3):
            anim[i].position[k] = AnimChannel(RT_ANIM_SIN_OFFSET, float(rng.uniform(0.3, 1.5)),
                                              float(rng.uniform(0.3, 2.0)), base[i].position[k])
        if i % 3 == 0:
            radius[i] = AnimChannel(RT_ANIM_SIN_OFFSET, 0.25, float(rng.uniform(0.3, 2.0)), base[i].radius)
    return base, anim, radius


def main():
    ctx = rt.Context(0)
    print(rt.lib().rt_version().decode(), flush=True)
    if CONFIG2:
        base, anim, radius = config2_animation()
        kw = {"radius": radius}

        def objects_at(t):
            return rt.animate_objects(base, anim, t, radius)
    else:
        base, anim = rt.reference_animation()
        kw, objects_at = {}, rt.reference_objects
    live = rt.Scene(ctx, objects_at(0.0))
    an1 = rt.Anim(ctx, base, anim, max_frames=1, **kw)
    an4 = rt.Anim(ctx, base, anim, max_frames=4, **kw)
    anb = rt.Anim(ctx, base, anim, max_frames=BATCH, **kw)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    big = torch.empty((BATCH, H, W, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    times = [frame_time(k) for k in range(BATCH)]
    views = [rt.make_view(None, t) for t in times]
    scenes = [rt.Scene(ctx, objects_at(t)) for t in times]
    torch.cuda.synchronize()

    def draw_a(k):
        t = frame_time(k)
        live.update(objects_at(t))
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

    def batch_static():
        rt.render_batch(ctx, scenes[0], big.data_ptr(), W, H, DEPTH, views, stream=stream.cuda_stream)

    # Host-built scenes of moving spheres need not share a layout (the BVH's
    # node count follows the spheres' positions), and rt_render_batch_scenes
    # then refuses them: the row is left out, and frame 200 is checked against
    # its own scene's render.
    prebuilt = True
    try:
        batch_prebuilt()
    except rt.RTError as e:
        prebuilt = False
        print("C  rt_render_batch_scenes refuses the prebuilt scenes: %s" % e, flush=True)
        rt.render_batch(ctx, scenes[200], big.data_ptr() + 200 * H * W * 16, W, H, DEPTH, [views[200]],
                        stream=stream.cuda_stream)
    torch.cuda.synchronize()
    want = big[200].cpu().numpy().copy()
    big.zero_()
    batch_animated()
    torch.cuda.synchronize()
    assert np.array_equal(big[200].cpu().numpy(), want), "C: prebuilt and animated differ"

    ctx.set_timing(False)  # (no per-launch events: the loops time themselves)
    res = {k: [] for k in ("A", "B", "B_async", "C_static", "C_prebuilt", "C_animated", "C_animated_host")}
    for rep in range(3):
        res["A"].append(wall(draw_a))
        res["B"].append(wall(draw_b))
        res["B_async"].append(wall(draw_b_async, drain=True))
        res["C_static"].append(events(batch_static) if CONFIG2 else 0.0)
        res["C_prebuilt"].append(events(batch_prebuilt) if prebuilt else float("nan"))
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
    if CONFIG2:
        print("C  rt_render_batch, one static scene         %8.2f" % med["C_static"])
    if prebuilt:
        print("C  rt_render_batch_scenes, prebuilt scenes   %8.2f" % med["C_prebuilt"])
    print("C  rt_render_batch_animated                  %8.2f  (%.3fx of %s; host %.2f us per frame of the call)"
          % (med["C_animated"], med["C_animated"] / med["C_prebuilt" if prebuilt else "C_static"],
             "prebuilt" if prebuilt else "the static scene", med["C_animated_host"]))
    for s in scenes:
        s.close()
    for a in (an1, an4, anb):
        a.close()
    live.close()
    ctx.close()


if __name__ == "__main__":
    main()
