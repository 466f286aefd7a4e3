"""Kernel time of the primary-hit kernel against the general depth-0 render:
    python tools/hits_time.py [--lib PATH] [--out profiles/NAME.log]

Config 2's scene (bench_objects(16)), 1920 x 1080, one process, device
buffers. The median of 21 rt_last_kernel_ms readings (HIP events around the
launch on the context's stream) after 3 warm-ups, for
  (a) rt_render_hits, all planes, RT_HITS_SHADOW;
  (b) all planes, no shadow rays;
  (c) the hits plane alone, no shadow rays (picking, depth);
  (d) rt_render at depth 0 with RT_OPT_SCENE_SHAPES 0: the general depth-0
      kernel, whose shape the hits kernel takes.
The four cases run interleaved, round by round, so a drift of the clocks
touches all of them alike. Recorded, not asserted: DESIGN.md §7 quotes the log.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (HIP runtime first)
import openglraytracer_amd as rt  # noqa: E402
from oracle import scenes  # noqa: E402

W, H, WARMUP, READINGS = 1920, 1080, 3, 21


def main():
    opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None  # noqa: E731
    out_path = opt("--out")
    if opt("--lib"):  # another build of the library (tools/ablate.sh rev REV), for A/B rounds in one GPU call
        rt.LIB_PATH = os.path.abspath(opt("--lib"))
    ctx = rt.Context(0)
    sc = rt.Scene(ctx, scenes.bench_objects(16))
    view = rt.make_view(None, 0.0)
    planes = [torch.empty((H, W, 16), dtype=torch.uint8, device="cuda") for _ in range(3)]
    colour = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    hp, np_, pp = [t.data_ptr() for t in planes]
    px = W * H

    def render_general():
        ctx.set_scene_shapes(False)
        try:
            rt.render_device(ctx, sc, colour.data_ptr(), W, H, 0, view=view)
        finally:
            ctx.set_scene_shapes(True)

    cases = [
        ("(a) hits + normals + points, shadow bits", 3 * 16 * px,
         lambda: rt.render_hits_device(ctx, sc, W, H, hp, np_, pp, view=view, shadow=True)),
        ("(b) hits + normals + points, no shadow rays", 3 * 16 * px,
         lambda: rt.render_hits_device(ctx, sc, W, H, hp, np_, pp, view=view, shadow=False)),
        ("(c) hits alone, no shadow rays", 16 * px,
         lambda: rt.render_hits_device(ctx, sc, W, H, hp, None, None, view=view, shadow=False)),
        ("(d) rt_render depth 0, RT_OPT_SCENE_SHAPES 0", 16 * px, render_general),
    ]
    ms = [[] for _ in cases]
    for i in range(WARMUP + READINGS):
        for k, (_, _, call) in enumerate(cases):
            call()
            if i >= WARMUP:
                ms[k].append(ctx.last_kernel_ms())
    kernel = rt.last_kernel(ctx)
    lines = ["# tools/hits_time.py: %s, config 2's scene, %d x %d, device buffers" % (rt.lib().rt_version().decode(), W, H),
             "# median of %d rt_last_kernel_ms readings after %d warm-ups, the cases interleaved" % (READINGS, WARMUP),
             "# (d) ran render kernel (depth, accum, dev, shape, launch, queued) = %s" % (kernel,)]
    for (name, nbytes, _), m in zip(cases, ms):
        lines.append("%-46s median %.4f ms  min %.4f  max %.4f  stores %.1f MB" % (
            name, np.median(m), np.min(m), np.max(m), nbytes / 1e6))
    d = float(np.median(ms[3]))
    lines.append("ratios to (d): (a) %.3f  (b) %.3f  (c) %.3f" % tuple(float(np.median(m)) / d for m in ms[:3]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    sc.close()
    ctx.close()


if __name__ == "__main__":
    main()
