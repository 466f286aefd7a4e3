"""Kernel time of the ray queries against the renders of the same frame:
    python tools/rays_time.py [--lib PATH] [--out profiles/NAME.log]

One process, device buffers, the rays of the orbit view at t = 0 as
rt_view_rays writes them. The median of 21 rt_last_kernel_ms readings (HIP
events around the call's launches on the context's stream) after 3 warm-ups:
  config 2's scene (bench_objects(16)), 1920 x 1080
    (a) rt_trace_rays, colours at depth 0, the rays in pixel order;
    (b) the same rays under a seeded permutation (no coherence within a wave);
    (c) the hits plane alone, with and without shadow bits, pixel order;
    beside them rt_render_view at depth 0 with RT_OPT_SCENE_SHAPES 0 (the
    general kernel, whose shape the ray kernel takes) and with the default
    options, and rt_render_hits_view (hits alone, with and without shadow bits);
  config 3's scene (bench_objects(64)), 1280 x 720
    (d) rt_trace_rays, colours at depth 2, pixel order and permuted;
    beside them rt_render_view at depth 2, RT_OPT_SCENE_SHAPES 0 and default.
The cases of a scene run interleaved, round by round, so a drift of the clocks
touches all of them alike. A ray costs 32 B of loads and 16 B of stores per
plane; a render's pixel 16 B of stores. Recorded, not asserted: DESIGN.md
quotes the log.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (HIP runtime first)
import openglraytracer_amd as rt  # noqa: E402
from oracle import scenes  # noqa: E402

WARMUP, READINGS, SEED = 3, 21, 0


def measure(ctx, cases):
    ms = [[] for _ in cases]
    for i in range(WARMUP + READINGS):
        for k, (_, call) in enumerate(cases):
            call()
            if i >= WARMUP:
                ms[k].append(ctx.last_kernel_ms())
    return ["%-58s median %.4f ms  min %.4f  max %.4f" % (name, np.median(m), np.min(m), np.max(m))
            for (name, _), m in zip(cases, ms)], [float(np.median(m)) for m in ms]


def general(ctx, call):
    def run():
        ctx.set_scene_shapes(False)
        try:
            call()
        finally:
            ctx.set_scene_shapes(True)
    return run


def scene_cases(ctx, sc, w, h, depth, with_hits):
    view = rt.make_view(None, 0.0)
    rays = rt.view_rays(ctx, view, w, h, device=True).reshape(-1, 8).contiguous()
    perm = torch.from_numpy(np.random.default_rng(SEED).permutation(w * h)).cuda()
    shuffled = rays[perm].contiguous()
    colour = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    plane = torch.empty((h, w, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    keep = [rays, shuffled, colour, plane]  # (alive while the cases run)
    render = lambda: rt.render_device(ctx, sc, colour.data_ptr(), w, h, depth, view=view)  # noqa: E731
    cases = [("rt_trace_rays colours depth %d, pixel order" % depth, lambda: rt.trace_rays(ctx, sc, rays, depth)),
             ("rt_trace_rays colours depth %d, permuted" % depth, lambda: rt.trace_rays(ctx, sc, shuffled, depth)),
             ("rt_render_view depth %d, RT_OPT_SCENE_SHAPES 0" % depth, general(ctx, render)),
             ("rt_render_view depth %d, default options" % depth, render)]
    if with_hits:
        for shadow in (True, False):
            tag = "shadow bits" if shadow else "no shadow rays"
            cases.append(("rt_trace_rays hits alone, %s, pixel order" % tag,
                          lambda s=shadow: rt.trace_rays(ctx, sc, rays, 0, colors=False, hits=True, shadow=s)))
            cases.append(("rt_render_hits_view hits alone, %s" % tag,
                          lambda s=shadow: rt.render_hits_device(ctx, sc, w, h, plane.data_ptr(), None, None,
                                                                 view=view, shadow=s)))
    return cases, keep


def main():
    opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None  # noqa: E731
    out_path = opt("--out")
    if opt("--lib"):  # another build of the library (tools/ablate.sh rev REV), for A/B rounds in one GPU call
        rt.LIB_PATH = os.path.abspath(opt("--lib"))
    ctx = rt.Context(0)
    lines = ["# tools/rays_time.py: %s" % rt.lib().rt_version().decode(),
             "# median of %d rt_last_kernel_ms readings after %d warm-ups, the cases of a scene interleaved; "
             "device buffers" % (READINGS, WARMUP)]
    for title, n_spheres, w, h, depth, with_hits in (("config 2's scene", 16, 1920, 1080, 0, True),
                                                     ("config 3's scene", 64, 1280, 720, 2, False)):
        sc = rt.Scene(ctx, scenes.bench_objects(n_spheres))
        try:
            cases, keep = scene_cases(ctx, sc, w, h, depth, with_hits)
            text, med = measure(ctx, cases)
        finally:
            sc.close()
        lines.append("%s, %d x %d (%d rays)" % (title, w, h, w * h))
        lines += ["  " + t for t in text]
        lines.append("  ratios to the general render: pixel order %.3f, permuted %.3f; to the default render: %.3f, %.3f"
                     % (med[0] / med[2], med[1] / med[2], med[0] / med[3], med[1] / med[3]))
        if with_hits:
            lines.append("  hits alone, ray kernel / hits kernel: shadow bits %.3f, no shadow rays %.3f"
                         % (med[4] / med[5], med[6] / med[7]))
        del keep
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
