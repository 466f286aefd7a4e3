"""Kernel time of rt_occluded against the closest-hit query of the same segments:
    python tools/occluded_time.py [--lib PATH] [--out profiles/NAME.log]

One process, device buffers. The median of 21 rt_last_kernel_ms readings (HIP
events around the call's launch on the context's stream) after 3 warm-ups, the
cases of a segment set interleaved round by round, so a drift of the clocks
touches all of them alike.
  config 2's scene (bench_objects(16)): the shadow segments of the 1920 x 1080
    orbit view towards light 0 (start = p + 0.01 n, dir = L0 - p, from
    rt_render_hits' points and normals), in pixel order and under a seeded
    permutation;
  bench_objects(64) without and with its room: 2 M seeded point pairs in
    [-10, 10]^3.
Each set is answered by rt_occluded (bytes; words; both) and, beside it, by what
the library offered for the question before: rt_trace_rays with the hits plane
alone and flags 0 over the same buffer (t < 1 is then compared by the caller).
With RT_OPT_CULLING on and off. A segment costs 32 B of loads; an answer 1 B,
1/8 B or both, a hit record 16 B. Recorded, not asserted: DESIGN.md quotes the
log.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (HIP runtime first)
import openglraytracer_amd as rt  # noqa: E402
from openglraytracer_amd import abi  # noqa: E402
from oracle import scenes  # noqa: E402

WARMUP, READINGS, SEED = 3, 21, 0
N_PAIRS = 2_000_000


def measure(ctx, cases):
    ms = [[] for _ in cases]
    for i in range(WARMUP + READINGS):
        for k, (_, call) in enumerate(cases):
            call()
            if i >= WARMUP:
                ms[k].append(ctx.last_kernel_ms())
    return ["%-58s median %.4f ms  min %.4f  max %.4f" % (name, np.median(m), np.min(m), np.max(m))
            for (name, _), m in zip(cases, ms)], [float(np.median(m)) for m in ms]


def shadow_segments(ctx, sc, lights, w, h):
    """The view's shadow segments towards light 0, hit pixels in pixel order."""
    hits, normals, points = rt.render_hits(ctx, sc, w, h, view=rt.make_view(None, 0.0), shadow=False)
    hit = hits["object"] >= 0
    p, n = points[hit][:, :3], normals[hit][:, :3]
    rays = np.zeros(len(p), abi.RAY_DTYPE)
    rays["origin"] = p + n * np.float32(0.01)
    rays["dir"] = np.array(lights[0].position[:], np.float32) - p
    return rays


def point_pairs(n):
    rng = np.random.default_rng(SEED)
    a = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    b = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    rays = np.zeros(n, abi.RAY_DTYPE)
    rays["origin"], rays["dir"] = a, b - a
    return rays


def set_cases(ctx, sc, rays):
    """The four calls over one device buffer, with culling on and off."""
    n = len(rays)
    rays_t = torch.from_numpy(rays.view(np.float32).reshape(n, 8)).cuda()
    bytes_t = torch.empty(n, dtype=torch.uint8, device="cuda")
    words_t = torch.empty((n + 63) // 64, dtype=torch.int64, device="cuda")
    hits_t = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = rt.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def occluded(b, w, cull):
        def run():
            ctx.set_culling(cull)
            rc = L.rt_occluded(ctx.handle, sc.handle, ptr(rays_t), n, ptr(b), ptr(w), 1, None)
            ctx.set_culling(True)
            assert rc == abi.RT_OK, L.rt_last_error()
        return run

    def closest(cull):
        def run():
            ctx.set_culling(cull)
            rc = L.rt_trace_rays(ctx.handle, sc.handle, ptr(rays_t), n, 0, 0, None, ptr(hits_t), None, None, 1, None)
            ctx.set_culling(True)
            assert rc == abi.RT_OK, L.rt_last_error()
        return run

    cases = []
    for cull in (True, False):
        tag = "culling" if cull else "no culling"
        cases += [("rt_occluded bytes, %s" % tag, occluded(bytes_t, None, cull)),
                  ("rt_occluded words, %s" % tag, occluded(None, words_t, cull)),
                  ("rt_occluded bytes and words, %s" % tag, occluded(bytes_t, words_t, cull)),
                  ("rt_trace_rays hits alone, flags 0, %s" % tag, closest(cull))]
    return cases, [rays_t, bytes_t, words_t, hits_t]


def agreement(ctx, sc, keep):
    """The two queries' answers over the set (a sanity line of the log, not a test)."""
    rays_t, bytes_t, _, hits_t = keep
    (hits,) = rt.trace_rays(ctx, sc, rays_t, 0, colors=False, hits=True, shadow=False)
    occ = rt.occluded(ctx, sc, rays_t)
    torch.cuda.synchronize()
    t = hits[:, 1].contiguous().view(torch.float32)
    want = (hits[:, 0] >= 0) & (t < 1.0)
    return int(occ.sum().item()), int((occ.bool() != want).sum().item())


def main():
    opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None  # noqa: E731
    out_path = opt("--out")
    if opt("--lib"):  # another build of the library, for A/B rounds in one GPU call
        rt.LIB_PATH = os.path.abspath(opt("--lib"))
    ctx = rt.Context(0)
    lights = rt.reference_lights()
    lines = ["# tools/occluded_time.py: %s" % rt.lib().rt_version().decode(),
             "# median of %d rt_last_kernel_ms readings after %d warm-ups, the cases of a set interleaved; "
             "device buffers" % (READINGS, WARMUP)]
    plan = (("config 2's scene (bench_objects(16)), 1920 x 1080 shadow segments to light 0", 16, True, "shadow"),
            ("bench_objects(64) without its room, point pairs in [-10, 10]^3", 64, False, "pairs"),
            ("bench_objects(64) with its room, point pairs in [-10, 10]^3", 64, True, "pairs"))
    for title, n_spheres, room, kind in plan:
        objs = scenes.bench_objects(n_spheres)
        sc = rt.Scene(ctx, objs if room else objs[1:])
        try:
            if kind == "shadow":
                rays = shadow_segments(ctx, sc, lights, 1920, 1080)
                perm = np.random.default_rng(SEED).permutation(len(rays))
                sets = (("pixel order", rays), ("permuted", np.ascontiguousarray(rays[perm])))
            else:
                sets = (("seeded", point_pairs(N_PAIRS)),)
            for order, r in sets:
                cases, keep = set_cases(ctx, sc, r)
                text, med = measure(ctx, cases)
                occ, differ = agreement(ctx, sc, keep)
                lines.append("%s, %s (%d segments, %d occluded, %d differ from the closest-hit query)"
                             % (title, order, len(r), occ, differ))
                lines += ["  " + t for t in text]
                lines.append("  rt_occluded bytes / rt_trace_rays hits: culling %.3f, no culling %.3f"
                             % (med[0] / med[3], med[4] / med[7]))
                del keep
        finally:
            sc.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
