"""An ambient-occlusion image of a view, through rt_render_hits and rt_occluded:
    python tools/ao.py [--scene scenes/shipped.json] [--width 640] [--height 360] [--samples 16]
                       [--radius 2.0] [--seed 0] [--time 0] --out ao.ppm

rt_render_hits gives every pixel's first hit: its point p and normal n. Each
hit pixel gets K segments (ao_segments): start p + 0.01 n (the reference's
shadow-ray offset, in float32), direction a seeded cosine-weighted sample of
the hemisphere around n, computed in float64, scaled to length R and rounded to
float32 once. rt_occluded is an any-hit query over 0 < t < 1 of origin + t *
dir, so the direction's length is the search radius and one call answers all
K n segments with one bit each. A pixel's value is the share of its segments
that are not occluded (ao_image; 1 for a pixel that hit nothing), written as a
grey frame with rt_write_ppm.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openglraytracer_amd import abi  # noqa: E402

OFFSET = np.float32(0.01)  # the start's offset along the normal (raytrace_compute.glsl:808)


def ao_segments(points, normals, samples, radius, seed=0):
    """(n, 3) float32 hit points and unit normals -> (n, samples) abi.RAY_DTYPE. No GPU."""
    p, n = np.asarray(points, np.float32)[:, :3], np.asarray(normals, np.float32)[:, :3]
    rng = np.random.default_rng(seed)
    u1, u2 = rng.random((len(p), samples)), rng.random((len(p), samples))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u1)], -1)  # (z along the normal)
    w = n.astype(np.float64)
    # a tangent frame: the world axis least aligned with the normal, made perpendicular to it
    e = np.eye(3)[np.argmin(np.abs(w), -1)]
    t = e - (e * w).sum(-1, keepdims=True) * w
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    b = np.cross(w, t)
    d = local[..., 0:1] * t[:, None] + local[..., 1:2] * b[:, None] + local[..., 2:3] * w[:, None]
    d *= radius / np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((len(p), samples), abi.RAY_DTYPE)
    rays["origin"] = (p + n * OFFSET)[:, None]  # (float32, one rounding per operation)
    rays["dir"] = d.astype(np.float32)  # (the one rounding)
    return rays


def ao_image(hit, occluded, samples):
    """hit: (h, w) bool; occluded: the bits of the hit pixels' segments in
    ao_segments' order -> (h, w, 4) float32, the unoccluded share as grey."""
    share = np.ones(hit.shape, np.float32)
    occ = np.asarray(occluded, bool).reshape(-1, samples)
    share[hit] = (samples - occ.sum(-1)).astype(np.float32) / np.float32(samples)
    out = np.ones(hit.shape + (4,), np.float32)
    out[..., :3] = share[..., None]
    return out


def ao(ctx, sc, view, width, height, samples, radius, seed=0):
    """The image of `view`: one rt_render_hits call, one rt_occluded call."""
    import openglraytracer_amd as rt
    hits, normals, points = rt.render_hits(ctx, sc, width, height, view=view, shadow=False)
    hit = hits["object"] >= 0
    if not hit.any():
        return ao_image(hit, np.zeros(0, bool), samples)
    rays = ao_segments(points[hit], normals[hit], samples, radius, seed)
    return ao_image(hit, rt.occluded(ctx, sc, rays), samples)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "shipped.json"))
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    import openglraytracer_amd as rt
    objs, mats, lights, cam = rt.parse_scene(open(a.scene).read(), a.time)
    ctx = rt.Context(0)
    sc = rt.Scene(ctx, objs, materials=mats, lights=lights)
    try:
        img = ao(ctx, sc, rt.make_view(cam, a.time), a.width, a.height, a.samples, a.radius, a.seed)
        ms = ctx.last_kernel_ms()
    finally:
        sc.close()
        ctx.close()
    rt.write_ppm(a.out, img)
    print("%s: %d x %d, %d segments of length %g per hit pixel, occlusion kernel %.3f ms" % (
        a.out, a.width, a.height, a.samples, a.radius, ms))


if __name__ == "__main__":
    main()
