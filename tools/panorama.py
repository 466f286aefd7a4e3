"""An equirectangular 360 x 180 degree capture from a point, through rt_trace_rays:
    python tools/panorama.py [--scene scenes/shipped.json] [--origin X Y Z] [--width 1024] [--height 512]
                             [--depth 2] [--time 0] --out pano.pfm

The grid (panorama_rays): column x looks at longitude 2 pi (x - W/2) / W, so
column W/2 looks forward and column 0 straight back (the image wraps, no column
twice); row y looks at latitude -pi/2 + pi y / (H - 1), so row 0 (the bottom
row, as in every frame of this library) is the -z pole and row H - 1 the +z
pole, both exactly (0, 0, -1) and (0, 0, 1) in every column. Forward is +y with z up and +x to the right, the camera convention of
rt_make_view at angles 0:

    d = (sin(lon) cos(lat), cos(lon) cos(lat), sin(lat))

computed in float64, normalised there and rounded to float32 once, so every
direction is a unit vector to within 2^-24 and the ray kernels keep their culled
paths (include/rt.h, rt_trace_rays). The frame is written with rt_write_pfm.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openglraytracer_amd import abi  # noqa: E402

FORWARD = (0.0, 1.0, 0.0)  # the centre column's direction on the horizon


def panorama_rays(origin, width, height):
    """The capture's rays, (height, width) of abi.RAY_DTYPE, row 0 the bottom row. No GPU."""
    lon = 2.0 * np.pi * (np.arange(width, dtype=np.float64) - width // 2) / width
    lat = -0.5 * np.pi + np.pi * np.arange(height, dtype=np.float64) / (height - 1) if height > 1 else np.zeros(1)
    cos_lat = np.cos(lat)
    if height > 1:
        cos_lat[0] = cos_lat[-1] = 0.0  # (cos(pi/2) in float64 is 6e-17: the pole rows are exactly (0, 0, -1) and (0, 0, 1))
    lon, cos_lat = np.meshgrid(lon, cos_lat)
    d = np.stack([np.sin(lon) * cos_lat, np.cos(lon) * cos_lat, np.repeat(np.sin(lat)[:, None], width, 1)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((height, width), abi.RAY_DTYPE)
    rays["origin"] = np.asarray(origin, np.float32)
    rays["dir"] = d.astype(np.float32)  # (the one rounding)
    return rays


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "shipped.json"))
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, -6.0, 3.0))  # (clear of the shipped scene's objects)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--time", type=float, default=0.0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    import openglraytracer_amd as rt
    objs, mats, lights, _ = rt.parse_scene(open(a.scene).read(), a.time)
    ctx = rt.Context(0)
    sc = rt.Scene(ctx, objs, materials=mats, lights=lights)
    try:
        (colors,) = rt.trace_rays(ctx, sc, panorama_rays(a.origin, a.width, a.height), a.depth)
        ms = ctx.last_kernel_ms()
    finally:
        sc.close()
        ctx.close()
    rt.write_pfm(a.out, colors.reshape(a.height, a.width, 4))
    print("%s: %d x %d from (%g, %g, %g), depth %d, kernel %.3f ms" % ((a.out, a.width, a.height) + tuple(a.origin) +
                                                                       (a.depth, ms)))


if __name__ == "__main__":
    main()
