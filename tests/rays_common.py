"""Ray sets for the ray-query tests (test_rays_host.py, test_gpu_rays.py), with
the oracle as the checker. No GPU.

For a camera c the oracle's probe 1 is the exact direction it traces for each
pixel and c.position the start; probe 0 is the ray's colour, probes 2, 3, 4 its
first hit's record, normal and point. A ray set concatenates several cameras'
frames and carries a seeded permutation, so that a wave of 64 consecutive rays
mixes origins.
"""
import math
import os
import sys

import numpy as np

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from oracle import port, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from panorama import FORWARD, panorama_rays  # noqa: E402,F401


def camera(pos, angles, fov=None):
    """The reference camera's fov, aspect and planes at another position and angles."""
    c = rt.reference_camera(0.0)
    c.position[:] = [float(x) for x in pos]
    c.angles[:] = [float(x) for x in angles]
    if fov is not None:
        c.v_fov = float(fov)
    return c


def aimed(pos, fov=None):
    """At `pos`, looking at the world's origin."""
    x, y, z = pos
    return camera(pos, (-math.degrees(math.atan2(z, math.hypot(x, y))), math.degrees(math.atan2(y, x)) + 90.0, 0.0), fov)


class RaySet:
    """rays: (n,) abi.RAY_DTYPE in camera order; perm: the order they are traced
    in; colors[depth], p2, p3, p4: the oracle's planes, (n, 4), camera order;
    cams: per camera (first ray, rays)."""

    def __init__(self, objs, cams, w, h, depths, materials=None, lights=None, time=0.0):
        self.objs, self.materials, self.lights = objs, materials, lights
        kw = dict(materials=materials, lights=lights)
        rays, self.cams, planes = [], [], {k: [] for k in (2, 3, 4)}
        self.colors = {d: [] for d in depths}
        at = 0
        for c in cams:  # (None: the orbit camera at `time`)
            pos = list((c if c is not None else port.reference_camera(time)).position)
            d = port.render(objs, w, h, 0, time, probe=1, camera=c, **kw).reshape(-1, 4)
            r = np.zeros(w * h, abi.RAY_DTYPE)
            r["origin"] = np.asarray(pos, np.float32)
            r["dir"] = d[:, :3]
            rays.append(r)
            for k in planes:
                planes[k].append(port.render(objs, w, h, 0, time, probe=k, camera=c, **kw).reshape(-1, 4))
            for dep in depths:
                self.colors[dep].append(port.render(objs, w, h, dep, time, camera=c, **kw).reshape(-1, 4))
            self.cams.append((at, w * h))
            at += w * h
        self.rays = np.concatenate(rays)
        self.p2, self.p3, self.p4 = (np.concatenate(planes[k]) for k in (2, 3, 4))
        self.colors = {d: np.concatenate(v) for d, v in self.colors.items()}
        self.n = at
        self.perm = np.random.default_rng(0).permutation(self.n)

    def permuted(self):
        return np.ascontiguousarray(self.rays[self.perm])

    def unpermute(self, plane):
        out = np.empty_like(plane)
        out[self.perm] = plane
        return out

    def objects(self, cam):
        a, n = self.cams[cam]
        return self.p2[a:a + n, 0].astype(np.int64)

    def t(self, cam):
        a, n = self.cams[cam]
        return self.p2[a:a + n, 1]


def hit_floats(hits):
    """The `hits` plane in the oracle's probe-2 encoding: (object, t, shadow mask) as floats."""
    return np.stack([hits["object"].astype(np.float32), hits["t"], hits["shadow"].astype(np.float32)], -1)


def check_records(got, rs, what, shadow=True):
    """hits / normals / points (camera order) against the oracle's probes of the set."""
    hits, normals, points = got
    want = rs.p2[:, :3].copy()
    if not shadow:
        want[:, 2] = 0
    assert np.array_equal(hit_floats(hits), want), what
    assert np.array_equal(normals, rs.p3), what
    assert np.array_equal(points, rs.p4), what
    miss = hits["object"] < 0
    mats = np.array([o.material for o in rs.objs] + [-1], np.int32)  # (index -1: a miss)
    assert np.array_equal(hits["material"], mats[hits["object"]]), what
    assert (hits["t"][miss] == 0).all() and (hits["shadow"][miss] == 0).all(), what
    assert (normals[miss] == 0).all() and (points[miss] == 0).all(), what


# ---- the sets ------------------------------------------------------------------
R_DEPTHS = (0, 1, 2, 5, 9)
R_INSIDE = (1, 3, 4, 5)  # material1 and the three glasses of bench_objects(16)


def set_r():
    """bench_objects(16): the orbit camera, one inside the room, four at sphere
    centres (every ray starts inside a sphere), one outside the room."""
    objs = scenes.bench_objects(16)
    cams = [None, camera((5.0, -6.0, 2.0), (10.0, 40.0, 0.0)),
            camera(objs[1].position[:], (20.0, 200.0, 0.0))]
    cams += [camera(objs[i].position[:], (0.0, 90.0, 0.0)) for i in R_INSIDE[1:]]
    cams.append(camera((30.0, -25.0, 12.0), (0.0, 0.0, 0.0)))
    return RaySet(objs, cams, 16, 9, R_DEPTHS)


def check_set_r(rs):
    """The conditions the set was chosen for, on the oracle's own output."""
    obj, shadow = rs.p2[:, 0], rs.p2[:, 2]
    assert [int((rs.objects(k) >= 0).sum()) for k in (0, 1, 6)] == [144, 144, 23]
    assert (obj < 0).sum() == 121  # misses: the camera outside the room
    a, n = rs.cams[0]
    assert ((shadow[a:a + n] != 0) & (obj[a:a + n] >= 0)).sum() == 36
    a, n = rs.cams[1]
    assert ((shadow[a:a + n] != 0) & (obj[a:a + n] >= 0)).sum() == 44
    own = 0
    for k, i in zip(range(2, 6), R_INSIDE):  # every ray leaves the sphere it starts in, at t = r up to rounding
        r = np.float32(rs.objs[i].radius)
        assert (rs.objects(k) == i).all(), i
        assert (np.abs(rs.t(k) - r) <= r * np.float32(2.0 ** -21)).all(), i
        own += int((rs.objects(k) == i).sum())
    assert own >= 4 * 144
    for d in R_DEPTHS:
        assert np.isfinite(rs.colors[d]).all(), d
    assert any((rs.colors[9] != rs.colors[0]).any(-1))  # (the recursion shows)


F_CAMERAS = (((30.0, -25.0, 12.0), 40.0), ((3000.0, -2000.0, 500.0), 0.4), ((6000.0, 4000.0, -3000.0), 0.2))
F_DEPTHS = (0, 2)


def set_f():
    """bench_objects(64) without its room (63 spheres: a sphere BVH, which every
    scene with a finite sphere has), three cameras aimed at it from 41, 3,640
    and 7,800 units: the last two lie outside the range the BVH's node test is
    proved for."""
    objs = scenes.bench_objects(64)[1:]
    return RaySet(objs, [aimed(p, fov) for p, fov in F_CAMERAS], 32, 18, F_DEPTHS)


def check_set_f(rs):
    for k in range(3):
        o = rs.objects(k)
        assert (o >= 0).sum() >= 5 and len(np.unique(o[o >= 0])) >= 2, k
    assert rs.t(1).max() > 3600.0 and rs.t(2).max() > 7700.0
