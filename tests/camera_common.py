"""Explicit cameras and views for the camera tests (test_camera_host.py,
test_gpu_camera.py): seeded camera families, a fixed list of degenerate
cameras, matrix families that rewrite a view's unprojection, the scenes they
look at, and the oracle's frame of any rt_view. No GPU.

The camera convention (rt_make_view, checked with the oracle by
test_camera_host.py): at angles 0 the camera looks along +y, pitch raises z,
yaw turns about z with x = -sin(yaw). angles = (pitch, yaw, roll), degrees.
"""
import ctypes as C
import math

import numpy as np

import openglraytracer_amd as rt
from openglraytracer_amd.abi import BLUE_GLASS, MATERIAL1, MIRROR, RED_GLASS
from oracle import port, scenes
from room_fast_common import room_proof  # noqa: F401  (the classification hook, for both test modules)

EVERYTHING = (-(2 ** 30), 2 ** 30 - 1, -(2 ** 30), 2 ** 30 - 1)  # view_frame_setup's "not culled" rectangle


# ---- cameras ------------------------------------------------------------------
def make_camera(pos, angles, fov=70.0, aspect=16.0 / 9.0, near=0.1, far=1000.0):
    cam = rt.Camera()
    cam.position[:] = [float(x) for x in pos]
    cam.angles[:] = [float(x) for x in angles]
    cam.v_fov, cam.aspect, cam.near_plane, cam.far_plane = float(fov), float(aspect), float(near), float(far)
    cam.target = None  # the index of the object the family placed the camera by
    return cam


def aim(pos, target, roll=0.0):
    """(pitch, yaw, roll) in degrees of a camera at `pos` looking at `target`."""
    d = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    d = d / np.linalg.norm(d)
    return (math.degrees(math.asin(max(-1.0, min(1.0, d[2])))), math.degrees(math.atan2(-d[0], d[1])), roll)


def is_box(o):
    return any(x != 0.0 for x in list(o.box_mins) + list(o.box_maxs))


def is_room(o):
    return is_box(o) and list(o.box_mins) == [-11.0] * 3 and list(o.box_maxs) == [11.0] * 3


def sphere_ids(objs):
    return [i for i, o in enumerate(objs) if not is_box(o) and o.radius != -1.0]


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _log(rng, lo, hi):
    return 10.0 ** rng.uniform(lo, hi)


def free(rng, objs):
    """Anywhere in [-10, 10]^3, any orientation, fov 20-120, aspect 0.5-2.4."""
    return make_camera(rng.uniform(-10.0, 10.0, 3),
                       (rng.uniform(-89.0, 89.0), rng.uniform(0.0, 360.0), rng.uniform(-180.0, 180.0)),
                       rng.uniform(20.0, 120.0), rng.uniform(0.5, 2.4), _log(rng, -2.0, 0.0), _log(rng, 1.7, 4.0))


def close(rng, objs):
    """Just off a random sphere's surface (r eps away, eps = 10^U(-4, -0.5)),
    looking at its centre, straight away from it or along a tangent: corners
    of the sphere's cube behind the camera, footprints many frames wide."""
    i = int(rng.choice(sphere_ids(objs)))
    c, r = np.array(objs[i].position[:], np.float64), abs(objs[i].radius)
    u = _unit(rng)
    pos = c + r * (1.0 + _log(rng, -4.0, -0.5)) * u
    mode = int(rng.integers(3))
    t = np.cross(u, _unit(rng))
    target = c if mode == 0 else pos + u if mode == 1 else pos + t / np.linalg.norm(t)
    cam = make_camera(pos, aim(pos, target, rng.uniform(-180.0, 180.0)), rng.uniform(30.0, 150.0),
                      rng.uniform(0.5, 2.4), _log(rng, -2.0, -1.0), _log(rng, 1.7, 4.0))
    cam.target = i
    return cam


def inside(rng, objs):
    """Inside a random sphere (0-0.99 r from its centre) or a random box that
    is not the room; any material, any orientation."""
    ids = [i for i, o in enumerate(objs) if (is_box(o) and not is_room(o)) or i in sphere_ids(objs)]
    i = int(rng.choice(ids))
    o = objs[i]
    if is_box(o):
        l2w = np.zeros(16, np.float32)
        w2l, nrm = np.zeros(16, np.float32), np.zeros(9, np.float32)
        assert rt.lib().rt_object_transforms(C.byref(o), l2w.ctypes.data, w2l.ctypes.data, nrm.ctypes.data) == 0
        lo, hi = np.array(o.box_mins[:], np.float64), np.array(o.box_maxs[:], np.float64)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        p = mid + 0.99 * half * rng.uniform(-1.0, 1.0, 3)
        pos = (l2w.reshape(4, 4).T.astype(np.float64) @ np.append(p, 1.0))[:3]  # (column-major)
    else:
        pos = np.array(o.position[:], np.float64) + abs(o.radius) * rng.uniform(0.0, 0.99) * _unit(rng)
    cam = make_camera(pos, (rng.uniform(-89.0, 89.0), rng.uniform(0.0, 360.0), rng.uniform(-180.0, 180.0)),
                      rng.uniform(20.0, 120.0), rng.uniform(0.5, 2.4), _log(rng, -2.0, -1.0), _log(rng, 1.7, 4.0))
    cam.target = i
    return cam


def _outside(rng, lo, hi):
    pos = rng.uniform(lo, hi) * _unit(rng)
    return make_camera(pos, aim(pos, rng.uniform(-6.0, 6.0, 3), rng.uniform(-180.0, 180.0)), rng.uniform(5.0, 60.0),
                       rng.uniform(0.5, 2.4), 0.1, _log(rng, 3.0, 4.0))


def outside(rng, objs):
    """25-100 units from the origin, aimed into [-6, 6]^3, fov 5-60, the
    reference's near plane 0.1 and far 10^U(3, 4): the room's outer faces,
    every light behind a wall."""
    return _outside(rng, 25.0, 100.0)


def outside_far(rng, objs):
    """150-300 units away: the float32 matrix no longer passes the pinhole
    test (view_projection), so culling falls back to off."""
    return _outside(rng, 150.0, 300.0)


FAMILIES = {"free": free, "close": close, "inside": inside, "outside": outside, "outside_far": outside_far}


def seeded(family, seed, objs, attempt=0):
    """The family's camera for (seed, scene, attempt): one generator per draw."""
    name = family if isinstance(family, str) else family.__name__
    return FAMILIES[name](np.random.default_rng([sorted(FAMILIES).index(name), seed, len(objs), attempt]), objs)


def draw(family, seed, objs, accept, attempts=256):
    """The first of the family's cameras for (seed, scene) that `accept` takes:
    a case's own conditions (a sphere in view, a fallback taken) met inside
    the family's ranges."""
    for attempt in range(attempts):
        cam = seeded(family, seed, objs, attempt)
        if accept(cam):
            return cam
    raise AssertionError("no %s camera in %d draws for seed %d" % (family, attempts, seed))


# ---- scenes ---------------------------------------------------------------------
EXACT_SPHERE = ((0.0, 3.0, 0.0), 0.75)  # exact floats: (0, 3.75, 0) lies on its surface
EXACT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4.0, -4.0, 0.5))  # unrotated: x = 5 is the plane of a face


def small_scene(with_box=False):
    """The room, four of the benchmark's spheres, three small ones, a glass
    sphere at exact coordinates (the last sphere) and (with_box) an unrotated
    mirror box at exact coordinates."""
    objs = scenes.bench_objects(4, seed=4) + [
        scenes.sphere((0.0, 7.0, 0.5), 0.5, MATERIAL1),   # (what the degenerate cameras see looking out of the
        scenes.sphere((8.0, -4.0, 0.5), 0.5, MIRROR),     # sphere, off the box's face and straight down)
        scenes.sphere((1.0, 2.0, -3.0), 0.5, BLUE_GLASS),
        scenes.sphere(EXACT_SPHERE[0], EXACT_SPHERE[1], RED_GLASS)]
    if with_box:
        objs.append(scenes.box(EXACT_BOX[0], EXACT_BOX[1], EXACT_BOX[2], (0.0, 0.0, 0.0), MIRROR))
    return objs


def degenerate():
    """[(name, objects, camera)]: positions and angles on the boundaries of
    the host's and the kernels' case distinctions."""
    room, boxes = small_scene(), small_scene(with_box=True)
    n = len(room) - 1  # the exact sphere
    out = [("sphere_centre", room, make_camera((0.0, 3.0, 0.0), (0.0, 0.0, 0.0)), n),
           ("on_sphere_looking_in", room, make_camera((0.0, 3.75, 0.0), (0.0, 180.0, 0.0)), n),
           ("on_sphere_looking_out", room, make_camera((0.0, 3.75, 0.0), (0.0, 0.0, 0.0)), n),
           ("on_box_face_looking_in", boxes, make_camera((5.0, -4.0, 0.5), (0.0, 90.0, 0.0)), n + 1),
           ("on_box_face_looking_out", boxes, make_camera((5.0, -4.0, 0.5), (0.0, 270.0, 0.0)), n + 1),
           ("on_room_wall", room, make_camera((11.0, 2.0, 1.0), (10.0, 80.0, 0.0)), 0),
           ("pitch_up_90", room, make_camera((1.0, 2.0, 0.5), (90.0, 30.0, 0.0)), None),
           ("pitch_down_90", room, make_camera((1.0, 2.0, 0.5), (-90.0, 30.0, 0.0)), None),
           ("negative_zero_x", room, make_camera((-0.0, -3.0, 1.0), (10.0, 30.0, 0.0)), None)]
    cases = []
    for name, objs, cam, target in out:
        cam.target = target
        cases.append((name, objs, cam))
    return cases


DEGENERATE = [c[0] for c in degenerate()]


def degenerate_case(name):
    return next(c for c in degenerate() if c[0] == name)


def moved_box_scene():
    """Boxes for the `inside` family beside the benchmark's spheres: a rotated
    glass box and a rotated mirror box (so the scene is no room scene)."""
    return scenes.bench_objects(16, seed=16) + [
        scenes.box((-1.5, -1.0, -0.5), (1.0, 1.5, 2.0), (-2.0, 5.0, 1.0), (20.0, 40.0, 70.0), BLUE_GLASS),
        scenes.box((-0.5, -2.0, -0.75), (0.5, 2.0, 0.75), (4.0, -5.0, -1.0), (0.0, 0.0, 35.0), MATERIAL1)]


# ---- views ----------------------------------------------------------------------
def _matrix(view):
    return np.array(view.unprojection[:], np.float32).reshape(4, 4)  # [c] = column c


def scaled(view, k=-40):
    """The unprojection times 2^k: the same rays (every quotient is the same),
    w outside the short divisions' range (camera_short_divisions)."""
    return rt.view_from_matrix(_matrix(view) * np.float32(2.0 ** k), list(view.origin))


def negated(view):
    """The unprojection times -1: the same rays, every w negative."""
    return rt.view_from_matrix(-_matrix(view), list(view.origin))


def displaced(view, by=(0.5, 0.0, 0.0)):
    """The ray start moved off the matrix's eye: no pinhole, no culling."""
    return rt.view_from_matrix(_matrix(view), [a + b for a, b in zip(view.origin, by)])


def crop(view, zoom=8.0, centre=(0.3, -0.2)):
    """The unprojection right-multiplied by NDC (x, y) -> centre + (x, y) /
    zoom: an off-axis pinhole looking at a window of the base view's frame."""
    m = _matrix(view).astype(np.float64)
    out = m.copy()
    out[0], out[1] = m[0] / zoom, m[1] / zoom
    out[3] = m[3] + centre[0] * m[0] + centre[1] * m[1]
    return rt.view_from_matrix(out.astype(np.float32), list(view.origin))


VIEW_FAMILIES = {"scaled_down": lambda v: scaled(v, -40), "scaled_up": lambda v: scaled(v, 30), "negated": negated,
                 "displaced": displaced, "crop8": lambda v: crop(v, 8.0), "crop64": lambda v: crop(v, 64.0)}


# ---- the oracle's frame of a view -----------------------------------------------
def oracle_view(objs, view, w, h, depth, probe=0, rows=None, accumulate=None, **kw):
    """The oracle's render of any rt_view: its unprojection pinned, the ray
    start from a camera at view.origin. accumulate: render_accumulate's
    (spp, sample0, seed, accum) instead of a frame."""
    cam = make_camera(list(view.origin), (0.0, 0.0, 0.0))
    m = np.ascontiguousarray(np.array(view.unprojection[:], np.float32))
    port.lib().oracle_pin_unprojection(m.ctypes.data_as(C.c_void_p))
    try:
        if accumulate is not None:
            spp, sample0, seed, accum = accumulate
            return port.render_accumulate(objs, w, h, depth, spp, sample0, seed=seed, accum=accum, rows=rows,
                                          camera=cam, **kw)
        return port.render(objs, w, h, depth, 0.0, rows=rows, probe=probe, camera=cam, **kw)
    finally:
        port.lib().oracle_pin_unprojection(None)


def hit_objects(objs, view, w, h, **kw):
    """Probe 2's object plane: the index of every pixel's closest object, -1 for a miss."""
    return oracle_view(objs, view, w, h, 0, probe=2, **kw)[..., 0].astype(np.int64)
