"""Shared by the room fast path's tests (test_room_fast_host.py,
test_gpu_room_fast.py): the scenes, the views and the host-only hooks.

The fast path (rt_kernel.hip closest_impl / resolve_impl<true, kRoom>) runs in
the room kernels of a plain launch; launch_shape gives a room scene the plain
launch only with the host's proof: the room's record is the identity as far
as a result can tell (room_record_identity) and every view's record of the
box says the camera is strictly inside it, finite, no component a negative
zero (room_view_inside)."""
import ctypes as C

import numpy as np

import openglraytracer_amd as rt
from openglraytracer_amd.abi import MATERIAL1, MIRROR, WALL
from oracle import scenes

ROOM, FIXED, PLAIN, PERSISTENT = 16, 64, 1, 2  # rt_internal.h kShapeRoom, kShapeFixed, kLaunchPlain, kLaunchPersistent


def room_proof(objs, view, w, h, lights=None, materials=None):
    """rt_debug_room_proof: (room, identity record, camera inside, short divisions, pinhole view)."""
    mats = materials if materials is not None else rt.reference_materials()
    lights = lights if lights is not None else rt.reference_lights()
    oa, ma, la = (rt.Object * len(objs))(*objs), (rt.Material * len(mats))(*mats), (rt.Light * len(lights))(*lights)
    out = (C.c_int32 * 5)()
    f = rt.lib().rt_debug_room_proof
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                  C.c_void_p]
    f.restype = C.c_int
    assert f(oa, len(objs), ma, len(mats), la, len(lights), C.byref(view), w, h, out) == 0
    return tuple(out)


def last_room_fast(ctx):
    """rt_debug_last_room_fast: the context's last launch took the fast path."""
    f = rt.lib().rt_debug_last_room_fast
    f.argtypes = [C.c_void_p]
    f.restype = C.c_int
    return f(ctx.handle)


def room_at(offset, angles=(0.0, 0.0, 0.0)):
    """The +-11 room placed at `offset`."""
    return scenes.box((-11.0,) * 3, (11.0,) * 3, offset, angles, WALL)


def room_scene(n_spheres, offset=(0.0, 0.0, 0.0), angles=(0.0, 0.0, 0.0), zero_sphere=False):
    """The room at `offset` with the benchmark's seeded spheres; zero_sphere:
    one more whose centre has two zero coordinates."""
    objs = [room_at(offset, angles)] + scenes.bench_objects(n_spheres, seed=n_spheres)[1:]
    if zero_sphere:
        objs.append(scenes.sphere((0.0, 3.0, 0.0), 0.75, MATERIAL1 if n_spheres % 2 else MIRROR))
    return objs


def zero_lights():
    """The reference's lights, the first moved onto the plane x = 0."""
    lights = rt.reference_lights()
    lights[0].position[0] = 0.0
    return lights


def camera(position, angles=(0.0, 0.0, 0.0)):
    cam = rt.Camera()
    cam.position[:] = position
    cam.angles[:] = angles
    cam.v_fov, cam.aspect, cam.near_plane, cam.far_plane = 60.0, 16.0 / 9.0, 0.1, 1000.0
    return cam


def explicit_view(o, a=0.9, b=0.5, p=-0.45, q=0.55):
    """A pinhole view written out as its unprojection: NDC (vx, vy, z) is the
    world point o + (a vx, 1, b vy) / (p z + q). With the coordinates of o
    powers of two, rows 0 and 2 of the matrix at vx = 0 / vy = 0 are exact
    multiples of row 3, so both of a ray's points have x = o.x on the centre
    column and z = o.z on the centre row, bit for bit: direction components
    that are exactly zero (both on the centre pixel, whose ray is (0, 1, 0))."""
    m = np.zeros((4, 4), np.float32)  # m[c] = column c
    m[0] = (a, 0.0, 0.0, 0.0)
    m[1] = (0.0, 0.0, b, 0.0)
    m[2] = (o[0] * p, o[1] * p, o[2] * p, p)
    m[3] = (o[0] * q, 1.0 + o[1] * q, o[2] * q, q)
    return rt.view_from_matrix(m.reshape(-1), o)
