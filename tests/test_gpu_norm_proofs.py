"""The room fast path without range votes (rt_internal.h kNormProofs), on the
GPU: the same bytes in every mode and launch kind, and the oracle's.

The modes are test_gpu_room_fast.py's: by default the plain room kernels (the
proofs as constants); RT_OPT_ROOM_FAST 0 the room kernels of the general launch
(votes); RT_OPT_SCENE_SHAPES 0 the general depth-0
kernels, which read the launch's proof at run time; both 0 the general code.
Each renders single frames, a tiled batch of 9 views and a persistent launch
forced with set_persistent0(8). (72, 24) has 9 wave tiles per row and 27 per
view. Which path ran: rt_debug_last_room_fast against the two proof hooks."""
import math

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from openglraytracer_amd.abi import MATERIAL1
from oracle import port, scenes
from room_fast_common import (PERSISTENT, PLAIN, ROOM, camera, explicit_view, last_room_fast, room_proof, room_scene,
                              zero_lights)

pytestmark = pytest.mark.gpu
SIZES = [(64, 40), (33, 17), (2, 2), (72, 24)]
DEFAULT, NO_FAST, NO_SHAPES, GENERAL = "default", "room_fast 0", "scene_shapes 0", "both 0"


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_persistent0(1)
    gpu_ctx.set_room_fast(True)
    gpu_ctx.set_scene_shapes(True)


def _batch(ctx, sc, w, h, views, persistent0):
    ctx.set_persistent0(persistent0)
    out = torch.zeros((len(views), h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(ctx, objs, views, cams_or_times, w, h, lights=None, expect=None):
    """cams_or_times: per view what the oracle renders it from (a Camera, a
    time of the orbit camera, or None: no oracle entry). expect: the case's own
    claim (scene half, view half) about the norm proofs."""
    room = [room_proof(objs, v, w, h, lights) for v in views]
    norm = [rt.norm_proof(objs, v, w, h, lights=lights)[0] for v in views]
    assert all(n[2] == 1 for n in norm)  # (the build asks for the proofs)
    if expect is not None:
        assert [n[:2] for n in norm] == [expect] * len(views), norm
    want = [int(all(r) and all(n)) for r, n in zip(room, norm)]
    want_general = [int(all(r[:3]) and all(n)) for r, n in zip(room, norm)]
    nine = [views[k % len(views)] for k in range(9)]
    sc = rt.Scene(ctx, objs, lights=lights)
    frames, ran = {}, {}
    try:
        for mode in (DEFAULT, NO_FAST, NO_SHAPES, GENERAL):
            ctx.set_room_fast(mode not in (NO_FAST, GENERAL))
            ctx.set_scene_shapes(mode not in (NO_SHAPES, GENERAL))
            single, fast = [], []
            for v in views:
                single.append(rt.render(ctx, sc, w, h, 0, view=v))
                fast.append(last_room_fast(ctx))
            tiled = _batch(ctx, sc, w, h, nine, 0)
            fast.append(last_room_fast(ctx))
            forced = _batch(ctx, sc, w, h, nine, 8)
            fast.append(last_room_fast(ctx))
            frames[mode], ran[mode] = (single, tiled, forced), (fast, rt.last_kernel(ctx))
    finally:
        sc.close()
    fast, key = ran[DEFAULT]
    assert fast == want + [int(all(want))] * 2, (fast, room, norm)
    assert key[3] & ROOM and (key[4] == PLAIN | PERSISTENT) == bool(all(want)), key
    assert ran[NO_FAST][0] == [0] * (len(views) + 2) and ran[NO_FAST][1][3] & ROOM and ran[NO_FAST][1][4] == 0
    assert ran[NO_SHAPES][0] == want_general + [int(all(want_general))] * 2 and ran[NO_SHAPES][1][3:5] == (0, 0)
    assert ran[GENERAL][0] == [0] * (len(views) + 2) and ran[GENERAL][1][3:5] == (0, 0)
    single, tiled, forced = frames[DEFAULT]
    for k in range(9):
        assert tiled[k].tobytes() == single[k % len(views)].tobytes(), k
    assert forced.tobytes() == tiled.tobytes()
    for mode in (NO_FAST, NO_SHAPES, GENERAL):
        for a, b in zip(frames[mode][0], single):
            assert a.tobytes() == b.tobytes(), (mode, parity_stats(a, b))
        assert frames[mode][1].tobytes() == tiled.tobytes(), mode
        assert frames[mode][2].tobytes() == tiled.tobytes(), mode
    for c, img in zip(cams_or_times, single):
        if c is None:
            continue
        o = (port.render(objs, w, h, 0, 0.0, lights=lights, camera=c) if isinstance(c, rt.Camera)
             else port.render(objs, w, h, 0, c, lights=lights))
        assert np.array_equal(img, o), parity_stats(img, o)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [1, 16, 40])
def test_orbit_camera(ctx, n, w, h):
    times = [0.0, 1.3, 7.0]
    _check(ctx, room_scene(n), [rt.make_view(None, t) for t in times], times, w, h, expect=(1, 1))


def _light_by_the_sphere(k):
    """One sphere the camera looks at and light 1 on the camera's side of it, k
    times the proof's margin from its surface."""
    c, r = (0.0, 4.0, 0.0), 0.75
    objs = [room_scene(1)[0], scenes.sphere(c, r, MATERIAL1)]
    _, (_, e2, gap) = rt.norm_proof(objs, rt.make_view(None, 0.0), 64, 40)
    lights = rt.reference_lights()
    lights[1].position[:] = (c[0], c[1] - (r + k * (math.sqrt(r * r + e2) + gap - r)), c[2])
    return objs, lights, camera((0.25, -2.0, 0.5), (0.0, 0.0, 0.0))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("k,ok", [(1.02, 1), (0.98, 0)])
def test_a_light_at_the_margin_from_a_sphere(ctx, k, ok, w, h):
    """Just outside the margin: short shadow directions on the vote-less path.
    Just inside it: the launch's proof fails, the kernels of the general launch
    run, and the frame is still the oracle's."""
    objs, lights, cam = _light_by_the_sphere(k)
    cams = [cam, camera((3.0, -3.0, 1.0), (5.0, 40.0, 0.0))]
    _check(ctx, objs, [rt.make_view(c, 0.0) for c in cams], cams, w, h, lights=lights, expect=(ok, 1))


@pytest.mark.parametrize("w,h", SIZES)
def test_a_camera_near_a_wall_and_a_corner(ctx, w, h):
    """Cameras a hundredth of a unit from a wall and in a corner: hit points
    right beside the camera (the shortest primary rays the room allows) and the
    room's edges and corners in view."""
    cams = [camera((10.98, 3.0, 1.0), (10.0, 30.0, 0.0)), camera((10.995, -10.995, 10.99), (-35.0, 225.0, 0.0)),
            camera((-10.99, 0.0, -10.9), (40.0, 135.0, 0.0))]
    _check(ctx, room_scene(16, zero_sphere=True), [rt.make_view(c, 0.0) for c in cams], cams, w, h, expect=(1, 1))


@pytest.mark.parametrize("w,h", SIZES)
def test_exactly_zero_direction_components(ctx, w, h):
    views = [explicit_view(o) for o in ((2.0, 1.0, 0.5), (-2.0, 1.0, -0.5), (0.25, -4.0, 4.0))]
    _check(ctx, room_scene(16, zero_sphere=True), views, [None] * 3, w, h, lights=zero_lights(), expect=(1, 1))
