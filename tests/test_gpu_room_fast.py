"""The room fast path (rt_kernel.hip closest_impl / resolve_impl<true, kRoom>:
the primary box hit of a room without the products by its identity matrices)
renders the same bytes as the general code, and as the oracle.

Every case renders small, ragged frames four ways: the default (the fast path
where the host's proof holds), RT_OPT_ROOM_FAST 0 (the room kernels of the
general launch shape), RT_OPT_SCENE_SHAPES 0 (the general kernel, which reads
the proof's answer from the launch and takes the same path at run time) and
both options 0 (the general kernel's general code), each as one frame, as a
tiled batch of 9 views and as a persistent launch forced the way
test_persistent0.py forces it. rt_debug_last_room_fast says which path a
launch took; the expectation comes from rt_debug_room_proof (host)."""
import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from oracle import port
from room_fast_common import (PERSISTENT, PLAIN, ROOM, camera, explicit_view, last_room_fast, room_proof, room_scene,
                              zero_lights)

pytestmark = pytest.mark.gpu
SIZES = [(64, 40), (33, 17), (2, 2)]
DEFAULT, NO_FAST, NO_SHAPES, GENERAL = "default", "room_fast 0", "scene_shapes 0", "both 0"


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_persistent0(1)
    gpu_ctx.set_room_fast(True)
    gpu_ctx.set_scene_shapes(True)


def _mode(ctx, mode):
    ctx.set_room_fast(mode not in (NO_FAST, GENERAL))
    ctx.set_scene_shapes(mode not in (NO_SHAPES, GENERAL))


def _batch(ctx, sc, w, h, views, persistent0):
    ctx.set_persistent0(persistent0)
    out = torch.zeros((len(views), h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(ctx, objs, views, cams_or_times, w, h, lights=None, expect_fast=None):
    """Renders the views in every mode and launch kind; returns the fast
    path's answers of the default mode. cams_or_times: per view, what the
    oracle renders it from (a Camera, a time of the orbit camera, or None: an
    explicit matrix the oracle has no entry for)."""
    proofs = [room_proof(objs, v, w, h, lights) for v in views]
    want = [int(all(p)) for p in proofs]
    want_general = [int(all(p[:3])) for p in proofs]  # (the general kernel asks for neither a shape nor the short divisions)
    if expect_fast is not None:  # (the case's own claim about its views, so the proof hook is not the only witness)
        assert want == [int(expect_fast)] * len(views), proofs
    # 9 views for the batches: the case's views in turn
    nine = [views[k % len(views)] for k in range(9)]
    sc = rt.Scene(ctx, objs, lights=lights)
    frames, ran = {}, {}
    try:
        for mode in (DEFAULT, NO_FAST, NO_SHAPES, GENERAL):
            _mode(ctx, mode)
            single, fast = [], []
            for v in views:
                single.append(rt.render(ctx, sc, w, h, 0, view=v))
                fast.append(last_room_fast(ctx))
            tiled = _batch(ctx, sc, w, h, nine, 0)
            fast.append(last_room_fast(ctx))
            forced = _batch(ctx, sc, w, h, nine, 8)
            fast.append(last_room_fast(ctx))
            key = rt.last_kernel(ctx)
            frames[mode], ran[mode] = (single, tiled, forced), (fast, key)
    finally:
        sc.close()
    # which path ran: per single view its own proof, per batch every view's
    fast, key = ran[DEFAULT]
    assert fast == want + [int(all(want))] * 2, (fast, proofs)
    assert key[3] & ROOM and (key[4] == PLAIN | PERSISTENT) == bool(all(want)), key
    assert ran[NO_FAST][0] == [0] * (len(views) + 2) and ran[NO_FAST][1][3] & ROOM and ran[NO_FAST][1][4] == 0
    assert ran[NO_SHAPES][0] == want_general + [int(all(want_general))] * 2 and ran[NO_SHAPES][1][3:5] == (0, 0)
    assert ran[GENERAL][0] == [0] * (len(views) + 2) and ran[GENERAL][1][3:5] == (0, 0)
    # the same bytes every way
    single, tiled, forced = frames[DEFAULT]
    for k in range(9):
        assert tiled[k].tobytes() == single[k % len(views)].tobytes(), k
    assert forced.tobytes() == tiled.tobytes()
    for mode in (NO_FAST, NO_SHAPES, GENERAL):
        for a, b in zip(frames[mode][0], single):
            assert a.tobytes() == b.tobytes(), (mode, parity_stats(a, b))
        assert frames[mode][1].tobytes() == tiled.tobytes(), mode
        assert frames[mode][2].tobytes() == tiled.tobytes(), mode
    # and the oracle's
    for v, c, img in zip(views, cams_or_times, single):
        if c is None:
            continue
        o = (port.render(objs, w, h, 0, 0.0, lights=lights, camera=c) if isinstance(c, rt.Camera)
             else port.render(objs, w, h, 0, c, lights=lights))
        assert np.array_equal(img, o), parity_stats(img, o)
    return want


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [1, 16, 40])
def test_orbit_camera(ctx, n, w, h):
    """The reference orbit camera (z = 0 exactly) at several times; 1, 16 and
    40 spheres: 2-byte and 8-byte masks."""
    times = [0.0, 0.1, 1.3, 7.0]
    _check(ctx, room_scene(n), [rt.make_view(None, t) for t in times], times, w, h, expect_fast=True)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("offset", [(0.5, -0.25, 0.0), (-1.0, -0.5, -0.125)])
def test_translated_room_zero_light_and_zero_sphere(ctx, offset, w, h):
    """The room moved by non-zero, negative and zero offsets; a light on
    x = 0 and a sphere centre with two zero coordinates."""
    times = [0.0, 2.5]
    _check(ctx, room_scene(16, offset, zero_sphere=True), [rt.make_view(None, t) for t in times], times, w, h,
           lights=zero_lights(), expect_fast=True)


@pytest.mark.parametrize("w,h", SIZES)
def test_exactly_zero_direction_components(ctx, w, h):
    """Explicit views whose centre column, centre row and centre pixel give
    rays with direction components that are exactly zero."""
    views = [explicit_view(o) for o in ((2.0, 1.0, 0.5), (-2.0, 1.0, -0.5), (0.25, -4.0, 4.0))]
    _check(ctx, room_scene(16, zero_sphere=True), views, [None] * 3, w, h, lights=zero_lights(), expect_fast=True)


@pytest.mark.parametrize("w,h", SIZES)
def test_cameras_on_x_zero_and_at_the_origin(ctx, w, h):
    """Box-local camera coordinates that are +0; axis-aligned cameras, whose
    rays have zero components too. (Whichever path the host picks for them —
    the proof hook says — the frames are the general code's and the oracle's.)"""
    cams = [camera((0.0, 3.0, 1.0), (10.0, 30.0, 0.0)), camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
            camera((0.0, 0.0, 0.0), (0.0, 90.0, 0.0)), camera((0.0, -5.0, 0.0), (-20.0, 200.0, 0.0))]
    _check(ctx, room_scene(16, zero_sphere=True), [rt.make_view(c, 0.0) for c in cams], cams, w, h)


@pytest.mark.parametrize("w,h", SIZES[:2])
@pytest.mark.parametrize("case", ["negative_zero_record", "on_the_wall", "outside"])
def test_outside_the_proof_the_general_path_renders_the_oracles_frame(ctx, case, w, h):
    objs = room_scene(16, angles=(0.0, 0.0, -0.0) if case == "negative_zero_record" else (0.0, 0.0, 0.0))
    pos = {"negative_zero_record": (3.0, 2.0, 1.0), "on_the_wall": (11.0, 2.0, 1.0), "outside": (20.0, 2.0, 1.0)}[case]
    cams = [camera(pos, (10.0, 30.0, 0.0)), camera(pos, (-15.0, 250.0, 0.0))]
    _check(ctx, objs, [rt.make_view(c, 0.0) for c in cams], cams, w, h, expect_fast=False)
