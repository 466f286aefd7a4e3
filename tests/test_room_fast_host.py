"""The room fast path's proof and its place in the kernel selection, on the
host (no GPU): rt_debug_room_proof runs build_scene, room_record_identity,
the host's frame constants and room_view_inside; rt_debug_select_kernel with
27 fields carries the launch's proof into select_kernel.

A launch with the proof keeps the plain (and persistent) room kernels, which
hold the fast path; one without it takes the room kernel of the general launch
shape, a row the table already had."""
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from room_fast_common import FIXED, PERSISTENT, PLAIN, ROOM, camera, explicit_view, room_proof, room_scene, zero_lights
from test_kernel_table_host import BASE

W, H = 64, 40


def _orbit(t):
    return rt.make_view(None, t)


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (0.5, -0.25, 0.0), (-1.0, -0.5, -0.125)])
@pytest.mark.parametrize("n", [1, 16, 40])
def test_the_benchmark_room_from_the_orbit_camera_is_inside_the_proof(n, offset):
    for t in (0.0, 0.1, 1.3, 7.0):
        assert room_proof(room_scene(n, offset), _orbit(t), W, H) == (1, 1, 1, 1, 1), (n, offset, t)
    assert room_proof(room_scene(n, offset, zero_sphere=True), _orbit(0.4), W, H, zero_lights()) == (1, 1, 1, 1, 1)


def test_explicit_views_with_zero_direction_components():
    for o in ((2.0, 1.0, 0.5), (-2.0, 1.0, -0.5), (0.25, -4.0, 4.0)):
        assert room_proof(room_scene(16), explicit_view(o), W, H) == (1, 1, 1, 1, 1), o


def test_cameras_on_a_coordinate_plane_and_at_the_origin():
    """Strictly inside, finite, +0 coordinates: the view half holds. (Whether
    such a view's divisions take the short form is camera_short_divisions'
    own question; a launch needs both.)"""
    for pos in ((0.0, 3.0, 1.0), (0.0, 0.0, 0.0), (0.0, -5.0, 0.0)):
        room, ident, inside, _, _ = room_proof(room_scene(16), rt.make_view(camera(pos, (10.0, 30.0, 0.0)), 0.0), W, H)
        assert (room, ident, inside) == (1, 1, 1), pos


def test_a_negative_zero_box_local_camera_coordinate_is_outside_the_proof():
    """The view half reads the view's own record of the box, the kernel's
    box_cam: ((1 x + 0 y) + -0 z) + -0 with the reference chain's zeros for the
    room at the origin, which is -0 only when every term is."""
    view = rt.make_view(camera((-0.0, -3.0, 1.0), (10.0, 30.0, 0.0)), 0.0)
    assert room_proof(room_scene(16), view, W, H)[:3] == (1, 1, 0)
    view = rt.make_view(camera((-0.0, 3.0, 1.0), (10.0, 30.0, 0.0)), 0.0)  # (-0 + +0 = +0)
    assert room_proof(room_scene(16), view, W, H)[:3] == (1, 1, 1)
    # the room moved so that the box-local coordinate is 1 + -1 = +0: inside it
    view = rt.make_view(camera((1.0, 3.0, 1.0), (10.0, 30.0, 0.0)), 0.0)
    assert room_proof(room_scene(16, (1.0, 0.0, 0.0)), view, W, H)[:3] == (1, 1, 1)


@pytest.mark.parametrize("pos,inside", [((10.5, 0.0, 0.0), 1), ((11.0, 0.0, 0.0), 0), ((0.0, -11.0, 2.0), 0),
                                        ((20.0, 0.0, 0.0), 0), ((0.0, 0.0, -40.0), 0),
                                        ((float("nan"), 0.0, 0.0), 0), ((float("inf"), 0.0, 0.0), 0)])
def test_a_camera_on_a_wall_or_outside_the_box_is_outside_the_proof(pos, inside):
    view = rt.make_view(None, 0.0)
    view.origin[:] = pos
    assert room_proof(room_scene(16), view, W, H)[:3] == (1, 1, inside)


def test_a_room_record_with_a_negative_zero_is_outside_the_proof():
    """A roll of -0 degrees moves the -0 terms of the normal matrix (sin(-0)
    = -0): still translate-only, still a room (the comparisons take -0 for 0),
    but the matrix then takes the axis (-1, -0, -0) to (-1, +0, -0), not to
    the (-1, +0, +0) that the reference's own room gives and the fast path
    writes."""
    objs = room_scene(16, angles=(0.0, 0.0, -0.0))
    assert room_proof(objs, _orbit(0.0), W, H)[:2] == (1, 0)
    # a rotated box is no room at all
    assert room_proof(room_scene(16, angles=(0.0, 5.0, 0.0)), _orbit(0.0), W, H)[:2] == (0, 0)
    # nor is a scene of two boxes
    assert room_proof(room_scene(16) + [room_scene(1)[0]], _orbit(0.0), W, H)[:2] == (0, 0)


def _select(proof=None, **kw):
    f = list(dict(BASE, **kw).values())
    return rt.select_kernel(f if proof is None else f + [proof])


@pytest.mark.parametrize("mask", [2, 4, 8])
def test_a_launch_whose_proof_fails_takes_the_general_launch_shape(mask):
    big = dict(n_views=300, width=1920, height=1080, n_rows=1080)
    # with the proof (27 fields, or 26: it holds): the plain and the persistent room kernels
    for proof in (None, 1):
        assert _select(proof, mask_bytes=mask) == (1, (0, 0, 1, mask | ROOM, PLAIN))
        assert _select(proof, mask_bytes=mask, dev_views=0) == (1, (0, 0, 0, mask | ROOM, PLAIN))
        assert _select(proof, mask_bytes=mask, **big) == (1, (0, 0, 1, mask | ROOM | FIXED, PLAIN | PERSISTENT))
        assert _select(proof, mask_bytes=mask, persistent0=8) == (1, (0, 0, 1, mask | ROOM | FIXED, PLAIN | PERSISTENT))
    # without it: the room kernel of the general launch, tiled, whatever the persistence option
    assert _select(0, mask_bytes=mask) == (1, (0, 0, 1, mask | ROOM, 0))
    assert _select(0, mask_bytes=mask, dev_views=0) == (1, (0, 0, 0, mask | ROOM, 0))
    assert _select(0, mask_bytes=mask, **big) == (1, (0, 0, 1, mask | ROOM, 0))
    assert _select(0, mask_bytes=mask, persistent0=8) == (1, (0, 0, 1, mask | ROOM, 0))
    # a scene that is no room does not ask for the proof
    assert _select(0, mask_bytes=mask, room=0) == (1, (0, 0, 1, mask, PLAIN))
    assert _select(0, mask_bytes=mask, room=0, **big) == (1, (0, 0, 1, mask | FIXED, PLAIN | PERSISTENT))
    # nor do the other kernels: Monte-Carlo, depth 2
    assert _select(0, mask_bytes=mask, spp=4, dev_views=0) == (1, (0, 1, 0, mask | ROOM, 0))
    assert _select(0, max_depth=2, dev_views=0, wide=1) == (1, (2, 0, 0, 32 | ROOM, 0))


def test_the_option_is_a_context_option():
    assert abi.RT_OPT_ROOM_FAST == 12
