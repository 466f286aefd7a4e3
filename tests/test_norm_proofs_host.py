"""The range proofs that let the room fast path take its inverse square
roots without per-wave votes (rt_internal.h kNormProofs), on the host (no
GPU): rt_debug_norm_proof runs build_scene with norm_proof_scene and
camera_norm_range; rt_debug_select_kernel shows what a launch with and
without the launch's proof takes. The unit-length forms (inv_sqrt_near_one for
the view vector and the reflected light direction) need no host data: a
float32 emulation here bounds how far those squared lengths stray from 1."""
import math

import numpy as np
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd.abi import MATERIAL1 as MAT, WALL
from oracle import scenes
from room_fast_common import FIXED, PERSISTENT, PLAIN, ROOM, camera, explicit_view, room_proof, room_scene, zero_lights
from test_kernel_table_host import BASE

W, H = 64, 40
SIZES = [(64, 40), (33, 17), (2, 2), (72, 24), (1920, 1080)]


def _proof(objs, view=None, w=W, h=H, lights=None):
    return rt.norm_proof(objs, view if view is not None else rt.make_view(None, 0.0), w, h, lights=lights)


def _live_lights():
    return [tuple(l.position) for l in rt.reference_lights()[1:]]  # (light 0 is dead: no material takes it)


def _sphere(o):
    return tuple(o.position), abs(o.radius)


@pytest.mark.parametrize("n,gap", [(16, 3.5), (40, 0.24), (64, 0.24), (256, 0.24)])
def test_the_bench_scenes_pass_by_a_wide_margin(n, gap):
    objs = scenes.bench_objects(n, seed=0)
    smallest = min(abs(math.dist(L, c) - r) for L in _live_lights() for c, r in map(_sphere, objs[1:]))
    assert abs(smallest - gap) < 0.02 * gap + 0.005, smallest  # the generator's formula: 3.537 and 0.2432
    for t in (0.0, 0.1, 1.3, 7.0, 100.0):
        for w, h in SIZES:
            flags, (B, e2, g) = _proof(objs, rt.make_view(None, t), w, h)
            assert flags == (1, 1, 1), (n, t, w, h)
    # what the scene half asked of that light and sphere: several times less
    assert B == 11.0 and e2 == 2.0 ** -12 * 121.0 and g == 2.0 ** -12 * 11.0
    need = max(math.sqrt(r * r + e2) + g - r for _, r in map(_sphere, objs[1:]))
    assert smallest > 4.0 * need, (smallest, need)


def _with_light(pos):
    lights = rt.reference_lights()
    lights[1].position[:] = pos
    return lights


def _target():
    """The room with one sphere, and the margins the proof asks of a light's
    distance from its centre: outside and inside the sphere."""
    c, r = (1.0, 2.0, -1.0), 0.75
    objs = [room_scene(1)[0], scenes.sphere(c, r, MAT)]
    _, (_, e2, g) = _proof(objs)
    return objs, c, r, math.sqrt(r * r + e2) + g - r, r - (math.sqrt(r * r - e2) - g)


def test_a_light_near_a_spheres_surface_fails_the_scene_half():
    objs, c, r, m_out, m_in = _target()
    at = lambda d: _with_light((c[0] + d, c[1], c[2]))
    assert _proof(objs, lights=at(r + 1.01 * m_out))[0] == (1, 1, 1)
    assert _proof(objs, lights=at(r - 1.01 * m_in))[0] == (1, 1, 1)
    for d in (r + 0.5 * m_out, r - 0.5 * m_in, r):  # half the margin outside and inside; on the surface
        assert _proof(objs, lights=at(d))[0] == (0, 1, 1), d


def test_a_light_on_a_wall_plane_fails_the_scene_half():
    objs = room_scene(16)
    _, (_, _, g) = _proof(objs)
    assert _proof(objs, lights=_with_light((10.5, 1.0, 1.0)))[0][0] == 1
    assert _proof(objs, lights=_with_light((11.0 - 0.5 * g, 1.0, 1.0)))[0][0] == 0


def test_radii_and_extents_outside_the_ranges_fail_the_scene_half():
    room = room_scene(1)[0]
    assert _proof([room, scenes.sphere((1.0, 2.0, -1.0), 0.75, MAT)])[0][0] == 1
    assert _proof([room, scenes.sphere((1.0, 2.0, -1.0), 2.0 ** -50, MAT)])[0][0] == 0
    # (a radius under sqrt(2 e2) = B / 45 fails too: the hit point's error could reach the centre)
    assert _proof([room, scenes.sphere((1.0, 2.0, -1.0), 0.2, MAT)])[0][0] == 0
    big = scenes.box((-2.0 ** 21,) * 3, (2.0 ** 21,) * 3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), WALL)
    flags, terms = _proof([big, scenes.sphere((1.0, 2.0, -1.0), 2.0 ** 16, MAT)])
    assert flags[0] == 0 and terms == (0.0, 0.0, 0.0)
    # a scene that is no room has no scene half
    assert _proof(room_scene(16, angles=(0.0, 5.0, 0.0)))[0][0] == 0


@pytest.mark.parametrize("scale,ok", [(1.0, 1), (2.0 ** 12, 1), (2.0 ** -12, 1), (2.0 ** 55, 0), (2.0 ** -60, 0)])
def test_an_unprojection_scaled_out_of_range_fails_the_view_half(scale, ok):
    """Rows 0-2 of the unprojection scaled: every point, and so e3 - s3, by `scale`."""
    o = (2.0, 1.0, 0.5)
    m = np.array(explicit_view(o).unprojection, np.float32).reshape(4, 4)  # m[c] = column c
    m[:, :3] *= np.float32(scale)
    view = rt.view_from_matrix(m.reshape(-1), o)
    assert _proof(room_scene(16), view)[0][1] == ok


def _coupled_cases():
    """Every scene and view of test_gpu_room_fast.py and test_room_fast_host.py."""
    for n in (1, 16, 40):
        for off in ((0.0, 0.0, 0.0), (0.5, -0.25, 0.0), (-1.0, -0.5, -0.125)):
            for t in (0.0, 0.1, 0.4, 1.3, 2.5, 7.0):
                yield room_scene(n, off), rt.make_view(None, t), None
                yield room_scene(n, off, zero_sphere=True), rt.make_view(None, t), zero_lights()
    for o in ((2.0, 1.0, 0.5), (-2.0, 1.0, -0.5), (0.25, -4.0, 4.0)):
        yield room_scene(16), explicit_view(o), None
        yield room_scene(16, zero_sphere=True), explicit_view(o), zero_lights()
    for pos, ang in (((0.0, 3.0, 1.0), (10.0, 30.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                     ((0.0, 0.0, 0.0), (0.0, 90.0, 0.0)), ((0.0, -5.0, 0.0), (-20.0, 200.0, 0.0)),
                     ((0.0, 0.0, 0.0), (10.0, 30.0, 0.0)), ((0.0, -5.0, 0.0), (10.0, 30.0, 0.0)),
                     ((-0.0, -3.0, 1.0), (10.0, 30.0, 0.0)), ((-0.0, 3.0, 1.0), (10.0, 30.0, 0.0)),
                     ((3.0, 2.0, 1.0), (10.0, 30.0, 0.0)), ((3.0, 2.0, 1.0), (-15.0, 250.0, 0.0)),
                     ((11.0, 2.0, 1.0), (10.0, 30.0, 0.0)), ((20.0, 2.0, 1.0), (-15.0, 250.0, 0.0))):
        for zero in (False, True):
            yield room_scene(16, zero_sphere=zero), rt.make_view(camera(pos, ang), 0.0), None
    yield room_scene(16, (1.0, 0.0, 0.0)), rt.make_view(camera((1.0, 3.0, 1.0), (10.0, 30.0, 0.0)), 0.0), None
    for pos in ((10.5, 0.0, 0.0), (11.0, 0.0, 0.0), (0.0, -11.0, 2.0), (20.0, 0.0, 0.0), (0.0, 0.0, -40.0)):
        view = rt.make_view(None, 0.0)
        view.origin[:] = pos
        yield room_scene(16), view, None
    yield room_scene(16, angles=(0.0, 0.0, -0.0)), rt.make_view(None, 0.0), None


def test_what_passes_the_room_proof_in_the_room_fast_tests_passes_these_too():
    """Those tests tell which path ran from the room proof's flags alone, and
    the norm proofs join the launch's room proof: a case of theirs inside the
    one must be inside the other."""
    inside = 0
    for objs, view, lights in _coupled_cases():
        for w, h in SIZES[:3]:
            if all(room_proof(objs, view, w, h, lights)[:3]):  # (the general kernels ask for no more)
                inside += 1
                assert _proof(objs, view, w, h, lights)[0] == (1, 1, 1), (w, h, list(view.origin))
    assert inside > 300


def test_unit_vectors_stay_within_64_steps_of_length_one():
    """float32 as the kernel orders it: view = -normalize(a), lref = -l + n (2 cos)
    with l and n normalised (n an axis for half the samples); vectors of
    magnitude 1e-3, 1 and 30. inv_sqrt_near_one is exact within +-2048 steps
    (tests/test_host.py); these stay within +-64."""
    f, rng, n = np.float32, np.random.default_rng(18), 4_000_000

    def dot(a, b):
        return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])

    def normalize(a):
        r = f(1) / np.sqrt(dot(a, a))  # (numpy's float32 sqrt and division round correctly)
        return [a[0] * r, a[1] * r, a[2] * r]

    def steps(d):
        return d.view(np.int32).astype(np.int64) - 0x3F800000

    lo, hi = 0, 0
    for scale in (1e-3, 1.0, 30.0):
        a, nrm, l = (normalize([(rng.standard_normal(n) * scale).astype(f) for _ in range(3)]) for _ in range(3))
        axis, sign, pick = rng.integers(0, 3, n), np.where(rng.random(n) < 0.5, f(-1), f(1)).astype(f), rng.random(n) < 0.5
        nrm = [np.where(pick, np.where(axis == k, sign, f(0)), nrm[k]).astype(f) for k in range(3)]
        view = [-a[0], -a[1], -a[2]]
        t = f(2) * -dot(l, nrm)
        lref = [-l[k] - nrm[k] * t for k in range(3)]
        for d in (dot(view, view), dot(lref, lref)):
            assert d.dtype == np.float32
            lo, hi = min(lo, int(steps(d).min())), max(hi, int(steps(d).max()))
    assert -64 <= lo and hi <= 64, (lo, hi)  # 1.2e7 samples of each


def _select(proof, **kw):
    return rt.select_kernel(list(dict(BASE, **kw).values()) + [proof])


@pytest.mark.parametrize("mask", [2, 4, 8])
def test_the_rows_inside_and_outside_the_proofs(mask):
    """No kernel is added: inside the launch's proof the rows are the plain
    room kernels as before, outside it the room kernels of the general launch."""
    big = dict(n_views=300, width=1920, height=1080, n_rows=1080)
    assert _select(1, mask_bytes=mask) == (1, (0, 0, 1, mask | ROOM, PLAIN))
    assert _select(1, mask_bytes=mask, **big) == (1, (0, 0, 1, mask | ROOM | FIXED, PLAIN | PERSISTENT))
    assert _select(0, mask_bytes=mask) == (1, (0, 0, 1, mask | ROOM, 0))
    assert _select(0, mask_bytes=mask, **big) == (1, (0, 0, 1, mask | ROOM, 0))
