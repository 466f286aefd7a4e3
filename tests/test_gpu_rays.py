"""Ray queries (rt_trace_rays, rt_view_rays) on the GPU.

The checker is the oracle: for a camera its probe 1 is the exact direction it
traces for each pixel, probe 0 the ray's colour, probes 2, 3, 4 its first hit's
record, normal and point (rays_common.RaySet). The rays of several cameras are
concatenated and traced in a seeded permutation, so a wave mixes origins; the
planes, un-permuted, must equal the oracle's. Then the existing paths: the
rays rt_view_rays writes, traced, are rt_render_view's and
rt_render_hits_view's frames byte for byte. Every comparison is np.array_equal
or equality of tobytes().
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import load_fixture, manifest
from openglraytracer_amd import abi
from oracle import scenes
from rays_common import (RaySet, camera, check_records, check_set_f, check_set_r, set_f, set_r)
from test_gpu_parity import box_scene, random_scene

pytestmark = pytest.mark.gpu
W, H = 33, 17  # the round trip's frame: ragged in both tile directions, 561 rays (ragged last wave)
CANARY = 0xA5


def trace_all(ctx, sc, rays, depth, shadow=True):
    """(colors, hits, normals, points) of host rays."""
    return rt.trace_rays(ctx, sc, rays, depth, colors=True, hits=True, normals=True, points=True, shadow=shadow)


def check_set(ctx, rs, depths, what):
    """The set's permuted rays against the oracle: colours at every depth, the records once."""
    sc = rt.Scene(ctx, rs.objs, materials=rs.materials, lights=rs.lights)
    try:
        rays = rs.permuted()
        for k, d in enumerate(depths):
            if k == 0:
                col, hits, normals, points = trace_all(ctx, sc, rays, d)
                check_records([rs.unpermute(p) for p in (hits, normals, points)], rs, what)
            else:
                (col,) = rt.trace_rays(ctx, sc, rays, d)
            assert col.shape == (rs.n, 4) and (col[:, 3] == 0).all(), (what, d)
            assert np.array_equal(rs.unpermute(col), rs.colors[d]), (what, d)
    finally:
        sc.close()


@pytest.fixture(params=[True, False], ids=["culling", "no_culling"])
def culling(request, gpu_ctx):
    gpu_ctx.set_culling(request.param)
    yield request.param
    gpu_ctx.set_culling(True)


# ---- 1. the oracle ------------------------------------------------------------
@pytest.fixture(scope="module")
def rset():
    rs = set_r()
    check_set_r(rs)
    return rs


@pytest.fixture(scope="module")
def fset():
    rs = set_f()
    check_set_f(rs)
    return rs


def test_set_r_matches_the_oracle(gpu_ctx, rset, culling):
    """bench_objects(16) from the orbit camera, from inside the room, from four
    sphere centres (every ray starts inside a sphere) and from outside the
    room, depths 0, 1, 2, 5, 9."""
    check_set(gpu_ctx, rset, rset.colors.keys(), "set R")


def test_set_f_far_origins_match_the_oracle(gpu_ctx, fset, culling):
    """63 spheres without a room from 41, 3,640 and 7,800 units away: the far
    origins lie outside the range the sphere BVH's node test is proved for and
    take the exhaustive tests; depths 0 and 2."""
    check_set(gpu_ctx, fset, fset.colors.keys(), "set F")


def test_config1_matches_the_oracle(gpu_ctx, culling):
    """Config 1 (no room): hits and misses from the orbit camera."""
    rs = RaySet(scenes.config1_objects(), [None], 16, 9, (0, 1))
    assert [(rs.objects(0) >= 0).sum(), (rs.objects(0) < 0).sum()] == [67, 77]
    check_set(gpu_ctx, rs, (0, 1), "config 1")


def test_shipped_scene_matches_the_oracle(gpu_ctx, culling):
    """The shipped scene at t = 3.7 (rotated boxes) from the orbit camera and from outside the room."""
    rs = RaySet(rt.reference_objects(3.7), [None, camera((30.0, -25.0, 12.0), (0.0, 0.0, 0.0))], 16, 9, (0, 3),
                time=3.7)
    assert (rs.objects(0) >= 0).all() and (rs.objects(1) >= 0).any() and (rs.objects(1) < 0).any()
    check_set(gpu_ctx, rs, (0, 3), "shipped t=3.7")


@pytest.mark.parametrize("make,seed", [(random_scene, s) for s in range(8)] + [(box_scene, s) for s in range(4)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_random_scenes_match_the_oracle(gpu_ctx, make, seed, culling):
    """random_scene / box_scene (test_gpu_parity): their own view's rays as the
    oracle traces them, permuted, depth 0, all four planes with shadow bits."""
    objs, mats, lights, t, _, w, h = make(seed)
    rs = RaySet(objs, [None], w, h, (0,), materials=mats, lights=lights, time=t)
    check_set(gpu_ctx, rs, (0,), (make.__name__, seed))


# ---- 2. the existing paths ------------------------------------------------------
@pytest.fixture(scope="module")
def room16(gpu_ctx):
    sc = rt.Scene(gpu_ctx, scenes.bench_objects(16))
    yield sc
    sc.close()


VIEWS = {"orbit": lambda: rt.make_view(None, 0.0),
         "inside": lambda: rt.make_view(camera((5.0, -6.0, 2.0), (10.0, 40.0, 0.0)), 0.0)}


@pytest.mark.parametrize("which", sorted(VIEWS))
def test_round_trip_equals_the_render_paths(gpu_ctx, room16, which, culling):
    """trace_rays(view_rays(view)) is rt_render_view at depths 0, 1, 3 and
    rt_render_hits_view with and without shadow bits, byte for byte."""
    view = VIEWS[which]()
    rays = rt.view_rays(gpu_ctx, view, W, H)
    assert rays.shape == (H, W) and (rays["origin"] == np.array(view.origin[:], np.float32)).all()
    assert (rays["reserved0"] == 0).all() and (rays["reserved1"] == 0).all()
    for depth in (0, 1, 3):
        (col,) = rt.trace_rays(gpu_ctx, room16, rays, depth)
        want = rt.render(gpu_ctx, room16, W, H, depth, view=view)
        assert col.reshape(H, W, 4).tobytes() == want.tobytes(), depth
    for shadow in (True, False):
        got = rt.trace_rays(gpu_ctx, room16, rays, 0, colors=False, hits=True, normals=True, points=True,
                            shadow=shadow)
        want = rt.render_hits(gpu_ctx, room16, W, H, view=view, shadow=shadow)
        for g, x in zip(got, want):
            assert g.tobytes() == np.ascontiguousarray(x).tobytes(), shadow
    assert (want[0]["object"] >= 0).any()


def test_view_rays_rows_and_device(gpu_ctx):
    view = rt.make_view(None, 0.0)
    full = rt.view_rays(gpu_ctx, view, W, H)
    band = rt.view_rays(gpu_ctx, view, W, H, rows=(5, 14))
    assert band.tobytes() == np.ascontiguousarray(full[5:14]).tobytes()
    dev = rt.view_rays(gpu_ctx, view, W, H, device=True)
    assert dev.shape == (H, W, 8) and dev.cpu().numpy().tobytes() == full.tobytes()


def test_view_rays_equal_the_reference_gl_directions(gpu_ctx):
    """The orbit view at 128 x 128 with llvmpipe's unprojection: the directions
    are the reference shader's own (tests/golden/probe_dir_t0_128)."""
    m = manifest()["probe_dir_t0_128"]
    assert (m["scene"], m["time"], m["width"], m["height"], m["probe"]) == ("shipped", 0.0, 128, 128, 1)
    gl, unproj = load_fixture("probe_dir_t0_128")
    view = rt.view_from_matrix(unproj, list(rt.reference_camera(0.0).position))
    rays = rt.view_rays(gpu_ctx, view, 128, 128)
    assert np.array_equal(rays["dir"], gl)


# ---- 3. shapes and plumbing -------------------------------------------------------
@pytest.fixture(scope="module")
def full_run(gpu_ctx, rset, room16):
    """Set R's permuted rays and their four planes at depth 2 (host buffers)."""
    rays = rset.permuted()
    return rays, trace_all(gpu_ctx, room16, rays, 2)


def _device_call(ctx, sc, rays_t, n, depth, bufs, flags=1, stream=None):
    ptrs = [C.c_void_p(b.data_ptr()) if b is not None else None for b in bufs]
    return rt.lib().rt_trace_rays(ctx.handle, sc.handle, C.c_void_p(rays_t.data_ptr()), n, depth, flags, *ptrs, 1,
                                  C.c_void_p(stream) if stream else None)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257])
def test_prefixes_and_canaries(gpu_ctx, room16, full_run, k):
    """The first k rays into device buffers of k + 8 records filled with a
    canary: the first k records are the full run's, the last 8 untouched."""
    rays, full = full_run
    rays_t = torch.from_numpy(rays[:k].view(np.float32).reshape(k, 8)).cuda()
    bufs = [torch.full((k + 8, 16), CANARY, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    assert _device_call(gpu_ctx, room16, rays_t, k, 2, bufs) == abi.RT_OK
    for b, want in zip(bufs, full):
        a = b.cpu().numpy()
        assert a[:k].tobytes() == np.ascontiguousarray(want[:k]).tobytes()
        assert (a[k:] == CANARY).all()


def test_zero_rays(gpu_ctx, room16):
    buf = np.full((4, 4), 7.0, np.float32)
    rays = np.zeros(1, abi.RAY_DTYPE)
    assert rt.lib().rt_trace_rays(gpu_ctx.handle, room16.handle, rays.ctypes.data, 0, 0, 1, buf.ctypes.data, None,
                                  None, None, 0, None) == abi.RT_OK
    assert rt.lib().rt_trace_rays(gpu_ctx.handle, room16.handle, None, 0, 0, 1, buf.ctypes.data, None, None, None,
                                  0, None) == abi.RT_OK
    assert (buf == 7.0).all()
    (col,) = rt.trace_rays(gpu_ctx, room16, np.zeros(0, abi.RAY_DTYPE))
    assert col.shape == (0, 4)


def test_device_buffers_and_a_caller_stream(gpu_ctx, room16, full_run):
    """torch tensors in and out equal the host-buffer run, synchronously and on a caller's stream."""
    rays, full = full_run
    rays_t = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).cuda()
    torch.cuda.synchronize()
    sync = rt.trace_rays(gpu_ctx, room16, rays_t, 2, hits=True, normals=True, points=True)
    stream = torch.cuda.Stream()
    asyn = rt.trace_rays(gpu_ctx, room16, rays_t, 2, hits=True, normals=True, points=True,
                         stream=stream.cuda_stream)
    stream.synchronize()
    for got in (sync, asyn):
        assert all(t.is_cuda for t in got)
        for g, want in zip(got, full):
            assert g.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    # float32 rows of 8 on the host are the same rays
    (col,) = rt.trace_rays(gpu_ctx, room16, rays.view(np.float32).reshape(-1, 8), 2)
    assert col.tobytes() == full[0].tobytes()


def test_every_plane_combination(gpu_ctx, room16, full_run):
    rays, full = full_run
    names = rt.RAY_PLANES
    for r in (1, 2, 4):
        for combo in itertools.combinations(range(4), r):
            got = rt.trace_rays(gpu_ctx, room16, rays, 2, **{names[k]: k in combo for k in range(4)})
            assert len(got) == r
            for g, k in zip(got, combo):
                assert g.tobytes() == full[k].tobytes(), (combo, k)


def test_reserved_words_are_ignored(gpu_ctx, room16, full_run):
    rays, full = full_run
    dirty = rays.copy()
    dirty["reserved0"] = np.nan
    dirty["reserved1"] = -1e30
    for g, want in zip(trace_all(gpu_ctx, room16, dirty, 2), full):
        assert g.tobytes() == want.tobytes()


def test_non_unit_and_non_finite_rays_stay_in_their_slots(gpu_ctx, room16, full_run):
    """A direction of another length is traced as given (its wave without
    culling): twice the direction halves t and keeps the hit; a ray with a
    non-finite component changes no other ray's record."""
    rays, full = full_run
    n = 256
    odd = rays[:n].copy()
    i = int(np.flatnonzero(full[1]["object"][:64] >= 0)[0])  # a ray of the first wave with a hit
    odd["dir"][i] *= np.float32(2.0)
    odd["origin"][70] = (np.nan, 0.0, 0.0)
    odd["dir"][130] = (np.inf, 0.0, 0.0)
    odd["origin"][200] = (np.inf, -np.inf, 0.0)
    got = trace_all(gpu_ctx, room16, odd, 2)
    keep = np.ones(n, bool)
    keep[[i, 70, 130, 200]] = False
    for g, want in zip(got, full):
        assert g[keep].tobytes() == np.ascontiguousarray(want[:n][keep]).tobytes()
    h, w = got[1][i], full[1][i]
    assert h["object"] == w["object"] and h["object"] >= 0 and h["t"] == np.float32(0.5) * w["t"]


def test_the_last_render_stays_the_last_kernel(gpu_ctx, room16, full_run):
    rays, full = full_run
    view = rt.make_view(None, 0.0)
    colour = rt.render(gpu_ctx, room16, W, H, 0, view=view)
    kernel = rt.last_kernel(gpu_ctx)
    got = trace_all(gpu_ctx, room16, rays, 2)
    assert all(g.tobytes() == x.tobytes() for g, x in zip(got, full))
    assert rt.last_kernel(gpu_ctx) == kernel
    assert gpu_ctx.last_kernel_ms() > 0.0  # (RT_OPT_TIMING: the call's launches are timed)
    assert rt.render(gpu_ctx, room16, W, H, 0, view=view).tobytes() == colour.tobytes()


def test_bad_arguments(gpu_ctx, room16):
    L = rt.lib()
    rays = np.zeros(8, abi.RAY_DTYPE)
    rays["dir"] = (0.0, 1.0, 0.0)
    buf = np.zeros((8, 4), np.float32)
    r, p = rays.ctypes.data, buf.ctypes.data
    ctx, sc = gpu_ctx.handle, room16.handle
    invalid = [
        lambda: L.rt_trace_rays(ctx, None, r, 8, 0, 1, p, None, None, None, 0, None),  # no scene
        lambda: L.rt_trace_rays(ctx, sc, None, 8, 0, 1, p, None, None, None, 0, None),  # no rays
        lambda: L.rt_trace_rays(ctx, sc, r, 8, 0, 1, None, None, None, None, 0, None),  # no plane
        lambda: L.rt_trace_rays(ctx, sc, r, -1, 0, 1, p, None, None, None, 0, None),
        lambda: L.rt_trace_rays(ctx, sc, r, abi.RT_MAX_RAYS + 1, 0, 1, p, None, None, None, 0, None),
        lambda: L.rt_trace_rays(ctx, sc, r, 8, 0, 2, p, None, None, None, 0, None),  # flag bits
        lambda: L.rt_view_rays(ctx, None, 4, 2, 0, 2, r, 0, None),  # no view
        lambda: L.rt_view_rays(ctx, C.byref(rt.make_view(None, 0.0)), 4, 2, 0, 3, r, 0, None),  # rows
        lambda: L.rt_view_rays(ctx, C.byref(rt.make_view(None, 0.0)), 0, 2, 0, 2, r, 0, None),  # size
        lambda: L.rt_view_rays(ctx, C.byref(rt.make_view(None, 0.0)), 4, 2, 0, 2, None, 0, None),  # no buffer
    ]
    for k, call in enumerate(invalid):
        assert call() == abi.RT_ERR_INVALID, k
    s = torch.cuda.Stream()  # an asynchronous call needs device buffers
    assert L.rt_trace_rays(ctx, sc, r, 8, 0, 1, p, None, None, None, 0, C.c_void_p(s.cuda_stream)) == abi.RT_ERR_INVALID
    for depth in (-1, abi.RT_MAX_DEPTH + 1):
        assert L.rt_trace_rays(ctx, sc, r, 8, depth, 1, p, None, None, None, 0, None) == abi.RT_ERR_UNSUPPORTED
        # max_depth applies to colors only
        assert L.rt_trace_rays(ctx, sc, r, 8, depth, 1, None, p, None, None, 0, None) == abi.RT_OK
