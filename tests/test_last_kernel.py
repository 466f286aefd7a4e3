"""rt_debug_last_kernel: the row of the kernel table the context's last
launch ran — (depth, accum, dev, shape with kShapeFixed, launch with
kLaunchPersistent, queued). The parity tests compare bytes with an option on
and off, and the shaped kernels are bit-identical to the general one by
design, so only this says that a launch took the kernel its scene and shape
name (rt_kernel.hip select_kernel) and not the general one.

33 x 17 frames of a room of 12 spheres (2-byte LDS masks, the one-box class's
fixed layout): shape 2 | kShapeRoom = 18, with kShapeFixed 82; the recursive
case on the room of 64 spheres that test_wide_scene_shapes_change_nothing
renders in the wide shape, kShapeWide | kShapeRoom = 48."""
import ctypes as C

import pytest
import torch

import openglraytracer_amd as rt
from oracle import scenes

pytestmark = pytest.mark.gpu
W, H = 33, 17


def _last_queued(ctx):
    f = rt.lib().rt_debug_last_queued
    f.argtypes, f.restype = [C.c_void_p], C.c_int
    return f(ctx.handle)


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_scene_shapes(True)
    gpu_ctx.set_launch_shapes(True)
    gpu_ctx.set_persistent0(1)
    gpu_ctx.set_fixed_layout(True)


@pytest.fixture(scope="module")
def room12(gpu_ctx):
    sc = rt.Scene(gpu_ctx, scenes.bench_objects(12, seed=12))
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def room64(gpu_ctx):
    sc = rt.Scene(gpu_ctx, scenes.bench_objects(64, seed=0))
    yield sc
    sc.close()


def _set(ctx, options):
    for name, value in options.items():
        getattr(ctx, "set_" + name)(value)


@pytest.mark.parametrize("options,want", [
    ({}, (0, 0, 0, 18, 1, 0)),
    (dict(launch_shapes=False), (0, 0, 0, 18, 0, 0)),
    (dict(scene_shapes=False), (0, 0, 0, 0, 0, 0)),
])
def test_a_frame(ctx, room12, options, want):
    _set(ctx, options)
    rt.render(ctx, room12, W, H, 0)
    assert rt.last_kernel(ctx) == want


@pytest.mark.parametrize("depth,options,want", [
    (0, {}, (0, 0, 1, 18, 1, 0)),
    (0, dict(persistent0=8), (0, 0, 1, 82, 3, 1)),
    (0, dict(persistent0=8, fixed_layout=False), (0, 0, 1, 18, 3, 1)),
    (1, {}, (1, 0, 1, 0, 0, 0)),
])
def test_a_batch_of_9_views(ctx, room12, depth, options, want):
    _set(ctx, options)
    views = [rt.make_view(None, 0.25 * k) for k in range(9)]
    out = torch.zeros((len(views), H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.render_batch(ctx, room12, out.data_ptr(), W, H, depth, views)
    torch.cuda.synchronize()
    assert rt.last_kernel(ctx) == want


@pytest.mark.parametrize("depth,want", [(0, (0, 1, 0, 18, 0)), (2, (2, 1, 0, 0, 0))])
def test_accumulation(ctx, room12, depth, want):
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.render_accumulate(ctx, room12, acc.data_ptr(), W, H, depth, 2)
    torch.cuda.synchronize()
    got = rt.last_kernel(ctx)
    assert got[:5] == want and got[5] == _last_queued(ctx)
    assert got[5] == 0 or depth >= 2


@pytest.mark.parametrize("shapes,want", [(True, (2, 0, 0, 48, 0)), (False, (2, 0, 0, 0, 0))])
def test_depth_2_takes_the_wide_shape(ctx, room64, shapes, want):
    ctx.set_scene_shapes(shapes)
    rt.render(ctx, room64, W, H, 2)
    got = rt.last_kernel(ctx)
    assert got[:5] == want and got[5] == _last_queued(ctx)
