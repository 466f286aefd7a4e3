"""RT_OPT_FIXED_LAYOUT: a scene staged in its layout class's fixed layout
(rt_internal.h fixed_layout) renders the same bytes whether the persistent
kernel takes the tables' offsets from the class (option 1, kShapeFixed) or
reads them per tile (option 0), tiled or on a forced persistent grid of 8 or 9
work-groups, and view 0 is the oracle's frame. Scenes outside a class (one
light, one material, one box too many; 44 spheres that the padding would cost
their 12-texel masks) keep the compact layout and run the same comparison.

Frames of 72 x 40 and 33 x 17 (tests/test_persistent0.py's sizes: ragged
edges, view changes inside a wave's run), 9 and 17 views.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from oracle import port, scenes
from test_fixed_layout_host import in_class_scenes, out_of_class_scenes

pytestmark = pytest.mark.gpu
SIZES = [(72, 40), (33, 17)]
FORCED = (8, 9)
TIME0 = 0.1


def _scenes():
    """name -> (objects, materials, lights, in its class)."""
    out = {k: v[:3] + (True,) for k, v in in_class_scenes().items()}
    out["room16"] = (scenes.bench_objects(16, seed=16),) + out["config2"][1:]
    out.update({k: v[:3] + (False,) for k, v in out_of_class_scenes().items()})
    return out


def _views(n):
    return [rt.make_view(None, 0.25 * k + TIME0) for k in range(n)]


def _last_fixed(ctx):
    f = rt.lib().rt_debug_last_fixed_layout
    f.argtypes, f.restype = [C.c_void_p], C.c_int
    return f(ctx.handle)


def _frames(ctx, sc, w, h, views, fixed, mode):
    ctx.set_fixed_layout(fixed)
    ctx.set_persistent0(mode)
    out = torch.zeros((len(views), h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views)
    torch.cuda.synchronize()
    return out.cpu().numpy(), _last_fixed(ctx)


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_persistent0(1)
    gpu_ctx.set_fixed_layout(True)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n_views", [9, 17])
@pytest.mark.parametrize("name", sorted(_scenes()))
def test_option_changes_no_byte(ctx, name, n_views, w, h):
    objs, mats, lights, in_class = _scenes()[name]
    views = _views(n_views)
    sc = rt.Scene(ctx, objs, mats, lights)
    try:
        want, _ = _frames(ctx, sc, w, h, views, False, 0)
        for mode in (0,) + FORCED:
            for fixed in (True, False):
                got, bit = _frames(ctx, sc, w, h, views, fixed, mode)
                assert bit == (1 if fixed and in_class else 0), (mode, fixed)
                assert got.tobytes() == want.tobytes(), (mode, fixed, parity_stats(got, want))
    finally:
        sc.close()
    o = port.render(objs, w, h, 0, TIME0, materials=mats, lights=lights)
    assert np.array_equal(want[0], o), parity_stats(want[0], o)


@pytest.mark.parametrize("w,h", SIZES)
def test_animated_scene(ctx, w, h):
    """The shipped animation through rt_anim (its frames share the class's
    layout; each view carries a blob of its own, so the launch is tiled):
    9 frames, option on against off, frame 0 against the oracle."""
    base, anim = rt.reference_animation()
    times = [0.25 * k + TIME0 for k in range(9)]
    an = rt.Anim(ctx, base, anim, max_frames=len(times))
    try:
        got = {}
        for fixed in (True, False):
            ctx.set_fixed_layout(fixed)
            out = torch.zeros((len(times), h, w, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rt.render_batch_animated(ctx, an, out.data_ptr(), w, h, 0, times)
            torch.cuda.synchronize()
            got[fixed] = out.cpu().numpy()
    finally:
        an.close()
    assert got[True].tobytes() == got[False].tobytes()
    o = port.render(rt.animate_objects(base, anim, times[0]), w, h, 0, times[0])
    assert np.array_equal(got[True][0], o), parity_stats(got[True][0], o)
