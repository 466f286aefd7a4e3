"""RT_OPT_LAUNCH_SHAPES: the depth-0 shaped kernels compiled for the plain
launch shape (rt_internal.h kLaunchPlain: a whole-frame, unsharded float4
render with the host's frame constants, short camera divisions, at least
2 x 2 pixels, no accumulation) fold the launch's uniform tests into
constants and change no arithmetic on pixel values, so every frame is the
same bytes with the option on and off; a render that is not plain keeps the
run-time tests and still equals its option-off render (and the oracle).

Frames of 72 x 40 and 33 x 17: ragged edges of the 16 x 16 work-group tile
and the 8 x 8 wave tile, more than one work-group.
"""
import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from camera_common import oracle_view
from conftest import parity_stats
from openglraytracer_amd import abi
from oracle import port, scenes

pytestmark = pytest.mark.gpu
SIZES = [(72, 40), (33, 17)]


def _objects(kind, n_spheres):
    """room: one translate-only box holding the lights (kShapeRoom);
    boxes: several boxes (12 spheres: the shipped scene itself)."""
    if kind == "boxes" and n_spheres == 12:
        return rt.reference_objects(0.0)
    objs = scenes.bench_objects(n_spheres, seed=n_spheres)
    if kind == "boxes":
        for k in (1, 2):
            objs.append(scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (2.0 * k - 3.0, -4.0, 1.5 * k),
                                   (0.0, 30.0 * k, 0.0), k % 7))
    return objs


def _views(n):
    return [rt.make_view(None, 0.25 * k + 0.1) for k in range(n)]


def _on_off(ctx, fn):
    """fn() with the launch shapes on, then off."""
    out = {}
    try:
        for on in (True, False):
            ctx.set_launch_shapes(on)
            out[on] = fn()
    finally:
        ctx.set_launch_shapes(True)
    return out[True], out[False]


def _batch(ctx, sc, w, h, views, rows=None, shard=(8, 1, 0)):
    rows = h if rows is None else rows
    shape = {abi.RT_OUTPUT_RGBA8: ((4,), torch.uint8), abi.RT_OUTPUT_RGB32F: ((3,), torch.float32)}.get(
        ctx.output, ((4,), torch.float32))
    out = torch.zeros((len(views), rows, w) + shape[0], dtype=shape[1], device="cuda")
    torch.cuda.synchronize()
    rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views, *shard)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n_views", [1, 3, 9])
@pytest.mark.parametrize("kind,n_spheres", [("room", 12), ("room", 24), ("room", 48),
                                            ("boxes", 12), ("boxes", 24), ("boxes", 48)])
def test_plain_launches_change_nothing(gpu_ctx, kind, n_spheres, n_views, w, h):
    """2-, 4- and 8-byte masks, a room and several boxes, 1 view (rt_render),
    3 views in the kernel arguments and 9 in the device buffer (the kDev
    instances): the same bytes on and off, and the oracle's frame."""
    objs = _objects(kind, n_spheres)
    views = _views(n_views)
    sc = rt.Scene(gpu_ctx, objs)
    try:
        if n_views == 1:
            on, off = _on_off(gpu_ctx, lambda: rt.render(gpu_ctx, sc, w, h, 0, view=views[0])[None])
        else:
            on, off = _on_off(gpu_ctx, lambda: _batch(gpu_ctx, sc, w, h, views))
    finally:
        sc.close()
    assert on.tobytes() == off.tobytes(), parity_stats(on, off)
    assert (on[..., 3] == 0).all()
    o = port.render(objs, w, h, 0, 0.1)
    assert np.array_equal(on[0], o), parity_stats(on[0], o)


def _tiny_w_view():
    """The reference view with its unprojection scaled by 2^-40: the same
    rays, but every w below the short divisions' range, so the host refuses
    the short form (rt_scene.cpp camera_short_divisions)."""
    v = rt.make_view(None, 0.1)
    m = np.array(v.unprojection[:], np.float32) * np.float32(2.0 ** -40)
    return rt.view_from_matrix(m.reshape(4, 4), list(v.origin))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("case", ["rgba8", "rgb32f", "sharded", "rows", "one_wide", "no_frame_consts",
                                  "long_divisions"])
def test_other_launches_keep_their_run_time_tests(gpu_ctx, case, w, h):
    """Launches that are not plain: the option changes nothing, and the
    frames are the oracle's."""
    objs = _objects("room", 12)
    view = rt.make_view(None, 0.1)
    rows = (0, h)
    sc = rt.Scene(gpu_ctx, objs)
    try:
        if case in ("rgba8", "rgb32f"):
            gpu_ctx.set_output(abi.RT_OUTPUT_RGBA8 if case == "rgba8" else abi.RT_OUTPUT_RGB32F)
            on, off = _on_off(gpu_ctx, lambda: rt.render(gpu_ctx, sc, w, h, 0, view=view))
        elif case == "sharded":  # blocks of 8 rows dealt to 3 shards; shard 1's rows of 3 views
            ids = rt.shard_row_ids(h, 8, 3, 1)
            on, off = _on_off(gpu_ctx, lambda: _batch(gpu_ctx, sc, w, h, _views(3), rows=len(ids), shard=(8, 3, 1)))
        elif case == "rows":
            rows = (5, h - 3)
            on, off = _on_off(gpu_ctx, lambda: rt.render(gpu_ctx, sc, w, h, 0, view=view, rows=rows))
        elif case == "one_wide":
            w = 1
            on, off = _on_off(gpu_ctx, lambda: rt.render(gpu_ctx, sc, w, h, 0, view=view))
        elif case == "no_frame_consts":
            gpu_ctx.set_host_frame_consts(False)
            on, off = _on_off(gpu_ctx, lambda: rt.render(gpu_ctx, sc, w, h, 0, view=view))
        else:
            view = _tiny_w_view()
            on, off = _on_off(gpu_ctx, lambda: rt.render(gpu_ctx, sc, w, h, 0, view=view))
    finally:
        gpu_ctx.set_output(abi.RT_OUTPUT_RGBA32F)
        gpu_ctx.set_host_frame_consts(True)
        sc.close()
    assert on.tobytes() == off.tobytes()
    if case == "long_divisions":
        # the oracle's frame of the scaled unprojection itself (and so, the
        # quotients being the same, of the unscaled one)
        o = oracle_view(objs, view, w, h, 0)
        assert np.array_equal(on, o), parity_stats(on, o)
        assert np.array_equal(o, port.render(objs, w, h, 0, 0.1)) and (on[..., :3] > 0).any()
        return
    o = port.render(objs, w, h, 0, 0.1, rows=rows)
    if case == "sharded":
        o = port.render(objs, w, h, 0, 0.1)[ids]
        on = on[0]
    elif case == "rgba8":
        o = rt.pack_rgba8(o)
    elif case == "rgb32f":
        o = o[..., :3]
    assert np.array_equal(on, o, equal_nan=case == "one_wide")
