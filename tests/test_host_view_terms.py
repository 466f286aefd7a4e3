"""The plain launches' per-view camera terms come from the host
(rt_internal.h FrameView::rcp_hw, rcp_hh, unproj_half; filled by fill_view):
the refined reciprocals of float(W / 2) and float(H / 2) and the four
products unproj[8 + k] * 0.5f, which camera_ray<kLaunchPlain> otherwise
computes per wave tile. They are the same floats (the refined reciprocal is
the correctly rounded 1 / b, the product is one IEEE multiplication), so a
plain launch is the same bytes as the same render with RT_OPT_LAUNCH_SHAPES 0,
whose kernels keep the device arithmetic.

The half-sizes W / 2 and H / 2 cover 1, 2, 3, odd values, powers of two and
their neighbours on both sides, and 540, 960, 2049; the other dimension stays
at 2 to 8 pixels, so every frame is tiny. Each size runs one view (views in
the kernel arguments), 9 views tiled and 9 views on a forced persistent grid
(views in device memory), on config 2's scene and the shipped one.
"""
import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from oracle import port, scenes

pytestmark = pytest.mark.gpu

HALVES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128, 129, 511, 512, 513, 540, 960,
          1023, 1024, 1025, 2047, 2048, 2049]
OTHER = [2, 3, 4, 5, 6, 7, 8]


def _sizes():
    """(W, H): each half-size as W / 2 of an even and an odd width and as
    H / 2 of an even and an odd height, the other dimension cycling 2..8."""
    out = []
    for i, v in enumerate(HALVES):
        o = OTHER[i % len(OTHER)]
        out += [(2 * v, o), (2 * v + 1, OTHER[(i + 3) % len(OTHER)]), (o, 2 * v), (OTHER[(i + 5) % len(OTHER)], 2 * v + 1)]
    return sorted(set(out + [(4099, 2), (3, 4098), (1080, 4), (2, 2), (1920, 2), (4, 1080)]))


SIZES = _sizes()


def _scene_objects(kind):
    return scenes.CONFIGS["config2"][0]() if kind == "config2" else rt.reference_objects(0.0)


@pytest.fixture(scope="module", params=["config2", "shipped"])
def scene(request, gpu_ctx):
    objs = _scene_objects(request.param)
    sc = rt.Scene(gpu_ctx, objs)
    yield objs, sc
    sc.close()
    gpu_ctx.set_launch_shapes(True)
    gpu_ctx.set_persistent0(1)


def _views(n):
    return [rt.make_view(None, 0.25 * k + 0.1) for k in range(n)]


def _batch(ctx, sc, w, h, views):
    out = torch.zeros((len(views), h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _renders(ctx, sc, w, h):
    views = _views(9)
    out = {"one": rt.render(ctx, sc, w, h, 0, view=views[0])[None]}
    for name, mode in (("tiled", 0), ("persistent", 8)):
        ctx.set_persistent0(mode)
        out[name] = _batch(ctx, sc, w, h, views)
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_host_terms_are_the_device_terms(gpu_ctx, scene, w, h):
    _, sc = scene
    try:
        gpu_ctx.set_launch_shapes(True)
        host = _renders(gpu_ctx, sc, w, h)  # plain launches: the host's terms
        gpu_ctx.set_launch_shapes(False)
        dev = _renders(gpu_ctx, sc, w, h)   # the device arithmetic
    finally:
        gpu_ctx.set_launch_shapes(True)
        gpu_ctx.set_persistent0(1)
    for name in host:
        assert host[name].tobytes() == dev[name].tobytes(), (name, parity_stats(host[name], dev[name]))
    assert host["tiled"].tobytes() == host["persistent"].tobytes()
    assert host["one"][0].tobytes() == host["tiled"][0].tobytes()


@pytest.mark.parametrize("w,h", [(2, 2), (7, 4), (4099, 2), (3, 4098), (1080, 4), (4, 1920)])
def test_plain_frames_are_the_oracle_frames(gpu_ctx, scene, w, h):
    objs, sc = scene
    gpu_ctx.set_launch_shapes(True)
    gpu = rt.render(gpu_ctx, sc, w, h, 0, view=rt.make_view(None, 0.1))
    o = port.render(objs, w, h, 0, 0.1)
    assert np.array_equal(gpu, o), parity_stats(gpu, o)
