"""Tile runs on the GPU (rt_kernel.hip render_persistent0 with kTileRuns: a
chunk walked run by run, the view's address, the slot, the frame's size and
the view's frame in the output derived once per run): a forced persistent
launch (RT_OPT_PERSISTENT0 8 and 9: 32 and 36 waves) gives the bytes of the
tiled launch, and frame 0 is the oracle's.

Frames (tests/test_tile_runs_host.py shows what their chunks hold):
  8 x 8 x 40 views     one tile per view: every run has length 1 and every
                       tile refills the slot
  9 x 8, 17 x 9 x 17   two and three tiles per row, ragged right and bottom edges
  136 x 16 x 40        17 tiles per row: chunks of 16 end a tile short of a row
                       end and the next begins on a row's last tile; chunks of
                       every size span row ends and view ends
  72 x 40 x 9          nine tiles per row
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from oracle import port, scenes

pytestmark = pytest.mark.gpu
FRAMES = [(8, 8, 40), (9, 8, 17), (17, 9, 17), (136, 16, 40), (72, 40, 9)]
FORCED = (8, 9)
# room + 16 / 20 / 40 spheres: 2-, 4- and 8-byte masks; the shipped scene's boxes: the instances without a room
SCENES = ["room16", "room20", "room40", "boxes"]


def _objects(kind):
    if kind == "boxes":
        return rt.reference_objects(0.0)
    n = int(kind[4:])
    return scenes.bench_objects(n, seed=n)


def _views(n):
    return [rt.make_view(None, 0.25 * k + 0.1) for k in range(n)]


@functools.lru_cache(maxsize=None)
def _oracle(kind, w, h):
    """Frame 0 (the view at t = 0.1) from the oracle: once per scene and size."""
    frame = port.render(_objects(kind), w, h, 0, 0.1)
    frame.setflags(write=False)
    return frame


def _batch(ctx, sc, w, h, views, out=None, stream=None):
    if out is None:
        out = torch.zeros((len(views), h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
    rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views, stream=stream)
    return out


def _queued(ctx):
    """The context's last launch ran on its queue counters (host-only hook)."""
    f = rt.lib().rt_debug_last_queued
    f.argtypes = [C.c_void_p]
    f.restype = C.c_int
    return f(ctx.handle)


def _frames(ctx, sc, w, h, views, mode):
    ctx.set_persistent0(mode)
    out = _batch(ctx, sc, w, h, views)
    torch.cuda.synchronize()
    assert _queued(ctx) == (1 if mode >= 8 else 0)
    return out.cpu().numpy()


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_persistent0(1)


@pytest.mark.parametrize("w,h,n_views", FRAMES)
@pytest.mark.parametrize("kind", SCENES)
def test_forced_persistent_launch_is_the_tiled_launch(ctx, kind, w, h, n_views):
    views = _views(n_views)
    sc = rt.Scene(ctx, _objects(kind))
    try:
        tiled = _frames(ctx, sc, w, h, views, 0)
        forced = {k: _frames(ctx, sc, w, h, views, k) for k in FORCED}
    finally:
        sc.close()
    for k in FORCED:
        assert forced[k].tobytes() == tiled.tobytes(), (k, parity_stats(forced[k], tiled))
    o = _oracle(kind, w, h)
    assert np.array_equal(forced[8][0], o), parity_stats(forced[8][0], o)


@pytest.mark.parametrize("k", FORCED)
def test_the_same_forced_launch_four_times_on_one_context(ctx, k):
    """The queue counters and the run state start afresh with every launch."""
    w, h, n_views = 136, 16, 40
    views = _views(n_views)
    sc = rt.Scene(ctx, _objects("room16"))
    try:
        tiled = _frames(ctx, sc, w, h, views, 0)
        again = [_frames(ctx, sc, w, h, views, k) for _ in range(4)]
    finally:
        sc.close()
    for a in again:
        assert a.tobytes() == tiled.tobytes(), parity_stats(a, tiled)


def test_two_forced_launches_in_flight_on_two_streams(ctx):
    """Each launch has its counters and each wave its own run state."""
    (w0, h0, n0), (w1, h1, n1) = (136, 16, 40), (17, 9, 17)
    v0, v1 = _views(n0), _views(n1)[::-1]
    sc = rt.Scene(ctx, _objects("room20"))
    try:
        t0, t1 = _frames(ctx, sc, w0, h0, v0, 0), _frames(ctx, sc, w1, h1, v1, 0)
        ctx.set_persistent0(9)
        s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
        o0 = torch.zeros((n0, h0, w0, 4), dtype=torch.float32, device="cuda")
        o1 = torch.zeros((n1, h1, w1, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(4):  # (back to back: the second stream's launch starts while the first's runs)
            _batch(ctx, sc, w0, h0, v0, out=o0, stream=s0.cuda_stream)
            _batch(ctx, sc, w1, h1, v1, out=o1, stream=s1.cuda_stream)
        torch.cuda.synchronize()
        assert _queued(ctx) == 1
        f0, f1 = o0.cpu().numpy(), o1.cpu().numpy()
    finally:
        sc.close()
    assert f0.tobytes() == t0.tobytes()
    assert f1.tobytes() == t1.tobytes()
