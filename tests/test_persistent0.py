"""RT_OPT_PERSISTENT0: the persistent distribution of a plain depth-0 batch
(rt_kernel.hip render_persistent0: a resident grid whose waves take chunks
of wave tiles from 32 queues, the view's records in a slot per wave) runs the
same per-pixel code as the tiled launch, so every frame is the same bytes
with the option 0 (tiled) and forced (k >= 8: at most k work-groups whatever
the launch's size). Forced to 8 work-groups every queue has one wave, to 9
queues 0-3 have two.

Frames of 72 x 40 (45 wave tiles) and 33 x 17 (15): ragged edges, item counts
that are no multiple of the chunk, and at 9, 17 and 40 views about a dozen
items per wave with view changes inside every wave's run.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from oracle import port, scenes

pytestmark = pytest.mark.gpu
SIZES = [(72, 40), (33, 17)]
FORCED = (8, 9)
# room + 16 / 20 / 40 spheres: 2-, 4- and 8-byte masks; the shipped scene: four boxes, no room
SCENES = ["room16", "room20", "room40", "boxes"]


def _objects(kind):
    if kind == "boxes":
        return rt.reference_objects(0.0)
    n = int(kind[4:])
    return scenes.bench_objects(n, seed=n)


def _views(n):
    return [rt.make_view(None, 0.25 * k + 0.1) for k in range(n)]


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
    assert _queued(ctx) == (1 if mode >= 8 else 0)  # (these frames are below the automatic threshold)
    return out.cpu().numpy()


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_persistent0(1)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n_views", [9, 17, 40])
@pytest.mark.parametrize("kind", SCENES)
def test_forced_persistent_launch_is_the_tiled_launch(ctx, kind, n_views, w, h):
    objs = _objects(kind)
    views = _views(n_views)
    sc = rt.Scene(ctx, objs)
    try:
        tiled = _frames(ctx, sc, w, h, views, 0)
        forced = {k: _frames(ctx, sc, w, h, views, k) for k in FORCED}
    finally:
        sc.close()
    for k in FORCED:
        assert forced[k].tobytes() == tiled.tobytes(), (k, parity_stats(forced[k], tiled))
    o = port.render(objs, w, h, 0, 0.1)  # (and the tiled frames are the oracle's)
    assert np.array_equal(tiled[0], o), parity_stats(tiled[0], o)


@pytest.mark.parametrize("w,h", [(33, 17), (16, 8)])
@pytest.mark.parametrize("k", FORCED)
def test_fewer_chunks_than_waves_and_counters_reset(ctx, k, w, h):
    """9 views of 33 x 17: 135 wave tiles, 17 chunks' worth against 32 (36)
    waves (all of them in the launch's tail, dealt tile by tile); 9 views of
    16 x 8: 18 tiles, so most waves leave at once. The same launch again on
    the same context finds the counters reset."""
    views = _views(9)
    sc = rt.Scene(ctx, _objects("room16"))
    try:
        tiled = _frames(ctx, sc, w, h, views, 0)
        first = _frames(ctx, sc, w, h, views, k)
        again = [_frames(ctx, sc, w, h, views, k) for _ in range(3)]
    finally:
        sc.close()
    assert first.tobytes() == tiled.tobytes()
    for a in again:
        assert a.tobytes() == tiled.tobytes()


def test_whole_resident_grid_and_automatic_mode_below_its_threshold(ctx):
    """9 views of 640 x 368 (33,120 wave tiles): forced with a cap above the
    resident work-groups the launch takes the whole resident grid (8,192
    waves on an MI355X: whole chunks and the tile-by-tile tail); the default
    keeps such a launch tiled (192 tiles per resident wave: host test)."""
    w, h = 640, 368
    views = _views(9)
    sc = rt.Scene(ctx, _objects("room16"))
    try:
        out = {}
        for mode, queued in ((0, 0), (1, 0), (1 << 16, 1)):
            ctx.set_persistent0(mode)
            out[mode] = _batch(ctx, sc, w, h, views)
            torch.cuda.synchronize()
            assert _queued(ctx) == queued
        for mode in (1, 1 << 16):
            assert torch.equal(out[mode].view(torch.int32), out[0].view(torch.int32))
    finally:
        sc.close()


def test_two_forced_launches_in_flight_on_two_streams(ctx):
    """Each launch takes a counter slot of its own from the context."""
    (w0, h0, n0), (w1, h1, n1) = (72, 40, 40), (33, 17, 17)
    v0, v1 = _views(n0), _views(n1)[::-1]
    sc = rt.Scene(ctx, _objects("room16"))
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
