"""The persistent depth-0 launch with chunk sizes that fall towards its end
(rt_internal.h persistent_chunk: the bulk in chunks of kChunk0, then regions
of halving sizes down to single tiles, each about a chunk per resident wave)
renders the bytes of the tiled launch: option 0 against forced 8 and 9
work-groups (32 / 36 waves, queues with one wave and with two).

Frames of 72 x 40 (45 wave tiles per view), 33 x 17 (15) and 16 x 8 (2) at
9, 17 and 40 views: at 32 waves 40 x 45 = 1,800 items pass through every
region of the schedule (bulk 16s, 8s, 4s, 2s, singles), 17 x 15 = 255 fall
short of the bulk, and 9 x 15 = 135 and 9 x 2 = 18 are smaller than the tail
regions together; 45 and 15 tiles per view put view changes inside chunks and
at chunk starts.
"""
import ctypes as C

import pytest
import torch

import openglraytracer_amd as rt
from conftest import parity_stats
from oracle import scenes

pytestmark = pytest.mark.gpu
SIZES = [(72, 40), (33, 17), (16, 8)]
N_VIEWS = (9, 17, 40)
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
@pytest.mark.parametrize("kind", SCENES)
def test_every_region_of_the_schedule_renders_the_tiled_bytes(ctx, kind, w, h):
    sc = rt.Scene(ctx, _objects(kind))
    try:
        for n_views in N_VIEWS:
            views = _views(n_views)
            tiled = _frames(ctx, sc, w, h, views, 0)
            for k in FORCED:
                forced = _frames(ctx, sc, w, h, views, k)
                assert forced.tobytes() == tiled.tobytes(), (n_views, k, parity_stats(forced, tiled))
    finally:
        sc.close()


@pytest.mark.parametrize("k", FORCED)
def test_three_launches_in_a_row_find_the_counters_reset(ctx, k):
    """The same forced launch three times on one context (the queue heads and
    done counters reset by the last wave of each queue), for a launch with
    every region and one smaller than its tail."""
    sc = rt.Scene(ctx, _objects("room20"))
    try:
        for (w, h), n_views in (((72, 40), 40), ((33, 17), 9)):
            views = _views(n_views)
            tiled = _frames(ctx, sc, w, h, views, 0)
            for _ in range(3):
                assert _frames(ctx, sc, w, h, views, k).tobytes() == tiled.tobytes()
    finally:
        sc.close()


def test_two_launches_on_two_streams_at_once(ctx):
    """Each launch takes a counter slot of its own from the context."""
    (w0, h0, n0), (w1, h1, n1) = (72, 40, 40), (33, 17, 17)
    v0, v1 = _views(n0), _views(n1)[::-1]
    sc = rt.Scene(ctx, _objects("room40"))
    try:
        t0, t1 = _frames(ctx, sc, w0, h0, v0, 0), _frames(ctx, sc, w1, h1, v1, 0)
        ctx.set_persistent0(8)
        s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
        o0 = torch.zeros((n0, h0, w0, 4), dtype=torch.float32, device="cuda")
        o1 = torch.zeros((n1, h1, w1, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(3):  # (back to back: the second stream's launch starts while the first's runs)
            _batch(ctx, sc, w0, h0, v0, out=o0, stream=s0.cuda_stream)
            _batch(ctx, sc, w1, h1, v1, out=o1, stream=s1.cuda_stream)
        torch.cuda.synchronize()
        assert _queued(ctx) == 1
        f0, f1 = o0.cpu().numpy(), o1.cpu().numpy()
    finally:
        sc.close()
    assert f0.tobytes() == t0.tobytes()
    assert f1.tobytes() == t1.tobytes()


def test_the_whole_resident_grid(ctx):
    """9 views of 640 x 368 (33,120 wave tiles) forced with a cap above the
    resident work-groups: the whole resident grid (8,192 waves on an MI355X),
    about four tiles per wave, so the launch is its tail regions alone."""
    w, h = 640, 368
    views = _views(9)
    sc = rt.Scene(ctx, _objects("room16"))
    try:
        out = {}
        for mode, queued in ((0, 0), (1 << 16, 1)):
            ctx.set_persistent0(mode)
            out[mode] = _batch(ctx, sc, w, h, views)
            torch.cuda.synchronize()
            assert _queued(ctx) == queued
        assert torch.equal(out[1 << 16].view(torch.int32), out[0].view(torch.int32))
    finally:
        sc.close()
