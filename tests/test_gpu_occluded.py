"""rt_occluded against the oracle (occlusion_common.py): the expected bit of a
segment is the oracle's closest hit with object >= 0 and t < 1, for every
segment, with no tolerance. Every scene x family runs with RT_OPT_CULLING on
and off in three arrangements (grouped; permuted together with PAIRS; poisoned,
one segment outside the kernel's walk range in lane 0, 31 or 63 of every other
wave), and the bytes and the words must both equal the oracle's bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import adversarial_rays as ar
import occlusion_common as oc
import openglraytracer_amd as rt
from openglraytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ao  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5


@pytest.fixture(params=[True, False], ids=["culling", "no_culling"])
def culling(request, gpu_ctx):
    gpu_ctx.set_culling(request.param)
    yield request.param
    gpu_ctx.set_culling(True)


@pytest.fixture(scope="module")
def room16(gpu_ctx):
    s = ar.scene("room16")
    sc = rt.Scene(gpu_ctx, s.objs, lights=s.lights)
    yield sc
    sc.close()


def same_bits(got, want, rays, what):
    """Equality of two bit planes; the message names the first differing segment."""
    got, want = np.asarray(got, bool), np.asarray(want, bool)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d of %d segments differ; first: segment %d (wave %d, lane %d) origin %s dir %s: got %d, "
                    "oracle %d" % (what, len(bad), len(got), i, i // 64, i % 64, ar.hexf(rays["origin"][i]),
                                   ar.hexf(rays["dir"][i]), got[i], want[i]))


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def check(ctx, sc, rays, want, what):
    """The bytes and the words of `rays` against the oracle's bits."""
    got = rt.occluded(ctx, sc, rays)
    assert got.dtype == np.bool_ and got.shape == (len(rays),)
    same_bits(got, want, rays, what + " bytes")
    words = rt.occluded(ctx, sc, rays, packed=True)
    assert words.dtype == np.uint64 and words.shape == ((len(rays) + 63) // 64,)
    same_bits(unpack(words, len(rays)), want, rays, what + " words")
    assert words.tobytes() == oc.pack_words(want).tobytes(), what + ": bits past the last segment"


# ---- 1. the families ----------------------------------------------------------------
@pytest.mark.parametrize("fam", oc.FAMILIES)
@pytest.mark.parametrize("sn", oc.SCENES)
def test_family_matches_the_oracle(gpu_ctx, sn, fam, culling):
    s = ar.scene(sn)
    sc = rt.Scene(gpu_ctx, s.objs, lights=s.lights)
    try:
        for how in oc.ARRANGEMENTS:
            rays, want = oc.arrange(sn, fam, how)
            check(gpu_ctx, sc, rays, want, "%s %s %s %s" % (sn, fam, how, "culling" if culling else "no culling"))
    finally:
        sc.close()


# ---- 2. sizes, guards, buffers --------------------------------------------------------
def _device_call(ctx, sc, rays_t, n, bytes_t, words_t, stream=None):
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return rt.lib().rt_occluded(ctx.handle, sc.handle, ptr(rays_t), n, ptr(bytes_t), ptr(words_t), 1,
                                C.c_void_p(stream) if stream else None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_tail_bits_and_guards(gpu_ctx, room16, n, culling):
    """The first n PAIRS of room16 into device planes with a guard region of
    0xA5 behind each: the oracle's answers, zero tail bits, the guards untouched."""
    f = oc.family("room16", "PAIRS")
    rays, want = f.rays[:n], f.want[:n]
    check(gpu_ctx, room16, rays, want, "n = %d" % n)
    n_words = (n + 63) // 64
    rays_t = torch.from_numpy(rays.view(np.float32).reshape(n, 8)).cuda()
    bytes_t = torch.full((n + 256,), GUARD, dtype=torch.uint8, device="cuda")
    words_t = torch.full((8 * (n_words + 32),), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert _device_call(gpu_ctx, room16, rays_t, n, bytes_t, words_t) == abi.RT_OK
    torch.cuda.synchronize()
    b, w = bytes_t.cpu().numpy(), words_t.cpu().numpy()
    same_bits(b[:n], want, rays, "n = %d device bytes" % n)
    assert set(np.unique(b[:n]).tolist()) <= {0, 1}
    assert (b[n:] == GUARD).all()
    assert w[:8 * n_words].tobytes() == oc.pack_words(want).tobytes()
    assert (w[8 * n_words:] == GUARD).all()
    if n % 64:
        assert int(w[:8 * n_words].view(np.uint64)[-1]) >> (n % 64) == 0


def test_output_and_buffer_combinations(gpu_ctx, room16):
    f = oc.family("room16", "PAIRS")
    n, n_words = f.n, (f.n + 63) // 64
    L, ctx, sc = rt.lib(), gpu_ctx.handle, room16.handle
    # host buffers: only bytes, only words, both
    planes = []
    for use_b, use_w in ((True, False), (False, True), (True, True)):
        b, w = np.full(n + 64, GUARD, np.uint8), np.full(n_words + 8, GUARD * 0x0101010101010101, np.uint64)
        assert L.rt_occluded(ctx, sc, f.rays.ctypes.data, n, b.ctypes.data if use_b else None,
                             w.ctypes.data if use_w else None, 0, None) == abi.RT_OK
        assert (b[n:] == GUARD).all() and (w[n_words:] == GUARD * 0x0101010101010101).all()
        if use_b:
            same_bits(b[:n], f.want, f.rays, "host bytes")
        else:
            assert (b == GUARD).all()
        if use_w:
            assert w[:n_words].tobytes() == oc.pack_words(f.want).tobytes()
        else:
            assert (w == GUARD * 0x0101010101010101).all()
        planes.append((b, w))
    # device buffers: synchronously, and on a caller's stream
    rays_t = torch.from_numpy(f.rays.view(np.float32).reshape(n, 8)).cuda()
    torch.cuda.synchronize()
    sync_b, sync_w = rt.occluded(gpu_ctx, room16, rays_t), rt.occluded(gpu_ctx, room16, rays_t, packed=True)
    stream = torch.cuda.Stream()
    asyn_b = rt.occluded(gpu_ctx, room16, rays_t, stream=stream.cuda_stream)
    asyn_w = rt.occluded(gpu_ctx, room16, rays_t, packed=True, stream=stream.cuda_stream)
    stream.synchronize()
    for b, w in ((sync_b, sync_w), (asyn_b, asyn_w)):
        assert b.is_cuda and b.dtype == torch.uint8 and b.shape == (n,)
        assert w.is_cuda and w.dtype == torch.int64 and w.shape == (n_words,)
        same_bits(b.cpu().numpy(), f.want, f.rays, "device bytes")
        assert w.cpu().numpy().tobytes() == oc.pack_words(f.want).tobytes()
    # float32 rows of 8 on the host are the same segments
    same_bits(rt.occluded(gpu_ctx, room16, f.rays.view(np.float32).reshape(-1, 8)), f.want, f.rays, "float32 rows")


def test_zero_rays(gpu_ctx, room16):
    b, w = np.full(8, GUARD, np.uint8), np.full(1, 7, np.uint64)
    rays = np.zeros(1, abi.RAY_DTYPE)
    L, ctx, sc = rt.lib(), gpu_ctx.handle, room16.handle
    assert L.rt_occluded(ctx, sc, rays.ctypes.data, 0, b.ctypes.data, w.ctypes.data, 0, None) == abi.RT_OK
    assert L.rt_occluded(ctx, sc, None, 0, b.ctypes.data, None, 0, None) == abi.RT_OK
    assert (b == GUARD).all() and w[0] == 7
    assert rt.occluded(gpu_ctx, room16, np.zeros(0, abi.RAY_DTYPE)).shape == (0,)
    assert rt.occluded(gpu_ctx, room16, np.zeros(0, abi.RAY_DTYPE), packed=True).shape == (0,)


def test_bad_arguments(gpu_ctx, room16):
    L, ctx, sc = rt.lib(), gpu_ctx.handle, room16.handle
    rays = np.zeros(8, abi.RAY_DTYPE)
    rays["dir"] = (0.0, 1.0, 0.0)
    b, w = np.full(8, GUARD, np.uint8), np.full(1, 7, np.uint64)
    r, pb, pw = rays.ctypes.data, b.ctypes.data, w.ctypes.data
    s = torch.cuda.Stream()
    invalid = [
        (lambda: L.rt_occluded(None, sc, r, 8, pb, pw, 0, None), b"null context"),
        (lambda: L.rt_occluded(ctx, None, r, 8, pb, pw, 0, None), b"null scene"),
        (lambda: L.rt_occluded(ctx, sc, None, 8, pb, pw, 0, None), b"null rays"),
        (lambda: L.rt_occluded(ctx, sc, r, 8, None, None, 0, None), b"no output plane"),
        (lambda: L.rt_occluded(ctx, sc, r, -1, pb, pw, 0, None), b"n_rays"),
        (lambda: L.rt_occluded(ctx, sc, r, abi.RT_MAX_RAYS + 1, pb, pw, 0, None), b"n_rays"),
        (lambda: L.rt_occluded(ctx, sc, r, 8, pb, pw, 0, C.c_void_p(s.cuda_stream)), b"device buffers"),
    ]
    for k, (call, fragment) in enumerate(invalid):
        assert call() == abi.RT_ERR_INVALID, k
        msg = L.rt_last_error()
        assert b"rt_occluded" in msg and fragment in msg, (k, msg)
    assert (b == GUARD).all() and w[0] == 7


def test_the_last_render_stays_the_last_kernel(gpu_ctx, room16):
    f = oc.family("room16", "PAIRS")
    view = rt.make_view(None, 0.0)
    colour = rt.render(gpu_ctx, room16, 32, 18, 0, view=view)
    kernel = rt.last_kernel(gpu_ctx)
    same_bits(rt.occluded(gpu_ctx, room16, f.rays), f.want, f.rays, "after a render")
    assert rt.last_kernel(gpu_ctx) == kernel
    assert gpu_ctx.last_kernel_ms() > 0.0  # (RT_OPT_TIMING: the call's launch is timed)
    assert rt.render(gpu_ctx, room16, 32, 18, 0, view=view).tobytes() == colour.tobytes()


def test_non_finite_segments_stay_in_their_slots(gpu_ctx, room16, culling):
    f = oc.family("room16", "PAIRS")
    odd = f.rays[:256].copy()
    odd["origin"][70] = (np.nan, 0.0, 0.0)
    odd["dir"][130] = (np.inf, 0.0, 0.0)
    odd["origin"][200] = (np.inf, -np.inf, 0.0)
    odd["dir"][255] = (np.nan, np.nan, np.nan)
    keep = np.ones(256, bool)
    keep[[70, 130, 200, 255]] = False
    got = rt.occluded(gpu_ctx, room16, odd)
    same_bits(got[keep], f.want[:256][keep], odd[keep], "beside non-finite segments")


# ---- 3. against the product's own queries ----------------------------------------------
def test_equals_the_closest_hit_query(gpu_ctx, culling):
    s = ar.scene("room100")
    f = oc.family("room100", "PAIRS")
    sc = rt.Scene(gpu_ctx, s.objs, lights=s.lights)
    try:
        (hits,) = rt.trace_rays(gpu_ctx, sc, f.rays, 0, colors=False, hits=True, shadow=False)
        want = (hits["object"] >= 0) & (hits["t"] < np.float32(1.0))
        same_bits(rt.occluded(gpu_ctx, sc, f.rays), want, f.rays, "room100 PAIRS against rt_trace_rays")
        assert np.array_equal(want, f.want)
    finally:
        sc.close()


def test_reproduces_render_hits_shadow_bits(gpu_ctx, culling):
    """The shadow segments built from the GPU's own points and normals of a
    32 x 18 view of room16, with a fourth light that has neither diffuse nor
    specular colour: every bit of rt_hit.shadow, the dead light's included."""
    s = ar.scene("room16")
    dead = abi.Light()
    C.memmove(C.byref(dead), C.byref(s.lights[0]), C.sizeof(abi.Light))
    dead.position[:] = [-4.0, 3.0, 6.0]
    dead.diffuse[:] = [0.0] * 4
    dead.specular[:] = [0.0] * 4
    lights = list(s.lights) + [dead]
    sc = rt.Scene(gpu_ctx, s.objs, lights=lights)
    try:
        hits, normals, points = rt.render_hits(gpu_ctx, sc, oc.VIEW_W, oc.VIEW_H, view=rt.make_view(None, 0.0))
        hit = hits["object"] >= 0
        assert hit.sum() >= 500
        rays = np.ascontiguousarray(oc.shadow_segments(points[hit], normals[hit], lights).reshape(-1))
        want = ((hits["shadow"][hit][:, None] >> np.arange(4, dtype=np.uint32)[None]) & 1).astype(bool).reshape(-1)
        assert want[3::4].any() and not want[3::4].all()  # (the dead light's bit is computed)
        same_bits(rt.occluded(gpu_ctx, sc, rays), want, rays, "shadow bits of rt_render_hits")
    finally:
        sc.close()


def test_ao_image_equals_the_oracle(gpu_ctx, room16):
    """tools/ao.py at 16 x 9, K = 4: its image is the one computed from the oracle's bits."""
    s = ar.scene("room16")
    view = rt.make_view(None, 0.0)
    img = ao.ao(gpu_ctx, room16, view, 16, 9, 4, 2.0, seed=1)
    hits, normals, points = rt.render_hits(gpu_ctx, room16, 16, 9, view=view, shadow=False)
    hit = hits["object"] >= 0
    rays = ao.ao_segments(points[hit], normals[hit], 4, 2.0, seed=1)
    bits = oc.oracle_bits(s, rays.reshape(-1))
    assert bits.any() and not bits.all()
    want = ao.ao_image(hit, bits, 4)
    assert img.shape == (9, 16, 4) and img.tobytes() == want.tobytes()
