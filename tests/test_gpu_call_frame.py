"""The C-ABI entry points' shared call frame on the GPU: what each entry point
answers to a bad argument, the context's grow-only staging buffers, and the
kernel-time span behind rt_last_kernel_ms.

The (code, rt_last_error) pairs of the error table are written out from the
entry points' source text as it stood before they shared their checks: the
codes, the wording and which check answers first are part of the interface.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from openglraytracer_amd import abi

pytestmark = pytest.mark.gpu
W, H = 16, 8
INVALID, UNSUPPORTED = abi.RT_ERR_INVALID, abi.RT_ERR_UNSUPPORTED
SIZE = (INVALID, "bad frame size")
DEPTH = (UNSUPPORTED, "max_depth 10 outside [0, 9]")


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """The shipped scene at time 0, its animated twin, a view, and buffers no failing call touches."""
    base, channels = rt.reference_animation()
    w = {"ctx": gpu_ctx, "scene": rt.Scene(gpu_ctx, rt.reference_objects(0.0)),
         "anim": rt.Anim(gpu_ctx, base, channels, max_frames=2), "view": rt.make_view(None, 0.0),
         "dev": torch.zeros(1 << 16, dtype=torch.float32, device="cuda"), "host": np.zeros(1 << 16, np.float32),
         "stream": torch.cuda.Stream(), "times": (C.c_float * 2)(0.0, 0.0)}
    yield w
    w["anim"].close()
    w["scene"].close()


def entry_points(w):
    """{name: (the C function, its arguments in order as (name, good value))}."""
    ctx, sc, an = w["ctx"].handle, w["scene"].handle, w["anim"].handle
    view, dev, times = C.addressof(w["view"]), w["dev"].data_ptr(), C.addressof(w["times"])
    frame = [("width", W), ("height", H)]
    rows = [("row_begin", 0), ("row_end", H)]
    planes = [("hits", dev), ("normals", dev), ("points", dev)]
    tail = [("is_device", 1), ("stream", None)]
    shard = [("block_rows", 8), ("n_shards", 1), ("shard", 0)]
    L = rt.lib()
    return {
        "rt_render_view": (L.rt_render_view, [("ctx", ctx), ("scene", sc), ("view", view)] + frame +
                           [("depth", 0)] + rows + [("out", dev)] + tail),
        "rt_render_hits_view": (L.rt_render_hits_view, [("ctx", ctx), ("scene", sc), ("view", view)] + frame + rows +
                                [("flags", 1)] + planes + tail),
        "rt_pick": (L.rt_pick, [("ctx", ctx), ("scene", sc), ("view", view)] + frame + [("x", 3), ("y", 2), ("flags", 1)] +
                    [(a, w["host"].ctypes.data) for a, _ in planes]),  # (rt_pick answers into host memory)
        "rt_trace_rays": (L.rt_trace_rays, [("ctx", ctx), ("scene", sc), ("rays", dev), ("n_rays", 4), ("depth", 0),
                                            ("flags", 1), ("colors", dev)] + planes + tail),
        "rt_view_rays": (L.rt_view_rays, [("ctx", ctx), ("view", view)] + frame + rows + [("rays", dev)] + tail),
        "rt_render_shard": (L.rt_render_shard, [("ctx", ctx), ("scene", sc), ("view", view)] + frame + [("depth", 0)] +
                            shard + [("out", dev), ("stream", None)]),
        "rt_render_batch": (L.rt_render_batch, [("ctx", ctx), ("scene", sc), ("views", view), ("n_views", 1)] + frame +
                            [("depth", 0)] + shard + [("out", dev), ("stream", None)]),
        "rt_render_accumulate": (L.rt_render_accumulate, [("ctx", ctx), ("scene", sc), ("view", view)] + frame +
                                 [("depth", 0), ("spp", 1), ("sample_offset", 0), ("seed", 0), ("jitter", 1)] + rows +
                                 [("out", dev), ("stream", None)]),
        "rt_render_aa_view": (L.rt_render_aa_view, [("ctx", ctx), ("scene", sc), ("view", view)] + frame +
                              [("depth", 0), ("spp", 2), ("seed", 0), ("threshold", 0.1), ("out", dev),
                               ("refined", None)] + tail),
        "rt_render_animated": (L.rt_render_animated, [("ctx", ctx), ("anim", an), ("cam", None), ("time", 0.0)] + frame +
                               [("depth", 0)] + rows + [("out", dev)] + tail),
        "rt_render_hits_animated": (L.rt_render_hits_animated, [("ctx", ctx), ("anim", an), ("cam", None), ("time", 0.0)] +
                                    frame + rows + [("flags", 1)] + planes + tail),
        "rt_render_batch_animated": (L.rt_render_batch_animated, [("ctx", ctx), ("anim", an), ("views", view),
                                                                  ("times", times), ("n_views", 1)] + frame +
                                     [("depth", 0)] + shard + [("out", dev), ("stream", None)]),
    }


ASYNC_HOST = {"is_device": 0, "stream": "STREAM"}
NO_PLANE = {"hits": None, "normals": None, "points": None}
BAD_ROWS = ({"row_begin": -1}, {"row_end": H + 1}, {"row_begin": 4, "row_end": 4})


def hits_table(who):
    return ([(bad, (INVALID, who + ": bad row range")) for bad in BAD_ROWS] +
            [(NO_PLANE, (INVALID, who + ": no output plane (hits, normals and points are all NULL)")),
             ({"flags": 2}, (INVALID, who + ": unknown flag bits")),
             (ASYNC_HOST, (INVALID, who + ": an asynchronous call needs device output buffers")),
             # two at once: the planes are looked at before the flag bits, the rows before both
             (dict(NO_PLANE, flags=2), (INVALID, who + ": no output plane (hits, normals and points are all NULL)")),
             (dict(NO_PLANE, row_begin=-1), (INVALID, who + ": bad row range"))])


def table():
    """[(entry point, the bad arguments, (code, message))]: one bad input per check the entry point makes."""
    t = []
    sized = ("rt_render_view", "rt_render_hits_view", "rt_pick", "rt_render_shard", "rt_render_batch",
             "rt_render_accumulate", "rt_render_aa_view", "rt_render_animated", "rt_render_hits_animated",
             "rt_render_batch_animated")
    for name in sized:
        t += [(name, {"width": 0}, SIZE), (name, {"height": 65537}, SIZE)]
    for name in ("rt_render_view", "rt_render_shard", "rt_render_batch", "rt_render_accumulate", "rt_render_aa_view",
                 "rt_render_animated", "rt_render_batch_animated", "rt_trace_rays"):
        t.append((name, {"depth": 10}, DEPTH))
    e = (INVALID, "rt_render: bad view / output / row range")
    t += [("rt_render_view", bad, e) for bad in ({"view": None}, {"out": None}) + BAD_ROWS]
    t += [("rt_render_view", ASYNC_HOST, (INVALID, "rt_render: an asynchronous render needs a device output buffer")),
          # two at once: the depth is looked at before the view, the rows before the asynchronous host buffer
          ("rt_render_view", {"view": None, "depth": 10}, DEPTH),
          ("rt_render_view", dict(ASYNC_HOST, row_end=H + 1), e)]
    t += [("rt_render_hits_view", bad, exp) for bad, exp in hits_table("rt_render_hits")]
    t += [("rt_render_hits_view", {"view": None}, (INVALID, "rt_render_hits: null view")),
          ("rt_render_hits_view", {"view": None, "flags": 2}, (INVALID, "rt_render_hits: unknown flag bits"))]
    t += [("rt_render_hits_animated", bad, exp) for bad, exp in hits_table("rt_render_hits_animated")]
    e = (INVALID, "rt_pick: null view, or a pixel outside the frame")
    t += [("rt_pick", NO_PLANE, (INVALID, "rt_pick: no output plane (hits, normals and points are all NULL)")),
          ("rt_pick", {"flags": 2}, (INVALID, "rt_pick: unknown flag bits")),
          ("rt_pick", {"view": None}, e), ("rt_pick", {"x": W}, e), ("rt_pick", {"y": -1}, e),
          ("rt_pick", {"view": None, "flags": 2}, (INVALID, "rt_pick: unknown flag bits"))]
    t += [("rt_trace_rays", {"scene": None}, (INVALID, "rt_trace_rays: null scene")),
          ("rt_trace_rays", {"rays": None}, (INVALID, "rt_trace_rays: null rays")),
          ("rt_trace_rays", {"n_rays": -1}, (INVALID, "rt_trace_rays: n_rays outside [0, RT_MAX_RAYS]")),
          ("rt_trace_rays", dict(NO_PLANE, colors=None),
           (INVALID, "rt_trace_rays: no output plane (colors, hits, normals and points are all NULL)")),
          ("rt_trace_rays", {"flags": 2}, (INVALID, "rt_trace_rays: unknown flag bits")),
          ("rt_trace_rays", ASYNC_HOST, (INVALID, "rt_trace_rays: an asynchronous call needs device buffers")),
          ("rt_trace_rays", {"flags": 2, "depth": 10}, (INVALID, "rt_trace_rays: unknown flag bits")),
          ("rt_trace_rays", dict(ASYNC_HOST, depth=10), (INVALID, "rt_trace_rays: an asynchronous call needs device buffers"))]
    e = (INVALID, "rt_view_rays: bad frame size or row range")
    t += [("rt_view_rays", bad, e) for bad in ({"width": 0}, {"height": 65537}) + BAD_ROWS]
    t += [("rt_view_rays", {"view": None}, (INVALID, "rt_view_rays: null view or ray buffer")),
          ("rt_view_rays", {"rays": None}, (INVALID, "rt_view_rays: null view or ray buffer")),
          ("rt_view_rays", ASYNC_HOST, (INVALID, "rt_view_rays: an asynchronous call needs a device buffer")),
          ("rt_view_rays", {"view": None, "width": 0}, (INVALID, "rt_view_rays: null view or ray buffer"))]
    e = (INVALID, "rt_render_shard: bad view / output / shard arguments")
    t += [("rt_render_shard", bad, e) for bad in ({"view": None}, {"out": None}, {"shard": 1})]
    e = (INVALID, "rt_render_batch: need 1..256 views and a device output")
    t += [("rt_render_batch", bad, e) for bad in ({"views": None}, {"out": None}, {"n_views": 0}, {"n_views": 257})]
    t.append(("rt_render_batch", {"n_shards": 2, "block_rows": 0}, (INVALID, "rt_render_batch: bad shard arguments")))
    e = (INVALID, "rt_render_accumulate: bad view / accumulator / spp / row range")
    t += [("rt_render_accumulate", bad, e) for bad in ({"view": None}, {"out": None}, {"spp": 0}) + BAD_ROWS]
    t.append(("rt_render_accumulate", {"spp": 0, "depth": 10}, DEPTH))
    e = (INVALID, "rt_render_aa: bad view / output / spp / threshold")
    t += [("rt_render_aa_view", bad, e) for bad in ({"view": None}, {"out": None}, {"spp": 0})]
    t += [("rt_render_aa_view", ASYNC_HOST, (INVALID, "rt_render_aa: an asynchronous render needs device output buffers")),
          ("rt_render_aa_view", dict(ASYNC_HOST, spp=0), e)]
    e = (INVALID, "rt_render_animated: bad output / row range, or an asynchronous render without a device buffer")
    t += [("rt_render_animated", bad, e) for bad in ({"out": None}, ASYNC_HOST) + BAD_ROWS]
    t += [("rt_render_animated", {"anim": None}, (INVALID, "rt_render_animated: null context or animated scene")),
          ("rt_render_hits_animated", {"anim": None}, (INVALID, "rt_render_hits_animated: null context or animated scene"))]
    e = (INVALID, "rt_render_batch_animated: need 1..256 views and a device output")
    t += [("rt_render_batch_animated", bad, e) for bad in ({"out": None}, {"n_views": 0})]
    t += [("rt_render_batch_animated", {"times": None},
           (INVALID, "rt_render_batch_animated: null context, animated scene or times")),
          ("rt_render_batch_animated", {"n_views": 3},
           (INVALID, "rt_render_batch_animated: 3 views but the animated scene holds 2 frames in flight (max_frames)")),
          ("rt_render_batch_animated", {"n_shards": 2, "block_rows": 0},
           (INVALID, "rt_render_batch_animated: bad shard arguments"))]
    return t


TABLE = table()


@pytest.mark.parametrize("k", range(len(TABLE)), ids=["%s-%d" % (row[0], k) for k, row in enumerate(TABLE)])
def test_error_table(world, k):
    name, bad, expected = TABLE[k]
    fn, args = entry_points(world)[name]
    assert set(bad) <= {a for a, _ in args}, "the table names an argument %s does not take" % name
    values = [bad.get(a, good) for a, good in args]
    values = [world["stream"].cuda_stream if v == "STREAM" else v for v in values]
    if bad.get("is_device") == 0:  # (a host buffer beside the stream, as such a caller would pass)
        values = [world["host"].ctypes.data if v == world["dev"].data_ptr() else v for v in values]
    rc = fn(*values)
    assert (rc, rt.lib().rt_last_error().decode()) == expected


def test_every_entry_point_accepts_its_good_arguments(world):
    """The table's base rows are valid calls: a bad row fails for its one change alone."""
    for name, (fn, args) in entry_points(world).items():
        assert fn(*[good for _, good in args]) == abi.RT_OK, (name, rt.lib().rt_last_error().decode())
    torch.cuda.synchronize()


# ---- the grow-only staging buffers --------------------------------------------
SIZES = ((24, 16), (72, 40), (24, 16))
AA = dict(max_depth=1, spp=2, threshold=0.05, seed=7)


def host_calls(ctx, sc, view, w, h):
    rays = rt.view_rays(ctx, view, w, h)
    aa, mask = rt.render_aa(ctx, sc, w, h, view=view, want_mask=True, **AA)
    return {"render": [rt.render(ctx, sc, w, h, 1, view=view)],
            "render_hits": list(rt.render_hits(ctx, sc, w, h, view=view)),
            "trace_rays": [rays] + list(rt.trace_rays(ctx, sc, rays, 1, colors=True, hits=True)),
            "render_aa": [aa, mask]}


def device_calls(ctx, sc, view, w, h):
    def dev(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device="cuda")
    frame, aa, mask = dev(h, w, 4), dev(h, w, 4), dev(h, w, dtype=torch.uint8)
    planes = [dev(h, w, 4, dtype=torch.int32), dev(h, w, 4), dev(h, w, 4)]
    rt.render_device(ctx, sc, frame.data_ptr(), w, h, 1, view=view)
    rt.render_hits_device(ctx, sc, w, h, *[p.data_ptr() for p in planes], view=view)
    rays = rt.view_rays(ctx, view, w, h, device=True).contiguous()
    traced = rt.trace_rays(ctx, sc, rays, 1, colors=True, hits=True)
    rt.render_aa(ctx, sc, w, h, view=view, out=aa.data_ptr(), want_mask=mask.data_ptr(), **AA)
    torch.cuda.synchronize()
    return {"render": [frame], "render_hits": planes, "trace_rays": [rays] + list(traced), "render_aa": [aa, mask]}


def test_staging_growth():
    """Host-destination calls of the four families, interleaved, at a small
    frame, a larger one and the small one again on one context: each result is,
    byte for byte, the same call with device buffers on a fresh context."""
    view = rt.make_view(None, 0.0)
    objs = rt.reference_objects(0.0)
    expected = {}
    ref_ctx = rt.Context(0)
    ref_sc = rt.Scene(ref_ctx, objs)
    try:
        for w, h in set(SIZES):
            expected[(w, h)] = {k: [t.cpu().numpy().tobytes() for t in v]
                                for k, v in device_calls(ref_ctx, ref_sc, view, w, h).items()}
    finally:
        ref_sc.close()
        ref_ctx.close()
    ctx = rt.Context(0)
    sc = rt.Scene(ctx, objs)
    try:
        for w, h in SIZES:
            got = host_calls(ctx, sc, view, w, h)
            for family, arrays in got.items():
                assert [np.ascontiguousarray(a).tobytes() for a in arrays] == expected[(w, h)][family], (family, w, h)
    finally:
        sc.close()
        ctx.close()


# ---- the kernel-time span -------------------------------------------------------
def timed_families(ctx, sc, n_split):
    """One call of each family that leaves a span, on device buffers of a 32 x 16 frame."""
    w, h = 32, 16
    view = rt.make_view(None, 0.0)
    out = torch.zeros((n_split, h, w, 4), dtype=torch.float32, device="cuda")
    plane = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
    rays = rt.view_rays(ctx, view, w, h, device=True).contiguous()
    views = [rt.make_view(None, 0.1 * k) for k in range(n_split)]
    p = out.data_ptr()
    return [("render", lambda: rt.render_device(ctx, sc, p, w, h, 1, view=view)),
            ("render_hits", lambda: rt.render_hits_device(ctx, sc, w, h, plane.data_ptr(), view=view)),
            ("pick", lambda: rt.pick(ctx, sc, w, h, 5, 5, view=view)),
            ("trace_rays, colours and records", lambda: rt.trace_rays(ctx, sc, rays, 1, colors=True, hits=True)),
            ("render_aa", lambda: rt.render_aa(ctx, sc, w, h, 1, 2, 0.05, view=view, out=p)),
            ("render_accumulate", lambda: rt.render_accumulate(ctx, sc, p, w, h, 0, 2, view=view)),
            ("render_shard", lambda: rt.render_shard(ctx, sc, p, w, h, 0, 8, 1, 0, view=view)),
            ("deep batch in several launches", lambda: rt.render_batch(ctx, sc, p, w, h, 2, views))], out


def test_timed_spans():
    ctx = rt.Context(0)
    sc = rt.Scene(ctx, rt.reference_objects(0.0))
    try:
        n_split = next(n for n in range(2, abi.RT_MAX_BATCH + 1) if rt.batch_launches(ctx, sc, n, 2) > 1)
        families, keep = timed_families(ctx, sc, n_split)
        ms = C.c_float()
        for name, call in families:
            ctx.set_timing(True)
            call()
            assert ctx.last_kernel_ms() > 0.0, name
            ctx.set_timing(False)
            call()
            assert rt.lib().rt_last_kernel_ms(ctx.handle, C.byref(ms)) == INVALID, name
            assert rt.lib().rt_last_error().decode() == "rt_last_kernel_ms: nothing timed yet", name
        # RT_OPT_TIMING outlives the split batch: the next single render is timed
        ctx.set_timing(True)
        families[-1][1]()
        assert ctx.last_kernel_ms() > 0.0
        ctx.set_timing(False)
        families[0][1]()
        assert rt.lib().rt_last_kernel_ms(ctx.handle, C.byref(ms)) == INVALID
        ctx.set_timing(True)
        families[-1][1]()
        families[0][1]()
        assert ctx.last_kernel_ms() > 0.0
        torch.cuda.synchronize()
        del keep
    finally:
        sc.close()
        ctx.close()
