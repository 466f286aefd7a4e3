"""Adaptive anti-aliasing on the GPU (rt_render_aa*): the base frame with the
pixels on a colour edge replaced by the mean of spp jittered samples. The
expected frame is np.where(mask, oracle accumulate / spp, oracle base) with
the mask from the numpy criterion (tests/aa_common.py) over the oracle's base
frame; every comparison is bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from oracle import port, scenes

from aa_common import expected_aa, np_edge_mask, np_tile_masks, oracle_base, oracle_samples, scene_objects
from conftest import ROOT, parity_stats
from test_gpu_parity import random_scene

pytestmark = pytest.mark.gpu
INF = float("inf")


def _counts(mask):
    return int(mask.sum()), int((np_tile_masks(mask.astype(bool)) != 0).sum())


def _check(ctx, got, mask, want, want_mask, what, equal_nan=False):
    assert np.array_equal(mask, want_mask), (what, int(mask.sum()), int(want_mask.sum()))
    assert np.array_equal(got, want, equal_nan=equal_nan), (what, parity_stats(got, want))
    assert rt.aa_last_counts(ctx) == _counts(want_mask), what


@pytest.fixture(params=[True, False], ids=["lists", "tiled"])
def queued(gpu_ctx, request):
    """RT_OPT_AA_QUEUED: the refine launch at depth 0-1 over the live-tile lists (the
    default) or tiled with the work-group early exit; deeper ones take the lists always."""
    gpu_ctx.set_aa_queued(request.param)
    yield request.param
    gpu_ctx.set_aa_queued(True)


@pytest.fixture(scope="module")
def shipped(gpu_ctx):
    sc = rt.Scene(gpu_ctx, scene_objects("shipped")[0])
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def bench16(gpu_ctx):
    sc = rt.Scene(gpu_ctx, scene_objects("bench16")[0])
    yield sc
    sc.close()


# ---- 1. threshold +inf: nothing is flagged ---------------------------------------
@pytest.mark.parametrize("depth", [0, 2])
def test_threshold_inf_is_the_base_frame(gpu_ctx, shipped, depth):
    w, h = 33, 17
    view = rt.make_view(None, 0.7)
    base = rt.render(gpu_ctx, shipped, w, h, depth, view=view)
    got, mask = rt.render_aa(gpu_ctx, shipped, w, h, depth, 3, INF, view=view, want_mask=True)
    assert got.tobytes() == base.tobytes()
    assert not mask.any() and rt.aa_last_counts(gpu_ctx) == (0, 0)
    assert np.array_equal(got, oracle_base("shipped", w, h, depth))


# ---- 2. threshold -1: every pixel is flagged -------------------------------------
@pytest.mark.parametrize("culling", [True, False])
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_threshold_below_zero_is_the_sample_mean(gpu_ctx, shipped, queued, depth, culling):
    w, h, spp = 33, 17, 3
    view = rt.make_view(None, 0.7)
    gpu_ctx.set_culling(culling)
    try:
        got, mask = rt.render_aa(gpu_ctx, shipped, w, h, depth, spp, -1.0, view=view, want_mask=True)
    finally:
        gpu_ctx.set_culling(True)
    assert mask.all()
    want = oracle_samples("shipped", w, h, depth, spp) / np.float32(spp)
    _check(gpu_ctx, got, mask, want, np.ones((h, w), np.uint8), (depth, culling))
    assert (got[..., 3] == 0).all()


# ---- 3. mixed frames: the early exit and the lane masks --------------------------
@pytest.mark.parametrize("name,depth", [("shipped", 0), ("shipped", 2), ("bench16", 0)])
def test_mixed_frames(gpu_ctx, shipped, bench16, queued, name, depth):
    w, h, spp, thr = 96, 54, 4, 0.25
    base = oracle_base(name, w, h, depth)
    want, want_mask = expected_aa(base, oracle_samples(name, w, h, depth, spp), spp, thr)
    # the inputs exercise what they are meant to
    flagged = want_mask.astype(bool)
    share = flagged.mean()
    print("%s depth %d: flagged share %.3f" % (name, depth, share))
    assert 0.05 < share < 0.5
    tiles = np_tile_masks(flagged)
    live = tiles != 0
    gh, gw = (live.shape[0] + 1) // 2, (live.shape[1] + 1) // 2
    groups = np.zeros((gh * 2, gw * 2), bool)
    groups[:live.shape[0], :live.shape[1]] = live
    per_group = groups.reshape(gh, 2, gw, 2).transpose(0, 2, 1, 3).reshape(gh, gw, 4)
    group_live = per_group.any(-1)
    print("live wave tiles %d of %d, live work-groups %d of %d" % (live.sum(), live.size, group_live.sum(),
                                                                   group_live.size))
    assert not group_live.all()  # a 16x16 work-group tile without a flagged pixel
    in_frame = np.zeros((gh * 2, gw * 2), bool)
    in_frame[:live.shape[0], :live.shape[1]] = True
    in_frame = in_frame.reshape(gh, 2, gw, 2).transpose(0, 2, 1, 3).reshape(gh, gw, 4)
    assert (group_live[..., None] & in_frame & ~per_group).any()  # an empty wave tile inside a live work-group
    full = np_tile_masks(np.ones_like(flagged))
    assert (live & (tiles != full)).any()  # a partly flagged wave tile
    sc = shipped if name == "shipped" else bench16
    got, mask = rt.render_aa(gpu_ctx, sc, w, h, depth, spp, thr, view=rt.make_view(None, scene_objects(name)[1]),
                             want_mask=True)
    _check(gpu_ctx, got, mask, want, want_mask, (name, depth))


# ---- 4. random scenes -----------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(gpu_ctx, seed):
    objs, mats, lights, t, depth, w, h = random_scene(seed)
    spp, thr = 2, 0.1
    base = port.render(objs, w, h, depth, t, materials=mats, lights=lights)
    samples = port.render_accumulate(objs, w, h, depth, spp, 0, seed=seed, time=t, materials=mats, lights=lights)
    want, want_mask = expected_aa(base, samples, spp, thr)
    sc = rt.Scene(gpu_ctx, objs, materials=mats, lights=lights)
    try:
        got, mask = rt.render_aa(gpu_ctx, sc, w, h, depth, spp, thr, seed=seed, view=rt.make_view(None, t),
                                 want_mask=True)
        _check(gpu_ctx, got, mask, want, want_mask, (seed, depth, w, h), equal_nan=True)
        gpu_ctx.set_aa_queued(False)
        got, mask = rt.render_aa(gpu_ctx, sc, w, h, depth, spp, thr, seed=seed, view=rt.make_view(None, t),
                                 want_mask=True)
        _check(gpu_ctx, got, mask, want, want_mask, (seed, depth, w, h, "tiled"), equal_nan=True)
    finally:
        gpu_ctx.set_aa_queued(True)
        sc.close()


# ---- 5. entry points and memory -------------------------------------------------
def test_entry_points_and_memory_variants(gpu_ctx, shipped):
    w, h, depth, spp, thr = 96, 54, 0, 4, 0.25
    want, want_mask = expected_aa(oracle_base("shipped", w, h, depth), oracle_samples("shipped", w, h, depth, spp),
                                  spp, thr)
    by_view = rt.render_aa(gpu_ctx, shipped, w, h, depth, spp, thr, view=rt.make_view(None, 0.7), want_mask=True)
    by_time = rt.render_aa(gpu_ctx, shipped, w, h, depth, spp, thr, cam=None, time=0.7, want_mask=True)
    for k in range(2):
        assert by_view[k].tobytes() == by_time[k].tobytes()
    _check(gpu_ctx, by_time[0], by_time[1], want, want_mask, "host")
    assert np.array_equal(rt.render_aa(gpu_ctx, shipped, w, h, depth, spp, thr, time=0.7), want)  # no mask wanted
    out = torch.full((h + 2, w, 4), 7.0, dtype=torch.float32, device="cuda")  # a guard row on each side
    plane = torch.full((h + 2, w), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.render_aa(gpu_ctx, shipped, w, h, depth, spp, thr, time=0.7, out=out.data_ptr() + w * 16,
                 want_mask=plane.data_ptr() + w)
    o, m = out.cpu().numpy(), plane.cpu().numpy()
    _check(gpu_ctx, o[1:-1], m[1:-1], want, want_mask, "device")
    assert (o[0] == 7.0).all() and (o[-1] == 7.0).all() and (m[0] == 9).all() and (m[-1] == 9).all()


def test_parameter_errors(gpu_ctx, shipped):
    L = rt.lib()
    v = C.byref(rt.make_view(None, 0.0))
    out = np.zeros((17, 33, 4), np.float32)
    o = out.ctypes.data
    c, s = gpu_ctx.handle, shipped.handle
    invalid = [
        lambda: L.rt_render_aa_view(c, None, v, 33, 17, 0, 2, 0, 0.1, o, None, 0, None),
        lambda: L.rt_render_aa_view(c, s, None, 33, 17, 0, 2, 0, 0.1, o, None, 0, None),
        lambda: L.rt_render_aa_view(c, s, v, 33, 17, 0, 2, 0, 0.1, None, None, 0, None),
        lambda: L.rt_render_aa_view(c, s, v, 33, 17, 0, 0, 0, 0.1, o, None, 0, None),
        lambda: L.rt_render_aa_view(c, s, v, 33, 17, 0, 2, 0, float("nan"), o, None, 0, None),
        lambda: L.rt_render_aa_view(c, s, v, 0, 17, 0, 2, 0, 0.1, o, None, 0, None),
        lambda: L.rt_render_aa_view(c, s, v, 33, 65537, 0, 2, 0, 0.1, o, None, 0, None),
    ]
    for k, call in enumerate(invalid):
        assert call() == abi.RT_ERR_INVALID, k
    assert L.rt_render_aa_view(c, s, v, 33, 17, abi.RT_MAX_DEPTH + 1, 2, 0, 0.1, o, None, 0, None) == abi.RT_ERR_UNSUPPORTED
    stream = torch.cuda.Stream()  # an asynchronous call needs device memory
    assert L.rt_render_aa_view(c, s, v, 33, 17, 0, 2, 0, 0.1, o, None, 0,
                               C.c_void_p(stream.cuda_stream)) == abi.RT_ERR_INVALID
    gpu_ctx.set_output(abi.RT_OUTPUT_RGBA8)
    try:
        assert L.rt_render_aa_view(c, s, v, 33, 17, 0, 2, 0, 0.1, o, None, 0, None) == abi.RT_ERR_UNSUPPORTED
        assert b"RT_OUTPUT_RGBA32F" in L.rt_last_error()
    finally:
        gpu_ctx.set_output(abi.RT_OUTPUT_RGBA32F)


# ---- 6. the scratch across streams ----------------------------------------------
def test_scratch_reuse_across_streams(gpu_ctx, shipped):
    """Two calls back to back on two streams (other threshold, other size), then
    the first again: the second waits on the device for the first's use of the
    masks, list and counters, and the counters start from zero each time."""
    spp = 4
    cases = [(96, 54, 0.25), (33, 17, 0.05)]
    wants = [expected_aa(oracle_base("shipped", w, h, 0), oracle_samples("shipped", w, h, 0, spp), spp, thr)
             for w, h, thr in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for w, h, _ in cases]
    planes = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h, _ in cases]
    torch.cuda.synchronize()

    def call(k):
        w, h, thr = cases[k]
        rt.render_aa(gpu_ctx, shipped, w, h, 0, spp, thr, time=0.7, out=outs[k].data_ptr(),
                     want_mask=planes[k].data_ptr(), stream=streams[k].cuda_stream)

    call(0)
    call(1)
    counts1 = rt.aa_last_counts(gpu_ctx)
    for s in streams:
        s.synchronize()
    for k in range(2):
        assert np.array_equal(planes[k].cpu().numpy(), wants[k][1]), k
        assert np.array_equal(outs[k].cpu().numpy(), wants[k][0]), k
    assert counts1 == _counts(wants[1][1])
    outs[0].zero_()
    planes[0].zero_()
    torch.cuda.synchronize()
    call(0)
    assert rt.aa_last_counts(gpu_ctx) == _counts(wants[0][1])
    streams[0].synchronize()
    assert np.array_equal(planes[0].cpu().numpy(), wants[0][1])
    assert np.array_equal(outs[0].cpu().numpy(), wants[0][0])


# ---- 7. a full-size frame -------------------------------------------------------
def test_full_size_frame_bands(gpu_ctx, bench16, queued):
    """1920x1080 (grid sizes the small frames do not reach): two full-width
    2-row bands against the oracle, whose base rows are taken one row wider on
    each side for the mask."""
    w, h, depth, spp, thr = 1920, 1080, 0, 4, 0.1
    objs = scene_objects("bench16")[0]
    got, mask = rt.render_aa(gpu_ctx, bench16, w, h, depth, spp, thr, time=0.0, want_mask=True)
    assert rt.aa_last_counts(gpu_ctx)[0] == int(mask.sum())
    assert 0 < mask.mean() < 0.5
    for r0, r1 in [(538, 540), (1078, 1080)]:
        b0, b1 = max(r0 - 1, 0), min(r1 + 1, h)
        base = port.render(objs, w, h, depth, 0.0, rows=(b0, b1))
        flagged = np_edge_mask(base, thr)[r0 - b0:r1 - b0]
        samples = port.render_accumulate(objs, w, h, depth, spp, 0, seed=0, rows=(r0, r1))
        want = np.where(flagged[..., None], samples / np.float32(spp), base[r0 - b0:r1 - b0])
        assert flagged.any() and not flagged.all()
        assert np.array_equal(mask[r0:r1], flagged.astype(np.uint8)), r0
        assert np.array_equal(got[r0:r1], want), (r0, parity_stats(got[r0:r1], want))


# ---- 8. no side effects ----------------------------------------------------------
def test_other_renders_are_unaffected(gpu_ctx, shipped):
    w, h, depth = 96, 54, 1
    view = rt.make_view(None, 0.7)

    def frame_and_sums():
        acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        rt.render_accumulate(gpu_ctx, shipped, acc.data_ptr(), w, h, depth, 2, 0, seed=5, view=view)
        torch.cuda.synchronize()
        return rt.render(gpu_ctx, shipped, w, h, depth, view=view), acc.cpu().numpy()

    before = frame_and_sums()
    for d in (0, 1, 2):
        rt.render_aa(gpu_ctx, shipped, w, h, d, 2, 0.1, view=view)
    after = frame_and_sums()
    for k in range(2):
        assert before[k].tobytes() == after[k].tobytes(), k


# ---- 9. the command-line tool ---------------------------------------------------
def _read_pfm(path, w, h):
    data = open(path, "rb").read()
    header = b"PF\n%d %d\n-1.0\n" % (w, h)
    assert data.startswith(header), data[:32]
    return np.frombuffer(data[len(header):], "<f4").reshape(h, w, 3)  # rows bottom-up: row 0 first


def test_cli_aa(gpu_ctx, tmp_path):
    w, h = 96, 54
    cli = os.path.join(ROOT, "openglraytracer_amd", "rt_cli")
    pfm = str(tmp_path / "aa.pfm")
    common = [cli, "--width", str(w), "--height", str(h), "--time", "0.7"]
    r = subprocess.run(common + ["--aa", "4:0.25", "--pfm", pfm], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sc = rt.Scene(gpu_ctx, rt.reference_objects(0.7))
    try:
        want, mask = rt.render_aa(gpu_ctx, sc, w, h, 0, 4, 0.25, time=0.7, want_mask=True)
        assert np.array_equal(_read_pfm(pfm, w, h), want[..., :3])
        assert "%d of %d pixels supersampled" % (int(mask.sum()), w * h) in r.stdout, r.stdout
        # the threshold defaults to 0.1
        r = subprocess.run(common + ["--aa", "2", "--pfm", pfm], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(_read_pfm(pfm, w, h), rt.render_aa(gpu_ctx, sc, w, h, 0, 2, 0.1, time=0.7)[..., :3])
    finally:
        sc.close()
    # one GPU only, and a well-formed value
    for extra in (["--aa", "4", "--gpus", "2"], ["--aa", "0"], ["--aa", "x"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (extra, r.stderr)
