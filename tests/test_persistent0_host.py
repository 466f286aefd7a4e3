"""Which depth-0 launches take the persistent distribution (rt_internal.h
kLaunchPersistent) is decided on the host from the launch parameters and the
kernel's resident work-groups alone (rt_kernel.hip persistent_groups, through
the host-only rt_debug_launch_shape_n): a plain batch of more than 8 views of
one scene in its scene's shape, views and records in device memory, a
queue-counter slot, a wave for every queue and, in automatic mode, at least
192 wave tiles per resident wave. Everything else keeps one work-group per tile."""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd import abi

PLAIN, PERSISTENT = 1, 2  # rt_internal.h kLaunchPlain, kLaunchPersistent
RESIDENT = 2048           # work-groups: 8 per CU on 256 CUs, 8,192 waves
# rt_debug_launch_shape_n's 23 fields: a 1920 x 1080 frame of 33 frame
# constants, 64 views in the device buffer (64 x 32,400 wave tiles)
BASE = dict(max_depth=0, option=1, width=1920, height=1080, row_begin=0, n_rows=1080, block_rows=0, n_shards=0,
            shard=0, out_format=abi.RT_OUTPUT_RGBA32F, n_frame_consts=33, cam_short=1, slice_begin=0, slice_rows=0,
            spp=0, n_views=64, dev_views=1, view_blobs=0, sched=1, persistent0=1, resident=RESIDENT, all_cull=1,
            mask_bytes=2)
SMALL = dict(width=72, height=40, n_rows=40)  # 45 wave tiles per view


def _shape(**kw):
    f = rt.lib().rt_debug_launch_shape_n
    f.argtypes = [C.c_void_p, C.c_int]
    f.restype = C.c_int
    fields = dict(BASE, **kw)
    assert list(fields) == list(BASE)
    a = np.array(list(fields.values()), np.int32)
    return f(a.ctypes.data, len(a))


@pytest.mark.parametrize("kw", [
    {}, dict(n_views=256), dict(mask_bytes=4), dict(mask_bytes=8),
    dict(SMALL, persistent0=8), dict(SMALL, persistent0=9),   # forced: the tile threshold does not apply
    dict(SMALL, persistent0=8, width=33, height=17, n_rows=17),  # 135 tiles, 17 chunks, 32 waves
    dict(persistent0=4096),                                    # a cap above the resident grid
    dict(resident=8),                                          # 32 waves: a wave per queue
])
def test_plain_device_view_batches_of_one_scene_are_persistent(kw):
    assert _shape(**kw) == PLAIN | PERSISTENT


@pytest.mark.parametrize("kw", [
    dict(n_views=8, dev_views=0), dict(n_views=1, dev_views=0), dict(n_views=8),  # views in the kernel arguments
    dict(dev_views=0),
    dict(view_blobs=1),                                        # rt_render_batch_scenes with distinct blobs
    dict(all_cull=0),                                          # a view with culling off: the general kernel
    dict(mask_bytes=0),                                        # no LDS masks: the general kernel
    dict(persistent0=0),                                       # RT_OPT_PERSISTENT0 0
    dict(sched=0),                                             # no queue counters
    dict(SMALL), dict(SMALL, n_views=256),                     # automatic, below 192 tiles per resident wave
    dict(n_views=9), dict(n_views=48),
    dict(resident=7), dict(persistent0=8, resident=7),         # 28 waves: a queue without a wave
    dict(SMALL, persistent0=8, resident=7),
])
def test_every_other_plain_launch_stays_tiled(kw):
    assert _shape(**kw) == PLAIN


def test_automatic_threshold_is_192_tiles_per_resident_wave():
    # 1,572,864 wave tiles at 8,192 resident waves: 48 views of 240 x 135 tiles (1,555,200) below,
    # 49 (1,587,600) above; with 32 resident waves (8 work-groups) 6,144: 9 views of 40 x 17 (6,120), 40 x 18 (6,480)
    assert _shape(n_views=48) == PLAIN
    assert _shape(n_views=49) == PLAIN | PERSISTENT
    assert _shape(n_views=9, resident=8, width=320, height=136, n_rows=136) == PLAIN
    assert _shape(n_views=9, resident=8, width=320, height=144, n_rows=144) == PLAIN | PERSISTENT


@pytest.mark.parametrize("kw", [
    dict(option=0),                                            # RT_OPT_LAUNCH_SHAPES 0
    dict(out_format=abi.RT_OUTPUT_RGBA8), dict(out_format=abi.RT_OUTPUT_RGB32F),
    dict(block_rows=8, n_shards=3, shard=1, n_rows=360),       # a sharded batch
    dict(row_begin=8, n_rows=1072), dict(n_rows=1079),         # a band of rows
    dict(n_frame_consts=0), dict(cam_short=0), dict(spp=1), dict(max_depth=1), dict(max_depth=2),
])
@pytest.mark.parametrize("persistent0", [1, 8])
def test_launches_that_are_not_plain_are_never_persistent(kw, persistent0):
    assert _shape(persistent0=persistent0, **kw) == 0


def test_the_15_field_hook_never_reports_persistence():
    f = rt.lib().rt_debug_launch_shape
    f.argtypes = [C.c_void_p]
    f.restype = C.c_int
    a = np.array(list(BASE.values())[:15], np.int32)
    assert f(a.ctypes.data) == PLAIN
