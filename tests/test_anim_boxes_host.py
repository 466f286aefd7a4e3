"""The animate kernel's box phases on the host (no GPU needed):
rt_debug_anim_host_blob runs them in plain loops over the kernel's table
(anim_apply_boxes_host, the arithmetic of rt_cull.h) — records, light_inside,
separating planes, the boxes' mask bits — against the scene the host builds of
rt_animate_objects2(time), host against host, exact."""
import numpy as np
import pytest

import openglraytracer_amd as rt
from anim_spheres_common import (BOX_SCENES, BOX_TIMES, ON_LIGHT_TIME, Blob, box_planes, box_records, f32,
                                 host_scene_blob, objects_extent, scene_steady_extent)

NO_W = np.float32(-np.inf)


def blobs_at(scene, t):
    base, anim, radius, mats, lights = scene
    objs = rt.animate_objects(base, anim, t, radius)
    return objs, host_scene_blob(objs, mats, lights), rt.anim_host_blob(base, anim, radius, mats, lights, t)


@pytest.mark.parametrize("name", list(BOX_SCENES))
def test_records_and_mask_bits_equal_the_host_built_scene(name):
    scene = BOX_SCENES[name]()
    inside = 0
    for t in BOX_TIMES:
        objs, (hbuf, hmeta), (buf, meta) = blobs_at(scene, t)
        got, host = box_records(buf, meta), box_records(hbuf, hmeta)
        assert len(got) == len(host) > 0
        for field in got.dtype.names:  # (every byte of the records: light_inside, translate_only, the padding)
            assert np.array_equal(got[field], host[field]), (name, t, field, got[field], host[field])
        inside |= int(np.bitwise_or.reduce(host["light_inside"]))
        g, h = Blob(buf, meta), Blob(hbuf, hmeta)
        assert (g.masks is None) == (h.masks is None) == (name == "two_boxes"), (name, t)
        if g.masks is not None:
            # by obj_index: the boxes' bits, and the spheres' as the sphere phases left them
            a, b = g.mask_bits_by_object(len(objs)), h.mask_bits_by_object(len(objs))
            assert np.array_equal(a, b), (name, t, np.argwhere(a != b)[:20])
            boxes_have_bits = a[:, list(g.box_obj)].any()
            assert boxes_have_bits == (name in ("shipped", "boxes_spheres")), (name, t)
    if name in ("two_boxes", "box_spheres"):
        # the box whose centre sits on a light at ON_LIGHT_TIME holds it there, and not at every time
        on, off = (box_records(*blobs_at(scene, t)[2])[0]["light_inside"] for t in (ON_LIGHT_TIME, 7.3))
        assert on != 0 and on != off, (name, on, off)
    assert inside != 0 or name == "boxes_spheres", name


def test_enough_box_mask_bits_for_the_device_comparison():
    """test_gpu_anim.py compares the boxes' bits of boxes_spheres at 3 times
    under a cap of 1 in 100,000: the layout gives it at least 10^4 bits."""
    base, anim, radius, mats, lights = BOX_SCENES["boxes_spheres"]()
    buf, meta = rt.anim_host_blob(base, anim, radius, mats, lights, 0.0)
    assert 3 * len(Blob(buf, meta).masks) * len(box_records(buf, meta)) >= 10000


def check_planes(got, host, what):
    """What follows from the text (rt_cull.h, box_light_plane) when the hook's
    extent, the plan's bound over the supported times, is no smaller than the
    host-built scene's: a plane the hook keeps is kept by the host-built
    scene, with a bit-equal normal and a w no smaller than the hook's."""
    gw, hw = f32(got[..., 3]), f32(host[..., 3])
    kept = gw > NO_W
    assert (hw[kept] > NO_W).all(), what
    assert np.array_equal(got[..., :3][kept], host[..., :3][kept]), what
    assert (gw[kept] <= hw[kept]).all(), what
    assert np.array_equal(got[~kept], np.broadcast_to(np.array([0, 0, 0, 0xFF800000], "<u4"), got[~kept].shape)), what
    return int(kept.sum())


@pytest.mark.parametrize("name", list(BOX_SCENES))
def test_planes_are_the_host_built_scenes_or_more_conservative(name):
    scene = BOX_SCENES[name]()
    kept = 0
    for t in BOX_TIMES:
        _, (hbuf, hmeta), (buf, meta) = blobs_at(scene, t)
        got, host = box_planes(buf, meta), box_planes(hbuf, hmeta)
        assert (got is None) == (host is None) == (name == "box_spheres"), (name, t)
        if got is not None:
            kept += check_planes(got, host, (name, t))
    assert (kept > 0) == (name != "box_spheres"), (name, kept)


def test_planes_where_the_extents_agree():
    """No channel grows and a static box far out sets the extent: the bound
    over all times and the extent at each time are then the same number
    (asserted). The plan's extent is never that number itself but that number
    times the 1 + 1e-6 of slack anim_plan gives every bound, so the two sides'
    margins differ by d = 1e-5 * 1e-6 * extent < 1e-9. The same face is chosen
    (the choice does not look at the extent), the normals are bit-equal, and
    the two w, float32 roundings of two float64 numbers d apart, lie within
    d plus one float32 step of each other — the hook's never above the host's."""
    base, anim, radius, mats, lights = scene = scene_steady_extent()
    bound = objects_extent(base[2:])  # the static box alone
    kept = 0
    for t in BOX_TIMES:
        objs, (hbuf, hmeta), (buf, meta) = blobs_at(scene, t)
        assert objects_extent(objs) == bound == max(objects_extent(objs[:2]) * 1.5, bound), t
        got, host = box_planes(buf, meta), box_planes(hbuf, hmeta)
        assert got.shape == (3, 2, 4)
        k = check_planes(got, host, t)
        gw, hw = f32(got[..., 3]), f32(host[..., 3])
        on = gw > NO_W
        d = 1e-5 * 1e-6 * bound * (1.0 + 1e-9)
        step = np.spacing(np.maximum(np.abs(gw[on]), np.abs(hw[on]))).astype(np.float64)
        assert d < 1e-9 and (hw[on].astype(np.float64) - gw[on] <= d + step).all(), (t, gw, hw)
        kept += k
    assert kept >= 10, kept
