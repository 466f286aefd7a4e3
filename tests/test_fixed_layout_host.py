"""The layout classes of the LDS-mask scenes (rt_internal.h fixed_layout;
build_scene, scene_shape), on the host: a scene inside its class's maxima
(one box or 2..4, at most 7 materials and 3 lights: the reference tables'
sizes) whose mask texels the padding does not change is staged at the class's
offsets and its depth-0 shape carries kShapeFixed, unless RT_OPT_FIXED_LAYOUT
is 0; every other scene keeps the compact layout, its 12-texel masks and its
shape value.

Config 2's scene, 20, 40 and 44 spheres, the shipped scene: read through the
host-only hooks rt_debug_fixed_layout and rt_debug_scene_blob.
"""
import ctypes as C
import os
import subprocess

import pytest

import openglraytracer_amd as rt
from anim_spheres_common import host_scene_blob
from oracle import scenes
from openglraytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED, ROOM = 64, 16
OFFSETS = ("off_spheres", "off_smeta", "off_boxes", "off_mats", "off_lights", "off_lightmat", "off_dmask")
MAX_LIGHTS, MAX_MATS, MAX_BOXES = 3, 7, 4


def hook(objs, mats, lights):
    """rt_debug_fixed_layout's 12 ints and rt_debug_scene_blob's meta."""
    f = rt.lib().rt_debug_fixed_layout
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    f.restype = C.c_int
    oa, ma, la = (rt.Object * len(objs))(*objs), (rt.Material * len(mats))(*mats), (rt.Light * len(lights))(*lights)
    out = (C.c_int32 * 12)()
    assert f(oa, len(objs), ma, len(mats), la, len(lights), out) == 0, rt.lib().rt_last_error()
    _, meta = host_scene_blob(objs, mats, lights)
    return list(out), meta


def compact_offsets(meta):
    """The tables back to back in the compact order: spheres, their meta
    records, boxes (12 units each), materials (4), lights (1), light x
    material records (3)."""
    ns, nb, nm, nl = meta["n_spheres"], meta["n_boxes"], meta["n_mats"], meta["n_lights"]
    sizes = [ns, ns, 12 * nb, 4 * nm, nl, 3 * nm * nl]
    return [sum(sizes[:k]) for k in range(len(sizes))]


def class_offsets(meta):
    """fixed_layout written out again: boxes, materials, lights and light x
    material records padded to the maxima, then the spheres, their meta
    records and the masks."""
    boxes = 1 if meta["n_boxes"] == 1 else MAX_BOXES
    off_mats = 12 * boxes
    off_lights = off_mats + 4 * MAX_MATS
    off_lm = off_lights + MAX_LIGHTS
    off_sph = off_lm + 3 * MAX_MATS * MAX_LIGHTS
    ns = meta["n_spheres"]
    return {"off_spheres": off_sph, "off_smeta": off_sph + ns, "off_boxes": 0, "off_mats": off_mats,
            "off_lights": off_lights, "off_lightmat": off_lm, "off_dmask": off_sph + 2 * ns}


def small_boxes(n):
    return [scenes.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (2.0 * k - 3.0, -4.0, 1.5 * k), (0.0, 30.0 * k, 0.0), k % 7)
            for k in range(n)]


def tables():
    return list(rt.reference_materials()), list(rt.reference_lights())


def in_class_scenes():
    mats, lights = tables()
    return {
        "config2": (scenes.CONFIGS["config2"][0](), mats, lights, 2 | ROOM),  # 7 materials, 3 lights: both maxima
        "room20": (scenes.bench_objects(20, seed=20), mats, lights, 4 | ROOM),
        "room40": (scenes.bench_objects(40, seed=40), mats, lights, 8 | ROOM),
        "shipped": (rt.reference_objects(0.0), mats, lights, 2),  # 4 boxes: the maximum
        "room12+1box": (scenes.bench_objects(12, seed=12) + small_boxes(1), mats, lights, 2),  # 2 boxes
        "room16, 2 lights, 5 materials": (_remap(scenes.bench_objects(16, seed=16), 2), mats[2:], lights[:2], 2 | ROOM),
    }


def _remap(objs, drop):
    for o in objs:
        o.material = max(o.material - drop, 0)
    return objs


def out_of_class_scenes():
    mats, lights = tables()
    extra = rt.Light.from_buffer_copy(lights[1])
    extra.position[0] += 1.0
    return {
        "4 lights": (scenes.bench_objects(8, seed=8), mats, lights + [extra], 2 | ROOM),
        "8 materials": (scenes.bench_objects(16, seed=16), mats + [mats[0]], lights, 2 | ROOM),
        "5 boxes": (scenes.bench_objects(8, seed=8) + small_boxes(4), mats, lights, 2),
        # 44 spheres, 6 materials: with the seventh material's 13 units of
        # padding the 12-texel masks no longer fit kMaskLdsBudget (the same
        # scene with 7 materials has 8-texel masks)
        "room44, 6 materials": (_remap(scenes.bench_objects(44, seed=44), 1), mats[1:], lights, 8 | ROOM),
    }


@pytest.mark.parametrize("name", sorted(in_class_scenes()))
def test_in_class_scene_takes_its_class_layout(name):
    objs, mats, lights, shape = in_class_scenes()[name]
    out, meta = hook(objs, mats, lights)
    want = class_offsets(meta)
    assert {k: meta[k] for k in OFFSETS} == want
    assert dict(zip(OFFSETS, out[5:12])) == want  # (the kernels' constexpr function says the same)
    assert out[0] == 1 and meta["dmask_n"] == out[3] == 12
    assert out[1] == shape | FIXED and out[2] == shape  # the bit, and gone with the option at 0
    # the planes right before the BVH, the BVH and its links behind the masks
    assert meta["off_dmask"] < meta["off_bvh"] <= meta["off_blink"] <= meta["blob_units"] == out[4]


@pytest.mark.parametrize("name", sorted(out_of_class_scenes()))
def test_scene_outside_a_class_keeps_the_compact_layout(name):
    objs, mats, lights, shape = out_of_class_scenes()[name]
    out, meta = hook(objs, mats, lights)
    assert [meta[k] for k in OFFSETS[:6]] == compact_offsets(meta)
    assert meta["off_dmask"] > meta["off_blink"] >= meta["off_bvh"]  # the masks last, as before
    assert out[0] == 0 and meta["dmask_n"] == 12
    assert out[1] == out[2] == shape


def test_budget_scene_would_lose_its_texels_padded():
    """The scene the budget rule is about: with all 7 materials (its padded
    size) 44 spheres have 8-texel masks, so the 6-material scene must stay
    compact to keep its 12."""
    mats, lights = tables()
    _, meta = hook(scenes.bench_objects(44, seed=44), mats, lights)
    assert meta["dmask_n"] == 8


def test_config2_blob_does_not_grow():
    """Config 2's scene sits at both maxima with one box: no padding, 382
    units (6,112 B) staged as before."""
    objs, mats, lights, _ = in_class_scenes()["config2"]
    _, meta = hook(objs, mats, lights)
    assert meta["blob_units"] == 382


def test_frames_of_an_animated_scene_share_their_layout():
    """Two frames of the shipped animation (boxes moving) and of config 2's
    scene with a sphere moved: equal offsets, both the class's."""
    mats, lights = tables()
    a = hook(rt.reference_objects(0.0), mats, lights)[1]
    b = hook(rt.reference_objects(1.7), mats, lights)[1]
    assert a == b and {k: a[k] for k in OFFSETS} == class_offsets(a)
    moved = scenes.CONFIGS["config2"][0]()
    sphere = next(o for o in moved if o.radius != 0.0)
    sphere.position[0] += 0.25
    c = hook(scenes.CONFIGS["config2"][0](), mats, lights)[1]
    d = hook(moved, mats, lights)[1]
    assert {k: c[k] for k in OFFSETS} == {k: d[k] for k in OFFSETS} == class_offsets(c)


def test_option_constant():
    assert abi.RT_OPT_FIXED_LAYOUT == 11


def test_layout_classes_under_address_and_ub_sanitizers():
    """tools/asan/fixed_layout_driver.cpp, a program of its own: the host
    sources with -fsanitize=address,undefined (host only) building these
    scenes; any report aborts the run."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "openglraytracer_amd", "csrc"), "asan-fixed-layout"],
                       capture_output=True, text=True, timeout=580)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "clean" in r.stdout
