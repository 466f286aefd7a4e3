"""Scenes as functions of time, host side (no GPU needed): the channel form of
the shipped scene's animation (include/rt.h, rt_object_anim), its host
evaluation, the error returns and the ABI."""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from openglraytracer_amd.abi import AnimChannel, Object, ObjectAnim, to_numpy

F = np.float32


def raw(objs):
    return to_numpy((Object * len(objs))(*objs)).tobytes()


def test_abi_every_new_symbol_loads_and_layouts_match():
    lib = rt.lib()
    for name in ("rt_reference_animation", "rt_animate_objects", "rt_anim_create", "rt_anim_destroy",
                 "rt_render_animated", "rt_render_batch_animated", "rt_debug_anim_blob"):
        assert hasattr(lib, name), name
    assert C.sizeof(AnimChannel) == 16
    assert C.sizeof(ObjectAnim) == 7 * 16
    assert (abi.RT_ANIM_NONE, abi.RT_ANIM_RATE, abi.RT_ANIM_RATE_OFFSET, abi.RT_ANIM_SIN,
            abi.RT_ANIM_SIN_OFFSET) == (0, 1, 2, 3, 4)


def test_reference_animation_equals_reference_objects_byte_for_byte():
    """rt_animate_objects(rt_reference_animation(), t) == rt_reference_objects(t)
    at 2,000 times in [-1e4, 1e4], the fixtures' times and both zeros among them."""
    base, anim = rt.reference_animation()
    rng = np.random.default_rng(20261019)
    times = np.concatenate([np.array([0.0, -0.0, 3.7, 11.25, 1e4, -1e4], F),
                            rng.uniform(-1e4, 1e4, 1000).astype(F),
                            rng.uniform(-20.0, 20.0, 994).astype(F)])
    assert len(times) == 2000
    for t in times:
        got, want = raw(rt.animate_objects(base, anim, float(t))), raw(rt.reference_objects(float(t)))
        assert got == want, float(t)


def test_zero_description_returns_the_base():
    base = rt.bench_objects(16, 3) + rt.reference_objects(2.5)
    anim = [ObjectAnim() for _ in base]
    for t in (0.0, -7.5, 1234.5):
        assert raw(rt.animate_objects(base, anim, t)) == raw(base)


def gl_sin_of_time_times_k(t):
    """gl_sin(t * k) for k = 0.4f * 3.0f, through the library's own reference
    scene: object 1's z position (rt_reference_objects, rt_scene.cpp)."""
    return F(rt.reference_objects(float(t))[1].position[2])


@pytest.mark.parametrize("t", [0.0, -0.0, 0.37, 3.7, -11.25, 812.0625])
def test_each_channel_kind_is_its_written_float32_expression(t):
    t = F(t)
    k = F(F(0.4) * F(3.0))
    s = gl_sin_of_time_times_k(t)
    a, c = F(2.75), F(-1.3)
    base = Object()
    base.box_mins[:] = [-1.0, -2.0, -3.0]
    base.box_maxs[:] = [1.5, 2.5, 3.5]
    base.radius = -1.0
    base.position[:] = [0.25, -4.0, 9.0]
    base.angles[:] = [10.0, 20.0, 30.0]
    want = {abi.RT_ANIM_NONE: None, abi.RT_ANIM_RATE: F(t * k), abi.RT_ANIM_RATE_OFFSET: F(c + F(t * k)),
            abi.RT_ANIM_SIN: F(s * a), abi.RT_ANIM_SIN_OFFSET: F(F(a * s) + c)}
    for kind, w in want.items():
        for field in ("position", "angles"):
            for i in range(3):
                an = ObjectAnim()
                getattr(an, field)[i] = AnimChannel(kind, a, k, c)
                o = rt.animate_objects([base], [an], float(t))[0]
                exp = Object.from_buffer_copy(base)
                if w is not None:
                    getattr(exp, field)[i] = w
                assert raw([o]) == raw([exp]), (kind, field, i)
        an = ObjectAnim()
        an.scale = AnimChannel(kind, a, k, c)
        o = rt.animate_objects([base], [an], float(t))[0]
        exp = Object.from_buffer_copy(base)
        if w is not None:
            for i in range(3):
                exp.box_mins[i] = F(F(base.box_mins[i]) * w)
                exp.box_maxs[i] = F(F(base.box_maxs[i]) * w)
        assert raw([o]) == raw([exp]), (kind, "scale")


def test_forms_are_kept_apart_for_negative_zero():
    """c + x with c = 0 and x = -0 is +0; the plain RATE form keeps -0."""
    base = Object()
    an = ObjectAnim()
    an.position[0] = AnimChannel(abi.RT_ANIM_RATE, 0.0, 1.0, 0.0)
    an.position[1] = AnimChannel(abi.RT_ANIM_RATE_OFFSET, 0.0, 1.0, 0.0)
    o = rt.animate_objects([base], [an], -0.0)[0]
    assert np.signbit(F(o.position[0])) and not np.signbit(F(o.position[1]))


def test_error_returns_without_a_gpu():
    lib = rt.lib()
    base, anim = rt.reference_animation()
    b, a, out = (Object * 5)(*base), (ObjectAnim * 5)(*anim), (Object * 5)()
    assert lib.rt_animate_objects(None, a, 5, 0.0, out) == abi.RT_ERR_INVALID
    assert lib.rt_animate_objects(b, None, 5, 0.0, out) == abi.RT_ERR_INVALID
    assert lib.rt_animate_objects(b, a, 5, 0.0, None) == abi.RT_ERR_INVALID
    assert lib.rt_animate_objects(b, a, -1, 0.0, out) == abi.RT_ERR_INVALID
    for bad in (5, -1, 1 << 20):
        a2 = (ObjectAnim * 5)(*anim)
        a2[3].angles[2].kind = bad
        assert lib.rt_animate_objects(b, a2, 5, 0.0, out) == abi.RT_ERR_INVALID
        assert b"kind" in lib.rt_last_error()
    assert lib.rt_reference_animation(None, a) == abi.RT_ERR_INVALID
    assert lib.rt_reference_animation(b, None) == abi.RT_ERR_INVALID
    h = C.c_void_p()
    mats, lts = (abi.Material * 7)(*rt.reference_materials()), (abi.Light * 3)(*rt.reference_lights())
    assert lib.rt_anim_create(None, b, a, 5, mats, 7, lts, 3, 1, C.byref(h)) == abi.RT_ERR_INVALID
    assert lib.rt_anim_create(None, b, a, 5, mats, 7, lts, 3, 1, None) == abi.RT_ERR_INVALID
    buf = np.zeros(16, F)
    assert lib.rt_render_animated(None, None, None, 0.0, 2, 2, 0, 0, 2, buf.ctypes.data, 0, None) == abi.RT_ERR_INVALID
    t = (C.c_float * 1)(0.0)
    assert lib.rt_render_batch_animated(None, None, None, t, 1, 2, 2, 0, 8, 1, 0, buf.ctypes.data,
                                        None) == abi.RT_ERR_INVALID
    lib.rt_anim_destroy(None)  # a no-op
