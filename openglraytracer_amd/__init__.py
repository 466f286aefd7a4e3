"""MI355X-native per-pixel ray tracer — host-side Python front-end of the C-ABI.

The hot path (raytrace_compute.glsl of blubs/OpenGLRaytracer) runs as a HIP
kernel in libopenglraytracer_amd.so (built in-tree by `make -C
openglraytracer_amd/csrc`, or __graft_entry__.build()). This module is a thin
ctypes binding of include/rt.h mirroring the reference's frame driver
(OpenGLRaytracer/main.cpp:219-238): build a scene, pick `time`, render a
W x H frame into a float RGBA surface.

There is no CPU fallback: if the library is missing, or no GPU is present,
every render call raises.
"""
import ctypes as C
import os

import numpy as np

from .abi import (RT_MAX_DEPTH, RT_OK, Camera, Light, Material, Object)  # noqa: F401
from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libopenglraytracer_amd.so")
_lib = None


class RTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rt error %d: %s" % (code, msg))
        self.code = code


class View(C.Structure):
    """rt_view: column-major inverse(proj*view) + ray origin (include/rt.h)."""
    _fields_ = [("unprojection", C.c_float * 16), ("origin", C.c_float * 3)]


def lib():
    """Load the HIP library (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libopenglraytracer_amd.so not built: run __graft_entry__.build() "
                               "or `make -C openglraytracer_amd/csrc`")
        # One HIP runtime per process: PyTorch-ROCm bundles its own
        # libamdhip64 (loaded by `import torch` under the unversioned name),
        # while this library links the SONAME libamdhip64.so.7. Importing torch
        # first lets the dynamic linker bind this library to torch's runtime,
        # so device pointers, streams and RCCL are shared; the other order
        # would load two runtimes and torch would find no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        sig = {
            "rt_reference_materials": ([vp], i), "rt_reference_lights": ([vp], i),
            "rt_reference_objects": ([f, vp], i), "rt_reference_camera": ([f, vp], i),
            "rt_bench_objects": ([i, C.c_uint64, vp], i), "rt_make_view": ([vp, f, vp], i),
            "rt_object_transforms": ([vp, vp, vp, vp], i),
            "rt_create": ([i, vp], i), "rt_destroy": ([vp], None),
            "rt_scene_create": ([vp, vp, i, vp, i, vp, i, vp], i), "rt_scene_destroy": ([vp], None),
            "rt_scene_update": ([vp, vp, vp, i, vp, i, vp, i], i),
            "rt_render": ([vp, vp, vp, f, i, i, i, i, i, vp, i, vp], i),
            "rt_render_view": ([vp, vp, vp, i, i, i, i, i, vp, i, vp], i),
            "rt_shard_rows": ([i, i, i, i], i),
            "rt_render_shard": ([vp, vp, vp, i, i, i, i, i, i, vp, vp], i),
            "rt_last_kernel_ms": ([vp, C.POINTER(C.c_float)], i),
            "rt_context_set": ([vp, i, i], i),
            "rt_render_batch": ([vp, vp, vp, i, i, i, i, i, i, i, vp, vp], i),
            "rt_batch_launches": ([vp, vp, i, i], i),
            "rt_render_batch_scenes": ([vp, vp, vp, i, i, i, i, i, i, i, vp, vp], i),
            "rt_render_accumulate": ([vp, vp, vp, i, i, i, i, i, C.c_uint32, i, i, i, vp, vp], i),
            "rt_pack_rgba8": ([vp, C.c_size_t, vp], i),
            "rt_write_ppm": ([C.c_char_p, vp, i, i], i), "rt_write_pfm": ([C.c_char_p, vp, i, i], i),
            "rt_last_error": ([], C.c_char_p), "rt_version": ([], C.c_char_p),
            "rt_scene_desc_parse": ([C.c_char_p, f, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp], i),
            "rt_multi_create": ([i, vp, i, vp], i), "rt_multi_destroy": ([vp], None),
            "rt_render_multi": ([vp, vp, vp, f, i, i, i, i, vp, i], i),
            "rt_render_multi_view": ([vp, vp, vp, i, i, i, i, vp, i], i),
            "rt_multi_last_ms": ([vp, vp, vp, vp], i),
            "rt_reference_animation": ([vp, vp], i), "rt_animate_objects": ([vp, vp, i, f, vp], i),
            "rt_anim_create": ([vp, vp, vp, i, vp, i, vp, i, i, vp], i), "rt_anim_destroy": ([vp], None),
            "rt_render_animated": ([vp, vp, vp, f, i, i, i, i, i, vp, i, vp], i),
            "rt_render_batch_animated": ([vp, vp, vp, vp, i, i, i, i, i, i, i, vp, vp], i),
            "rt_debug_anim_blob": ([vp, f, vp, C.c_longlong], C.c_longlong),
            "rt_animate_objects2": ([vp, vp, vp, i, f, vp], i),
            "rt_anim_create2": ([vp, vp, vp, vp, i, vp, i, vp, i, i, vp], i),
            "rt_debug_anim_validate": ([vp, vp, vp, i, vp, i, vp, i, i, i], i),
            "rt_debug_anim_host_blob": ([vp, vp, vp, i, vp, i, vp, i, f, vp, C.c_longlong, vp], C.c_longlong),
            "rt_debug_select_kernel": ([vp, i, vp], i), "rt_debug_last_kernel": ([vp, vp], i),
            "rt_debug_norm_proof": ([vp, i, vp, i, vp, i, vp, i, i, vp, vp], i),
            "rt_render_hits_view": ([vp, vp, vp, i, i, i, i, i, vp, vp, vp, i, vp], i),
            "rt_render_hits": ([vp, vp, vp, f, i, i, i, i, i, vp, vp, vp, i, vp], i),
            "rt_render_hits_animated": ([vp, vp, vp, f, i, i, i, i, i, vp, vp, vp, i, vp], i),
            "rt_pick": ([vp, vp, vp, i, i, i, i, i, vp, vp, vp], i),
            "rt_render_aa_view": ([vp, vp, vp, i, i, i, i, C.c_uint32, f, vp, vp, i, vp], i),
            "rt_render_aa": ([vp, vp, vp, f, i, i, i, i, C.c_uint32, f, vp, vp, i, vp], i),
            "rt_aa_last_counts": ([vp, vp, vp], i),
            "rt_aa_edge_mask": ([vp, i, i, f, vp, vp], i),
            "rt_trace_rays": ([vp, vp, vp, C.c_int64, i, i, vp, vp, vp, vp, i, vp], i),
            "rt_view_rays": ([vp, vp, i, i, i, i, vp, i, vp], i),
            "rt_occluded": ([vp, vp, vp, C.c_int64, vp, vp, i, vp], i),
        }
        for name, (args, res) in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


def _check(rc):
    if rc != RT_OK:
        raise RTError(rc, lib().rt_last_error().decode())


# ---- reference scene / camera (raytrace_compute.glsl:74-364) ---------------
def reference_materials():
    m = (Material * 7)()
    _check(lib().rt_reference_materials(m))
    return list(m)


def reference_lights():
    ls = (Light * 3)()
    _check(lib().rt_reference_lights(ls))
    return list(ls)


def reference_objects(time=0.0):
    o = (Object * 5)()
    _check(lib().rt_reference_objects(time, o))
    return list(o)


def reference_camera(time=0.0):
    c = Camera()
    _check(lib().rt_reference_camera(time, C.byref(c)))
    return c


def reference_animation():
    """rt_reference_animation: the shipped scene as (base objects, channels)."""
    base = (Object * 5)()
    anim = (abi.ObjectAnim * 5)()
    _check(lib().rt_reference_animation(base, anim))
    return list(base), list(anim)


def animate_objects(base, anim, time, radius=None):
    """rt_animate_objects: the objects at `time` (host, float32 as written);
    with `radius` (an AnimChannel per object), rt_animate_objects2."""
    n = len(base)
    b = (Object * max(n, 1))(*base)
    a = (abi.ObjectAnim * max(n, 1))(*anim)
    out = (Object * max(n, 1))()
    if radius is None:
        _check(lib().rt_animate_objects(b, a, n, time, out))
    else:
        r = (abi.AnimChannel * max(n, 1))(*radius)
        _check(lib().rt_animate_objects2(b, a, r, n, time, out))
    return list(out[:n])


def _is_box(o):
    return any(x != 0.0 for x in list(o.box_mins) + list(o.box_maxs))


def _anim_args(base, anim, radius, materials, lights):
    materials = materials if materials is not None else reference_materials()
    lights = lights if lights is not None else reference_lights()
    objs = (Object * max(len(base), 1))(*base)
    an = (abi.ObjectAnim * max(len(anim), 1))(*anim)
    rad = (abi.AnimChannel * max(len(base), 1))(*radius) if radius is not None else None
    mats = (Material * len(materials))(*materials)
    lts = (Light * max(len(lights), 1))(*lights)
    return objs, an, rad, len(base), mats, len(materials), lts, len(lights)


def anim_validate(base, anim, radius=None, materials=None, lights=None, max_frames=1, boxes_only=False):
    """rt_debug_anim_validate (host only): the (code, message) rt_anim_create2
    — rt_anim_create with boxes_only — would return for this description."""
    rc = lib().rt_debug_anim_validate(*_anim_args(base, anim, radius, materials, lights), max_frames,
                                      1 if boxes_only else 0)
    return rc, (lib().rt_last_error().decode() if rc != RT_OK else "")


def anim_host_blob(base, anim, radius=None, materials=None, lights=None, time=0.0):
    """rt_debug_anim_host_blob (host only): (the slot blob at `time` as the
    host makes it with the animate kernel's functions, rt_debug_scene_blob's
    24 meta ints)."""
    args = _anim_args(base, anim, radius, materials, lights)
    meta = (C.c_int32 * 24)()
    n = lib().rt_debug_anim_host_blob(*args, time, None, 0, meta)
    if n < 0:
        raise RTError(int(n), lib().rt_last_error().decode())
    buf = np.zeros(int(n), np.uint8)
    n = lib().rt_debug_anim_host_blob(*args, time, buf.ctypes.data, buf.size, meta)
    if n < 0:
        raise RTError(int(n), lib().rt_last_error().decode())
    return buf, list(meta)


def select_kernel(fields):
    """rt_debug_select_kernel (host only): (the hook's return value, the key
    (depth, accum, dev, shape, launch) of the kernel a launch with these 26
    fields takes)."""
    f, key = (C.c_int32 * len(fields))(*fields), (C.c_int32 * 5)()
    return lib().rt_debug_select_kernel(f, len(fields), key), tuple(key)


def last_kernel(ctx):
    """rt_debug_last_kernel: (depth, accum, dev, shape, launch, queued) of the
    kernel the context's last launch ran."""
    out = (C.c_int32 * 6)()
    _check(lib().rt_debug_last_kernel(ctx.handle, out))
    return tuple(out)


def norm_proof(objects, view, width, height, materials=None, lights=None):
    """rt_debug_norm_proof (host only): ((scene half, view half, the build asks
    launches for the proofs), (B, e2, gap)) of the range proofs that let the
    room fast path take its inverse square roots without votes."""
    mats = materials if materials is not None else reference_materials()
    lights = lights if lights is not None else reference_lights()
    oa, ma, la = (Object * len(objects))(*objects), (Material * len(mats))(*mats), (Light * len(lights))(*lights)
    flags, terms = (C.c_int32 * 3)(), (C.c_double * 3)()
    _check(lib().rt_debug_norm_proof(oa, len(objects), ma, len(mats), la, len(lights), C.byref(view), width, height,
                                     flags, terms))
    return tuple(flags), tuple(terms)


def view_consts(objects, view, width, height, materials=None, lights=None):
    """rt_debug_view_consts (host only): (culling flag, [(object index, x0, x1,
    y0, y1) per sphere], [(object index, rx, ry, rz, inside) per box]) of the
    host's frame constants for `view`; no records for a scene too large for them."""
    mats = materials if materials is not None else reference_materials()
    lights = lights if lights is not None else reference_lights()
    oa, ma = (Object * max(len(objects), 1))(*objects), (Material * len(mats))(*mats)
    la = (Light * max(len(lights), 1))(*lights)
    n = 256  # rt_internal.h kMaxViewConsts
    head, sph, ids, cam = (C.c_int32 * 3)(), (C.c_int32 * (5 * n))(), (C.c_int32 * (2 * n))(), (C.c_float * (3 * n))()
    f = lib().rt_debug_view_consts
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    _check(f(oa, len(objects), ma, len(mats), la, len(lights), C.byref(view), width, height, head, sph, ids, cam))
    spheres = [tuple(sph[5 * s:5 * s + 5]) for s in range(head[1])]
    boxes = [(ids[2 * b], cam[3 * b], cam[3 * b + 1], cam[3 * b + 2], ids[2 * b + 1]) for b in range(head[2])]
    return head[0], spheres, boxes


def bench_objects(n_spheres, seed=0):
    o = (Object * (n_spheres + 1))()
    _check(lib().rt_bench_objects(n_spheres, seed, o))
    return list(o)


def parse_scene(text, time=0.0):
    """rt_scene_desc_parse: a JSON scene description -> (objects, materials,
    lights, camera or None) as ctypes records (format:
    openglraytracer_amd/csrc/rt_scene_json.cpp)."""
    objs = (Object * abi.RT_MAX_OBJECTS)()
    mats = (Material * abi.RT_MAX_MATERIALS)()
    lts = (Light * abi.RT_MAX_LIGHTS)()
    cam = Camera()
    no, nm, nl, hc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    data = text.encode() if isinstance(text, str) else bytes(text)
    _check(lib().rt_scene_desc_parse(data, time, objs, abi.RT_MAX_OBJECTS, C.byref(no), mats, abi.RT_MAX_MATERIALS,
                                     C.byref(nm), lts, abi.RT_MAX_LIGHTS, C.byref(nl), C.byref(cam), C.byref(hc)))
    return list(objs[:no.value]), list(mats[:nm.value]), list(lts[:nl.value]), (cam if hc.value else None)


def make_view(camera=None, time=0.0):
    v = View()
    _check(lib().rt_make_view(C.byref(camera) if camera is not None else None, time, C.byref(v)))
    return v


def view_from_matrix(unprojection, origin):
    """An explicit view: 16 column-major floats + 3-float origin."""
    v = View()
    v.unprojection[:] = [float(x) for x in np.asarray(unprojection, np.float32).reshape(-1)]
    v.origin[:] = [float(x) for x in np.asarray(origin, np.float32).reshape(-1)]
    return v


def shard_rows(height, block_rows, n_shards, shard):
    n = lib().rt_shard_rows(height, block_rows, n_shards, shard)
    if n < 0:
        raise RTError(n, "bad shard arguments")
    return n


def shard_row_ids(height, block_rows, n_shards, shard):
    """Frame rows owned by `shard`, in the order rt_render_shard packs them."""
    rows = np.arange(height)
    return rows[(rows // block_rows) % n_shards == shard]


def pack_rgba8(rgba):
    """GL_RGBA8 unorm packing of a float frame (the shipped surface)."""
    a = np.ascontiguousarray(rgba, np.float32)
    out = np.zeros(a.shape, np.uint8)
    _check(lib().rt_pack_rgba8(a.ctypes.data, a.size // 4, out.ctypes.data))
    return out


def write_ppm(path, rgba):
    """8-bit PPM of a frame (RGBA8 rounding, top row first)."""
    a = np.ascontiguousarray(rgba, np.float32)
    _check(lib().rt_write_ppm(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]))


def write_pfm(path, rgba):
    """Float PFM of a frame (bottom row first, little-endian)."""
    a = np.ascontiguousarray(rgba, np.float32)
    _check(lib().rt_write_pfm(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]))


class Context:
    """One device (rt_create). Not thread-safe, like a GL context."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().rt_create(device, C.byref(self._h)))
        self.device = device
        self.output = abi.RT_OUTPUT_RGBA32F  # RT_OPT_OUTPUT (set_output)

    def close(self):
        if self._h:
            lib().rt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_culling(self, on):
        """RT_OPT_CULLING: conservative sphere culling (output identical)."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_CULLING, 1 if on else 0))

    def set_timing(self, on):
        """RT_OPT_TIMING: HIP events around every launch (for last_kernel_ms)."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_TIMING, 1 if on else 0))

    def set_host_frame_consts(self, on):
        """RT_OPT_FRAME_CONSTS: per-frame constants from the host when they fit
        (default), else derived by every work-group (output identical)."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_FRAME_CONSTS, 1 if on else 0))

    def set_origin_lists(self, on):
        """RT_OPT_ORIGIN_LISTS: secondary rays leaving a sphere test its
        precomputed candidate list instead of walking the BVH (output identical)."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_ORIGIN_LISTS, 1 if on else 0))

    def set_scene_shapes(self, on):
        """RT_OPT_SCENE_SHAPES: a render whose scene has a common shape runs
        the kernel compiled for it (include/rt.h): at depth 0, LDS-mask scenes
        (the mask width as a constant); at depth >= 2 without Monte-Carlo,
        scenes with wide masks, their candidate lists and origin-sphere lists;
        each with or without the room (one translate-only box holding every
        live light). Output identical either way."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_SCENE_SHAPES, 1 if on else 0))

    def set_launch_shapes(self, on):
        """RT_OPT_LAUNCH_SHAPES: a whole-frame float4 depth-0 render of a
        shaped scene runs the kernel compiled for that launch shape too
        (include/rt.h). Output identical either way."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_LAUNCH_SHAPES, 1 if on else 0))

    def set_persistent0(self, value):
        """RT_OPT_PERSISTENT0: the distribution of a plain depth-0 batch of
        more than 8 views of one scene (include/rt.h). 1: the resident grid
        when the launch is large enough (default); 0: one work-group per
        tile; k >= 8: the resident grid of at most k work-groups whatever the
        launch's size. Output identical either way."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_PERSISTENT0, int(value)))

    def set_fixed_layout(self, on):
        """RT_OPT_FIXED_LAYOUT: a plain persistent launch of a scene staged
        in its layout class's fixed layout runs the kernel that takes the
        table offsets from the class (include/rt.h). Output identical either
        way."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_FIXED_LAYOUT, 1 if on else 0))

    def set_room_fast(self, on):
        """RT_OPT_ROOM_FAST: a plain depth-0 launch of a room scene inside
        the host's proof (identity matrices, cameras strictly inside) takes
        the primary box hit without the matrix products (include/rt.h).
        Output identical either way."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_ROOM_FAST, 1 if on else 0))

    def set_aa_queued(self, on):
        """RT_OPT_AA_QUEUED: render_aa's refine launch at depth 0-1 takes the
        live wave tiles from the edge kernel's lists on a resident grid (on,
        the default, as depths 2-9 always do), or runs one work-group per
        16 x 16 tile that leaves when none of its pixels is flagged. Output
        identical either way."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_AA_QUEUED, 1 if on else 0))

    def set_output(self, fmt):
        """RT_OPT_OUTPUT: abi.RT_OUTPUT_RGBA32F (float4 per pixel),
        abi.RT_OUTPUT_RGBA8 (the shipped GL_RGBA8 surface, 4 bytes per pixel)
        or abi.RT_OUTPUT_RGB32F (packed float3, the constant alpha dropped)."""
        _check(lib().rt_context_set(self._h, abi.RT_OPT_OUTPUT, fmt))
        self.output = fmt

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(lib().rt_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


class Scene:
    """Device-resident scene (rt_scene_create). Defaults: the reference's
    7 materials and 3 lights."""

    def __init__(self, ctx, objects, materials=None, lights=None):
        materials = materials if materials is not None else reference_materials()
        lights = lights if lights is not None else reference_lights()
        objs = (Object * max(len(objects), 1))(*objects)
        mats = (Material * len(materials))(*materials)
        lts = (Light * max(len(lights), 1))(*lights)
        self._h = C.c_void_p()
        _check(lib().rt_scene_create(ctx.handle, objs, len(objects), mats, len(materials), lts,
                                     len(lights), C.byref(self._h)))
        self.ctx = ctx

    def update(self, objects, materials=None, lights=None):
        """Replace the contents (rt_scene_update), e.g. the next animation frame."""
        materials = materials if materials is not None else reference_materials()
        lights = lights if lights is not None else reference_lights()
        objs = (Object * max(len(objects), 1))(*objects)
        mats = (Material * len(materials))(*materials)
        lts = (Light * max(len(lights), 1))(*lights)
        _check(lib().rt_scene_update(self.ctx.handle, self._h, objs, len(objects), mats, len(materials), lts,
                                     len(lights)))

    def close(self):
        if self._h:
            lib().rt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h


class Anim:
    """Device-resident animated scene (rt_anim_create): base objects and their
    channels; `max_frames` frames may be in flight at once. With `radius` (an
    AnimChannel per object), or a channel on an object that is not a box,
    rt_anim_create2: spheres move too. Defaults: the reference's 7 materials
    and 3 lights."""

    def __init__(self, ctx, base, anim, materials=None, lights=None, max_frames=1, radius=None):
        objs, an, rad, n, mats, nm, lts, nl = _anim_args(base, anim, radius, materials, lights)
        self._h = C.c_void_p()
        moving = [any(c.kind != abi.RT_ANIM_NONE for c in [a.scale] + list(a.position) + list(a.angles))
                  for a in anim]
        if radius is not None or any(m and not _is_box(o) for m, o in zip(moving, base)):
            _check(lib().rt_anim_create2(ctx.handle, objs, an, rad, n, mats, nm, lts, nl, max_frames,
                                         C.byref(self._h)))
        else:
            _check(lib().rt_anim_create(ctx.handle, objs, an, n, mats, nm, lts, nl, max_frames, C.byref(self._h)))
        self.ctx = ctx
        self.max_frames = max_frames

    def close(self):
        if self._h:
            lib().rt_anim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def debug_blob(self, time):
        """The slot blob the animate kernel leaves at `time` (bytes; a
        development hook, rt_debug_anim_blob)."""
        n = lib().rt_debug_anim_blob(self._h, time, None, 0)
        if n < 0:
            raise RTError(int(n), lib().rt_last_error().decode())
        buf = np.zeros(int(n), np.uint8)
        n = lib().rt_debug_anim_blob(self._h, time, buf.ctypes.data, buf.size)
        if n < 0:
            raise RTError(int(n), lib().rt_last_error().decode())
        return buf


def render_animated(ctx, anim, width, height, max_depth=0, time=0.0, camera=None, rows=None):
    """rt_render_animated to a host array, synchronously: the objects and (with
    camera None) the orbit camera at `time`."""
    r0, r1 = rows if rows is not None else (0, height)
    out = surface(ctx.output, max(r1 - r0, 1), max(width, 1))
    _check(lib().rt_render_animated(ctx.handle, anim.handle, C.byref(camera) if camera is not None else None, time,
                                    width, height, max_depth, r0, r1, out.ctypes.data, 0, None))
    return out[: r1 - r0, :width]


def render_animated_device(ctx, anim, out_ptr, width, height, max_depth=0, time=0.0, camera=None, rows=None,
                           stream=None):
    """rt_render_animated into device memory; asynchronous on `stream`."""
    r0, r1 = rows if rows is not None else (0, height)
    _check(lib().rt_render_animated(ctx.handle, anim.handle, C.byref(camera) if camera is not None else None, time,
                                    width, height, max_depth, r0, r1, C.c_void_p(out_ptr), 1,
                                    C.c_void_p(stream) if stream else None))


def render_batch_animated(ctx, anim, out_ptr, width, height, max_depth, times, views=None, block_rows=8, n_shards=1,
                          shard=0, stream=None):
    """K = len(times) animated frames (rt_render_batch_animated): frame k
    shows the objects at times[k] through views[k] (None: the orbit camera at
    times[k]), into device memory (K, rows, width, C)."""
    t = (C.c_float * len(times))(*[float(x) for x in times])
    arr = (View * len(views))(*views) if views is not None else None
    _check(lib().rt_render_batch_animated(ctx.handle, anim.handle, arr, t, len(times), width, height, max_depth,
                                          block_rows, n_shards, shard, C.c_void_p(out_ptr),
                                          C.c_void_p(stream) if stream else None))


def surface(fmt, *shape):
    """A zeroed host array for `shape` pixels in surface format `fmt`
    (RT_OPT_OUTPUT): float32 x4 (RGBA32F), float32 x3 (RGB32F) or uint8 x4
    (RGBA8)."""
    if fmt == abi.RT_OUTPUT_RGBA8:
        return np.zeros(shape + (4,), np.uint8)
    if fmt == abi.RT_OUTPUT_RGB32F:
        return np.zeros(shape + (3,), np.float32)
    return np.zeros(shape + (4,), np.float32)


def render(ctx, scene, width, height, max_depth=0, time=0.0, camera=None, view=None, rows=None):
    """Render rows [r0, r1) to a host array, synchronously (the reference's
    glDispatchCompute + glFinish): (r1-r0, width, C) in the context's surface
    format (ctx.set_output): float32 RGBA (default), float32 RGB or uint8
    RGBA."""
    r0, r1 = rows if rows is not None else (0, height)
    out = surface(ctx.output, max(r1 - r0, 1), max(width, 1))  # the C-ABI validates the range
    if view is None:
        view = make_view(camera, time)
    _check(lib().rt_render_view(ctx.handle, scene.handle, C.byref(view), width, height, max_depth,
                                r0, r1, out.ctypes.data, 0, None))
    return out[: r1 - r0, :width]


def render_rgba8(ctx, scene, width, height, max_depth=0, time=0.0, camera=None, view=None, rows=None):
    """Render rows [r0, r1) as the shipped app's GL_RGBA8 surface: a host
    array (r1-r0, width, 4) uint8, packed by the kernel's epilogue (equal to
    pack_rgba8 of the float frame)."""
    r0, r1 = rows if rows is not None else (0, height)
    out = np.zeros((max(r1 - r0, 1), max(width, 1), 4), np.uint8)
    if view is None:
        view = make_view(camera, time)
    prev = getattr(ctx, "output", abi.RT_OUTPUT_RGBA32F)
    ctx.set_output(abi.RT_OUTPUT_RGBA8)
    try:
        _check(lib().rt_render_view(ctx.handle, scene.handle, C.byref(view), width, height, max_depth,
                                    r0, r1, out.ctypes.data, 0, None))
    finally:
        ctx.set_output(prev)
    return out[: r1 - r0, :width]


def render_device(ctx, scene, out_ptr, width, height, max_depth=0, view=None, rows=None,
                  stream=None):
    """Render into device memory `out_ptr` (e.g. torch tensor.data_ptr()),
    laid out (rows, width, C) in the context's surface format; with `stream`
    (a hipStream_t as int) the call is asynchronous on that stream."""
    r0, r1 = rows if rows is not None else (0, height)
    if view is None:
        view = make_view(None, 0.0)
    _check(lib().rt_render_view(ctx.handle, scene.handle, C.byref(view), width, height, max_depth,
                                r0, r1, C.c_void_p(out_ptr), 1,
                                C.c_void_p(stream) if stream else None))


# ---- primary-hit buffers and picking (rt_render_hits*, rt_pick) -------------
HIT_PLANES = ("hits", "normals", "points")


def _hit_planes(planes, rows, width):
    """Host arrays for the requested planes, in HIT_PLANES' order (None: not wanted)."""
    unknown = [p for p in planes if p not in HIT_PLANES]
    if unknown or not planes:
        raise ValueError("planes: a non-empty choice of %s, not %r" % (HIT_PLANES, tuple(planes)))
    shape = (max(rows, 1), max(width, 1))
    return [None if name not in planes else
            (np.zeros(shape, abi.HIT_DTYPE) if name == "hits" else np.zeros(shape + (4,), np.float32))
            for name in HIT_PLANES]


def _plane_ptrs(arrays):
    return [C.c_void_p(a.ctypes.data) if a is not None else None for a in arrays]


def render_hits(ctx, scene, width, height, time=0.0, camera=None, view=None, rows=None, shadow=True,
                planes=HIT_PLANES):
    """rt_render_hits_view to host arrays, synchronously: for rows [r0, r1) the
    planes asked for, in the order of `planes` — "hits" (r1-r0, width) of
    abi.HIT_DTYPE (object, t, shadow, material), "normals" and "points"
    (r1-r0, width, 4) float32. shadow=False: no shadow rays, shadow = 0."""
    r0, r1 = rows if rows is not None else (0, height)
    arrays = _hit_planes(planes, r1 - r0, width)
    if view is None:
        view = make_view(camera, time)
    _check(lib().rt_render_hits_view(ctx.handle, scene.handle, C.byref(view), width, height, r0, r1,
                                     abi.RT_HITS_SHADOW if shadow else 0, *_plane_ptrs(arrays), 0, None))
    by_name = dict(zip(HIT_PLANES, arrays))
    return tuple(by_name[name][: r1 - r0, :width] for name in planes)


def render_hits_device(ctx, scene, width, height, hits_ptr=None, normals_ptr=None, points_ptr=None, view=None,
                       rows=None, shadow=True, stream=None):
    """rt_render_hits_view into device memory (e.g. torch tensors' data_ptr();
    16 bytes per pixel and plane, None: the plane is not wanted); with `stream`
    (a hipStream_t as int) the call is asynchronous on that stream."""
    r0, r1 = rows if rows is not None else (0, height)
    if view is None:
        view = make_view(None, 0.0)
    ptrs = [C.c_void_p(p) if p else None for p in (hits_ptr, normals_ptr, points_ptr)]
    _check(lib().rt_render_hits_view(ctx.handle, scene.handle, C.byref(view), width, height, r0, r1,
                                     abi.RT_HITS_SHADOW if shadow else 0, *ptrs, 1,
                                     C.c_void_p(stream) if stream else None))


def render_hits_animated(ctx, anim, width, height, time=0.0, camera=None, rows=None, shadow=True,
                         planes=HIT_PLANES):
    """rt_render_hits_animated to host arrays (render_hits' result): the objects
    and (with camera None) the orbit camera at `time`."""
    r0, r1 = rows if rows is not None else (0, height)
    arrays = _hit_planes(planes, r1 - r0, width)
    _check(lib().rt_render_hits_animated(ctx.handle, anim.handle, C.byref(camera) if camera is not None else None,
                                         time, width, height, r0, r1, abi.RT_HITS_SHADOW if shadow else 0,
                                         *_plane_ptrs(arrays), 0, None))
    by_name = dict(zip(HIT_PLANES, arrays))
    return tuple(by_name[name][: r1 - r0, :width] for name in planes)


def pick(ctx, scene, width, height, x, y, view=None, time=0.0, shadow=True):
    """rt_pick: pixel (x, y)'s records (y = 0: the bottom row) as (abi.Hit,
    normal (3,), point (3,)); view None: the orbit camera at `time`."""
    if view is None:
        view = make_view(None, time)
    hit = abi.Hit()
    normal, point = np.zeros(3, np.float32), np.zeros(3, np.float32)
    _check(lib().rt_pick(ctx.handle, scene.handle, C.byref(view), width, height, x, y,
                         abi.RT_HITS_SHADOW if shadow else 0, C.byref(hit), C.c_void_p(normal.ctypes.data),
                         C.c_void_p(point.ctypes.data)))
    return hit, normal, point


# ---- ray queries (rt_trace_rays, rt_view_rays) ------------------------------
RAY_PLANES = ("colors", "hits", "normals", "points")


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def trace_rays(ctx, scene, rays, max_depth=0, colors=True, hits=False, normals=False, points=False, shadow=True,
               stream=None):
    """rt_trace_rays: traces caller-supplied rays and returns the requested
    planes as a tuple, in RAY_PLANES' order.

    rays: a numpy array of abi.RAY_DTYPE, or of float32 with 8 values per ray
    (origin, reserved, direction, reserved), any shape; or a torch tensor on
    the context's GPU, float32, contiguous, 8 values per ray. Directions are
    used as given (not normalised). numpy in, numpy out, synchronously: colors
    (n, 4) float32, hits (n,) abi.HIT_DTYPE, normals and points (n, 4) float32.
    torch in, torch out on the same device: hits as (n, 4) int32 (the record's
    four words; .cpu().numpy().view(abi.HIT_DTYPE) names them); with `stream`
    (a hipStream_t as int) the call is asynchronous on that stream.
    shadow=False: no shadow rays, hits' shadow = 0."""
    want = dict(zip(RAY_PLANES, (colors, hits, normals, points)))
    flags = abi.RT_HITS_SHADOW if shadow else 0
    sp = C.c_void_p(stream) if stream else None
    if _is_torch(rays):
        import torch
        if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8:
            raise ValueError("rays: a contiguous float32 tensor on the GPU, 8 values per ray")
        n = rays.numel() // 8
        out = {k: torch.empty((max(n, 1), 4), dtype=torch.int32 if k == "hits" else torch.float32, device=rays.device)
               for k in RAY_PLANES if want[k]}
        ptrs = [C.c_void_p(out[k].data_ptr()) if k in out else None for k in RAY_PLANES]
        _check(lib().rt_trace_rays(ctx.handle, scene.handle, C.c_void_p(rays.data_ptr()), n, max_depth, flags, *ptrs,
                                   1, sp))
        return tuple(out[k][:n] for k in RAY_PLANES if want[k])
    a = np.ascontiguousarray(rays)
    if a.dtype != abi.RAY_DTYPE:
        a = np.ascontiguousarray(a, np.float32)
        if a.size % 8:
            raise ValueError("rays: abi.RAY_DTYPE records, or 8 float32 values per ray")
        a = a.reshape(-1, 8)
    n = a.size if a.dtype == abi.RAY_DTYPE else a.shape[0]
    out = {k: (np.zeros(max(n, 1), abi.HIT_DTYPE) if k == "hits" else np.zeros((max(n, 1), 4), np.float32))
           for k in RAY_PLANES if want[k]}
    ptrs = [C.c_void_p(out[k].ctypes.data) if k in out else None for k in RAY_PLANES]
    _check(lib().rt_trace_rays(ctx.handle, scene.handle, C.c_void_p(a.ctypes.data), n, max_depth, flags, *ptrs, 0, sp))
    return tuple(out[k][:n] for k in RAY_PLANES if want[k])


def occluded(ctx, scene, rays, packed=False, stream=None):
    """rt_occluded: one bit per segment origin + t * dir, 0 < t < 1 (dir is the
    vector to the far end): is any object in between? Equal to trace_rays'
    (hits.object >= 0) & (hits.t < 1) for the same buffer.

    rays: as trace_rays takes them. numpy in: a numpy bool array (n,) out,
    synchronously. torch in: a torch uint8 tensor (n,) on the same device;
    with `stream` (a hipStream_t as int) asynchronous on that stream.
    packed=True: the bits as words instead, bit i % 64 of word i // 64,
    (n + 63) // 64 of them: numpy uint64, or torch int64."""
    sp = C.c_void_p(stream) if stream else None
    if _is_torch(rays):
        import torch
        if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8:
            raise ValueError("rays: a contiguous float32 tensor on the GPU, 8 values per ray")
        if rays.device.index != ctx.device:
            raise ValueError("rays: a tensor on the context's GPU (cuda:%d), not %s" % (ctx.device, rays.device))
        n = rays.numel() // 8
        m = (n + 63) // 64 if packed else n
        out = torch.empty(max(m, 1), dtype=torch.int64 if packed else torch.uint8, device=rays.device)
        ptrs = (None, C.c_void_p(out.data_ptr())) if packed else (C.c_void_p(out.data_ptr()), None)
        _check(lib().rt_occluded(ctx.handle, scene.handle, C.c_void_p(rays.data_ptr()), n, *ptrs, 1, sp))
        return out[:m]
    a = np.ascontiguousarray(rays)
    if a.dtype != abi.RAY_DTYPE:
        a = np.ascontiguousarray(a, np.float32)
        if a.size % 8:
            raise ValueError("rays: abi.RAY_DTYPE records, or 8 float32 values per ray")
        a = a.reshape(-1, 8)
    n = a.size if a.dtype == abi.RAY_DTYPE else a.shape[0]
    m = (n + 63) // 64 if packed else n
    out = np.zeros(max(m, 1), np.uint64 if packed else np.uint8)
    ptrs = (None, C.c_void_p(out.ctypes.data)) if packed else (C.c_void_p(out.ctypes.data), None)
    _check(lib().rt_occluded(ctx.handle, scene.handle, C.c_void_p(a.ctypes.data), n, *ptrs, 0, sp))
    return out[:m] if packed else out[:m].astype(bool)


def view_rays(ctx, view, width, height, rows=None, device=False):
    """rt_view_rays: the camera rays of `view` for rows [r0, r1) in rt_render's
    pixel order — a numpy array (r1-r0, width) of abi.RAY_DTYPE, or with
    device=True a float32 torch tensor (r1-r0, width, 8) on the context's GPU.
    trace_rays of them equals render / render_hits of the view."""
    r0, r1 = rows if rows is not None else (0, height)
    shape = (max(r1 - r0, 1), max(width, 1))  # the C-ABI validates the range
    if device:
        import torch
        out = torch.empty(shape + (8,), dtype=torch.float32, device="cuda:%d" % ctx.device)
        _check(lib().rt_view_rays(ctx.handle, C.byref(view), width, height, r0, r1, C.c_void_p(out.data_ptr()), 1,
                                  None))
        return out[: r1 - r0, :width]
    out = np.zeros(shape, abi.RAY_DTYPE)
    _check(lib().rt_view_rays(ctx.handle, C.byref(view), width, height, r0, r1, C.c_void_p(out.ctypes.data), 0, None))
    return out[: r1 - r0, :width]


def render_batch(ctx, scene, out_ptr, width, height, max_depth, views, block_rows=8, n_shards=1,
                 shard=0, stream=None):
    """K frames (K = len(views) <= abi.RT_MAX_BATCH = 256) in one launch
    (depth 0-1; deeper frames in even queued launches of as many views as fit
    beside the scene in LDS, include/rt.h) into device memory laid out
    (K, rows, width, C) (C and dtype: the context's surface format); rows =
    height, or this shard's rows."""
    arr = (View * len(views))(*views)
    _check(lib().rt_render_batch(ctx.handle, scene.handle, arr, len(views), width, height, max_depth,
                                 block_rows, n_shards, shard, C.c_void_p(out_ptr),
                                 C.c_void_p(stream) if stream else None))


def batch_launches(ctx, scene, n_views, max_depth):
    """Kernel launches render_batch makes for n_views views of `scene` at
    max_depth (deep batches split into queued launches of as many views as
    fit beside the scene in LDS)."""
    n = lib().rt_batch_launches(ctx.handle, scene.handle, n_views, max_depth)
    if n < 0:
        raise RTError(n, lib().rt_last_error().decode())
    return n


def render_batch_scenes(ctx, scenes, out_ptr, width, height, max_depth, views, block_rows=8, n_shards=1,
                        shard=0, stream=None):
    """K animated frames in one launch: views[k] of scenes[k] (same layout),
    into device memory (K, rows, width, C) in the context's surface format."""
    arr = (View * len(views))(*views)
    sarr = (C.c_void_p * len(scenes))(*[s.handle for s in scenes])
    _check(lib().rt_render_batch_scenes(ctx.handle, sarr, arr, len(views), width, height, max_depth, block_rows,
                                        n_shards, shard, C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))


def render_accumulate(ctx, scene, accum_ptr, width, height, max_depth, spp, sample_offset=0, seed=0,
                      jitter=True, view=None, rows=None, stream=None):
    """Monte-Carlo: add the sum of samples [sample_offset, sample_offset+spp)
    of every pixel to the float4 device accumulator at accum_ptr."""
    r0, r1 = rows if rows is not None else (0, height)
    if view is None:
        view = make_view(None, 0.0)
    _check(lib().rt_render_accumulate(ctx.handle, scene.handle, C.byref(view), width, height, max_depth, spp,
                                      sample_offset, seed, 1 if jitter else 0, r0, r1, C.c_void_p(accum_ptr),
                                      C.c_void_p(stream) if stream else None))


def render_aa(ctx, scene, width, height, max_depth, spp, threshold, seed=0, view=None, cam=None, time=0.0,
              out=None, stream=None, want_mask=False):
    """Adaptive anti-aliasing (rt_render_aa_view; with view None rt_render_aa
    of `cam` — None: the orbit camera — at `time`): the base frame with every
    pixel on a colour edge (a 4-neighbour differing by more than `threshold`
    in some channel) replaced by the mean of `spp` jittered samples.
    out None: host arrays, synchronously — the frame (height, width, 4)
    float32, or (frame, mask) with want_mask, mask (height, width) uint8,
    1 = supersampled. out a device pointer (e.g. tensor.data_ptr()): the frame
    goes there, want_mask is then a device pointer for the byte plane (or
    False), and with `stream` (a hipStream_t as int) the call is asynchronous."""
    device = out is not None
    if device:
        frame, mask = None, None
        out_ptr = C.c_void_p(out)
        mask_ptr = C.c_void_p(want_mask) if want_mask else None
    else:
        frame = np.zeros((max(height, 1), max(width, 1), 4), np.float32)  # the C-ABI validates the size
        mask = np.zeros((max(height, 1), max(width, 1)), np.uint8) if want_mask else None
        out_ptr = C.c_void_p(frame.ctypes.data)
        mask_ptr = C.c_void_p(mask.ctypes.data) if want_mask else None
    tail = (width, height, max_depth, spp, seed, threshold, out_ptr, mask_ptr, 1 if device else 0,
            C.c_void_p(stream) if stream else None)
    if view is not None:
        _check(lib().rt_render_aa_view(ctx.handle, scene.handle, C.byref(view), *tail))
    else:
        _check(lib().rt_render_aa(ctx.handle, scene.handle, C.byref(cam) if cam is not None else None, time, *tail))
    if device:
        return None
    frame = frame[:height, :width]
    return (frame, mask[:height, :width]) if want_mask else frame


def aa_last_counts(ctx):
    """(flagged pixels, wave tiles with a flagged pixel) of the context's last
    render_aa, after waiting for it (rt_aa_last_counts)."""
    px, tiles = C.c_int64(0), C.c_int64(0)
    _check(lib().rt_aa_last_counts(ctx.handle, C.byref(px), C.byref(tiles)))
    return px.value, tiles.value


def aa_edge_mask(frame, threshold):
    """The anti-aliasing criterion on the host (rt_aa_edge_mask; no GPU): for a
    (height, width, 4) float32 frame, (mask, tile_masks) — mask (height, width)
    uint8, 1 = a 4-neighbour differs by more than `threshold` in some channel;
    tile_masks (ceil(height / 8), ceil(width / 8)) uint64, bit l of a word =
    pixel (8 wx + l % 8, 8 wy + l / 8) of its 8 x 8 wave tile."""
    frame = np.ascontiguousarray(frame, np.float32)
    if frame.ndim != 3 or frame.shape[2] != 4:
        raise ValueError("aa_edge_mask: a (height, width, 4) float32 frame")
    height, width = frame.shape[:2]
    mask = np.zeros((height, width), np.uint8)
    tiles = np.zeros(((height + 7) // 8, (width + 7) // 8), np.uint64)
    _check(lib().rt_aa_edge_mask(C.c_void_p(frame.ctypes.data), width, height, threshold,
                                 C.c_void_p(mask.ctypes.data), C.c_void_p(tiles.ctypes.data)))
    return mask, tiles


def render_shard(ctx, scene, out_ptr, width, height, max_depth, block_rows, n_shards, shard,
                 view=None, stream=None):
    """Render this shard's interleaved row blocks into device memory
    (rows, width, C) in the context's surface format."""
    if view is None:
        view = make_view(None, 0.0)
    _check(lib().rt_render_shard(ctx.handle, scene.handle, C.byref(view), width, height, max_depth,
                                 block_rows, n_shards, shard, C.c_void_p(out_ptr),
                                 C.c_void_p(stream) if stream else None))


class Multi:
    """One frame on several GPUs of this process (rt_multi_create /
    rt_render_multi): interleaved row blocks per context, gathered to the
    first context's GPU (RCCL, or peer copies with transport=RT_MULTI_COPY,
    which also serves contexts sharing a device) and de-interleaved there."""

    def __init__(self, contexts, transport=abi.RT_MULTI_RCCL):
        self.contexts = list(contexts)
        arr = (C.c_void_p * len(self.contexts))(*[c.handle for c in self.contexts])
        self._h = C.c_void_p()
        _check(lib().rt_multi_create(len(self.contexts), arr, transport, C.byref(self._h)))

    def render(self, scenes, width, height, max_depth=0, time=0.0, camera=None, view=None, block_rows=8):
        """The whole frame as a host array in the root context's surface format."""
        out = surface(self.contexts[0].output, max(height, 1), max(width, 1))
        self._render(scenes, width, height, max_depth, time, camera, view, block_rows, out.ctypes.data, 0)
        return out[:height, :width]

    def render_device(self, scenes, out_ptr, width, height, max_depth=0, time=0.0, camera=None, view=None,
                      block_rows=8):
        """The whole frame into device memory of the root context's GPU."""
        self._render(scenes, width, height, max_depth, time, camera, view, block_rows, out_ptr, 1)

    def _render(self, scenes, width, height, max_depth, time, camera, view, block_rows, ptr, is_device):
        sarr = (C.c_void_p * len(scenes))(*[s.handle for s in scenes])
        if view is not None:
            _check(lib().rt_render_multi_view(self._h, sarr, C.byref(view), width, height, max_depth, block_rows,
                                              C.c_void_p(ptr), is_device))
        else:
            _check(lib().rt_render_multi(self._h, sarr, C.byref(camera) if camera is not None else None, time,
                                         width, height, max_depth, block_rows, C.c_void_p(ptr), is_device))

    def last_ms(self):
        """(per-GPU kernel ms, gather ms, assembly ms) of the last render."""
        k = (C.c_float * len(self.contexts))()
        g, a = C.c_float(), C.c_float()
        _check(lib().rt_multi_last_ms(self._h, k, C.byref(g), C.byref(a)))
        return list(k), g.value, a.value

    def close(self):
        if self._h:
            lib().rt_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
