"""ctypes mirror of include/rt.h (data layout only; loads nothing).

Every struct follows the GLSL struct it replaces
(/root/reference/OpenGLRaytracer/raytrace_compute.glsl:36-50, 56-69, 190-196,
244-258); see include/rt.h for the field-by-field citations.
"""
import ctypes as C

import numpy as np

RT_OK = 0
RT_ERR_INVALID = -1
RT_ERR_HIP = -2
RT_ERR_NOMEM = -3
RT_ERR_UNSUPPORTED = -4
RT_ERR_NO_DEVICE = -5
RT_MAX_DEPTH = 9
RT_MAX_OBJECTS = 1024
RT_MAX_LIGHTS = 16
RT_MAX_MATERIALS = 256
RT_OPT_CULLING = 1
RT_OPT_TIMING = 2
RT_OPT_OUTPUT = 3
RT_OPT_FRAME_CONSTS = 4
RT_OPT_ORIGIN_LISTS = 7
RT_OPT_SCENE_SHAPES = 8
RT_OPT_LAUNCH_SHAPES = 9
RT_OPT_PERSISTENT0 = 10
RT_OPT_FIXED_LAYOUT = 11
RT_OPT_ROOM_FAST = 12
RT_OPT_AA_QUEUED = 13
RT_OUTPUT_RGBA32F = 0
RT_OUTPUT_RGBA8 = 1
RT_OUTPUT_RGB32F = 2
RT_MAX_BATCH = 256
RT_MULTI_RCCL = 0
RT_MULTI_COPY = 1
RT_ANIM_NONE = 0
RT_ANIM_RATE = 1
RT_ANIM_RATE_OFFSET = 2
RT_ANIM_SIN = 3
RT_ANIM_SIN_OFFSET = 4

# material indices of the reference table (raytrace_compute.glsl:74-157)
MATERIAL1, MATERIAL2, RED_GLASS, GREEN_GLASS, BLUE_GLASS, MIRROR, WALL = range(7)
MATERIAL_NAMES = ["material1", "material2", "red_glass_material", "green_glass_material",
                  "blue_glass_material", "mirror_material", "wall_material"]

F3 = C.c_float * 3
F4 = C.c_float * 4


class Material(C.Structure):
    _fields_ = [("ambient", F4), ("diffuse", F4), ("specular", F4), ("shininess", C.c_float),
                ("emissive", F4), ("reflectivity", C.c_float), ("transparency", C.c_float),
                ("refraction_index", C.c_float)]


class Object(C.Structure):
    _fields_ = [("box_mins", F3), ("box_maxs", F3), ("radius", C.c_float), ("position", F3),
                ("angles", F3), ("material", C.c_int32)]


class Light(C.Structure):
    _fields_ = [("position", F3), ("ambient", F4), ("diffuse", F4), ("specular", F4)]


class Camera(C.Structure):
    _fields_ = [("position", F3), ("angles", F3), ("v_fov", C.c_float), ("aspect", C.c_float),
                ("near_plane", C.c_float), ("far_plane", C.c_float)]


class AnimChannel(C.Structure):
    """rt_anim_channel: one scalar of an object as a function of time."""
    _fields_ = [("kind", C.c_int32), ("a", C.c_float), ("k", C.c_float), ("c", C.c_float)]


class ObjectAnim(C.Structure):
    """rt_object_anim: zero-initialised = static."""
    _fields_ = [("scale", AnimChannel), ("position", AnimChannel * 3), ("angles", AnimChannel * 3)]


RT_HITS_SHADOW = 1


class Hit(C.Structure):
    """rt_hit: one pixel's primary hit (rt_render_hits, rt_pick), 16 bytes."""
    _fields_ = [("object", C.c_int32), ("t", C.c_float), ("shadow", C.c_uint32), ("material", C.c_int32)]


# the same record as a numpy dtype (the `hits` plane of render_hits)
HIT_DTYPE = np.dtype([("object", np.int32), ("t", np.float32), ("shadow", np.uint32), ("material", np.int32)])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) == 16


RT_MAX_RAYS = 1 << 28


class Ray(C.Structure):
    """rt_ray: one caller-supplied ray (rt_trace_rays, rt_view_rays), 32 bytes;
    the reserved words are ignored on input."""
    _fields_ = [("origin", F3), ("reserved0", C.c_float), ("dir", F3), ("reserved1", C.c_float)]


# the same record as a numpy dtype (the `rays` buffer of trace_rays)
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("reserved0", np.float32), ("dir", np.float32, 3),
                      ("reserved1", np.float32)])
assert RAY_DTYPE.itemsize == C.sizeof(Ray) == 32


def array(struct, items):
    """Build a ctypes array of `struct` from a list of structs."""
    arr = (struct * max(len(items), 1))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


def to_numpy(arr, n=None):
    """Flat float32 view of a ctypes struct array (for fixtures / hashing)."""
    n = len(arr) if n is None else n
    raw = bytes(memoryview(arr).cast("B"))[: n * C.sizeof(arr._type_)]
    return np.frombuffer(raw, dtype=np.uint8).copy()
