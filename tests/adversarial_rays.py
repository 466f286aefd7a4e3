"""Adversarial ray families for rt_trace_rays (test_adversarial_rays_host.py,
test_gpu_adversarial_rays.py), with the oracle's ray entry point
(port.trace_rays) as the checker. No GPU; seeded and deterministic.

The camera-shaped sets of rays_common have one origin per camera and
normalised directions with no zero component. The families here are built on
the boundaries the ray kernels' pre-tests name for themselves: a zero direction
component (safe_rcp, slab_may_hit), 2^-60 (slab_may_hit), 1024 per axis
(kRayNearOrigin), | |d|^2 - 1 | <= 2^-19 (kRayUnitDir), and an origin exactly on
a surface. Every family is generated per scene from the scene's own objects and
lights, in float64, rounded to float32 once.

    AXIS       the 26 directions of {-1, 0, 1}^3 from points on, in and around
               every object, every light, the world's origin
    GRAZE      tangents of spheres and silhouettes of boxes, a few 1e-7 rad off
    SCALE      a subsample of both with the direction multiplied by s
    FAR        origins at and beyond 1024 on one axis, aimed at a sphere
    CONTINUED  rays that start on the oracle's own hit points
    LENGTH     rays of length 1.2 and 0.8 aimed at spheres: their reflection and
               refraction children start on spheres with the parent's length
"""
import ctypes as C
import functools

import numpy as np

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from oracle import port, scenes
from rays_common import RaySet, set_r

FAMILIES = ("AXIS", "GRAZE", "SCALE", "FAR", "CONTINUED", "LENGTH")
SCENES = ("room16", "spheres63", "room100", "shipped", "aabox", "lights_edge")
DEPTHS = (0, 1, 2, 5)
MAX_RAYS = 20000  # per family and scene
F32 = np.float32

EPS = (0.0, 1e-7, -1e-7, 3e-7, -3e-7, 1e-6, -1e-6, 1e-4, -1e-4)  # rad off the tangent / the silhouette
# SCALE's factors. 2^-10 is the one chosen between 2^-8 and 2^-12: t grows by
# 1024, so a unit ray's hit beyond t = 9.765625 passes the 10000 horizon and
# becomes a miss; SCALE_HORIZON holds the oracle's (hits, misses) at that
# factor per scene (asserted by the host test).
S_CHOSEN = 2.0 ** -10
SCALES = (1 + 2.0 ** -21, 1 - 2.0 ** -21, 1 + 2.0 ** -19, 1 - 2.0 ** -19, 1 + 2.0 ** -18, 1 - 2.0 ** -18, 0.5, 2.0,
          2.0 ** -8, 2.0 ** 20, 2.0 ** -62, 1e-38, 0.0, S_CHOSEN, 0.75, 1.2)
# (0.75 and 1.2: lengths well off 1 that a unit gate widened by a constant
# factor would still admit: | |d|^2 - 1 | = 0.44 — the probe build P1 of
# test_gpu_adversarial_rays.py; every factor above is either within 2^-17 of 1
# or beyond 0.5)
S_IN_GATE, S_OUT_OF_GATE = SCALES[:2], SCALES[2:6]
SCALE_HORIZON = {}  # filled in below, after the definitions
FAR_V = (F32(1023.99), F32(1024.0), np.nextafter(F32(1024.0), F32(np.inf)), F32(4096.0), F32(1e5), F32(1e7))
POISON_LANES = (0, 31, 63)


# ---- scenes --------------------------------------------------------------------
class Scn:
    def __init__(self, name, objs, lights=None, time=0.0):
        self.name, self.objs, self.time = name, objs, time
        self.lights = lights if lights is not None else port.reference_lights()
        self.kw = dict(lights=self.lights)


def is_box(o):
    return any(o.box_mins[:]) or any(o.box_maxs[:])


def is_room(o):
    return is_box(o) and o.box_mins[:] == [-11.0] * 3 and o.box_maxs[:] == [11.0] * 3


def _light_at(like, pos):
    lt = abi.Light()
    C.memmove(C.byref(lt), C.byref(like), C.sizeof(abi.Light))
    lt.position[:] = [float(F32(x)) for x in pos]
    return lt


def aabox_objects():
    """Two spheres and four translate-only boxes: the world's axes are the
    boxes' own, so a zero direction component reaches the slab tests as one."""
    return [scenes.sphere((-3.0, 4.0, 1.0), 2.0, abi.RED_GLASS),
            scenes.sphere((3.0, -4.0, 1.0), 1.5, abi.MIRROR),
            scenes.box((-10.0, -10.0, -1.0), (10.0, 10.0, 1.0), (0.0, 0.0, -3.0), (0.0, 0.0, 0.0), abi.WALL),  # floor
            scenes.box((-1.0, -0.5, -0.5), (1.0, 0.5, 0.5), (3.0, 2.0, 0.0), (0.0, 0.0, 0.0), abi.MATERIAL1),  # brick
            scenes.box((-0.25, -0.25, -3.0), (0.25, 0.25, 3.0), (-4.0, -3.0, 1.0), (0.0, 0.0, 0.0), abi.GREEN_GLASS),
            scenes.box((-2.0, -0.01, -1.5), (2.0, 0.01, 1.5), (0.0, 5.0, 0.5), (0.0, 0.0, 0.0), abi.MATERIAL2)]  # sheet


@functools.lru_cache(None)
def scene(name):
    if name == "room16":
        return Scn(name, scenes.bench_objects(16))
    if name == "spheres63":
        return Scn(name, scenes.bench_objects(64)[1:])
    if name == "room100":
        return Scn(name, scenes.bench_objects(100))
    if name == "shipped":
        return Scn(name, rt.reference_objects(3.7), time=3.7)
    if name == "aabox":
        return Scn(name, aabox_objects())
    if name == "lights_edge":
        objs = scenes.bench_objects(16)
        ref = port.reference_lights()
        a, b = objs[2], objs[5]
        on_surface = (b.position[0], b.position[1], F32(b.position[2]) + F32(b.radius))
        return Scn(name, objs, [_light_at(ref[0], a.position[:]), _light_at(ref[1], on_surface),
                                _light_at(ref[2], (10.5, 2.0, -1.0))])
    raise KeyError(name)


def transforms(o):
    """(local_to_world, world_to_local) of a box as float64 (4, 4), row vectors: world = local4 @ l2w."""
    out = (C.c_float * 41)()
    port.lib().oracle_object_transforms(C.byref(o), out)
    a = np.array(out[:32], np.float64)
    return a[:16].reshape(4, 4), a[16:].reshape(4, 4)


def _xf(m, p):
    p = np.atleast_2d(np.asarray(p, np.float64))
    return (np.concatenate([p, np.ones((len(p), 1))], 1) @ m)[:, :3]


def make_rays(origins, dirs):
    """Float64 (or float32) origins and directions, rounded to float32 once."""
    r = np.zeros(len(origins), abi.RAY_DTYPE)
    r["origin"] = np.asarray(origins).astype(F32)
    r["dir"] = np.asarray(dirs).astype(F32)
    return r


# A (scene, family) whose first seed missed a condition of the host test (the
# seed changes, never the condition): shipped's one sphere stood behind the
# rotated floor from five of the first seed's six origins.
SEEDS = {("shipped", "GRAZE"): 7}


def _rng(sc, fam):
    return np.random.default_rng([20260, SCENES.index(sc.name), FAMILIES.index(fam), SEEDS.get((sc.name, fam), 0)])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(rng, w):
    """A seeded unit vector perpendicular to the unit vector w."""
    while True:
        u = rng.standard_normal(3)
        u -= u.dot(w) * w
        if np.linalg.norm(u) > 0.1:
            return _unit(u)


# ---- the families ----------------------------------------------------------------
class Family:
    """rays: (n,) abi.RAY_DTYPE in generation order; meta: per-ray arrays the
    conditions are stated on; color(depth), p2, p3, p4: the oracle's planes."""

    def __init__(self, sc, name, rays, **meta):
        self.sc, self.name, self.rays, self.meta, self.n = sc, name, rays, meta, len(rays)
        assert 0 < self.n <= MAX_RAYS, (sc.name, name, self.n)
        self._planes = {}

    def plane(self, probe, depth=0):
        key = (probe, depth if probe == 0 else 0)
        if key not in self._planes:
            out = port.trace_rays(self.sc.objs, self.rays, key[1], probe, **self.sc.kw)
            out.setflags(write=False)
            self._planes[key] = out
        return self._planes[key]

    def color(self, depth):
        return self.plane(0, depth)

    p2 = property(lambda self: self.plane(2))
    p3 = property(lambda self: self.plane(3))
    p4 = property(lambda self: self.plane(4))
    obj = property(lambda self: self.p2[:, 0].astype(np.int64))
    t = property(lambda self: self.p2[:, 1])
    colors = property(lambda self: {d: self.color(d) for d in DEPTHS})
    objs = property(lambda self: self.sc.objs)


AXIS_DIRS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)],
                     F32)
AXIS_DIRS = AXIS_DIRS / np.sqrt((AXIS_DIRS * AXIS_DIRS).sum(-1, keepdims=True, dtype=F32))  # (in float32)
assert AXIS_DIRS.dtype == F32 and len(AXIS_DIRS) == 26


def axis_origins(sc):
    pts = []
    for o in sc.objs:
        if is_box(o):
            l2w, _ = transforms(o)
            lo, hi = np.array(o.box_mins[:], np.float64), np.array(o.box_maxs[:], np.float64)
            mid = 0.5 * (lo + hi)
            lv = np.stack([lo, mid, hi])  # lv[level][axis]
            grid = np.array([(lv[i, 0], lv[j, 1], lv[k, 2]) for i in range(3) for j in range(3) for k in range(3)])
            pts.append(_xf(l2w, grid))
            pts.append(_xf(l2w, grid + np.sign(grid - mid)))  # (pushed out by 1 on every axis off the middle)
        elif o.radius != -1.0:
            c, r = np.array(o.position[:], np.float64), float(o.radius)
            pts.append(np.array([c, c + (r, 0, 0), c - (0, r, 0), c + (0, 0, r), c + (2 * r, 0, 0),
                                 c - (0, 0.5 * r, 1.5 * r)]))
    pts.append(np.array([lt.position[:] for lt in sc.lights], np.float64))
    pts.append(np.array([(0.0, 0.0, 0.0), (0.0, 2.5, -1.5), (1.5, 0.0, 2.0), (-2.0, 3.0, 0.0),  # one zero coordinate
                         (0.0, 0.0, 3.0), (0.0, -4.0, 0.0), (5.0, 0.0, 0.0)]))  # two
    return np.concatenate(pts)


def make_axis(sc):
    o = axis_origins(sc).astype(F32)
    return Family(sc, "AXIS", make_rays(np.repeat(o, 26, 0), np.tile(AXIS_DIRS, (len(o), 1))),
                  dir_index=np.tile(np.arange(26), len(o)))


def make_graze(sc):
    rng = _rng(sc, "GRAZE")
    org, dirs, target, kind = [], [], [], []
    spheres = [i for i, o in enumerate(sc.objs) if not is_box(o) and o.radius != -1.0]
    for i in [spheres[k] for k in np.unique(np.linspace(0, len(spheres) - 1, min(24, len(spheres))).astype(int))]:
        c, r = np.array(sc.objs[i].position[:], np.float64), float(sc.objs[i].radius)
        for _ in range(6):
            while True:
                p = rng.uniform(-9.5, 9.5, 3).astype(F32).astype(np.float64)
                dist = np.linalg.norm(c - p)
                if dist > r + 0.05:
                    break
            w = (c - p) / dist
            u = _perp(rng, w)
            alpha = np.arcsin(r / dist)
            for e in EPS:  # (e < 0: inside the tangent cone)
                org.append(p)
                dirs.append(np.cos(alpha + e) * w + np.sin(alpha + e) * u)
                target.append(i)
                kind.append(0)
    for i, o in enumerate(sc.objs):
        if not is_box(o) or is_room(o):
            continue
        l2w, w2l = transforms(o)
        lo, hi = np.array(o.box_mins[:], np.float64), np.array(o.box_maxs[:], np.float64)
        mid = 0.5 * (lo + hi)
        corners = np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        edges = np.array([np.where(np.arange(3) == a, mid, c) for a in range(3) for c in corners
                          if c[a] == lo[a]])  # 12 edge midpoints
        aims = np.concatenate([corners[rng.choice(8, 4, replace=False)], edges[rng.choice(12, 4, replace=False)]])
        for _ in range(3):
            while True:
                p = rng.uniform(-9.5, 9.5, 3).astype(F32).astype(np.float64)
                q = _xf(w2l, p)[0]
                if ((q < lo - 0.05) | (q > hi + 0.05)).any():
                    break
            for a in _xf(l2w, aims):
                w = _unit(a - p)
                u = _perp(rng, w)
                for e in EPS:
                    org.append(p)
                    dirs.append(np.cos(e) * w + np.sin(e) * u)
                    target.append(i)
                    kind.append(1)
    return Family(sc, "GRAZE", make_rays(np.array(org), np.array(dirs)), target=np.array(target),
                  kind=np.array(kind), eps=np.tile(np.array(EPS), len(org) // len(EPS)))


def scale_base(sc):
    """The unit rays SCALE multiplies: 100 of AXIS and 100 of GRAZE, a seeded choice in generation order."""
    rng = _rng(sc, "SCALE")
    parts = []
    for fam in (family(sc.name, "AXIS"), family(sc.name, "GRAZE")):
        parts.append(fam.rays[np.sort(rng.choice(fam.n, min(100, fam.n), replace=False))])
    return np.concatenate(parts)


def make_scale(sc):
    base = scale_base(sc)
    rays = np.tile(base, len(SCALES))
    s = np.repeat(np.array(SCALES, np.float64).astype(F32), len(base))
    rays["dir"] = base["dir"][np.tile(np.arange(len(base)), len(SCALES))] * s[:, None]  # (float32 products)
    assert rays["dir"].dtype == F32
    return Family(sc, "SCALE", rays, s_index=np.repeat(np.arange(len(SCALES)), len(base)),
                  base=np.tile(np.arange(len(base)), len(SCALES)), n_base=len(base))


def make_far(sc):
    rng = _rng(sc, "FAR")
    spheres = [o for o in sc.objs if not is_box(o) and o.radius != -1.0]
    org, dirs = [], []
    for v in FAR_V:
        for axis in range(3):
            for sign in (1.0, -1.0):
                for _ in range(8):
                    p = rng.uniform(-8.0, 8.0, 3).astype(F32)
                    p[axis] = F32(sign) * v
                    p = p.astype(np.float64)
                    o = spheres[rng.integers(len(spheres))]
                    off = _unit(rng.standard_normal(3)) * rng.uniform(0.0, 0.3)
                    org.append(p)
                    dirs.append(_unit(np.array(o.position[:], np.float64) + off - p))
    return Family(sc, "FAR", make_rays(np.array(org), np.array(dirs)),
                  v=np.repeat(np.array(FAR_V, np.float64), 48))


def _dot32(a, b):
    return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])


def continued_rays(rays, obj, n, p, keep=None):
    """From hit records (object, normal, point: float32) of `rays`: per hit four
    rays in the order (p, reflected), (p, -d), (p + 0.01 n, reflected),
    (p + 0.01 n, -d), float32 arithmetic. Misses are dropped; `keep`: at most
    so many hits. Returns (rays, start object, offset index, direction index)."""
    hit = np.flatnonzero(obj >= 0)
    if keep is not None and len(hit) > keep:
        hit = np.sort(np.random.default_rng(7).choice(hit, keep, replace=False))
    d, n, p = rays["dir"][hit].astype(F32), n[hit, :3].astype(F32), p[hit, :3].astype(F32)
    refl = d - n * (F32(2.0) * _dot32(n, d))[:, None]
    starts = (p, p + F32(0.01) * n)
    org = np.stack([starts[0], starts[0], starts[1], starts[1]], 1).reshape(-1, 3)
    dirs = np.stack([refl, -d, refl, -d], 1).reshape(-1, 3)
    assert org.dtype == F32 and dirs.dtype == F32
    k = len(hit)
    return (make_rays(org, dirs), np.repeat(obj[hit], 4), np.tile(np.array([0, 0, 1, 1]), k),
            np.tile(np.array([0, 1, 0, 1]), k))


def make_continued(sc):
    src = [family(sc.name, "AXIS"), family(sc.name, "GRAZE")]
    rays = np.concatenate([f.rays for f in src])
    obj = np.concatenate([f.obj for f in src])
    r, start, offset, kind = continued_rays(rays, obj, np.concatenate([f.p3 for f in src]),
                                            np.concatenate([f.p4 for f in src]), keep=1500)
    return Family(sc, "CONTINUED", r, start=start, offset=offset, dir_kind=kind)


# LENGTH: a reflection or refraction child keeps its parent's length, starts on
# a sphere and (at depth >= 2, RT_OPT_ORIGIN_LISTS) reads that sphere's
# candidate list, whose stored distance bounds are compared with the child's
# ray parameter: a longer direction shortens t and ends the list early. SCALE's
# 200 rays mostly hit a wall first; here every ray is aimed at a sphere, from a
# seeded point of +-9.5, and three in four are 1.2 long (| |d|^2 - 1 | = 0.44:
# inside a unit gate of 0.5, the probe build P1), the fourth 0.8.
LENGTHS = (1.2, 1.2, 1.2, 0.8)
LENGTH_PER_SPHERE = 160


def make_length(sc):
    rng = _rng(sc, "LENGTH")
    org, dirs = [], []
    for o in sc.objs:
        if is_box(o) or o.radius == -1.0:
            continue
        c, r = np.array(o.position[:], np.float64), float(o.radius)
        p = rng.uniform(-9.5, 9.5, (LENGTH_PER_SPHERE, 3))
        aim = c + _unit(rng.standard_normal((LENGTH_PER_SPHERE, 3))) * rng.uniform(0.0, 0.9 * r, (LENGTH_PER_SPHERE, 1))
        org.append(p)
        dirs.append(_unit(aim - p))
    rays = make_rays(np.concatenate(org), np.concatenate(dirs))
    length = np.tile(np.array(LENGTHS, np.float64).astype(F32), (len(rays) + 3) // 4)[:len(rays)]
    rays["dir"] = rays["dir"] * length[:, None]  # (float32 products)
    return Family(sc, "LENGTH", rays, length=length)


_MAKERS = {"LENGTH": make_length, "AXIS": make_axis, "GRAZE": make_graze, "SCALE": make_scale, "FAR": make_far, "CONTINUED": make_continued}


@functools.lru_cache(None)
def family(scene_name, name):
    return _MAKERS[name](scene(scene_name))


# ---- the arrangements of the GPU test ----------------------------------------------
@functools.lru_cache(None)
def camera_set(scene_name):
    """The camera-shaped rays a family is permuted with: set R in room16, the
    scene's orbit camera at 16 x 9 elsewhere."""
    if scene_name == "room16":
        return set_r()
    sc = scene(scene_name)
    return RaySet(sc.objs, [None], 16, 9, DEPTHS, lights=sc.lights, time=sc.time)


@functools.lru_cache(None)
def poison(scene_name):
    """One ray outside the origin gate (x = 5000, unit direction towards the
    scene) as a one-ray family: its own oracle record is what its slot holds."""
    sc = scene(scene_name)
    p = np.array([5000.0, 0.75, -0.5])
    return Family(sc, "POISON", make_rays(p[None], _unit(np.array(sc.objs[-1].position[:], np.float64) - p)[None]))


def poison_slots(n):
    """Lane 0, 31 or 63 of every other wave of 64, in turn."""
    slots = [64 * w + POISON_LANES[(w // 2) % 3] for w in range(0, (n + 63) // 64, 2)]
    return np.array([s for s in slots if s < n], np.int64)


def kernel_norm2(d):
    """|d|^2 as the ray kernels' gate computes it: float32, x x + (y y + z z)."""
    d = d.astype(F32)
    return d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def hexf(v):
    return "(" + ", ".join(float(x).hex() for x in v) + ")"


# The oracle's (hits, misses) of SCALE's rays at s = S_CHOSEN = 2^-10.
SCALE_HORIZON.update({"room16": (63, 137), "spheres63": (116, 84), "room100": (147, 53), "shipped": (140, 60),
                      "aabox": (96, 104), "lights_edge": (87, 113)})
