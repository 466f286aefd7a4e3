"""Shared by test_anim_spheres_host.py and test_gpu_anim_spheres.py: the three
blob scenes of the moving-sphere tests, a reader of the scene blob, and the
checks (a)-(e) on a slot blob at a time — from the host hook
(rt_debug_anim_host_blob) or from the device (rt_debug_anim_blob) — against
the scene the host builds of rt_animate_objects2(time). And by
test_anim_boxes_host.py and test_gpu_anim.py: the scenes of the box phases'
tests and readers of the records and planes."""
import ctypes as C

import numpy as np

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from openglraytracer_amd.abi import AnimChannel, Light, Material, Object, ObjectAnim
from oracle import scenes

SPHEREREC = np.dtype([("c", "<u4", 3), ("rr", "<u4")])
SPHEREMETA = np.dtype([("obj_index", "<i4"), ("material", "<i4"), ("radius", "<u4"), ("pad", "<i4")])
BVHNODE = np.dtype([("lo", "<f4", 3), ("skip", "<i4"), ("hi", "<f4", 3), ("leaf", "<i4")])
SHADOWCONE = np.dtype([("v", "<f4", 3), ("far", "<f4"), ("sph", "<f4"), ("cph", "<f4"), ("near", "<f4"),
                       ("pad", "<f4")])
BOXREC_BYTES, BOX_OBJ_INDEX_AT = 192, 39 * 4
META = ("blob_units", "off_spheres", "off_smeta", "off_boxes", "off_mats", "off_lights", "off_lightmat", "off_bvh",
        "n_bvh", "off_blink", "off_cone", "off_dmask", "dmask_n", "dmask_bytes", "off_gmask", "gmask_words",
        "off_glist", "n_spheres", "n_boxes", "n_mats", "n_lights", "off_olist")


def sin_offset(rng, amp, centre):
    return AnimChannel(abi.RT_ANIM_SIN_OFFSET, float(amp), float(rng.uniform(0.3, 2.0)), float(centre))


def move_sphere(rng, obj, an, amp=1.5):
    for k in range(3):
        an.position[k] = sin_offset(rng, rng.uniform(0.2, amp), obj.position[k])


def scene_room16():
    """(i) config 2's scene: the room and 16 spheres, every sphere moving, 5 of
    them breathing."""
    rng = np.random.default_rng(501)
    base = scenes.bench_objects(16)
    anim = [ObjectAnim() for _ in base]
    radius = [AnimChannel() for _ in base]
    for i in range(1, 17):
        move_sphere(rng, base[i], anim[i])
        if i % 3 == 0:
            radius[i] = sin_offset(rng, 0.25, base[i].radius)
    return base, anim, radius, rt.reference_materials(), rt.reference_lights()


def scene_boxes_spheres():
    """(ii) 3 moving boxes and 30 spheres, half of them moving: 33 mask bits,
    so 8-byte masks with box bits."""
    rng = np.random.default_rng(502)
    base, anim, radius = [], [], []
    for b in range(3):
        ext = rng.uniform(0.4, 1.0, 3)
        base.append(scenes.box(tuple(-ext), tuple(ext), tuple(rng.uniform(-5.0, 5.0, 3)),
                               tuple(rng.uniform(0.0, 360.0, 3)), int(rng.integers(7))))
        an = ObjectAnim()
        for k in range(3):
            an.position[k] = sin_offset(rng, 1.0, base[-1].position[k])
        an.angles[b] = AnimChannel(abi.RT_ANIM_RATE, 0.0, float(rng.uniform(10.0, 40.0)), 0.0)
        anim.append(an)
        radius.append(AnimChannel())
    for s in range(30):
        base.append(scenes.sphere(tuple(rng.uniform(-6.0, 6.0, 3)), float(rng.uniform(0.2, 0.9)), int(rng.integers(7))))
        an, rad = ObjectAnim(), AnimChannel()
        if s % 2 == 0:
            move_sphere(rng, base[-1], an)
            if s % 6 == 0:
                rad = sin_offset(rng, 0.15, base[-1].radius)
        anim.append(an)
        radius.append(rad)
    order = rng.permutation(len(base))
    return ([base[i] for i in order], [anim[i] for i in order], [radius[i] for i in order],
            rt.reference_materials(), rt.reference_lights())


def scene_cone_table():
    """(iii) 10 moving spheres and 56 static boxes: 66 mask bits, no direction
    masks, so the layout carries the ShadowCone table."""
    rng = np.random.default_rng(503)
    base, anim, radius = [], [], []
    for b in range(56):
        ext = rng.uniform(0.1, 0.4, 3)
        base.append(scenes.box(tuple(-ext), tuple(ext), tuple(rng.uniform(-7.0, 7.0, 3)),
                               tuple(rng.uniform(0.0, 360.0, 3)), int(rng.integers(7))))
        anim.append(ObjectAnim())
        radius.append(AnimChannel())
    for s in range(10):
        base.append(scenes.sphere(tuple(rng.uniform(-5.0, 5.0, 3)), float(rng.uniform(0.3, 1.0)), int(rng.integers(7))))
        an = ObjectAnim()
        move_sphere(rng, base[-1], an, 2.5)
        anim.append(an)
        radius.append(sin_offset(rng, 0.2, base[-1].radius) if s % 2 else AnimChannel())
    order = rng.permutation(len(base))
    return ([base[i] for i in order], [anim[i] for i in order], [radius[i] for i in order],
            rt.reference_materials(), rt.reference_lights())


BLOB_SCENES = {"room16": scene_room16, "boxes_spheres": scene_boxes_spheres, "cone_table": scene_cone_table}


# ---- the box phases (test_anim_boxes_host.py, test_gpu_anim.py) ---------------
BOXREC = np.dtype([("w2l", "<u4", 12), ("l2w", "<u4", 12), ("nrm", "<u4", 9), ("mins", "<u4", 3), ("maxs", "<u4", 3),
                   ("obj_index", "<i4"), ("material", "<i4"), ("light_inside", "<u4"), ("translate_only", "<i4"),
                   ("w2l_w0", "<u4", 3), ("pad", "<i4", 2)])
assert BOXREC.itemsize == BOXREC_BYTES
ON_LIGHT_TIME = 1.0  # box 0 of two_boxes and of box_spheres has its centre on a light
BOX_TIMES = [0.0, 0.8125, -2.375, 7.3, ON_LIGHT_TIME]


def live_lights(rng, n):
    out = []
    for _ in range(n):
        lt = Light()
        lt.position[:] = rng.uniform(-6.0, 6.0, 3)
        lt.ambient[:] = rng.uniform(0.0, 0.2, 4)
        lt.diffuse[:] = rng.uniform(0.2, 1.0, 4)
        lt.specular[:] = rng.uniform(0.2, 1.0, 4)
        out.append(lt)
    return out


def moving_box(rng, through=None, grow=True):
    """(box, channels). through: the position the box's centre has at
    ON_LIGHT_TIME, on RATE_OFFSET channels; else SIN_OFFSET positions. grow:
    a RATE angle channel and a breathing scale."""
    ext = rng.uniform(0.4, 1.0, 3)
    pos = rng.uniform(-5.0, 5.0, 3)
    an = ObjectAnim()
    for k in range(3):
        if through is None:
            an.position[k] = sin_offset(rng, 1.0, pos[k])
        else:
            rate = np.float32(rng.uniform(0.5, 3.0))
            at = np.float32(through[k]) - rate * np.float32(ON_LIGHT_TIME)
            an.position[k] = AnimChannel(abi.RT_ANIM_RATE_OFFSET, 0.0, float(rate), float(at))
    an.angles[int(rng.integers(3))] = AnimChannel(abi.RT_ANIM_RATE, 0.0, float(rng.uniform(10.0, 40.0)), 0.0)
    if grow:
        an.scale = sin_offset(rng, 0.3, 1.0)
    return scenes.box(tuple(-ext), tuple(ext), tuple(pos), tuple(rng.uniform(0.0, 360.0, 3)), int(rng.integers(7))), an


def scene_two_boxes():
    """(iii) two moving boxes, two lights, no sphere: planes and no masks."""
    rng = np.random.default_rng(504)
    lights = live_lights(rng, 2)
    boxes = [moving_box(rng, through=lights[0].position), moving_box(rng)]
    return [b for b, _ in boxes], [a for _, a in boxes], [AnimChannel(), AnimChannel()], rt.reference_materials(), lights


def scene_box_spheres():
    """(iv) one moving box and 12 spheres, 4 of them moving: no planes and no
    box bits."""
    rng = np.random.default_rng(505)
    lights = rt.reference_lights()
    box, an = moving_box(rng, through=lights[1].position)
    base, anim, radius = [box], [an], [AnimChannel()]
    for s in range(12):
        base.append(scenes.sphere(tuple(rng.uniform(-6.0, 6.0, 3)), float(rng.uniform(0.2, 0.9)), int(rng.integers(7))))
        anim.append(ObjectAnim())
        radius.append(AnimChannel())
        if s % 3 == 0:
            move_sphere(rng, base[-1], anim[-1])
    return base, anim, radius, rt.reference_materials(), lights


def scene_steady_extent():
    """Two moving boxes without a channel that grows, two lights, and a static
    box far out that alone sets the scene's extent at every time."""
    rng = np.random.default_rng(506)
    boxes = [moving_box(rng, grow=False), moving_box(rng, grow=False)]
    far = scenes.box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (30.0, -20.0, 10.0), (10.0, 20.0, 30.0), 1)
    return ([b for b, _ in boxes] + [far], [a for _, a in boxes] + [ObjectAnim()], [AnimChannel()] * 3,
            rt.reference_materials(), live_lights(rng, 2))


def scene_shipped():
    """(i) the shipped animation: the room, three moving boxes and a sphere."""
    base, anim = rt.reference_animation()
    return base, anim, [AnimChannel() for _ in base], rt.reference_materials(), rt.reference_lights()


BOX_SCENES = {"shipped": scene_shipped, "boxes_spheres": scene_boxes_spheres, "two_boxes": scene_two_boxes,
              "box_spheres": scene_box_spheres}


def box_records(buf, meta):
    m = meta if isinstance(meta, dict) else dict(zip(META, meta))
    off = m["off_boxes"] * 16
    return np.frombuffer(buf[off:off + m["n_boxes"] * BOXREC_BYTES].tobytes(), BOXREC)


def box_planes(buf, meta):
    """The (box, light) separating planes as uint32 [box, light, 4], or None:
    scenes of several boxes keep them right before the BVH (SceneLayout)."""
    m = meta if isinstance(meta, dict) else dict(zip(META, meta))
    nb, nl = m["n_boxes"], m["n_lights"]
    if nb < 2:
        return None
    off = (m["off_bvh"] - nb * nl) * 16
    assert off >= m["off_lightmat"] * 16
    return np.frombuffer(buf[off:off + nb * nl * 16].tobytes(), "<u4").reshape(nb, nl, 4)


def host_scene_blob(objs, mats, lights):
    """(blob bytes, meta dict) of rt_debug_scene_blob: what rt_scene_create uploads."""
    f = rt.lib().rt_debug_scene_blob
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    f.restype = C.c_int
    oa, ma, la = (Object * len(objs))(*objs), (Material * len(mats))(*mats), (Light * max(len(lights), 1))(*lights)
    meta = (C.c_int32 * 24)()
    n = f(oa, len(objs), ma, len(mats), la, len(lights), None, 0, meta)
    assert n > 0, rt.lib().rt_last_error()
    buf = np.zeros(n, np.uint8)
    assert f(oa, len(objs), ma, len(mats), la, len(lights), buf.ctypes.data, n, meta) == n
    return buf, dict(zip(META, meta))


class Blob:
    """The sections of a scene blob the sphere phases touch."""

    def __init__(self, buf, meta):
        m = meta if isinstance(meta, dict) else dict(zip(META, meta))
        self.meta, ns, nb = m, m["n_spheres"], m["n_boxes"]

        def sect(off, dtype, count):
            return np.frombuffer(buf[off * 16:off * 16 + count * dtype.itemsize].tobytes(), dtype)

        self.sph = sect(m["off_spheres"], SPHEREREC, ns)
        self.smeta = sect(m["off_smeta"], SPHEREMETA, ns)
        self.bvh = sect(m["off_bvh"], BVHNODE, m["n_bvh"])
        self.blink = sect(m["off_blink"], np.dtype("<u4"), m["n_bvh"] * 8)
        boxes = buf[m["off_boxes"] * 16:m["off_boxes"] * 16 + nb * BOXREC_BYTES].reshape(nb, BOXREC_BYTES)
        self.box_obj = np.frombuffer(boxes[:, BOX_OBJ_INDEX_AT:BOX_OBJ_INDEX_AT + 4].tobytes(), "<i4")
        lights = sect(m["off_lights"], np.dtype("<f4"), 4 * m["n_lights"]).reshape(-1, 4)
        self.n_live = int((lights[:, 3] == 0.0).sum())
        self.cones = (sect(m["off_cone"], SHADOWCONE, m["n_lights"] * ns).reshape(m["n_lights"], ns)
                      if m["off_cone"] >= 0 else None)
        self.masks = None
        if m["off_dmask"] >= 0:
            n = self.n_live * 6 * m["dmask_n"] ** 2
            self.masks = sect(m["off_dmask"], np.dtype("<u%d" % m["dmask_bytes"]), n).astype(np.uint64)

    def mask_bits_by_object(self, n_objs):
        """bool [live light x texel, object]: the mask bits, mapped from slot
        (spheres) and box number to obj_index."""
        out = np.zeros((len(self.masks), n_objs), bool)
        for s, i in enumerate(self.smeta["obj_index"]):
            out[:, i] = (self.masks >> np.uint64(s)) & np.uint64(1)
        if len(self.box_obj) >= 2:  # (build_scene: the boxes carry mask bits in scenes of several boxes)
            for b, i in enumerate(self.box_obj):
                out[:, i] = (self.masks >> np.uint64(len(self.smeta) + b)) & np.uint64(1)
        return out

    def subtree_slots(self, node):
        """Sphere slots under `node`, by the skip and leaf words: the nodes
        [node, skip) in depth-first order."""
        end = self.bvh["skip"][node] if self.bvh["skip"][node] >= 0 else len(self.bvh)
        slots = []
        for k in range(node, end):
            leaf = int(self.bvh["leaf"][k])
            if leaf:
                slots += list(range(leaf & 0xFFFFFF, (leaf & 0xFFFFFF) + (leaf >> 24)))
        return slots


def objects_extent(objs):
    """rt_scene.cpp objects_extent, float64."""
    ext = 0.0
    for o in objs:
        e = float(np.sqrt(sum(float(x) ** 2 for x in o.position)))
        corner = max([abs(float(o.radius))] + [abs(float(x)) for x in list(o.box_mins) + list(o.box_maxs)])
        e += corner * np.sqrt(3.0)
        if np.isfinite(e):
            ext = max(ext, e)
    return ext


def f32(u):
    return np.asarray(u, "<u4").view("<f4")


def ulps(a, b):
    """Distance in float32 steps between two float32 arrays of one sign pattern."""
    ia, ib = np.asarray(a, "<f4").view("<i4").astype(np.int64), np.asarray(b, "<f4").view("<i4").astype(np.int64)
    return np.abs(ia - ib)


def check_blob(got, host, objs_at_t, what):
    """Checks (a), (b), (d), (e) of a slot blob `got` at a time against the
    host-built scene `host` of the objects at that time. Returns (compared
    mask bits, differing mask bits as a list of (mask index, obj_index))."""
    n_objs = len(objs_at_t)
    # (a) records by obj_index, bitwise
    assert sorted(got.smeta["obj_index"]) == sorted(host.smeta["obj_index"]), what
    hslot = {int(i): s for s, i in enumerate(host.smeta["obj_index"])}
    for s, i in enumerate(got.smeta["obj_index"]):
        h = hslot[int(i)]
        assert np.array_equal(got.sph[s]["c"], host.sph[h]["c"]) and got.sph[s]["rr"] == host.sph[h]["rr"], (what, i)
        assert got.smeta[s]["radius"] == host.smeta[h]["radius"], (what, i, "SphereMeta::radius")
        assert got.smeta[s]["material"] == host.smeta[h]["material"], (what, i)
    # (b) every node's bounds hold every sphere of its subtree with build_bvh's margin (float64)
    extent = objects_extent(objs_at_t)
    covered = []
    for node in range(len(got.bvh)):
        slots = got.subtree_slots(node)
        assert slots, (what, node)
        if got.bvh["leaf"][node]:
            covered += slots
        lo, hi = got.bvh["lo"][node].astype(np.float64), got.bvh["hi"][node].astype(np.float64)
        for s in slots:
            c = f32(got.sph[s]["c"]).astype(np.float64)
            r = float(f32(got.smeta[s]["radius"]))
            reach = r + 1e-3 + 1e-4 * max(float(np.abs(c).max()) + r, extent)
            assert (lo <= c - reach).all() and (c + reach <= hi).all(), (what, node, s, lo, hi, c, reach)
    finite = [s for s in range(len(got.sph)) if np.isfinite(f32(got.sph[s]["c"])).all()
              and np.isfinite(np.sqrt(np.float64(f32(got.sph[s]["rr"]))))]
    assert sorted(covered) == finite, (what, "the leaves cover every finite sphere once")
    # (e) the ShadowCone entries, by obj_index
    assert (got.cones is None) == (host.cones is None), what
    if got.cones is not None:
        for s, i in enumerate(got.smeta["obj_index"]):
            g, h = got.cones[:, s], host.cones[:, hslot[int(i)]]
            assert np.array_equal(g["near"], h["near"]), (what, i, "near")
            for name in ("v", "far", "sph", "cph"):
                assert (ulps(g[name], h[name]) <= 1).all(), (what, i, name, g[name], h[name])
    # (d) the mask bits, by obj_index
    assert (got.masks is None) == (host.masks is None), what
    if got.masks is None:
        return 0, []
    assert got.meta["dmask_n"] == host.meta["dmask_n"] and got.meta["dmask_bytes"] == host.meta["dmask_bytes"], what
    a, b = got.mask_bits_by_object(n_objs), host.mask_bits_by_object(n_objs)
    n_bits = a.shape[0] * (len(got.smeta) + (len(got.box_obj) if len(got.box_obj) >= 2 else 0))
    diff = [(int(t), int(i)) for t, i in zip(*np.nonzero(a != b))]
    return n_bits, diff


def check_words(got, template, what):
    """(c) the topology is the template's: skip, leaf and link words, and the
    order of the spheres in their slots."""
    assert np.array_equal(got.bvh["skip"], template.bvh["skip"]), what
    assert np.array_equal(got.bvh["leaf"], template.bvh["leaf"]), what
    assert np.array_equal(got.blink, template.blink), what
    assert np.array_equal(got.smeta["obj_index"], template.smeta["obj_index"]), what
