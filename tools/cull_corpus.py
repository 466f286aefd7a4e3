#!/usr/bin/env python3
"""Digests of what the scene builder and the animate kernel's host run derive
(rt_debug_scene_blob, rt_debug_anim_host_blob, rt_debug_anim_validate) over a
corpus of scenes: one line per case, sha256 of the blob and its 24 meta ints.
Run it on two builds and diff the outputs: a change that only moves text
(rt_cull.h) leaves every line as it was.

    python tools/cull_corpus.py > tree.txt      (in each checkout)
"""
import glob
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import openglraytracer_amd as rt  # noqa: E402
from anim_spheres_common import BLOB_SCENES, host_scene_blob  # noqa: E402
from openglraytracer_amd import abi  # noqa: E402
from openglraytracer_amd.abi import AnimChannel, ObjectAnim  # noqa: E402
from test_anim_spheres_host import TIMES, room_and_spheres  # noqa: E402
from test_gpu_anim import EDGE_TIMES, edge_scene  # noqa: E402

GOLDEN_TIMES = [float(t) for t in np.load(os.path.join(ROOT, "tests", "golden", "box_llvmpipe.npz"))["time"]]


def line(what, buf, meta):
    meta = [meta[k] for k in meta] if isinstance(meta, dict) else list(meta)
    print(what, hashlib.sha256(bytes(buf)).hexdigest()[:24], hashlib.sha256(repr(meta).encode()).hexdigest()[:12])


def scene(what, objs, mats=None, lights=None):
    mats = mats if mats is not None else rt.reference_materials()
    lights = lights if lights is not None else rt.reference_lights()
    line("scene " + what, *host_scene_blob(objs, mats, lights))


def main():
    for n in (16, 64, 256):
        scene("bench%d" % n, rt.bench_objects(n, 0))
    base, anim = rt.reference_animation()
    for t in GOLDEN_TIMES:
        scene("shipped t=%r" % t, rt.animate_objects(base, anim, t))
    for path in sorted(glob.glob(os.path.join(ROOT, "scenes", "*.json"))):
        objs, mats, lights, _ = rt.parse_scene(open(path).read(), 0.0)
        scene(os.path.basename(path), objs, mats, lights)
    for seed in range(17):
        b, a, mats, lights, _ = edge_scene(seed)
        for t in EDGE_TIMES:
            scene("edge%d t=%r" % (seed, t), rt.animate_objects(b, a, t), mats, lights)
    shipped = (base, anim, [AnimChannel() for _ in base], rt.reference_materials(), rt.reference_lights())
    for name, make in list(BLOB_SCENES.items()) + [("shipped", lambda: shipped)]:
        b, a, r, mats, lights = make()
        for t in TIMES + GOLDEN_TIMES:
            scene("%s t=%r" % (name, t), rt.animate_objects(b, a, t, r), mats, lights)
            line("hook %s t=%r" % (name, t), *rt.anim_host_blob(b, a, r, mats, lights, t))
    # non-finite objects: a box and a sphere at infinity, among finite ones
    b, a, r, mats, lights = BLOB_SCENES["boxes_spheres"]()
    is_box = [any(x != 0.0 for x in list(o.box_mins) + list(o.box_maxs)) for o in b]
    for i in (is_box.index(True), len(b) - 1 - is_box[::-1].index(True), is_box.index(False)):
        for k, v in enumerate((float("inf"), float("-inf"), float("nan"))):
            objs = rt.animate_objects(b, a, 0.5, r)
            objs[i].position[k] = v
            scene("non-finite object %d (%s) %r" % (i, "box" if is_box[i] else "sphere", v), objs, mats, lights)
    # the validation hook's codes and messages
    mv = AnimChannel(abi.RT_ANIM_SIN_OFFSET, 1.0, 1.0, 0.5)
    for n, field, boxes_only in ((32, None, False), (32, None, True), (33, None, False), (8, "a", False),
                                 (8, "k", False)):
        b, a, r = room_and_spheres(n)
        a[5].position[1] = mv
        if field:
            setattr(a[5].position[1], field, float("nan"))
        print("validate", n, field, boxes_only, rt.anim_validate(b, a, r, boxes_only=boxes_only))
    b, a, r = room_and_spheres(4)
    print("validate frames", rt.anim_validate(b, a, r, max_frames=0), [ObjectAnim().scale.kind])


if __name__ == "__main__":
    main()
