"""The oracle's side of the adversarial ray families (adversarial_rays.py; no GPU).

First the tie to the reference's GL: the oracle's ray entry point and its
camera path are one function on the same input (the camera sets' rays, traced
as rays, give the camera frames' planes byte for byte, and the camera path is
pinned to llvmpipe by test_oracle_golden.py). Then the conditions each family
is built for, asserted on the oracle alone, so that the GPU comparison checks
what it is meant to check and can be plain equality.
"""
import numpy as np
import pytest

import adversarial_rays as ar
from oracle import port
from rays_common import set_f, set_r

F32 = np.float32


# ---- the ray path is the camera path ---------------------------------------------------
@pytest.mark.parametrize("make", [set_r, set_f], ids=["set_r", "set_f"])
def test_ray_path_equals_camera_path(make):
    rs = make()
    for d, want in rs.colors.items():
        assert port.trace_rays(rs.objs, rs.rays, d).tobytes() == want.tobytes(), d
    for probe, want in ((2, rs.p2), (3, rs.p3), (4, rs.p4)):
        assert port.trace_rays(rs.objs, rs.rays, probe=probe).tobytes() == want.tobytes(), probe
    assert np.array_equal(port.trace_rays(rs.objs, rs.rays, probe=1)[:, :3], rs.rays["dir"])
    # (n, 8) float32 rows are the same rays; the reserved words are ignored
    rows = rs.rays.view(F32).reshape(-1, 8).copy()
    rows[:, 3], rows[:, 7] = np.nan, -1e30
    assert port.trace_rays(rs.objs, rows, probe=2).tobytes() == rs.p2.tobytes()


def test_trace_rays_arguments():
    sc = ar.scene("aabox")
    assert port.trace_rays(sc.objs, np.zeros((0, 8), F32)).shape == (0, 4)
    with pytest.raises(ValueError):
        port.trace_rays(sc.objs, np.zeros((1, 8), F32), probe=5)
    with pytest.raises(ValueError):
        port.trace_rays(sc.objs, np.zeros((1, 8), F32), max_depth=-1)
    # the direction as given: never normalised
    r = ar.make_rays([(0.0, 0.0, 5.0)], [(0.0, 0.0, -4.0)])
    assert port.trace_rays(sc.objs, r, probe=1)[0].tolist() == [0.0, 0.0, -4.0, 0.0]
    assert port.trace_rays(sc.objs, r, probe=2, **sc.kw)[0, :2].tolist() == [2.0, 1.75]  # the floor's top, z = -2
    # one thread or many: the same planes
    f = ar.family("aabox", "GRAZE")
    assert port.trace_rays(sc.objs, f.rays, 2, threads=1, **sc.kw).tobytes() == f.color(2).tobytes()


# ---- the families' conditions ------------------------------------------------------------
@pytest.mark.parametrize("fam", ar.FAMILIES)
@pytest.mark.parametrize("sn", ar.SCENES)
def test_every_plane_is_finite_and_the_family_is_small(sn, fam):
    f = ar.family(sn, fam)
    assert 0 < f.n <= ar.MAX_RAYS
    assert np.isfinite(f.rays["origin"]).all() and np.isfinite(f.rays["dir"]).all()
    for d in ar.DEPTHS:
        assert np.isfinite(f.color(d)).all(), d
    for k in (2, 3, 4):
        assert np.isfinite(f.plane(k)).all(), k
    miss = f.obj < 0
    assert (f.p2[miss, 1:] == 0).all() and (f.p3[miss] == 0).all() and (f.p4[miss] == 0).all()
    # seeded: a second build gives the same rays
    assert ar._MAKERS[fam](f.sc).rays.tobytes() == f.rays.tobytes()


@pytest.mark.parametrize("sn", ar.SCENES)
def test_axis(sn):
    f = ar.family(sn, "AXIS")
    d = ar.AXIS_DIRS
    assert sorted(((d == 0).sum(-1)).tolist()) == [0] * 8 + [1] * 12 + [2] * 6
    assert (np.abs(ar.kernel_norm2(f.rays["dir"]) - F32(1)) <= F32(2.0 ** -22)).all()
    obj, t = f.obj, f.t
    assert (obj >= 0).mean() >= 0.25
    assert len(np.unique(obj[obj >= 0])) >= min(6, len(f.sc.objs))
    if sn in ("room16", "aabox"):  # origins on surfaces
        assert ((obj >= 0) & (t > 0) & (t < 1e-3)).sum() >= 20
    o = f.rays["origin"]
    assert ((o == 0).sum(-1) == 1).any() and ((o == 0).sum(-1) == 2).any() and ((o == 0).sum(-1) == 3).any()
    for lt in f.sc.lights:
        assert (o == np.array(lt.position[:], F32)).all(-1).any()


@pytest.mark.parametrize("sn", ar.SCENES)
def test_graze(sn):
    f = ar.family(sn, "GRAZE")
    sph = f.meta["kind"] == 0
    share = (f.obj[sph] == f.meta["target"][sph]).mean()
    assert 0.2 <= share <= 0.8, share
    assert (np.abs(ar.kernel_norm2(f.rays["dir"]) - F32(1)) <= F32(2.0 ** -22)).all()
    assert (np.abs(f.rays["origin"]) <= 9.5).all()
    boxes = [o for o in f.sc.objs if ar.is_box(o) and not ar.is_room(o)]
    assert (~sph).sum() == len(boxes) * 3 * 8 * len(ar.EPS)
    if boxes:  # the silhouettes are hit and missed
        own = f.obj[~sph] == f.meta["target"][~sph]
        assert own.any() and not own.all()


@pytest.mark.parametrize("sn", ar.SCENES)
def test_scale(sn):
    f = ar.family(sn, "SCALE")
    nb, si = f.meta["n_base"], f.meta["s_index"]
    assert 150 <= nb <= 200 and f.n == nb * len(ar.SCALES)
    base = ar.scale_base(f.sc)
    unit = port.trace_rays(f.sc.objs, base, probe=2, **f.sc.kw)
    uobj, ut = unit[:, 0], unit[:, 1]
    assert (uobj >= 0).sum() >= 50
    for s in (2.0, 0.5):
        k = si == ar.SCALES.index(s)
        assert np.array_equal(f.rays["dir"][k], base["dir"] * F32(s))
        assert np.array_equal(f.p2[k, 0], uobj)
        normal = (uobj >= 0) & (ut >= np.finfo(F32).tiny * 4)
        assert normal.sum() >= 50
        assert np.array_equal(f.t[k][normal], (ut / F32(s))[normal])
    for s in (0.0, 1e-38, 2.0 ** -62):
        k = si == ar.SCALES.index(s)
        assert (f.obj[k] < 0).all(), s
    d = f.rays["dir"][si == ar.SCALES.index(1e-38)]
    tiny = np.finfo(F32).tiny
    assert ((d != 0) & (np.abs(d) < tiny)).any()  # denormal components
    assert (f.rays["dir"][si == ar.SCALES.index(0.0)] == 0).all()
    # the unit gate as the kernel computes it
    gate = F32(2.0 ** -19)
    for s in ar.SCALES:
        err = np.abs(ar.kernel_norm2(f.rays["dir"][si == ar.SCALES.index(s)]) - F32(1))
        if s in ar.S_IN_GATE:
            assert (err <= gate).all(), s
        else:
            assert (err > gate).all(), s
    # the chosen factor: hits and misses across the 10000 horizon
    assert 2.0 ** -12 < ar.S_CHOSEN < 2.0 ** -8
    k = si == ar.SCALES.index(ar.S_CHOSEN)
    hits, misses = int((f.obj[k] >= 0).sum()), int((f.obj[k] < 0).sum())
    assert (hits, misses) == ar.SCALE_HORIZON[sn]
    assert hits >= 20 and misses - int((uobj < 0).sum()) >= 20  # (misses the unit rays do not have)


@pytest.mark.parametrize("sn", ar.SCENES)
def test_far(sn):
    f = ar.family(sn, "FAR")
    o = f.rays["origin"]
    assert f.n == len(ar.FAR_V) * 3 * 2 * 8
    for v in ar.FAR_V:
        for axis in range(3):
            for sign in (1, -1):
                assert (o[:, axis] == F32(sign) * v).sum() >= 8
    assert ar.FAR_V[1] == 1024 and ar.FAR_V[2] > 1024 and ar.FAR_V[0] < 1024
    assert (np.abs(ar.kernel_norm2(f.rays["dir"]) - F32(1)) <= F32(2.0 ** -22)).all()
    if sn == "spheres63":
        assert (f.obj >= 0).mean() >= 0.3 and len(np.unique(f.obj[f.obj >= 0])) >= 10
        assert f.t.max() > 4000.0 and (f.obj[f.meta["v"] >= 1e5] < 0).all()  # (beyond the 10000 horizon: misses)


@pytest.mark.parametrize("sn", ar.SCENES)
def test_continued(sn):
    f = ar.family(sn, "CONTINUED")
    for off in (0, 1):
        k = f.meta["offset"] == off
        same = f.obj[k] == f.meta["start"][k]
        leaves = (f.obj[k] >= 0) & ~same
        assert same.sum() >= 10 and leaves.sum() >= 10, (off, same.sum(), leaves.sum())
    # the origins are the source families' hit points, exactly, and those pushed out by 0.01 n
    src = [ar.family(sn, "AXIS"), ar.family(sn, "GRAZE")]
    pts = {tuple(p) for fam in src for p in fam.p4[fam.obj >= 0, :3].tolist()}
    on = f.rays["origin"][f.meta["offset"] == 0]
    assert all(tuple(p) in pts for p in on.tolist())
    # (a float32 reflection keeps the length to a few ulps: nearly every ray stays inside the unit gate)
    assert (np.abs(ar.kernel_norm2(f.rays["dir"]) - F32(1)) <= F32(2.0 ** -19)).mean() >= 0.9


@pytest.mark.parametrize("sn", ar.SCENES)
def test_length(sn):
    f = ar.family(sn, "LENGTH")
    spheres = [i for i, o in enumerate(f.sc.objs) if not ar.is_box(o) and o.radius != -1.0]
    assert f.n == ar.LENGTH_PER_SPHERE * len(spheres)
    err = np.abs(ar.kernel_norm2(f.rays["dir"]) - F32(1))
    assert (err > F32(2.0 ** -19)).all() and (err <= F32(0.5)).all()  # outside the unit gate, inside one of 0.5
    assert (f.meta["length"] == F32(1.2)).mean() == 0.75
    # the rays reach spheres that reflect or refract, so the children start on spheres (shipped and aabox have a
    # floor slab across the scene: the origins below it, under half of them, see no sphere)
    on_sphere = np.isin(f.obj, spheres)
    assert on_sphere.mean() >= 0.5
    mats = port.reference_materials()
    deep = np.array([mats[o.material].reflectivity > 0 or mats[o.material].transparency > 0 for o in f.sc.objs] + [False])
    assert (deep[f.obj] & on_sphere).mean() >= 0.5
    assert (f.color(5) != f.color(0)).any()


def test_scenes():
    assert [len(ar.scene(s).objs) for s in ar.SCENES] == [17, 64, 101, 5, 6, 17]  # (spheres63: bench_objects(64) less its room)
    assert not any(ar.is_room(o) for o in ar.scene("spheres63").objs)
    for o in ar.scene("aabox").objs:
        assert o.angles[:] == [0.0, 0.0, 0.0]
    sheet = ar.scene("aabox").objs[5]
    assert F32(sheet.box_maxs[1]) == F32(0.01) and F32(sheet.box_mins[1]) == F32(-0.01)
    le = ar.scene("lights_edge")
    a, b = le.objs[2], le.objs[5]
    assert le.lights[0].position[:] == a.position[:]
    off = np.array(le.lights[1].position[:], F32) - np.array(b.position[:], F32)
    assert off[0] == 0 and off[1] == 0 and abs(float(off[2]) - b.radius) <= 2.0 ** -21
    assert le.lights[2].position[0] == 10.5  # the wall at x = 11, minus 0.5


def test_arrangements():
    assert ar.poison_slots(64 * 7 + 5).tolist() == [0, 128 + 31, 256 + 63, 384]
    assert ar.poison_slots(30).tolist() == [0]
    for sn in ar.SCENES:
        p = ar.poison(sn)
        assert p.rays["origin"][0, 0] == 5000 and abs(ar.kernel_norm2(p.rays["dir"])[0] - 1) <= 2.0 ** -22
        assert np.isfinite(p.color(5)).all()
        cs = ar.camera_set(sn)
        assert cs.n >= 144 and set(ar.DEPTHS) <= set(cs.colors)
    assert ar.hexf(np.array([1.0, -0.5, 0.0], F32)) == "(0x1.0000000000000p+0, -0x1.0000000000000p-1, 0x0.0p+0)"
