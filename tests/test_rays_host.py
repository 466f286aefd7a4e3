"""Host side of the ray queries (rt_trace_rays, rt_view_rays; no GPU): the
record's layout, the exported symbols, the NULL-context errors, the panorama
tool's ray generator, and the oracle's side of the GPU tests' ray sets."""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd import abi
from rays_common import FORWARD, check_set_f, check_set_r, panorama_rays, set_f, set_r

SYMBOLS = ["rt_trace_rays", "rt_view_rays"]


def test_ray_record_layout():
    assert C.sizeof(abi.Ray) == 32
    assert [getattr(abi.Ray, f).offset for f in ("origin", "reserved0", "dir", "reserved1")] == [0, 12, 16, 28]
    assert abi.RAY_DTYPE.itemsize == 32
    assert [abi.RAY_DTYPE.fields[f][1] for f in ("origin", "reserved0", "dir", "reserved1")] == [0, 12, 16, 28]
    # the two descriptions are one record
    r = abi.Ray((1.0, 2.0, 3.0), 4.0, (5.0, 6.0, 7.0), 8.0)
    a = np.frombuffer(bytes(memoryview(r)), abi.RAY_DTYPE)[0]
    assert a["origin"].tolist() == [1.0, 2.0, 3.0] and a["dir"].tolist() == [5.0, 6.0, 7.0]
    assert (float(a["reserved0"]), float(a["reserved1"])) == (4.0, 8.0)
    assert abi.RT_MAX_RAYS == 1 << 28


@pytest.mark.parametrize("name", SYMBOLS)
def test_library_exports_the_ray_symbols(name):
    assert hasattr(rt.lib(), name)


def _null_context_calls():
    L = rt.lib()
    view = rt.make_view(None, 0.0)
    rays = np.zeros(16, abi.RAY_DTYPE)
    planes = np.zeros((4, 16, 4), np.float32)
    c, h, n, p = (planes[k].ctypes.data for k in range(4))
    return {
        "rt_trace_rays": lambda: L.rt_trace_rays(None, None, rays.ctypes.data, 16, 0, 1, c, h, n, p, 0, None),
        "rt_view_rays": lambda: L.rt_view_rays(None, C.byref(view), 4, 4, 0, 4, rays.ctypes.data, 0, None),
    }


@pytest.mark.parametrize("name", SYMBOLS)
def test_null_context_is_refused(name):
    L = rt.lib()
    # another failure first, so that the message below is this call's own
    assert L.rt_write_pfm(None, None, 0, 0) == abi.RT_ERR_INVALID
    rc = _null_context_calls()[name]()
    assert rc == abi.RT_ERR_INVALID
    msg = L.rt_last_error()
    assert len(msg) > 0 and b"null context" in msg, msg


def test_panorama_rays():
    """8 x 4: unit directions, the centre column forward, the poles in the top and bottom rows."""
    origin = (1.5, -2.0, 0.25)
    rays = panorama_rays(origin, 8, 4)
    assert rays.shape == (4, 8) and rays.dtype == abi.RAY_DTYPE
    assert (rays["origin"] == np.asarray(origin, np.float32)).all()
    assert (rays["reserved0"] == 0).all() and (rays["reserved1"] == 0).all()
    d = rays["dir"].astype(np.float64)
    assert (np.abs(np.linalg.norm(d, axis=-1) - 1.0) <= 2.0 ** -23).all()
    eps = 2.0 ** -23
    # the centre column: no sideways component, forward of the vertical axis
    assert FORWARD == (0.0, 1.0, 0.0)
    assert (np.abs(d[:, 4, 0]) <= eps).all() and (d[1:3, 4, 1] > 0.5).all()
    # column 0 looks straight back, the quarter columns left and right
    assert (d[1:3, 0, 1] < -0.5).all() and (d[1:3, 2, 0] < -0.5).all() and (d[1:3, 6, 0] > 0.5).all()
    # row 0 (the bottom row) is the -z pole, the top row the +z pole, in every column
    assert (np.abs(d[0] - np.array([0.0, 0.0, -1.0])) <= eps).all()
    assert (np.abs(d[3] - np.array([0.0, 0.0, 1.0])) <= eps).all()
    # the rows between lie at latitudes -30 and +30 degrees
    assert (np.abs(d[1, :, 2] + 0.5) <= eps).all() and (np.abs(d[2, :, 2] - 0.5) <= eps).all()
    # no direction twice off the poles
    assert len({tuple(v) for v in rays["dir"][1:3].reshape(-1, 3).tolist()}) == 16


def test_ray_sets_meet_their_conditions():
    """The oracle's output for the GPU tests' ray sets: what each set was built to hold."""
    r = set_r()
    assert r.n == 7 * 144 and sorted(r.perm.tolist()) == list(range(r.n))
    assert np.array_equal(r.unpermute(r.p2[r.perm]), r.p2)
    check_set_r(r)
    f = set_f()
    assert f.n == 3 * 32 * 18
    check_set_f(f)
    # unit directions: the ray kernels keep such rays on their culled paths unless the origin is far
    for s in (r, f):
        d = s.rays["dir"]
        assert (np.abs((d * d).sum(-1) - 1.0) <= 2.0 ** -21).all()
