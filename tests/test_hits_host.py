"""Host side of the primary-hit buffers (rt_render_hits*, rt_pick; no GPU):
the record's layout, the exported symbols and the NULL-context errors."""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd import abi

SYMBOLS = ["rt_render_hits_view", "rt_render_hits", "rt_render_hits_animated", "rt_pick"]


def test_hit_record_layout():
    assert C.sizeof(abi.Hit) == 16
    assert [getattr(abi.Hit, f).offset for f in ("object", "t", "shadow", "material")] == [0, 4, 8, 12]
    assert abi.HIT_DTYPE.itemsize == 16
    assert [abi.HIT_DTYPE.fields[f][1] for f in ("object", "t", "shadow", "material")] == [0, 4, 8, 12]
    # the two descriptions are one record
    h = abi.Hit(3, 1.5, 5, 2)
    a = np.frombuffer(bytes(memoryview(h)), abi.HIT_DTYPE)[0]
    assert (int(a["object"]), float(a["t"]), int(a["shadow"]), int(a["material"])) == (3, 1.5, 5, 2)
    assert abi.RT_HITS_SHADOW == 1


@pytest.mark.parametrize("name", SYMBOLS)
def test_library_exports_the_hits_symbols(name):
    assert hasattr(rt.lib(), name)


def _null_context_calls():
    L = rt.lib()
    view = rt.make_view(None, 0.0)
    hits = np.zeros((4, 4), abi.HIT_DTYPE)
    planes = np.zeros((2, 4, 4, 4), np.float32)
    h, n, p = hits.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data
    hit = abi.Hit()
    return {
        "rt_render_hits_view": lambda: L.rt_render_hits_view(None, None, C.byref(view), 4, 4, 0, 4, 1, h, n, p, 0, None),
        "rt_render_hits": lambda: L.rt_render_hits(None, None, None, 0.0, 4, 4, 0, 4, 1, h, n, p, 0, None),
        "rt_render_hits_animated": lambda: L.rt_render_hits_animated(None, None, None, 0.0, 4, 4, 0, 4, 1, h, n, p, 0,
                                                                     None),
        "rt_pick": lambda: L.rt_pick(None, None, C.byref(view), 4, 4, 1, 1, 1, C.byref(hit), n, p),
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
