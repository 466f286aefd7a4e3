"""Host side of adaptive anti-aliasing (rt_render_aa*, rt_aa_last_counts,
rt_aa_edge_mask; no GPU): the exported symbols, the NULL-context errors, and
the criterion itself — rt_aa_edge_mask against its restatement in numpy
(tests/aa_common.py) over oracle frames."""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt
from openglraytracer_amd import abi

from aa_common import np_edge_mask, np_tile_masks, oracle_base

SYMBOLS = ["rt_render_aa_view", "rt_render_aa", "rt_aa_last_counts", "rt_aa_edge_mask"]
THRESHOLDS = [-1.0, 0.0, 0.25, float("inf")]


@pytest.mark.parametrize("name", SYMBOLS)
def test_library_exports_the_aa_symbols(name):
    assert hasattr(rt.lib(), name)


def test_python_wrappers_exist():
    assert callable(rt.render_aa) and callable(rt.aa_last_counts) and callable(rt.aa_edge_mask)


def _null_context_calls():
    L = rt.lib()
    view = rt.make_view(None, 0.0)
    out = np.zeros((4, 4, 4), np.float32)
    mask = np.zeros((4, 4), np.uint8)
    px, tiles = C.c_int64(0), C.c_int64(0)
    o, m = out.ctypes.data, mask.ctypes.data
    return {
        "rt_render_aa_view": lambda: L.rt_render_aa_view(None, None, C.byref(view), 4, 4, 0, 2, 0, 0.1, o, m, 0, None),
        "rt_render_aa": lambda: L.rt_render_aa(None, None, None, 0.0, 4, 4, 0, 2, 0, 0.1, o, m, 0, None),
        "rt_aa_last_counts": lambda: L.rt_aa_last_counts(None, C.byref(px), C.byref(tiles)),
    }


@pytest.mark.parametrize("name", SYMBOLS[:3])
def test_null_context_is_refused(name):
    L = rt.lib()
    # another failure first, so that the message below is this call's own
    assert L.rt_write_pfm(None, None, 0, 0) == abi.RT_ERR_INVALID
    rc = _null_context_calls()[name]()
    assert rc == abi.RT_ERR_INVALID
    msg = L.rt_last_error()
    assert len(msg) > 0 and b"null context" in msg, msg


def _planted():
    """An oracle frame with NaNs and infinities planted: a whole NaN pixel, a
    NaN in one channel beside a large step in another, +inf, -inf next to +inf
    (their difference is infinite) and two equal infinities side by side
    (their difference is NaN)."""
    f = oracle_base("shipped", 33, 17, 0).copy()
    f[3, 4, :3] = np.nan
    f[8, 20, 0] = np.nan
    f[8, 20, 1] = 50.0
    f[12, 7, :3] = np.inf
    f[12, 8, :3] = -np.inf
    f[5, 30, 2] = np.inf
    f[5, 31, 2] = np.inf
    f[16, 32, 1] = np.inf  # the frame's last pixel
    f[0, 0, 0] = np.nan
    return f


FRAMES = {
    "shipped_d0": lambda: oracle_base("shipped", 96, 54, 0),
    "shipped_d2": lambda: oracle_base("shipped", 96, 54, 2),
    "bench16_d0": lambda: oracle_base("bench16", 96, 54, 0),
    "ragged_33x17": lambda: oracle_base("shipped", 33, 17, 0),
    "one_pixel": lambda: oracle_base("shipped", 33, 17, 0)[5:6, 9:10],
    "one_by_five": lambda: oracle_base("shipped", 33, 17, 0)[4:9, 16:17],
    "five_by_one": lambda: oracle_base("shipped", 33, 17, 0)[4:5, 14:19],
    "planted": _planted,
}


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_edge_mask_equals_the_numpy_criterion(name, threshold):
    frame = np.ascontiguousarray(FRAMES[name]())
    want = np_edge_mask(frame, threshold)
    mask, tiles = rt.aa_edge_mask(frame, threshold)
    h, w = frame.shape[:2]
    assert mask.shape == (h, w) and mask.dtype == np.uint8
    assert tiles.shape == ((h + 7) // 8, (w + 7) // 8) and tiles.dtype == np.uint64
    assert np.array_equal(mask, want.astype(np.uint8)), (name, threshold, int(mask.sum()), int(want.sum()))
    # the tile words, the ragged right and top tiles included: bits outside the frame are 0
    assert np.array_equal(tiles, np_tile_masks(want)), (name, threshold)
    if threshold == float("inf"):
        assert not mask.any() and not tiles.any()
    if threshold < 0 and h * w > 1 and name != "planted":
        assert mask.all()  # every pixel has a neighbour, and |difference| >= 0 > threshold
    if h * w == 1:
        assert not mask.any()  # no neighbour inside the frame


def test_the_criterion_on_nan_and_inf():
    """A NaN difference does not flag, an infinite one does, both sides of an edge are flagged."""
    f = np.zeros((1, 6, 4), np.float32)
    f[0, 1, :3] = np.nan  # pixels 0-2: only NaN differences
    f[0, 4, 0] = np.inf   # pixels 3-5: infinite differences on both sides of pixel 4
    mask, tiles = rt.aa_edge_mask(f, 1e30)
    assert mask.tolist() == [[0, 0, 0, 1, 1, 1]]
    assert int(tiles[0, 0]) == 0b111000
    assert not rt.aa_edge_mask(f, float("inf"))[0].any()
    g = np.zeros((2, 2, 4), np.float32)
    g[:, :, 3] = [[0.0, 9.0], [7.0, 3.0]]  # alpha is not a colour channel
    assert not rt.aa_edge_mask(g, 0.0)[0].any()
    g[1, 1, 2] = 0.5
    assert rt.aa_edge_mask(g, 0.25)[0].tolist() == [[0, 1], [1, 1]]
    assert rt.aa_edge_mask(g, 0.5)[0].tolist() == [[0, 0], [0, 0]]  # strictly greater


def test_edge_mask_outputs_are_optional_but_not_both():
    L = rt.lib()
    f = np.ascontiguousarray(oracle_base("shipped", 33, 17, 0))
    want = np_edge_mask(f, 0.25)
    mask = np.zeros((17, 33), np.uint8)
    tiles = np.zeros((3, 5), np.uint64)
    assert L.rt_aa_edge_mask(f.ctypes.data, 33, 17, 0.25, mask.ctypes.data, None) == abi.RT_OK
    assert L.rt_aa_edge_mask(f.ctypes.data, 33, 17, 0.25, None, tiles.ctypes.data) == abi.RT_OK
    assert np.array_equal(mask, want.astype(np.uint8)) and np.array_equal(tiles, np_tile_masks(want))
    assert L.rt_aa_edge_mask(f.ctypes.data, 33, 17, 0.25, None, None) == abi.RT_ERR_INVALID


@pytest.mark.parametrize("args", [
    ("null", 4, 4, 0.1), ("frame", 0, 4, 0.1), ("frame", 4, 0, 0.1), ("frame", -1, 4, 0.1), ("frame", 65537, 1, 0.1),
    ("frame", 4, 4, float("nan")),
])
def test_edge_mask_parameter_errors(args):
    L = rt.lib()
    f = np.zeros((4, 4, 4), np.float32)
    mask = np.zeros((4, 4), np.uint8)
    which, w, h, thr = args
    assert L.rt_write_pfm(None, None, 0, 0) == abi.RT_ERR_INVALID
    rc = L.rt_aa_edge_mask(f.ctypes.data if which == "frame" else None, w, h, thr, mask.ctypes.data, None)
    assert rc == abi.RT_ERR_INVALID
    assert len(L.rt_last_error()) > 0
    assert not mask.any()
