"""Tile runs of the persistent depth-0 launch (rt_internal.h persistent_first_run
and persistent_next_run, the pair render_persistent0 walks a chunk with, here
through the host-only rt_debug_persistent_runs; the chunks through
rt_debug_persistent_chunk): the runs of every chunk are exactly the chunk's
items in order, a run lies in one tile row of one view and is as long as the
row and the chunk allow, and every item of the launch is in one run.

The small launches are those of tests/test_gpu_tile_runs.py on the forced
grids of 8 and 9 work-groups (32 and 36 waves); the file asserts that they
hold the cases they were chosen for.
"""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt

# (width, height, views) of tests/test_gpu_tile_runs.py
SHAPES = [(8, 8, 40), (9, 8, 17), (17, 9, 17), (136, 16, 40), (72, 40, 9)]
WAVES = [32, 36]  # set_persistent0(8), (9): four waves per work-group
CAP = 64

_RANGE = np.zeros(2, np.int32)
_RUNS = np.zeros(4 * CAP, np.int32)


def _hooks():
    chunk = rt.lib().rt_debug_persistent_chunk
    chunk.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    chunk.restype = C.c_int
    runs = rt.lib().rt_debug_persistent_runs
    runs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    runs.restype = C.c_int
    return chunk, runs


def _tiles(w, h):
    return (w + 7) // 8, (h + 7) // 8


def _chunks(chunk, total, waves):
    """The launch's chunks [(t, t_end)]: ids 0, 1, ... up to the first empty one; they tile [0, total)."""
    out, t = [], 0
    ptr = _RANGE.ctypes.data
    for c in range(total + 1):
        assert chunk(c, total, waves, ptr) == 0
        a, b = int(_RANGE[0]), int(_RANGE[1])
        if a >= b:
            break
        assert a == t and b <= total
        out.append((a, b))
        t = b
    assert t == total
    return out


def _runs(runs, t, t_end, w, h):
    _RUNS[:] = -7
    n = runs(t, t_end, w, h, _RUNS.ctypes.data, CAP)
    assert 0 < n <= CAP
    return [tuple(int(x) for x in _RUNS[4 * k:4 * k + 4]) for k in range(n)]


def _check_chunk(got, t, t_end, wtx, wty):
    """`got`, the runs (view, row, column, tiles) of items [t, t_end): the items in order, none
    across a row's end, each as long as its row and the chunk allow."""
    at = t
    for z, wy, wx, n in got:
        assert 0 <= wx < wtx and 0 <= wy < wty and z >= 0 and n >= 1
        assert (z * wty + wy) * wtx + wx == at  # the run begins where the one before ended
        assert wx + n <= wtx  # one row of one view
        at += n
        assert at == t_end or wx + n == wtx  # maximal: it ends with the chunk or with its row
    assert at == t_end


def _expected(t, t_end, wtx, wty):
    """The runs from the items themselves: item -> (view, row, column), consecutive items of one row."""
    out = []
    for i in range(t, t_end):
        z, r = divmod(i, wtx * wty)
        wy, wx = divmod(r, wtx)
        if out and out[-1][:2] == (z, wy):
            out[-1] = out[-1][:3] + (out[-1][3] + 1,)
        else:
            out.append((z, wy, wx, 1))
    return out


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("w,h,views", SHAPES)
def test_runs_partition_every_chunk_in_order(w, h, views, waves):
    chunk, runs = _hooks()
    wtx, wty = _tiles(w, h)
    total = wtx * wty * views
    seen = np.zeros(total, np.int32)
    for t, t_end in _chunks(chunk, total, waves):
        got = _runs(runs, t, t_end, w, h)
        _check_chunk(got, t, t_end, wtx, wty)
        assert got == _expected(t, t_end, wtx, wty)
        for z, wy, wx, n in got:
            first = (z * wty + wy) * wtx + wx
            seen[first:first + n] += 1
    assert (seen == 1).all()  # every item of the launch once


def test_the_flagship_launch_on_the_whole_chip():
    """256 views of 1920 x 1080 on 2,048 work-groups (8,192 waves): every chunk."""
    chunk, runs = _hooks()
    w, h, views, waves = 1920, 1080, 256, 8192
    wtx, wty = _tiles(w, h)
    total = wtx * wty * views
    rptr, optr = _RANGE.ctypes.data, _RUNS.ctypes.data
    t, c, n_runs, longest = 0, 0, 0, 0
    while t < total:
        assert chunk(c, total, waves, rptr) == 0
        a, b = int(_RANGE[0]), int(_RANGE[1])
        assert a == t and a < b <= total  # the chunks tile the items, so every item is in one chunk
        n = runs(a, b, w, h, optr, CAP)
        assert 1 <= n <= 2  # (240 tiles per row, chunks of 16 at most)
        _check_chunk([tuple(int(x) for x in _RUNS[4 * k:4 * k + 4]) for k in range(n)], a, b, wtx, wty)
        n_runs += n
        longest = max(longest, int(_RUNS[3]))
        t, c = b, c + 1
    assert longest == 16
    # a row of 240 tiles is a whole number of chunks of every size and the regions start on
    # multiples of their sizes: at this frame size a chunk is one run
    assert n_runs == c


def _spans(chunks, period):
    """Chunks with a multiple of `period` strictly inside: they hold the end of a row (view)."""
    return [(a, b) for a, b in chunks if (b - 1) // period > a // period]


def test_the_small_launches_hold_the_cases_they_are_for():
    chunk, runs = _hooks()
    for waves in WAVES:
        # 8 x 8: one tile per view, every run has length 1 (and the slot is refilled for every tile)
        for a, b in _chunks(chunk, 40, waves):
            assert all(r[3] == 1 for r in _runs(runs, a, b, 8, 8))
        # 136 x 16 x 40: 17 tiles per row, 34 per view, 1,360 items: chunks of every size
        w, h, views = 136, 16, 40
        wtx, wty = _tiles(w, h)
        assert (wtx, wty) == (17, 2)
        chunks = _chunks(chunk, wtx * wty * views, waves)
        for size in (16, 8, 4, 2):
            rows = [ab for ab in _spans(chunks, wtx) if ab[1] - ab[0] == size]
            assert rows, (waves, size)  # a chunk of this size spans a row end
            assert len(_runs(runs, *rows[0], w, h)) >= 2
        crossing = _spans(chunks, wtx * wty)
        assert crossing  # a chunk spans a view end
        got = _runs(runs, *crossing[0], w, h)
        assert len({r[0] for r in got}) == 2
        last_first = [(a, b) for a, b in chunks if a % wtx == wtx - 1 and b - a > 1]
        assert last_first  # a chunk's first item is its row's last tile
        got = _runs(runs, *last_first[0], w, h)
        assert got[0][2:] == (wtx - 1, 1) and got[1][2] == 0
        assert any(b - a == 16 and (b % wtx) == wtx - 1 for a, b in chunks)  # ... and one ends a tile short of a row end
        # 9 x 8 and 17 x 9: two and three tiles per row, 72 x 40: nine; runs cut by row ends and by chunk ends
        for w, h, views in ((9, 8, 17), (17, 9, 17), (72, 40, 9)):
            wtx, wty = _tiles(w, h)
            chunks = _chunks(chunk, wtx * wty * views, waves)
            lengths = {r[3] for a, b in chunks for r in _runs(runs, a, b, w, h)}
            assert 1 in lengths and max(lengths) <= wtx
            assert _spans(chunks, wtx) or max(b - a for a, b in chunks) == 1


def test_the_hook_rejects_what_the_kernel_never_passes():
    _, runs = _hooks()
    ptr = _RUNS.ctypes.data
    for t, t_end, w, h in ((-1, 4, 8, 8), (5, 4, 8, 8), (0, 1 << 30, 8, 8), (0, 4, 0, 8), (0, 4, 8, 0)):
        assert runs(t, t_end, w, h, ptr, CAP) < 0
    assert runs(0, 4, 8, 8, None, CAP) < 0 and runs(0, 4, 8, 8, ptr, -1) < 0
    assert runs(3, 3, 8, 8, ptr, CAP) == 0  # an empty chunk has no run
    _RUNS[:] = -7
    assert runs(0, 40, 8, 8, ptr, 2) == 40  # more runs than `cap`: counted, not written
    assert (_RUNS[8:] == -7).all() and tuple(_RUNS[4:8]) == (1, 0, 0, 1)
