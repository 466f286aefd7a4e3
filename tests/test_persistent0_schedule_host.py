"""The persistent depth-0 launch's schedule (rt_internal.h persistent_chunk,
the one function render_persistent0 calls for a chunk id, here through the
host-only rt_debug_persistent_chunk): the ranges of chunk ids 0, 1, ... tile
[0, total) exactly once and in order, their sizes never grow along the ids
(the bulk in chunks of kChunk0, then regions of halving sizes down to single
tiles, each about a chunk per resident wave), the first id past the end gives
an empty range, and nothing leaves int for totals up to 2^30 - 1."""
import ctypes as C

import numpy as np
import pytest

import openglraytracer_amd as rt

WAVES = [32, 36, 64, 8192]
LARGE = [32400, 256 * 32400, (1 << 30) - 1]
INT_MAX = (1 << 31) - 1
EDGE = 10000  # ids checked at either end of a large total


_OUT = np.zeros(2, np.int32)
_OUT_PTR = _OUT.ctypes.data


def _hook():
    f = rt.lib().rt_debug_persistent_chunk
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    f.restype = C.c_int
    return f


def _range(f, c, total, waves):
    _OUT[:] = -7
    assert f(c, total, waves, _OUT_PTR) == 0
    out = _OUT
    t, t_end = int(out[0]), int(out[1])
    assert 0 <= t <= t_end <= total <= INT_MAX
    return t, t_end


def _walk(f, total, waves, c0, t0, limit, last_size=None):
    """Ranges of ids c0, c0 + 1, ... from item t0: contiguous, in order, sizes
    never growing; stops at `limit` ids or at the end of the items. Returns
    (next id, next item, last size)."""
    c, t = c0, t0
    while c < c0 + limit and t < total:
        a, b = _range(f, c, total, waves)
        assert a == t and b > a, (c, total, waves, a, b, t)
        if last_size is not None:
            assert b - a <= last_size, (c, total, waves)
        last_size = b - a
        c, t = c + 1, b
    return c, t, last_size


@pytest.mark.parametrize("waves", WAVES)
def test_small_totals_are_tiled_exactly_once_in_order(waves):
    f = _hook()
    for total in range(1, 601):
        c, t, _ = _walk(f, total, waves, 0, 0, total + 1)
        assert t == total and c <= total
        assert _range(f, c, total, waves) == (total, total)  # the first id past the end: empty
        assert _range(f, c + 1, total, waves)[0] == _range(f, c + 1, total, waves)[1]


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("total", LARGE)
def test_large_totals_at_both_ends_and_by_count(total, waves):
    """The first and last 10,000 ids and the number of ranges: the head walked
    from id 0, the count found as the first empty id (sizes never grow, so
    emptiness is monotonic in the id), the tail walked up to the end; between
    them the head's last size bounds the tail's first."""
    f = _hook()
    c_head, t_head, size_head = _walk(f, total, waves, 0, 0, EDGE)
    lo, hi = 0, total  # the first empty id: lo is not empty or 0, hi is empty
    assert _range(f, hi, total, waves) == (total, total)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        a, b = _range(f, mid, total, waves)
        lo, hi = (mid, hi) if b > a else (lo, mid)
    count = hi
    assert _range(f, count - 1, total, waves)[1] == total
    assert _range(f, count, total, waves) == (total, total)
    if t_head == total:
        assert c_head == count
        return
    c0 = max(c_head, count - EDGE)
    t0 = _range(f, c0, total, waves)[0]
    assert t0 >= t_head
    if c0 == c_head:
        assert t0 == t_head
    c_end, t_end, size_end = _walk(f, total, waves, c0, t0, EDGE + 1, last_size=size_head)
    assert (c_end, t_end) == (count, total)
    assert size_end == 1  # a launch larger than its tail ends tile by tile
    # the ids between the two walks all have the head's last size at most and
    # the tail's first size at least: with sizes powers of two that never grow,
    # the items between must be a whole number of ranges of sizes in between
    between_ids, between_items = c0 - c_head, t0 - t_head
    first_tail = _range(f, c0, total, waves)
    assert between_ids * (first_tail[1] - first_tail[0]) <= between_items <= between_ids * size_head


@pytest.mark.parametrize("waves", WAVES)
def test_every_region_holds_about_a_chunk_per_wave(waves):
    """A chunk that starts last in its region has at least its own length of
    smaller work per wave behind it, and a region is no longer than that:
    where the size drops from s to s2, at least s2 * waves and fewer than
    s * waves + s items are left."""
    f = _hook()
    total = 40 * waves + 17
    c, t, size = 0, 0, None
    while t < total:
        a, b = _range(f, c, total, waves)
        if size is not None and b - a < size:
            left = total - a
            assert (b - a) * waves <= left < size * waves + size, (waves, size, b - a, left)
        size = b - a
        c, t = c + 1, b
    assert size == 1


@pytest.mark.parametrize("waves", [32, 33, 36, 63, 64, 100, 8192, 8192 + 12])
def test_every_queue_has_its_waves_and_the_first_chunks_are_the_first_ids(waves):
    """Wave g's queue (rt_internal.h persistent_queue, rotated round by round
    so that no queue is tied to one part of the chip), the queue's wave count
    and the wave's first chunk, through rt_debug_persistent_queue: every
    round of 32 waves maps onto the 32 queues one to one, the counts are the
    waves that name the queue, every queue of a grid of 32 waves or more has
    one, the first chunks are distinct ids of the wave's own queue (id % 32),
    the k-th wave of a queue starting with the queue's k-th id: the head then
    continues from the queue's wave count."""
    f = rt.lib().rt_debug_persistent_queue
    f.argtypes = [C.c_int, C.c_int, C.c_void_p]
    f.restype = C.c_int
    out = np.zeros(3, np.int32)
    rows = []
    for g in range(waves):
        assert f(g, waves, out.ctypes.data) == 0
        rows.append(tuple(int(x) for x in out))
    q, n, first = (np.array(x) for x in zip(*rows))
    assert ((q >= 0) & (q < 32)).all()
    for r in range(waves // 32):
        assert sorted(q[32 * r:32 * r + 32]) == list(range(32))
    counts = np.bincount(q, minlength=32)
    assert (counts >= 1).all() and counts.max() - counts.min() <= 1
    assert np.array_equal(n, counts[q])
    assert len(set(first)) == waves and np.array_equal(first % 32, q)
    for k in range(32):
        assert sorted(first[q == k] // 32) == list(range(counts[k]))
    # the rotation: the four waves of a work-group's slot on the chip (work-groups go to the
    # eight XCDs in turn) serve several queues, where 32 rounds or more exist
    if waves >= 32 * 32:
        for slot in range(32):
            assert len(set(q[slot::32])) == 32
    assert f(waves, waves, out.ctypes.data) != 0 and f(-1, waves, out.ctypes.data) != 0


def test_the_hook_rejects_what_the_launch_never_passes():
    f = _hook()
    out = np.zeros(2, np.int32)
    for c, total, waves in ((-1, 10, 32), (0, -1, 32), (0, 1 << 30, 32), (0, 10, 0)):
        assert f(c, total, waves, out.ctypes.data) != 0
    assert f(0, 10, 32, None) != 0
    assert _range(f, 0, 0, 32) == (0, 0)
