"""CPU model of the persistent depth-0 launch's end (development probe).

    python tools/model/persistent_model.py [--views 256] [--waves 8192]

Replays the schedule of render_persistent0 (rt_internal.h persistent_chunk:
the bulk in chunks of B, then regions of B / 2 ... 2 and single tiles, the
region of size s ending where K * s * waves items are left; K = 1 is the
kernel's) on `waves` waves that take chunks from one pool (the rotated queues
end within a few microseconds of each other, profiles/r09a_persistent_trace.log,
so the 32 queues are not modelled). A wave's time per tile is fixed for the
launch: one of eight values, its place in its SIMD's age order (a SIMD issues
its oldest wave first, so that place is its speed all launch long), spaced
between the fastest and the slowest traced wave of config 2 at 1080p (3.8 and
23.8 us per tile: 1,843 and 296 tiles in 7,035 us; traced p10 4.0, mean 9.7,
p90 21.8) with a few per cent of scatter. A wave either reserves its next
chunk when it starts the current one (`ahead`, the first version of the
launch) or takes it when it needs it. Prints the mean and maximum idle after a
wave's last tile and the dequeues per wave.

Against the traces (idle 45 / 21 / 45 us for B 8 ahead / B 8 at need / B 16 at
need) the model gives 225 / 104 / 214 us: the same order, about five times
too much. It puts regions of four chunks per wave (K = 4) at a fifth of K = 1.

The model keeps a slow wave slow to the end, where on the chip it speeds up as
its SIMD empties: its idle figures are upper bounds, its ordering of the
variants is what it is for.
"""
import argparse
import heapq

import numpy as np


def chunk_sizes(total, waves, bulk, k):
    """sizes of chunk ids 0, 1, ... (persistent_chunk with regions of k chunks per wave)"""
    out, start, s = [], 0, bulk
    while s >= 2:
        n = max(0, (total - start) // s - k * waves)
        out.append(np.full(n, s, np.int64))
        start += n * s
        s //= 2
    out.append(np.ones(total - start, np.int64))
    return np.concatenate(out)


def replay(sizes, per_tile, ahead):
    """every wave takes the next chunk id when free (or a chunk earlier: ahead)"""
    n = len(per_tile)
    nxt = n  # ids 0 .. n - 1 are the waves' first chunks
    end = np.zeros(n)
    deq = np.zeros(n, np.int64)
    heap = []
    for w in range(n):
        if w >= len(sizes):
            continue
        if ahead:  # the id of the chunk after the first is taken at once
            held, nxt = (nxt, nxt + 1)
        else:
            held = -1
        heapq.heappush(heap, (sizes[w] * per_tile[w], w, held))
        deq[w] += 1
    while heap:
        t, w, held = heapq.heappop(heap)
        end[w] = t
        if ahead:
            c = held
            if c >= len(sizes):
                continue
            held, nxt = (nxt, nxt + 1)  # reserved as the chunk starts
        else:
            c, nxt = (nxt, nxt + 1)
            if c >= len(sizes):
                continue
        deq[w] += 1
        heapq.heappush(heap, (t + sizes[c] * per_tile[w], w, held))
    return end, deq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--waves", type=int, default=8192)
    ap.add_argument("--tiles-per-view", type=int, default=32400)
    a = ap.parse_args()
    rng = np.random.default_rng(9)
    ranks = np.array([3.8, 4.6, 5.6, 6.9, 8.8, 11.5, 16.0, 23.8])  # us per tile by age on the SIMD
    per_tile = ranks[np.arange(a.waves) % 8] * rng.uniform(0.95, 1.05, a.waves)
    total = a.views * a.tiles_per_view
    print("%d views, %d tiles on %d waves; wave-time per tile p10 %.1f mean %.1f p90 %.1f us"
          % (a.views, total, a.waves, np.percentile(per_tile, 10), per_tile.mean(), np.percentile(per_tile, 90)))
    print("%-34s %10s %10s %10s %10s" % ("schedule", "span us", "idle mean", "idle max", "dequeues"))
    for bulk, k, ahead in ((8, 1, True), (8, 1, False), (16, 1, False), (32, 1, False), (16, 2, False),
                           (16, 4, False), (32, 2, False), (32, 4, False)):
        end, deq = replay(chunk_sizes(total, a.waves, bulk, k), per_tile, ahead)
        idle = end.max() - end
        print("%-34s %10.1f %10.1f %10.1f %10.1f" % (
            "B %2d, %d chunk(s)/wave/region, %s" % (bulk, k, "ahead" if ahead else "at need"), end.max(), idle.mean(),
            idle.max(), deq.mean()))


if __name__ == "__main__":
    main()
