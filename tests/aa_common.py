"""What the adaptive anti-aliasing tests share (tests/test_aa_host.py,
tests/test_gpu_aa.py): the criterion restated in numpy — float32 shifts,
differences and maxima, no call into the library — and the oracle's frames,
each computed once and handed out read-only."""
import functools

import numpy as np

from oracle import port, scenes


def np_edge_mask(frame, threshold):
    """(height, width) bool: the pixel has a 4-neighbour inside the frame with
    max over r, g, b of |difference| > threshold. float32; the maximum ignores
    a NaN channel (np.fmax, IEEE maxNum), so a NaN difference never flags."""
    rgb = np.asarray(frame)[..., :3]
    assert rgb.dtype == np.float32
    thr = np.float32(threshold)
    flagged = np.zeros(rgb.shape[:2], bool)
    with np.errstate(invalid="ignore"):
        for axis in (0, 1):
            a = rgb[1:] if axis == 0 else rgb[:, 1:]
            b = rgb[:-1] if axis == 0 else rgb[:, :-1]
            d = np.abs(a - b)
            assert d.dtype == np.float32
            differs = np.fmax(np.fmax(d[..., 0], d[..., 1]), d[..., 2]) > thr
            if axis == 0:
                flagged[1:] |= differs
                flagged[:-1] |= differs
            else:
                flagged[:, 1:] |= differs
                flagged[:, :-1] |= differs
    return flagged


def np_tile_masks(mask):
    """(ceil(h / 8), ceil(w / 8)) uint64: bit l of tile (wy, wx) is pixel
    (8 wx + l % 8, 8 wy + l / 8); bits of pixels outside the frame are 0."""
    h, w = mask.shape
    th, tw = (h + 7) // 8, (w + 7) // 8
    padded = np.zeros((th * 8, tw * 8), np.uint64)
    padded[:h, :w] = mask.astype(np.uint64)
    tiles = padded.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th, tw, 64)
    return (tiles << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def scene_objects(name):
    if name == "shipped":
        return port.reference_objects(0.7), 0.7
    if name == "bench16":
        return scenes.bench_objects(16), 0.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_base(name, width, height, depth):
    """The oracle's frame of scene `name` (scene_objects) — read-only."""
    objs, t = scene_objects(name)
    out = port.render(objs, width, height, depth, t)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_samples(name, width, height, depth, spp, seed=0):
    """The oracle's in-order sums of samples [0, spp) — read-only."""
    objs, t = scene_objects(name)
    out = port.render_accumulate(objs, width, height, depth, spp, 0, seed=seed, time=t)
    out.setflags(write=False)
    return out


def expected_aa(base, samples, spp, threshold):
    """(frame, mask) of the anti-aliased render from the oracle's base frame
    and sample sums: the mean where the numpy criterion flags, else the base."""
    mask = np_edge_mask(base, threshold)
    with np.errstate(invalid="ignore"):
        mean = samples / np.float32(spp)
    assert mean.dtype == np.float32
    return np.where(mask[..., None], mean, base), mask.astype(np.uint8)
