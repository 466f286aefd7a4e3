"""Tiled against the persistent grid near the automatic threshold: config 2's
scene, 9 or 16 views of small frames, option 0 against forced (cap above the
resident grid), interleaved rounds, sustained blocks."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openglraytracer_amd as rt
from oracle import scenes

ctx = rt.Context(0)
ctx.set_timing(False)
sc = rt.Scene(ctx, scenes.CONFIGS["config2"][0]())
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
for n_views, w, h in [(9, 320, 184), (9, 640, 368), (9, 960, 544), (16, 960, 544), (32, 960, 544),
                      (9, 1920, 1080), (12, 1920, 1080), (16, 1920, 1080), (24, 1920, 1080), (32, 1920, 1080),
                      (48, 1920, 1080), (64, 1920, 1080), (128, 1920, 1080), (256, 1920, 1080)]:
    views = [rt.make_view(None, k / 60.0) for k in range(n_views)]
    out = torch.empty((n_views, h, w, 4), dtype=torch.float32, device="cuda")
    tiles = n_views * ((w + 7) // 8) * ((h + 7) // 8)
    reps = max(4, int(40e-3 / (tiles * 64 * 26e-6 / (1920 * 1080))))
    times = {0: [], 65536: []}
    for _ in range(7):
        for mode in times:
            ctx.set_persistent0(mode)
            for _ in range(reps // 2):
                rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views, stream=stream.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                rt.render_batch(ctx, sc, out.data_ptr(), w, h, 0, views, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1) / reps * 1e3)
    t0, t1 = np.median(times[0]), np.median(times[65536])
    print("%3d views %4dx%-4d tiles %7d (%.1f per resident wave)  tiled %8.1f us  persistent %8.1f us  %+.1f %%"
          % (n_views, w, h, tiles, tiles / 8192.0, t0, t1, (t1 / t0 - 1) * 100), flush=True)
