"""What adaptive anti-aliasing costs and what it skips (rt_render_aa):
    python tools/aa_time.py [--out LOG]               the timing run
    python tools/aa_time.py --child                   the launches alone, for a kernel trace run of its own
    python tools/aa_time.py --trace DIR --append LOG  the trace's rows (DIR/trace_kernel_trace.csv)
(tools/gpu_session.sh TAG aa runs the three, each under its own time limit.)

Workloads, all at 16 spp and threshold 0.1, device buffers, one process:
config 2's scene at 1920 x 1080 and depth 0, the shipped scene (time 0) at
1280 x 720 and depth 0, config 3's scene at 3840 x 2160 and depth 2. Per
workload the median of READINGS rt_last_kernel_ms readings (HIP events around
the call's launches on the context's stream) after WARMUP warm-ups of
  (a) one rt_render,
  (b) rt_render_aa (base frame + edge kernel + refine launch), and (b') the same with
      RT_OPT_AA_QUEUED 0 (the refine launch of depth 0-1 tiled, with the work-group early exit),
  (c) a full-frame rt_render_accumulate of 16 spp,
interleaved round by round so that a drift of the clocks touches all alike;
then the flagged-pixel share, the live-tile share, the lane utilisation
(flagged pixels / (64 x live wave tiles)), (b) - (a) beside (c) x the
live-tile share, and the max and mean |difference| between (b)'s frame and the
full 16-spp mean: the price of the pixels that were not supersampled.
The trace's rows give each of the three launches alone, the edge kernel beside
the time to read the frame once at the HBM rate bench.py's roofline uses.
Recorded, not asserted: DESIGN.md §7 quotes the log.
"""
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP, THRESHOLD, WARMUP, READINGS, CHILD_CALLS = 16, 0.1, 3, 15, 7
HBM_PEAK_GBS = 8000.0  # bench.py's roofline rate
WORKLOADS = [  # name, objects, time, width, height, depth
    ("config 2's scene, 1920 x 1080, depth 0", "bench16", 0.0, 1920, 1080, 0),
    ("the shipped scene, 1280 x 720, depth 0", "shipped", 0.0, 1280, 720, 0),
    ("config 3's scene, 3840 x 2160, depth 2", "bench64", 0.0, 3840, 2160, 2),
]


def objects(rt, scenes, name):
    return rt.reference_objects(0.0) if name == "shipped" else scenes.bench_objects(int(name[5:]))


def tiled_aa(ctx, call):
    """The call with RT_OPT_AA_QUEUED 0: at depth 0-1 the refine launch tiled, a work-group per
    16 x 16 tile with the early exit (the recursive depths take the lists either way)."""
    ctx.set_aa_queued(False)
    try:
        call()
    finally:
        ctx.set_aa_queued(True)


def timing():
    import torch  # noqa: F401  (HIP runtime first)
    import openglraytracer_amd as rt
    from oracle import scenes
    child = "--child" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    ctx = rt.Context(0)
    lines = ["# tools/aa_time.py: %s" % rt.lib().rt_version().decode(),
             "# %d spp, threshold %g; medians of %d rt_last_kernel_ms readings after %d warm-ups, the cases interleaved"
             % (SPP, THRESHOLD, READINGS, WARMUP)]
    for label, name, t, w, h, depth in WORKLOADS:
        sc = rt.Scene(ctx, objects(rt, scenes, name))
        view = rt.make_view(None, t)
        frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        aa = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        cases = [
            ("(a) rt_render", lambda: rt.render_device(ctx, sc, frame.data_ptr(), w, h, depth, view=view)),
            ("(b) rt_render_aa", lambda: rt.render_aa(ctx, sc, w, h, depth, SPP, THRESHOLD, view=view, out=aa.data_ptr())),
            ("(b') rt_render_aa, RT_OPT_AA_QUEUED 0", lambda: tiled_aa(ctx, lambda: rt.render_aa(
                ctx, sc, w, h, depth, SPP, THRESHOLD, view=view, out=aa.data_ptr()))),
            ("(c) rt_render_accumulate, %d spp" % SPP,
             lambda: rt.render_accumulate(ctx, sc, acc.data_ptr(), w, h, depth, SPP, 0, seed=0, view=view)),
        ]
        if child:  # the launches alone: CHILD_CALLS anti-aliased renders per workload and distribution
            for k in (1, 2):
                for _ in range(CHILD_CALLS):
                    cases[k][1]()
            sc.close()
            continue
        ms = [[] for _ in cases]
        for i in range(WARMUP + READINGS):
            for k, (_, call) in enumerate(cases):
                call()
                if i >= WARMUP:
                    ms[k].append(ctx.last_kernel_ms())
        cases[1][1]()
        base_kernel = rt.last_kernel(ctx)  # (the debug hooks report the call's base render)
        px, tiles = rt.aa_last_counts(ctx)
        n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
        acc.zero_()
        torch.cuda.synchronize()
        cases[-1][1]()
        torch.cuda.synchronize()
        diff = (aa[..., :3] - acc[..., :3] / SPP).abs()
        med = [float(np.median(m)) for m in ms]
        lines.append("")
        lines.append("## %s (base render kernel (depth, accum, dev, shape, launch, queued) = %s)" % (label, base_kernel))
        for (cname, _), m in zip(cases, ms):
            lines.append("%-36s median %9.4f ms  min %9.4f  max %9.4f" % (cname, np.median(m), np.min(m), np.max(m)))
        lines.append("flagged pixels %d of %d (%.2f %%), live wave tiles %d of %d (%.2f %%), lane utilisation %.3f"
                     % (px, w * h, 100.0 * px / (w * h), tiles, n_tiles, 100.0 * tiles / n_tiles,
                        px / (64.0 * tiles) if tiles else 0.0))
        want = med[-1] * tiles / n_tiles
        lines.append("(b) - (a) = %.4f ms; (c) x live-tile share = %.4f ms; ratio %.2f" % (
            med[1] - med[0], want, (med[1] - med[0]) / want if want > 0 else float("nan")))
        lines.append("(b) / (c) = %.3f; |(b) - full %d-spp mean|: max %.4f, mean %.6f" % (
            med[1] / med[-1], SPP, float(diff.max()), float(diff.mean())))
        sc.close()
    ctx.close()
    if child:
        return
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def trace_rows():
    """Per workload the medians of the three launches of the child's calls,
    from the kernel trace: the dispatches of our kernels in order are
    CHILD_CALLS x (base render, edge kernel, refine launch) per workload."""
    src = sys.argv[sys.argv.index("--trace") + 1]
    rows = []
    for dirpath, _, files in os.walk(src):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                for r in csv.DictReader(open(os.path.join(dirpath, f))):
                    kname = r.get("Kernel_Name", "")
                    if "render_kernel" in kname or "aa_edge_kernel" in kname or "aa_refine_kernel" in kname:
                        rows.append((int(r["Dispatch_Id"]), kname, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    lines = ["", "## the three launches alone (rocprofv3 --kernel-trace, a run of its own: %d calls per workload and "
                 "distribution of the refine launch, the first 2 dropped)" % CHILD_CALLS]
    groups = [(label, w, h, mode) for label, _, _, w, h, _ in WORKLOADS for mode in ("lists", "RT_OPT_AA_QUEUED 0")]
    if len(rows) != 3 * CHILD_CALLS * len(groups):
        lines.append("unexpected dispatch count %d (wanted %d): no rows" % (len(rows), 3 * CHILD_CALLS * len(groups)))
    else:
        for k, (label, w, h, mode) in enumerate(groups):
            mine = rows[3 * CHILD_CALLS * k: 3 * CHILD_CALLS * (k + 1)]
            calls = [mine[3 * i: 3 * i + 3] for i in range(2, CHILD_CALLS)]
            assert all("render_kernel" in c[0][1] and "aa_edge" in c[1][1] and "aa_refine" in c[2][1] for c in calls)
            us = [float(np.median([c[j][2] for c in calls])) / 1e3 for j in range(3)]
            read_us = w * h * 16 / (HBM_PEAK_GBS * 1e9) * 1e6
            lines.append("%s, %s: base %.1f us, edge kernel %.1f us (the frame read once at %.0f GB/s: %.1f us; x %.1f), "
                         "refine %.1f us" % (label, mode, us[0], us[1], HBM_PEAK_GBS, read_us, us[1] / read_us, us[2]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--append" in sys.argv:
        with open(sys.argv[sys.argv.index("--append") + 1], "a") as f:
            f.write(text)


if __name__ == "__main__":
    trace_rows() if "--trace" in sys.argv else timing()
