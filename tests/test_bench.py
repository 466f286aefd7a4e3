"""bench.py's multi-rank paths, rehearsed on one GPU with the gloo backend.

The driver runs `torch.distributed.run --nproc-per-node N bench.py --gpus N`
over RCCL on an 8-GPU node; here two ranks share the box's one GPU and their
collectives go through gloo on host copies (bench.py --dist-backend gloo), so
the step structure, the timing fields and the JSON line of every workload's
N>1 path run end to end. Values are not performance numbers (two ranks share
one GPU).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(n, *args, timeout=240):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"),
           "--gpus", str(n), "--dist-backend", "gloo", "--full", "--no-cpu-baseline", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]  # rank 0 alone prints
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n,frames", [(2, 3), (3, 5)])
def test_config2_row_tiled_spread_default(n, frames):
    """The default config2 shape at N>1: every frame of the step row-tiled
    over the ranks (GL_RGBA8 shards packed to RGB8), one all-to-all assembling
    frame k on rank k % N; every assembled frame equals its rank's own
    whole-frame render byte for byte (bench.py checks, `verified`, summed over
    the ranks), through the HIP kernel."""
    line = run_bench(n, "--steps", "3", "--warmup", "1", "--frames", str(frames))
    assert line["n_gpus"] == n and line["scaling"] == "strong" and line["value"] > 0
    assert line["config"]["frames_per_step"] == frames and "all_to_all" in line["timing"]["collective"]
    assert "GL_RGBA8" in line["config"]["output"] and "RGB8" in line["config"]["output"]
    ranks = line["timing"]["per_rank"]
    assert [r["rank"] for r in ranks] == list(range(n))
    assert all(r["kernel_ms"] > 0 and r["collective_ms"] > 0 for r in ranks)
    rows0 = 8 * len(range(0, 135, n))  # rank 0's 8-row blocks of the 135
    assert line["roofline"]["bytes_per_launch"] == frames * 1920 * rows0 * 4
    # (both rounded to 5 decimals in the line)
    assert line["roofline"]["frac_float4_equivalent"] == pytest.approx(4 * line["roofline"]["frac"], rel=1e-3,
                                                                         abs=4e-5)
    v = line["verified"]
    assert v["bit_exact"] and v["frames_checked"] == frames and v["mismatched_pixels"] == 0
    ind = line["independent_frames"]
    assert ind["frames_per_step"] == n * frames and ind["scaling"] == "weak" and ind["value"] > 0
    check_prediction(line)


def check_prediction(line):
    """N>1 lines judge themselves: DESIGN.md §6's predicted step time (from
    the committed one-GPU shard timings, at 50 and 100 GB/s per link) beside
    the measured one, and every rank's collective bytes / collective time."""
    pred = line["predicted_ms_per_step"]
    assert pred["measured_ms_per_step"] == line["ms_per_step"]
    assert pred["ms_per_step_B50"] >= pred["ms_per_step_B100"] > 0
    assert pred["busiest_link_bytes"] == max(r["link_bytes"] for r in line["timing"]["per_rank"])
    for r in line["timing"]["per_rank"]:
        assert r["link_GBps"] > 0 and r["collective_GBps"] >= r["link_GBps"]


@pytest.mark.gpu
def test_config2_two_ranks_row_tiled_gather():
    """--frame-exchange gather (north_star's literal shape): the GL_RGBA8
    shards of every frame gathered to rank 0 and de-interleaved there; the
    assembled frames equal rank 0's whole-frame render byte for byte."""
    line = run_bench(2, "--steps", "3", "--warmup", "1", "--frames", "3", "--frame-exchange", "gather")
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    assert line["config"]["frames_per_step"] == 3 and "gather" in line["timing"]["collective"]
    assert "GL_RGBA8" in line["config"]["output"] and "RGB8" in line["config"]["output"]
    ranks = line["timing"]["per_rank"]
    assert [r["rank"] for r in ranks] == [0, 1] and all(r["kernel_ms"] > 0 and r["collective_ms"] > 0 for r in ranks)
    assert line["roofline"]["bytes_per_launch"] == 3 * 1920 * 544 * 4  # 4 B per pixel, rank 0: 68 of 135 8-row blocks
    v = line["verified"]
    assert v["bit_exact"] and v["frames_checked"] == 3 and v["mismatched_pixels"] == 0
    ind = line["independent_frames"]
    assert ind["frames_per_step"] == 6 and ind["scaling"] == "weak" and ind["value"] > 0
    check_prediction(line)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["none", "all_to_all"])
def test_config2_two_ranks_other_modes(mode):
    line = run_bench(2, "--steps", "3", "--warmup", "1", "--frames", "2", "--frame-exchange", mode)
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert line["config"]["frames_per_step"] == 4
    ranks = line["timing"]["per_rank"]
    assert [r["rank"] for r in ranks] == [0, 1] and all(r["kernel_ms"] > 0 for r in ranks)
    if mode == "none":
        assert line["timing"]["collective"] == "none" and "no collective" in line["config"]["parallelism"]
        assert line["roofline"]["bytes_per_launch"] == 2 * 1920 * 1080 * 16
        assert "verified" not in line
    else:
        assert "all_to_all" in line["timing"]["collective"]
        assert all(r["collective_ms"] > 0 for r in ranks)
        assert line["verified"]["bit_exact"] and line["verified"]["frames_checked"] == 4


@pytest.mark.gpu
def test_config3_two_ranks_gather():
    line = run_bench(2, "--workload", "config3", "--steps", "3", "--warmup", "1")
    assert line["scaling"] == "strong" and line["timing"]["collective"] == "gather to rank 0"
    assert all(r["collective_ms"] > 0 and r["kernel_ms"] > 0 for r in line["timing"]["per_rank"])
    # each rank stores its float3 row blocks: half the frame's rows each
    assert line["roofline"]["bytes_per_launch"] == 3840 * 1080 * 12
    assert line["verified"]["bit_exact"] and line["verified"]["frames_checked"] == 1
    # (no one-GPU shard timings of config 3's row tiles are committed)
    assert "predicted_ms_per_step" not in line
    assert all(r["link_GBps"] > 0 for r in line["timing"]["per_rank"])


@pytest.mark.gpu
def test_config5_two_ranks_all_reduce():
    line = run_bench(2, "--workload", "config5", "--steps", "2", "--warmup", "1")
    assert "all_reduce" in line["timing"]["collective"] and line["value"] > 0
    check_prediction(line)


def test_pmc_summary_of_other_sources_is_not_reported(tmp_path, monkeypatch):
    """bench.py reads the committed PMC summary only when it was profiled on
    the same sources (the src hash of rt_version()); otherwise the line says
    which build the summary belongs to instead of mixing builds."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    prof = tmp_path / "profiles"
    prof.mkdir()
    summary = {"workload": "config4", "n_gpus": 1, "frames_per_launch": 1, "sq_insts_valu_per_launch": 1e9,
               "hbm_bytes_per_launch": 5e9,
               "build": "openglraytracer_amd 0.3 (gfx950, src 0123456789ab, git abc-dirty)"}
    (prof / "pmc_config4_latest.json").write_text(json.dumps(summary))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    same = bench.pmc_latest("config4", 1, "openglraytracer_amd 0.3 (gfx950, src 0123456789ab, git def)")
    assert same["hbm_bytes_per_launch"] == 5e9 and bench.valu_bound(same, 10.0)["wave_insts_per_launch"] == 1e9
    other = bench.pmc_latest("config4", 1, "openglraytracer_amd 0.3 (gfx950, src fedcba987654, git abc)")
    assert "hbm_bytes_per_launch" not in other and other["stale_build"] == summary["build"]
    assert "stale_build" in bench.valu_bound(other, 10.0)
    assert bench.pmc_latest("config3", 1, summary["build"]) == {}


@pytest.mark.gpu
def test_config3_one_gpu_batches_frames():
    """config3 at N=1: a step is F animated frames in one queued launch
    (by default the views one launch holds for this scene); the line
    carries the one-frame-per-launch rate of the same frames, on one stream
    and on two, and the two-stream step rate."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "config3", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0
    cfg = line["config"]
    F = cfg["frames_per_step"]
    assert 2 <= F <= 64 and cfg["frames_per_launch"] == F and cfg["max_depth"] == 2
    assert line["roofline"]["bytes_per_launch"] == F * 3840 * 2160 * 16
    assert line["verified"]["bit_exact"] and line["verified"]["frames_checked"] == [0, (F - 1) // 2, F - 1]
    one = line["single_frame"]
    assert one["frames_per_launch"] == 1 and one["us_per_frame"] > 0 and one["two_streams"]["us_per_frame"] > 0
    assert line["pipelined"]["render_streams"] == 2 and "rgba8_surface" not in line


def run_ranks(n, *args, env_extra=None, timeout=180, port=29541):
    """bench.py --gpus n as n processes of our own (no torchrun, whose agent
    would terminate the survivors itself): every rank's exit code and stderr."""
    procs = []
    for r in range(n):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r),
                   WORLD_SIZE=str(n), **(env_extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n),
                                       "--dist-backend", "gloo", "--no-cpu-baseline", *args],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT))
    out = []
    try:
        for p in procs:
            _, err = p.communicate(timeout=timeout)
            out.append((p.returncode, err))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return out


def test_a_rank_that_dies_fails_every_rank():
    """SURVEY.md §5 (an RCCL error aborts the frame): a rank that exits right
    after joining the group, without a word to its peers, makes the surviving
    rank's next collective fail; bench.py then ends that rank too, with a
    message and a nonzero exit, instead of hanging or exiting 0 (gloo on the
    CPU; no GPU work happens before the startup barrier)."""
    res = run_ranks(2, "--collective-timeout", "60", env_extra={"RT_BENCH_FAULT": "1:init"})
    (rc0, err0), (rc1, err1) = res
    assert rc1 == 3 and "injected fault at init" in err1
    assert rc0 == 17, (rc0, err0[-2000:])
    assert "rank 0: step failed, aborting the frame" in err0


@pytest.mark.gpu
def test_a_rank_that_dies_mid_step_fails_every_rank():
    """The same, with the fault at rank 1's first timed collective (config 2,
    spread): rank 0 has rendered and packed, its all-to-all fails, and it
    exits nonzero with a message (two ranks on one GPU, gloo)."""
    res = run_ranks(2, "--steps", "3", "--warmup", "1", "--frames", "3", "--collective-timeout", "60",
                    env_extra={"RT_BENCH_FAULT": "1:step"}, port=29542)
    (rc0, err0), (rc1, err1) = res
    assert rc1 == 3 and "injected fault at step" in err1
    assert rc0 == 17, (rc0, err0[-2000:])
    assert "aborting the frame" in err0


@pytest.mark.gpu
def test_config2_one_gpu_line_checks_itself():
    """The headline line at N=1: frames 0, 127 and 255 of the last timed step
    are byte-identical to single renders of the same views; every one-stream
    figure is the kernel's own (kernel time x launches per step within
    [0.97, 1.01] of the step time, for the float4 line and for the GL_RGBA8
    surface); the single-frame rates are medians of 3 repeats."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "12", "--warmup", "3", "--full",
           "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    v = line["verified"]
    assert v["bit_exact"] and v["frames_checked"] == [0, 127, 255] and v["mismatched_pixels"] == 0
    cfg = line["config"]
    launches = cfg["frames_per_step"] // cfg["frames_per_launch"]
    assert launches == 1 and line["timing"]["render_streams"] == 1
    ratio = line["roofline"]["kernel_ms"] * launches / line["ms_per_step"]
    assert 0.97 <= ratio <= 1.01, ratio
    r8 = line["rgba8_surface"]
    ratio8 = r8["kernel_ms"] * (cfg["frames_per_step"] // r8["frames_per_launch"]) / r8["ms_per_step"]
    assert 0.97 <= ratio8 <= 1.01, ratio8
    one = line["single_frame"]
    assert len(one["repeats_us"]) == 3 and len(one["two_streams"]["repeats_us"]) == 3
    # the general depth-0 kernel (scene shapes off) on the same frames: the
    # same frame, at a bounded price ("Scene shapes")
    gk = line["general_kernel"]
    assert gk["frame0_identical_to_shaped"] and gk["frames_per_launch"] == cfg["frames_per_launch"]
    assert 1.0 <= gk["vs_shaped"] <= 1.6, gk  # measured 1.42 (r06zi)


STUB_RANK = r'''
import json, os, sys
import torch
import torch.distributed as dist
dist.init_process_group("gloo")
t = torch.tensor([float(dist.get_rank() + 1)])
dist.all_reduce(t)
if dist.get_rank() == 0:
    print(json.dumps({"world": dist.get_world_size(), "sum": t.item(), "argv": sys.argv[1:],
                      "local_rank": int(os.environ["LOCAL_RANK"])}), flush=True)
dist.destroy_process_group()
'''


def test_self_launch_starts_every_rank(tmp_path, capfd):
    """bench.py --gpus N with no launcher (the driver's N=1 command shape,
    `python3 bench.py --gpus N`): launch_ranks starts N processes with
    torch.distributed.run's environment, and rank 0's line comes through
    (a stub rank: gloo all-reduce on the CPU)."""
    sys.path.insert(0, ROOT)
    import bench
    stub = tmp_path / "stub_rank.py"
    stub.write_text(STUB_RANK)
    assert bench.launch_ranks(3, ["--steps", "2"], script=str(stub)) == 0
    out = capfd.readouterr().out
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert lines == [{"world": 3, "sum": 6.0, "argv": ["--steps", "2"], "local_rank": 0}]


def test_self_launch_fails_when_a_rank_fails():
    """The same entry through bench.py itself (gloo, CPU: rank 1 dies right
    after joining the group, before any GPU work): the launcher's exit is
    nonzero, every rank has ended, and it says which ranks failed."""
    env = dict(os.environ, RT_BENCH_FAULT="1:init")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                        "--no-cpu-baseline", "--collective-timeout", "60"],
                       capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert "injected fault at init" in r.stderr
    assert "rank 0: step failed, aborting the frame" in r.stderr
    assert "ranks failed" in r.stderr


@pytest.mark.gpu
def test_self_launched_two_ranks_on_one_gpu():
    """`python3 bench.py --gpus 2` with no launcher on the one-GPU box: the
    two self-started ranks render config 2's row-tiled frames through the
    HIP kernel (gloo), and the assembled frames are verified byte for byte."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                        "--full", "--no-cpu-baseline", "--steps", "3", "--warmup", "1", "--frames", "4"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["verified"]["bit_exact"]


def _bench_line(*args, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_shipped_workload_line():
    """The reference app's own workload (main.cpp:17-19, raytrace_compute.glsl:
    22, :261-321): 1280x720, the shipped scene at every frame's time, depth
    0, 256 frames per launch each with its own scene; frames 0, 127, 255
    byte-identical to single renders; the draw() shape with the host's
    scene update is reported beside it."""
    line = _bench_line("--workload", "shipped", "--steps", "3", "--warmup", "1")
    cfg = line["config"]
    assert (cfg["width"], cfg["height"], cfg["max_depth"], cfg["frames_per_launch"]) == (1280, 720, 0, 256)
    assert line["verified"]["bit_exact"] and line["verified"]["frames_checked"] == [0, 127, 255]
    assert line["roofline"]["bytes_per_launch"] == 256 * 1280 * 720 * 16
    d = line["draw_loop"]
    assert d["us_per_frame"] > 0 and d["scene_update_us"] > 0 and len(d["repeats_us"]) == 3
    assert line["rgba8_surface"]["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["config4", "config5"])
def test_one_frame_workloads_verify_what_they_time(workload):
    """Configs 4 and 5 at N=1 check the buffers of their last timed step:
    two 8-row bands of the 8K frame against renders of those rows alone,
    two 2-row bands of the Monte-Carlo estimate against the same samples of
    those rows accumulated by a call of their own (raytrace_compute.glsl:404)."""
    line = _bench_line("--workload", workload, "--steps", "1", "--warmup", "1", "--no-pipelined")
    v = line["verified"]
    assert v["bit_exact"] and v["mismatched_pixels"] == 0 and len(v["rows"]) == 2


SECONDARY = ("verified", "single_frame", "pipelined", "rgba8_surface", "general_kernel", "draw_loop",
             "independent_frames")


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_skips_what_full_adds(monkeypatch):
    """Without --full every secondary measurement, the verification and the
    CPU baseline are off; --full leaves them to their --no-* options."""
    bench = _load_bench()
    offs = ("no_verify", "no_independent", "no_cpu_baseline", "no_single_frame", "no_pipelined", "no_rgba8",
            "no_general")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    plain = bench.parse()
    assert not plain.full and plain.steps == 7 and plain.warmup == 2 and plain.dump_outputs is None
    assert all(getattr(plain, k) for k in offs)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-rgba8", "--dump-outputs", "d"])
    full = bench.parse()
    assert full.full and full.dump_outputs == "d"
    assert [k for k in offs if getattr(full, k)] == ["no_rgba8"]


def test_dump_outputs_writes_whole_small_buffers_and_seeded_samples(tmp_path, monkeypatch):
    """bench.dump_outputs on host tensors: a small float4 buffer is written
    whole; a buffer above the budget as the same seeded sample every time,
    with its pixel indices; GL_RGBA8 texels as their four byte values."""
    import numpy as np
    import torch
    bench = _load_bench()
    buf = torch.arange(5 * 7 * 4, dtype=torch.float32)
    rec = bench.dump_outputs(torch, str(tmp_path / "a"), "frames", buf, 4)
    got = np.load(tmp_path / "a" / "frames.npy")
    assert rec == {"name": "frames", "pixels": 35, "of": 35, "channels": 4}
    assert got.dtype == np.float32 and np.array_equal(got, buf.numpy().reshape(35, 4))
    assert np.array_equal(np.load(tmp_path / "a" / "frames_pixel_index.npy"), np.arange(35, dtype=np.float64))
    monkeypatch.setattr(bench, "DUMP_PIXELS", 16)
    texels = torch.arange(1000, dtype=torch.int32) * 65793  # bytes (k, k, k, 0) for k < 256
    for d in ("b", "c"):
        rec = bench.dump_outputs(torch, str(tmp_path / d), "frames", texels, 1)
    idx = np.load(tmp_path / "b" / "frames_pixel_index.npy")
    val = np.load(tmp_path / "b" / "frames.npy")
    assert idx.dtype == np.float64 and 1 < idx.size <= 16 and np.all(np.diff(idx) > 0) and idx.max() < 1000
    assert rec["pixels"] == idx.size and rec["of"] == 1000 and val.shape == (idx.size, 4)
    want = texels.numpy()[idx.astype(np.int64)].view(np.uint8).reshape(-1, 4).astype(np.float32)
    assert np.array_equal(val, want)
    assert np.array_equal(idx, np.load(tmp_path / "c" / "frames_pixel_index.npy"))
    assert np.array_equal(val, np.load(tmp_path / "c" / "frames.npy"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path, gpu_ctx):
    """`bench.py --gpus 1 --steps K --warmup W` alone: the headline fields
    and none of --full's; --dump-outputs writes a seeded sample of the last
    timed step's frames, equal bit for bit to a render of the same views
    made here (2 frames of config 2: more pixels than the dump keeps)."""
    import numpy as np
    import torch

    import openglraytracer_amd as rt
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--frames", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(2 * 1920 * 1080 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert line["cpu_baseline"] is None and not [k for k in SECONDARY if k in line]
    W, H, F = 1920, 1080, 2
    val = np.load(out / "frames.npy")
    idx = np.load(out / "frames_pixel_index.npy").astype(np.int64)
    assert sorted(p.name for p in out.iterdir()) == ["frames.npy", "frames_pixel_index.npy"]
    assert val.dtype == np.float32 and val.shape == (idx.size, 4) and val.nbytes + 8 * idx.size <= 64 << 20
    assert 1 << 20 < idx.size <= 1 << 21 and np.all(np.diff(idx) > 0) and idx[-1] < F * H * W
    assert line["dumped_outputs"] == {"name": "frames", "pixels": idx.size, "of": F * H * W, "channels": 4}
    scene = rt.Scene(gpu_ctx, rt.bench_objects(16, 0))
    ref = torch.zeros((F * H * W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.set_output(rt.abi.RT_OUTPUT_RGBA32F)
    rt.render_batch(gpu_ctx, scene, ref.data_ptr(), W, H, 0, [rt.make_view(None, k / 60.0) for k in range(F)])
    torch.cuda.synchronize()
    want = ref[torch.as_tensor(idx, device="cuda")].cpu().numpy()
    scene.close()
    assert np.array_equal(val.view(np.uint32), want.view(np.uint32))
