"""bench.py's plain and --full runs and --dump-outputs.

CPU: the options parse, and dump_outputs writes the frame itself below the size cap and a fixed
seeded pixel sample above it. GPU: a plain run at a small size times exactly --steps steps, prints
the contract fields and none of the legs that moved behind --full, and its dump is the frame
rrt.render returns for the same scene, bit for bit; a two-rank run dumps rank 0's gathered frame;
a --full run carries the roofline again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL_ONLY = ("roofline", "rank0_rays_per_launch", "wall_clock_breakdown", "c3_one_gpu", "c1", "f64_books",
             "cpu_baseline", "reference_gpu_slot")
SMALL = ["--gpus", "1", "--config", "C2", "--width", "96", "--spp", "4", "--steps", "3", "--warmup", "1"]


def test_full_and_dump_outputs_parse():
    plain = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert plain.full is False and plain.dump_outputs is None and plain.steps == 7 and plain.warmup == 3
    args = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert args.full is True and args.dump_outputs == "somewhere"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dump_outputs_whole_frame_below_the_cap(tmp_path, dtype):
    import torch

    frame = np.arange(5 * 7 * 4, dtype=dtype).reshape(5, 7, 4)
    bench.dump_outputs(str(tmp_path / "d"), torch.from_numpy(frame))
    assert os.listdir(tmp_path / "d") == ["accum.npy"]
    got = np.load(tmp_path / "d" / "accum.npy")
    assert got.dtype == frame.dtype and np.array_equal(got, frame)


def test_dump_outputs_samples_a_frame_above_the_cap(tmp_path, monkeypatch):
    import torch

    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    frame = np.random.default_rng(1).random((33, 47, 4)).astype(np.float32)  # 24816 B > the cap
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(frame))
    a, pix = np.load(tmp_path / "a" / "accum.npy"), np.load(tmp_path / "a" / "accum_pixels.npy")
    assert a.dtype == np.float32 and pix.dtype == np.float64 and a.shape == (len(pix), 4)
    assert a.nbytes + pix.nbytes <= 4096 and len(pix) == 4096 // 24
    idx = pix.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 33 * 47
    assert np.array_equal(a, frame.reshape(-1, 4)[idx])
    assert np.array_equal(pix, np.load(tmp_path / "b" / "accum_pixels.npy"))  # the same pixels every run
    assert np.array_equal(a, np.load(tmp_path / "b" / "accum.npy"))


def _run(extra):
    r = subprocess.run([sys.executable, "bench.py"] + SMALL + extra, capture_output=True, text=True, cwd=ROOT,
                       timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1  # stdout holds exactly the result line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_contract_line_and_dumps_the_frame(tmp_path):
    import rustraytrace_amd as rrt

    line = _run(["--dump-outputs", str(tmp_path / "out")])
    assert line["metric"] == bench.METRIC and line["unit"] == "Mrays/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0
    assert line["ms_per_step"] > 0 and abs(line["ms_per_step"] - line["wall_clock_s_per_frame"] * 1e3) < 0.1
    assert not [k for k in FULL_ONLY if k in line]
    scene = rrt.config_scene("C2", image_width=96, samples_per_pixel=4)
    want = rrt.render(scene)
    assert line["rays_per_step"] > 0 and line["config"]["image"] == [scene.width, scene.height]
    assert os.listdir(tmp_path / "out") == ["accum.npy"]
    got = np.load(tmp_path / "out" / "accum.npy")
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
def test_two_rank_run_dumps_the_gathered_frame(tmp_path):
    """N > 1 (2 ranks sharing the GPU over gloo, bench.py starting them itself): the dump is rank
    0's gathered frame of the last step, equal to the 1-GPU render bit for bit; f64 with --f64."""
    import rustraytrace_amd as rrt

    args = ["--gpus", "2", "--config", "C3", "--width", "128", "--spp", "4", "--steps", "2", "--warmup", "1", "--f64",
            "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(RRT_BENCH_BACKEND="gloo", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "bench.py"] + args, capture_output=True, text=True, cwd=ROOT, env=env,
                       timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout)
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["dtype"] == "f64"
    assert not [k for k in FULL_ONLY + ("scaling_efficiency",) if k in line]
    want = rrt.render_f64(rrt.config_scene("C3", image_width=128, samples_per_pixel=4))
    got = np.load(tmp_path / "out" / "accum.npy")
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
def test_full_run_carries_the_roofline():
    line = _run(["--full", "--no-cpu-baseline", "--no-breakdown", "--no-extra", "--no-f64"])
    assert line["steps"] == 3 and line["roofline"]["algorithmic_flop_per_launch"] > 0
    assert line["rank0_rays_per_launch"] == line["rays_per_step"]
