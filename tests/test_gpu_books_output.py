"""The books path's output step on the device: the color.rs quantiser kernel (rrt_books64.hip
rrt_quantize_books, entries rrt_quantize_accum_books[_f64]_async) byte for byte against the host
quantiser — which tests/test_books_output.py holds to color.rs on the same case set, chosen at the
quantisation steps where an inexact square root moves a byte; the one-shot rrt_hip_render_f64_rgb8
against quantize_accum_books_f64 of rrt_hip_render_f64's sums and of the oracle's books render, on one
and on several workers; the CLI's --books-f64; and multi_gpu's --gather rgb8."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import books_output_cases as C
import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rustraytrace_amd", "rrt")
GUARD = 16


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _host_bytes(acc, spp, f64):
    fn = rrt.quantize_accum_books_f64 if f64 else rrt.quantize_accum_books
    return fn(len(acc), 1, acc, spp).reshape(-1)


def _check_device_quantiser(acc, spp, f64):
    """Device bytes == host bytes on the current stream and on a stream of its own; the 16 guard
    bytes after 3 * n_px stay as they were (the ragged last group is stored byte by byte)."""
    torch = _torch()
    n_px = len(acc)
    want = _host_bytes(acc, spp, f64)
    d_acc = torch.from_numpy(np.array(acc)).to("cuda:0")  # a copy: the shared case arrays are read-only
    side = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), side):
        d_rgb = torch.full((3 * n_px + GUARD,), 77, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rrt.quantize_accum_books_async(n_px, d_acc.data_ptr(), spp, d_rgb.data_ptr(), stream.cuda_stream, f64=f64)
        stream.synchronize()
        got = d_rgb.cpu().numpy()
        diff = np.flatnonzero(got[: 3 * n_px] != want)
        assert diff.size == 0, (f"{diff.size} bytes differ, first at pixel {diff[0] // 3} channel {diff[0] % 3}: "
                                f"sum {acc[diff[0] // 3, diff[0] % 3]!r} device {got[diff[0]]} host {want[diff[0]]}")
        assert np.all(got[3 * n_px:] == 77), "bytes past 3 * n_pixels were written"


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("n_px", [1, 3, 4, 5, 1000])
def test_device_quantiser_ragged_sizes(n_px, f64):
    # from the byte-128 step's neighbours on (spp 13): whole groups, a ragged tail, one lone pixel
    spp = 13
    acc = (C.accum64 if f64 else C.accum32)(spp)
    _check_device_quantiser(C.fill(acc[9 * 128 - 2:], n_px), spp, f64)


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("spp", C.SPPS)
def test_device_quantiser_whole_case_set(spp, f64):
    acc = (C.accum64 if f64 else C.accum32)(spp)
    assert len(acc) % 4 == 0
    _check_device_quantiser(np.ascontiguousarray(acc), spp, f64)
    _check_device_quantiser(np.ascontiguousarray(acc[:-1]), spp, f64)  # the same set ending in a 3-pixel group


@functools.lru_cache(maxsize=None)
def _frame(cfg):
    """(scene, f64 sums of rrt_hip_render_f64, their books-path bytes): rendered once per config."""
    _torch()
    scene = rrt.config_scene(cfg, image_width=48, samples_per_pixel=16)
    assert scene.height == 27
    sums = rrt.render_f64(scene)
    want = rrt.quantize_accum_books_f64(scene.width, scene.height, sums, scene.spp)
    want.setflags(write=False)
    return scene, sums, want


@pytest.mark.parametrize("cfg", ["C1", "C2", "C4"])
def test_one_shot_f64_rgb8(cfg):
    scene, sums, want = _frame(cfg)
    got = rrt.render_f64_rgb8(scene)
    assert got.shape == (27, 48, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    books, _, _ = oracle.render(scene, oracle.BOOKS, threads=16)
    assert np.array_equal(got, rrt.quantize_accum_books_f64(scene.width, scene.height, books, scene.spp))
    assert rrt.format_pnm_from_rgb8(48, 27, got) == rrt.format_pnm_from_rgb8(48, 27, want)
    assert len(np.unique(got)) > 20  # an image, not a constant


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("cfg", ["C2", "C4"])
def test_one_shot_f64_rgb8_several_workers(cfg, n):
    """27 rows in 16-row bands: worker 1 owns a partial band of 11 rows, and of 3 workers the last none."""
    scene, _, want = _frame(cfg)
    lib = _lib.load()
    lib.rrt_testing_device_wrap(1)
    try:
        got = rrt.render_f64_rgb8(scene, n_gpus=n)
    finally:
        lib.rrt_testing_device_wrap(0)
    assert np.array_equal(got, want)


def test_errors():
    torch = _torch()
    scene, _, _ = _frame("C1")
    lib = _lib.load()
    args = (_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres), _lib.ptr(scene.materials),
            len(scene.materials), None, 0, 0, 1, _lib.FLAG_QUIET)
    assert lib.rrt_hip_render_f64_rgb8(*args, None) == -1  # RRT_E_INVALID
    assert b"rgb8_out" in lib.rrt_hip_last_error()
    d_acc = torch.zeros((4, 4), dtype=torch.float64, device="cuda:0")
    d_rgb = torch.full((12,), 77, dtype=torch.uint8, device="cuda:0")
    for f64 in (True, False):
        with pytest.raises(rrt.RrtError, match="samples_per_pixel must be >= 1") as e:
            rrt.quantize_accum_books_async(4, d_acc.data_ptr(), 0, d_rgb.data_ptr(), 0, f64=f64)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert np.all(d_rgb.cpu().numpy() == 77)
    book2 = rrt.next_week_scene(1, dict(image_width=32, samples_per_pixel=2, max_depth=4))
    with pytest.raises(ValueError, match="book-1"):
        rrt.render_f64_rgb8(book2)
    # the library's own refusal (scene creation), for a caller that passes book-2 materials through the C entry
    out = np.zeros((book2.height, book2.width, 3), np.uint8)
    rc = lib.rrt_hip_render_f64_rgb8(_lib.ptr(book2.camera), _lib.ptr(book2.spheres), len(book2.spheres),
                                     _lib.ptr(book2.materials), len(book2.materials), None, 0, 0, 1,
                                     book2.flags | _lib.FLAG_QUIET, _lib.ptr(out))
    assert rc == -1 and b"RRT_FLAG_F64 renders book-1 scenes" in lib.rrt_hip_last_error()


def test_cli_books_f64(tmp_path):
    _torch()
    args = [CLI, "--backend", "hip", "in_one_weekend", "--books-f64", "--image_width", "64", "--samples_per_pixel", "4",
            "--max_depth", "6"]
    outs = {}
    for name, extra in [("dev", []), ("host", ["--host-quantise"]), ("p6", ["--p6"])]:
        path = tmp_path / f"{name}.ppm"
        r = subprocess.run(args + extra + ["-o", str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[name] = path.read_bytes()
    assert outs["dev"] == outs["host"]
    head, px = outs["p6"].split(b"\n255\n", 1)
    assert head == b"P6\n64 36"
    assert list(px) == [int(v) for v in outs["dev"].split(b"\n255\n", 1)[1].split()]
    scene = rrt.rtow(image_width=64, samples_per_pixel=4, max_depth=6)  # the CLI's default seed is Python's
    assert outs["dev"] == rrt.format_pnm_from_rgb8(scene.width, scene.height, rrt.render_f64_rgb8(scene))
    r = subprocess.run([CLI, "--backend", "hip", "the_next_week", "1", "--books-f64", "--image_width", "32",
                        "--samples_per_pixel", "2", "--max_depth", "4", "-o", str(tmp_path / "nw.ppm")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "HIP render failed: " in r.stderr and "RRT_FLAG_F64" in r.stderr
    assert not (tmp_path / "nw.ppm").exists()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _multi_gpu(ranks, args):
    """rustraytrace_amd.multi_gpu under torch.distributed.run: a fresh child process per rank (sharing the
    GPU over gloo), the launch under a time limit; returns rank 0's JSON line."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", "-m", "rustraytrace_amd.multi_gpu",
           "--config", "C2", "--width", "64", "--spp", "8", "--backend", "gloo"] + args
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_multi_gpu_gather_rgb8(tmp_path, f64):
    """2 ranks quantise their tiles on the device and gather 3 B/pixel: the PPM of the 1-rank run that
    gathers the accum and quantises on the host (color.rs's bytes with --f64, render_io's without)."""
    _torch()
    mode = ["--f64"] if f64 else []
    one, two = str(tmp_path / "one.ppm"), str(tmp_path / "two.ppm")
    base = _multi_gpu(1, mode + ["--out", one])
    line = _multi_gpu(2, mode + ["--gather", "rgb8", "--out", two])
    assert "gather" not in base and "gather_bytes" not in base  # the default line is unchanged
    assert line["gather"] == "rgb8" and line["gather_bytes"] == 64 * 36 * 3 and line["ranks"] == 2
    assert line["dtype"] == ("f64" if f64 else "f32") and line["rays"] == base["rays"]
    with open(one, "rb") as a, open(two, "rb") as b:
        want, got = a.read(), b.read()
    assert want.startswith(b"P3\n64 36\n255\n") and got == want
