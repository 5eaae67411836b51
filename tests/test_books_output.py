"""CPU side of the books path's output step: the host quantisers (rrt_quantize_accum_books[_f64],
color.rs:6-32) on the case set of tests/books_output_cases.py against a numpy f64 restatement and
the oracle's write_color; gather_rows (rustraytrace_amd/distributed.py) over 3-channel uint8 tiles,
what `multi_gpu --gather rgb8` moves; and the new entries' presence in the library and the package.
The device quantiser is held to the host one byte for byte in tests/test_gpu_books_output.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import books_output_cases as C
import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.distributed import band_rows, gather_rows


def test_case_set_is_the_documented_one():
    seen = set()
    for spp in C.SPPS:
        a = C.accum64(spp)
        assert a.shape == (C.N_ROWS, 4) and a.dtype == np.float64 and not a.flags.writeable
        assert np.array_equal(a[:, 1], a[::-1, 0], equal_nan=True) and np.all(a[:, 3] == spp)
        seen |= set(np.unique(C.write_color_numpy(a, spp)).tolist())
        # the steps themselves: k / 256 squared is exact, times spp rounds once; each lands on its byte
        k = np.arange(1, 256, dtype=np.float64)
        step = np.zeros((255, 4))
        step[:, 0] = spp * (k / 256.0) ** 2
        assert np.isin(step[:, 0], a[:, 0]).all()
    assert seen == set(range(256))  # every byte value occurs


@pytest.mark.parametrize("spp", C.SPPS)
def test_host_quantisers_equal_color_rs(spp):
    a64, a32 = C.accum64(spp), C.accum32(spp)
    got64 = rrt.quantize_accum_books_f64(C.N_ROWS, 1, a64, spp).reshape(-1, 3)
    got32 = rrt.quantize_accum_books(C.N_ROWS, 1, a32, spp).reshape(-1, 3)
    assert np.array_equal(got64, C.write_color_numpy(a64, spp))
    assert np.array_equal(got32, C.write_color_numpy(a32, spp))  # the f32 sums widened exactly, then the same
    scale = 1.0 / np.float64(spp)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(50):
            assert list(got64[i]) == list(oracle.write_color(scale * a64[i, :3])), (spp, i)
            assert list(got32[i]) == list(oracle.write_color(scale * a32[i, :3].astype(np.float64))), (spp, i)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


H, W, BAND = 27, 5, 16  # bands of 16 and 11 rows: with 3 ranks, rank 2 owns no rows


def _image(channels, dtype):
    rng = np.random.default_rng(channels)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(H, W, channels), dtype=np.uint8)
    return rng.uniform(0, 9, size=(H, W, channels)).astype(dtype)


def _gather_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rows = band_rows(H, BAND, rank, world)
        for name, ch, dt in (("rgb8", 3, np.uint8), ("f32", 4, np.float32), ("f64", 4, np.float64)):
            local = torch.from_numpy(np.ascontiguousarray(_image(ch, dt)[rows]))
            assert local.shape == (len(rows), W, ch)
            img = gather_rows(local, H, BAND, dist)
            if rank == 0:
                np.save(os.path.join(out_dir, name + ".npy"), img.numpy())
            else:
                assert img is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_rows_of_rgb8_tiles(tmp_path, world):
    """(rows, W, 3) uint8 tiles reassemble to the serpentine image; 4-channel float tiles as before."""
    mp.start_processes(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, start_method="spawn")
    for name, ch, dt in (("rgb8", 3, np.uint8), ("f32", 4, np.float32), ("f64", 4, np.float64)):
        got = np.load(str(tmp_path / (name + ".npy")))
        assert got.dtype == dt and got.shape == (H, W, ch) and np.array_equal(got, _image(ch, dt))
    if world == 3:
        assert len(band_rows(H, BAND, 2, 3)) == 0 and len(band_rows(H, BAND, 1, 3)) == 11


def test_new_entries_are_bound():
    lib = _lib.load()
    for name, nargs in (("rrt_quantize_accum_books_async", 5), ("rrt_quantize_accum_books_f64_async", 5),
                        ("rrt_hip_render_f64_rgb8", 11)):
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is not None
    assert lib.rrt_hip_abi_version() == 11  # additive: the version stays
    for name in ("render_f64_rgb8", "quantize_accum_books_async"):
        assert name in rrt.__all__ and callable(getattr(rrt, name))


def test_render_f64_rgb8_refuses_book2_scenes():
    with pytest.raises((ValueError, rrt.RrtError)):
        rrt.render_f64_rgb8(rrt.next_week_scene(1))


@pytest.mark.parametrize("book", [["the_next_week", "1"], ["the_next_week", "5"], ["the_rest_of_your_life"]])
def test_cli_books_f64_refuses_other_books(book):
    """Scene creation's refusal comes before any device call, so this holds with and without a GPU."""
    import subprocess

    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustraytrace_amd", "rrt")
    r = subprocess.run([cli, *book, "--books-f64", "--image_width", "32", "--samples_per_pixel", "4"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "HIP render failed: RRT_FLAG_F64 renders book-1 scenes" in r.stderr
    assert r.stdout == ""


def test_multi_gpu_gather_argument(capsys):
    from rustraytrace_amd import multi_gpu

    assert multi_gpu.parse([]).gather == "accum"  # the default: today's gather
    assert multi_gpu.parse(["--f64", "--gather", "rgb8", "--out", "x.ppm"]).gather == "rgb8"
    with pytest.raises(SystemExit) as e:
        multi_gpu.parse(["--gather", "rgb8", "--save-accum", "a.npy"])
    assert e.value.code == 2 and "--save-accum" in capsys.readouterr().err


def test_async_entries_check_their_arguments_before_any_device_call():
    """spp = 0 and null pointers are refused on the host with the host entries' messages (no device is
    touched: this runs on a box without one); n_pixels = 0 enqueues nothing."""
    for f64 in (False, True):
        with pytest.raises(rrt.RrtError, match="samples_per_pixel must be >= 1") as e:
            rrt.quantize_accum_books_async(4, 0x1000, 0, 0x2000, 0, f64=f64)
        assert e.value.code == -1
        for acc, out in ((0, 0x2000), (0x1000, 0)):
            with pytest.raises(rrt.RrtError, match="null accum or rgb8") as e:
                rrt.quantize_accum_books_async(4, acc, 8, out, 0, f64=f64)
            assert e.value.code == -1
        rrt.quantize_accum_books_async(0, 0, 8, 0, 0, f64=f64)
