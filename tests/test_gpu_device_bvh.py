"""The device BVH builder (RRT_FLAG_DEVICE_BVH, rustraytrace_amd/csrc/rrt_bvh_build.hip) on the GPU.

The builder is held to its sequential host twin (rrt_build_bvh_binned, the same header): equal node
bytes and leaf order for every scene of tests/device_bvh_scenes.py plus a 10^5-sphere scene. Renders
with the flag are checked the way every render here is: bit for bit against the oracle walking the
tree the scene holds (render_kbvh over rrt_scene_read_bvh), against TWIN and, for the f64 kernel,
against BOOKS, which does not depend on the tree. Without the flag scene creation holds the bytes
of rrt_build_bvh_ex.
"""
import os
import subprocess

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh, build_bvh_binned

import device_bvh_scenes as D

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustraytrace_amd", "rrt")


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def read_device_tree(sc, f64=False):
    ds = rrt.DeviceScene(sc, device=0, f64=f64, device_bvh=True)
    nodes, order, info = ds.read_bvh()
    ds.close()
    return nodes, order, info


def twin_of(sc, info, f64=False):
    """The twin's tree for the shape scene creation kept: the LDS shape's node price is 2, or 1.5
    for the f64 kernel; the global shapes' is 2."""
    cost = 1.5 if (f64 and info["node_stride"] == 80) else 2.0
    return build_bvh_binned(sc, info["max_leaf_param"], cost, info["node_stride"])


def assert_same_tree(a, b):
    assert a[2]["node_stride"] == b[2]["node_stride"] and a[2]["n_nodes"] == b[2]["n_nodes"]
    assert np.array_equal(a[1], b[1]), "leaf order differs"
    assert np.array_equal(a[0], b[0]), "node bytes differ"
    for k in ("n_leaves", "max_depth", "max_leaf_size", "n_unbounded", "node_bytes"):
        assert a[2][k] == b[2][k], k


def scale_scene():
    sc = rrt.rtow(image_width=32, samples_per_pixel=1, max_depth=4, grid_half=160)
    assert 90_000 < len(sc.spheres) < 110_000
    return sc


@pytest.mark.parametrize("name", list(D.SCENES))
def test_device_equals_twin_f32(name):
    sc = D.scene(name)
    dev = read_device_tree(sc)
    assert_same_tree(dev, twin_of(sc, dev[2]))


@pytest.mark.parametrize("name", D.BOOK1)
def test_device_equals_twin_f64(name):
    sc = D.scene(name)
    dev = read_device_tree(sc, f64=True)
    assert_same_tree(dev, twin_of(sc, dev[2], f64=True))


def test_device_equals_twin_at_1e5_spheres():
    """The scale case; the host sweep builder is never called on it."""
    sc = scale_scene()
    dev = read_device_tree(sc)
    assert dev[2]["node_stride"] == 32 and dev[2]["max_leaf_size"] == 1
    assert_same_tree(dev, twin_of(sc, dev[2]))
    gpu = rrt.render(sc, device_bvh=True)
    assert np.all(gpu[..., 3] == sc.spp) and np.isfinite(gpu).all()


@pytest.mark.parametrize("name", ["C2", "C5"])
def test_default_path_untouched(name):
    sc = D.scene(name)
    ds = rrt.DeviceScene(sc, device=0)
    nodes, order, info = ds.read_bvh()
    ds.close()
    h_nodes, h_order, h_info = build_bvh(sc)
    assert np.array_equal(nodes, h_nodes) and np.array_equal(order, h_order)
    assert info == h_info


def gpu_render_with_rays(sc, f64=False):
    torch = _torch()
    ds = rrt.DeviceScene(sc, device=0, f64=f64, device_bvh=True)
    tile = ds.tile(16, 0, 1, 0, sc.spp)
    rows = ds.tile_rows(tile)
    buf = torch.full((rows, sc.width, 4), float("nan"), dtype=torch.float64 if f64 else torch.float32, device="cuda:0")
    ds.reset_counters()
    render = ds.render_tile_f64_async if f64 else ds.render_tile_async
    render(tile, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rays = int(ds.counters()["rays"])
    tree = ds.read_bvh()
    ds.close()
    return buf.cpu().numpy(), rays, tree


def _book3():
    return rrt.rest_of_your_life_scene(D.KW)


@pytest.mark.parametrize("name", ["C2", "C5", "NW1", "NW7", "NW9", "B3"])
def test_render_parity_f32(name):
    sc = _book3() if name == "B3" else D.scene(name)
    gpu, rays, (nodes, order, info) = gpu_render_with_rays(sc)
    kref, krays, _ = oracle.render_kbvh(sc, nodes, order, info, threads=16)
    assert np.array_equal(gpu.astype(np.float64), kref), "flagged render differs from the oracle over its own tree"
    assert rays == krays
    if name in ("C2", "C5"):
        twin, twin_rays, _ = oracle.render(sc, oracle.TWIN, threads=16)
        assert np.array_equal(gpu.astype(np.float64), twin)


@pytest.mark.parametrize("name", ["C2", "C5"])
def test_render_parity_f64_books(name):
    """BOOKS never reads a tree: equal bits and query counts prove the f64 kernel's box test never
    prunes a hit on the device tree."""
    sc = rrt.config_scene(name, image_width=64, samples_per_pixel=16)
    gpu, rays, _ = gpu_render_with_rays(sc, f64=True)
    books, books_rays, _ = oracle.render(sc, oracle.BOOKS, threads=16)
    assert np.array_equal(gpu, books)
    assert rays == books_rays


def test_two_creations_give_the_same_bytes():
    for name in ("C5", "NW9"):
        a, b = read_device_tree(D.scene(name)), read_device_tree(D.scene(name))
        assert_same_tree(a, b)


def test_three_workers_equal_one():
    sc = D.scene("C5")
    lib = _lib.load()
    one = rrt.render(sc, device_bvh=True)
    lib.rrt_testing_device_wrap(1)
    try:
        three = rrt.render(sc, n_gpus=3, device_bvh=True)
    finally:
        lib.rrt_testing_device_wrap(0)
    assert np.array_equal(one, three)


def test_one_shot_entries_equal_the_device_scene_route():
    sc = D.scene("C5")
    accum, _, _ = gpu_render_with_rays(sc)
    assert np.array_equal(rrt.render(sc, device_bvh=True), accum)
    assert np.array_equal(rrt.render_rgb8(sc, device_bvh=True), rrt.quantize_accum(sc.width, sc.height, accum, sc.spp))
    nw = D.scene("NW9")
    nw_accum, _, _ = gpu_render_with_rays(nw)
    assert np.array_equal(rrt.render(nw, device_bvh=True), nw_accum)  # rrt_hip_render_ex
    assert np.array_equal(rrt.render_rgb8(nw, device_bvh=True),
                          rrt.quantize_accum(nw.width, nw.height, nw_accum, nw.spp))  # rrt_hip_render_rgb8_ex
    accum64, _, _ = gpu_render_with_rays(sc, f64=True)
    assert np.array_equal(rrt.render_f64(sc, device_bvh=True), accum64)
    assert np.array_equal(rrt.render_f64_rgb8(sc, device_bvh=True),
                          rrt.quantize_accum_books_f64(sc.width, sc.height, accum64, sc.spp))
    # the entries without an RrtSceneExt argument
    lib = _lib.load()
    flags = sc.flags | _lib.FLAG_QUIET | _lib.FLAG_DEVICE_BVH
    plain = np.zeros((sc.height, sc.width, 4), np.float32)
    _lib.check(lib.rrt_hip_render(_lib.ptr(sc.camera), _lib.ptr(sc.spheres), len(sc.spheres), _lib.ptr(sc.materials),
                                  len(sc.materials), None, 0, 0, 1, flags, _lib.ptr(plain)))
    assert np.array_equal(plain, accum)
    rgb = np.zeros((sc.height, sc.width, 3), np.uint8)
    _lib.check(lib.rrt_hip_render_rgb8(_lib.ptr(sc.camera), _lib.ptr(sc.spheres), len(sc.spheres),
                                       _lib.ptr(sc.materials), len(sc.materials), None, 0, 0, 1, flags, _lib.ptr(rgb)))
    assert np.array_equal(rgb, rrt.quantize_accum(sc.width, sc.height, accum, sc.spp))


def test_cli_device_bvh_equals_python(tmp_path):
    path = tmp_path / "nw9.ppm"
    r = subprocess.run([CLI, "--backend", "hip", "the_next_week", "9", "--image_width", "32", "--samples_per_pixel", "4",
                        "--device-bvh", "-o", str(path)], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    sc = D.scene("NW9")
    acc = rrt.render(sc, device_bvh=True)
    assert path.read_bytes() == rrt.format_ppm_from_accum(sc.width, sc.height, acc, sc.spp)


def test_width_4_is_refused_with_the_flag(monkeypatch):
    monkeypatch.setenv("RRT_BVH_WIDTH", "4")
    with pytest.raises(rrt.RrtError) as e:
        rrt.DeviceScene(D.scene("C2"), device=0, device_bvh=True)
    assert e.value.code == -1 and "RRT_FLAG_DEVICE_BVH" in str(e.value)
