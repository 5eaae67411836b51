"""GPU: every book-2/3 instantiation of the f32 kernel (classes 1 moving spheres, 2 quads, 3 media,
4 the book-3 integrator) against the oracle, on the scenes of tests/book2_class_scenes.py.

The stock scenes (tests/test_gpu_book2.py, test_gpu_book3.py) reach nine of the sixteen class x noise
x placement cells, on staged trees of 1 to 10 nodes. Here each cell renders a tree of 30 to 80 nodes
with every primitive kind and material in it; then the noise builds with their Perlin tables left in
global memory (RRT_PERLIN_IN_LDS=0), stacks of more than 60 entries in classes 2 to 4 (staged: over
64 KiB of LDS, the raised limit), the 32-bit-stack kernel in classes 1 to 3, trees built on the
device, and the one-shot entry. Every frame is held bit for bit to the oracle's walk of the tree the
scene holds (KBVH) and to the oracle's own tree (TWIN), with equal ray and path counts; the launch
plan is asserted with each render, so a case cannot pass in another instantiation than it names.
tests/test_book2_class_scenes.py checks on the CPU that the scenes are what this file assumes.
"""
import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle

import book2_class_scenes as B
from test_book2_class_scenes import (DEEP, PLACEMENT_IDS, PLACEMENTS, check_cell, check_deep, check_wide, kbvh, place,
                                     twin)
from test_gpu_device_bvh import gpu_render_with_rays
from test_gpu_parity import assert_bit_exact, gpu_tile

pytestmark = pytest.mark.gpu

_CELL_FRAMES = {}  # (cls, noise, in_lds) -> the frame of test_cells, for the Perlin-placement cases


def _render_and_compare(in_lds, name, *args, use_twin=True, twin_rays=True):
    """One tile render with counters and the counting twin, against KBVH over the host tree of the
    placement and (use_twin) against TWIN; returns the frame."""
    scene = B.built(in_lds, name, *args)[0]
    gpu, idx, ctr, work = gpu_tile(scene, count=True)
    assert len(idx) == scene.height
    ref, krays = kbvh(in_lds, name, *args)
    assert_bit_exact(gpu, ref, scene.spp)
    assert ctr["rays"] == krays == work["rays"]
    assert ctr["paths"] == work["paths"] == scene.width * scene.height * scene.spp
    assert np.all(gpu[..., 3] == scene.spp)
    if use_twin:
        tw, trays = twin(name, *args)
        assert_bit_exact(gpu, tw, scene.spp)
        assert trays == krays or not twin_rays
    return gpu


# ---- A: the 16 cells ------------------------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("cls", B.CLASSES)
def test_cells(monkeypatch, cls, noise, in_lds):
    place(monkeypatch, in_lds)
    scene, _, order, info = B.built(in_lds, "composite", cls, noise)
    check_cell(scene, info, order, cls, noise, in_lds)
    _CELL_FRAMES[cls, noise, in_lds] = _render_and_compare(in_lds, "composite", cls, noise)


# ---- B: Perlin tables outside LDS -----------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("cls", B.CLASSES)
def test_perlin_tables_in_global_memory(monkeypatch, cls, in_lds):
    """noise_at's generic-pointer branch: the tables are read where scene creation uploaded them and
    the block's carve-up has no table region. The oracle does not know the variable, and the frame
    equals the staged tables' too."""
    place(monkeypatch, in_lds)
    scene, _, order, info = B.built(in_lds, "composite", cls, True)
    if (cls, True, in_lds) not in _CELL_FRAMES:  # run on its own
        _CELL_FRAMES[cls, True, in_lds] = gpu_tile(scene)[0]
    place(monkeypatch, in_lds, "0")
    check_cell(scene, info, order, cls, True, in_lds, "0")
    gpu = _render_and_compare(in_lds, "composite", cls, True)
    assert np.array_equal(gpu, _CELL_FRAMES[cls, True, in_lds])


# ---- C: deep stacks in classes 2 to 4 -------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("cls", [2, 3, 4])
def test_deep_stacks(monkeypatch, cls, in_lds):
    """A stack of more than 60 entries. Staged: more than 64 KiB of LDS in a 256-thread block, the
    raised dynamic-LDS limit. Forced to global memory: the deep chain on the f16 nodes. The coincident
    spheres tie, so TWIN's ray count is not compared."""
    place(monkeypatch, in_lds)
    scene, _, order, info = B.built(in_lds, "composite", cls, *DEEP)
    check_deep(scene, info, order, cls, in_lds)
    _render_and_compare(in_lds, "composite", cls, *DEEP, twin_rays=False)


# ---- D: the 32-bit stack in classes 1 to 3 --------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2, 3])
def test_32_bit_stack(monkeypatch, cls):
    """More than 65,535 nodes: kArmStack32 with the class's primitives (KBVH alone is the reference:
    test_gpu_launch_shapes.py test_32_bit_stack_kernel)."""
    place(monkeypatch, None)
    scene, _, order, info = B.built(None, "moving_wide", cls)
    check_wide(scene, info, order, cls)
    _render_and_compare(None, "moving_wide", cls, use_twin=False)


# ---- E: device-built trees ------------------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("cls", B.CLASSES)
def test_device_built_trees(monkeypatch, cls, in_lds):
    """RRT_FLAG_DEVICE_BVH: the binned builder's tree of the noise composite, read back and walked by
    the oracle."""
    place(monkeypatch, in_lds)
    scene = B.composite(cls, True)
    gpu, rays, (nodes, order, info) = gpu_render_with_rays(scene)
    check_cell(scene, info, order, cls, True, in_lds, min_depth=0)
    ref, krays, _ = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    assert_bit_exact(gpu, ref, scene.spp)
    assert rays == krays
    tw, trays = twin("composite", cls, True)
    assert_bit_exact(gpu, tw, scene.spp)
    assert trays == krays
    assert np.all(gpu[..., 3] == scene.spp)


# ---- F: the one-shot entry ------------------------------------------------------------------------
@pytest.mark.parametrize("cls", B.CLASSES)
def test_one_shot_entry_equals_the_tile_route(monkeypatch, cls):
    place(monkeypatch, None)
    scene = B.built(None, "composite", cls, True)[0]
    if (cls, True, None) not in _CELL_FRAMES:
        _CELL_FRAMES[cls, True, None] = gpu_tile(scene)[0]
    assert np.array_equal(rrt.render(scene), _CELL_FRAMES[cls, True, None])
