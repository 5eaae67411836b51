"""rrt_refit_bvh_binned_ex: the host twin of the device refit with new quads as well, the specification
rrt_scene_refit_geometry's tree is held to (tests/test_gpu_scene_geometry.py). No GPU. Checked here:
with the built quads it reproduces the builder's tree and cost; with new_quads NULL it is
rrt_refit_bvh_binned; after a move of the quads the tree keeps links and order, every stored box
contains its subtree's new primitive boxes (the numpy specification of tests/test_bvh_binned.py), and
its SAH cost is not below that of a fresh build over the moved quads. Nothing compares with a tolerance.
"""
import ctypes

import numpy as np
import pytest

from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned, decode_bvh2, refit_bvh_binned, scene_ext

import device_bvh_scenes as D
import geometry_scenes as G
from test_bvh_refit import child_unions, numpy_sah

NODE_COST = 2.0
SCENES = ["NW5", "NW7", "mixed", "big"]
# "A refitted tree costs at least what a fresh build of the moved scene costs" is asserted on the books'
# scenes. It is no theorem: the binned builder is greedy (each task takes its locally cheapest plane),
# so a fresh build is not a lower bound, and on the random 300-quad scene `big` the kept topology comes
# out cheaper after the 0.01 jitter (3 / 80: 31.0066 refitted against 31.1686 built afresh; 1 / 32:
# 32.4210 against 32.5258). There the test prints both figures and asserts only that sah_out is its
# definition, which it asserts everywhere.
BOOK_SCENES = ("NW5", "NW7", "mixed")


@pytest.mark.parametrize("max_leaf,stride", D.SHAPES)
@pytest.mark.parametrize("name", SCENES)
def test_refit_over_the_built_quads_is_the_built_tree(name, max_leaf, stride):
    sc = G.scene(name)
    built = build_bvh_binned(sc, max_leaf, NODE_COST, stride)
    at_build = refit_bvh_binned(sc, sc.spheres, sc.motion, max_leaf, NODE_COST, stride)[3]
    nodes, order, info, sah = refit_bvh_binned(sc, sc.spheres, sc.motion, max_leaf, NODE_COST, stride, new_quads=sc.quads)
    assert info == built[2]
    assert np.array_equal(order, built[1])
    assert nodes.tobytes() == built[0].tobytes()
    assert np.float64(sah).tobytes() == np.float64(at_build).tobytes() and np.isfinite(sah) and sah > 0.0


@pytest.mark.parametrize("name", SCENES)
def test_null_quads_is_the_sphere_refit(name):
    sc = G.scene(name)
    sp = G.jitter_spheres(sc.spheres, 11, 0.2)
    nodes, order, info, sah = refit_bvh_binned(sc, sp, sc.motion, 3, NODE_COST, 80, new_quads=None)
    # rrt_refit_bvh_binned itself, sized by the info above
    lib = _lib.load()
    ext, keep = scene_ext(sc)
    info2, sah2 = _lib.RrtBvhInfo(), ctypes.c_double(0.0)
    nodes2, order2 = np.zeros(nodes.size, np.uint8), np.zeros(max(len(order), 1), np.uint32)
    m = None if sc.motion is None else np.ascontiguousarray(sc.motion, np.float32)
    _lib.check(lib.rrt_refit_bvh_binned(_lib.ptr(sc.spheres), len(sc.spheres), ctypes.byref(ext), 3, NODE_COST, 80,
                                        _lib.ptr(sp), _lib.ptr(m), _lib.ptr(nodes2), nodes2.size, _lib.ptr(order2),
                                        ctypes.byref(info2), ctypes.byref(sah2)))
    del keep
    assert nodes2.tobytes() == nodes.tobytes() and np.array_equal(order2[:len(order)], order)
    assert info2.as_dict() == info and np.float64(sah2.value).tobytes() == np.float64(sah).tobytes()


@pytest.mark.parametrize("seed,scale", [(11, 0.01), (12, 0.1)])
@pytest.mark.parametrize("max_leaf,stride", [(3, 80), (1, 32)])
@pytest.mark.parametrize("name", SCENES)
def test_stored_boxes_and_cost_after_a_move_of_the_quads(name, max_leaf, stride, seed, scale):
    sc = G.scene(name)
    built = build_bvh_binned(sc, max_leaf, NODE_COST, stride)
    spheres, quads, _ = G.moved(sc, seed, scale)
    new = G.with_geometry(sc, spheres, sc.motion, quads)
    tree = refit_bvh_binned(sc, spheres, sc.motion, max_leaf, NODE_COST, stride, new_quads=quads)
    nodes, order, info, sah = tree
    assert info == built[2] and np.array_equal(order, built[1])
    b_first, b_cnt = decode_bvh2(built[0], stride)[2:]
    ulo, uhi, real, _, (lo, hi, first, cnt) = child_unions(tree, new)
    assert np.array_equal(first, b_first) and np.array_equal(cnt, b_cnt), "the refit changed a link"
    assert nodes.tobytes() != built[0].tobytes(), "the move did not change a box"
    assert (lo[real].astype(np.float64) <= ulo[real]).all() and (hi[real].astype(np.float64) >= uhi[real]).all()
    # sah_out is its definition over the refitted boxes, bit for bit
    assert np.float64(sah).tobytes() == np.float64(numpy_sah(tree, new, NODE_COST)).tobytes()
    # the cost of the tree a fresh build makes of the moved scene: its identity refit's
    fresh = refit_bvh_binned(new, spheres, sc.motion, max_leaf, NODE_COST, stride, new_quads=quads)[3]
    print(f"{name} {max_leaf}/{stride} jitter {scale}: sah {sah!r} refitted, {fresh!r} built afresh")
    if name in BOOK_SCENES:
        assert sah >= fresh
