"""The host twin of the fast device builder (rrt_build_bvh_lbvh, rrt_refit_bvh_lbvh_world;
rustraytrace_amd/csrc/rrt_bvh_lbvh.h is the algorithm both sides compile). No GPU: the twin is the
specification the device builder behind RRT_FLAG_FAST_BVH is held to (tests/test_gpu_fast_bvh.py), so
its trees are checked here for structure, for their leaf order against a numpy restatement of the sort
key, for their stored boxes (containment, and a build being its own refit), for being conservative in
use (the oracle walking them renders what a linear scan renders) and, as a tripwire for an interleave
that is valid but useless, for quality against the binned builder's trees."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned, build_bvh_lbvh, refit_bvh_lbvh_world

import device_bvh_scenes as D
import lbvh_scenes as L
import test_bvh_binned as B  # walk(), prim_boxes(): the binned twin's own restatements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 80), (1, 32), (1, 80)]
CASES = [(name, ml, st) for name in list(D.SCENES) + [k for k in L.SCENES if k not in D.SCENES] for ml, st in SHAPES]
IDS = [f"{n}-leaf{ml}-{st}B" for n, ml, st in CASES]

_trees = {}


def twin(name, max_leaf, stride):
    key = (name, max_leaf, stride)
    if key not in _trees:
        _trees[key] = build_bvh_lbvh(L.lookup(name), max_leaf, stride)
    return _trees[key]


@pytest.mark.parametrize("name,max_leaf,stride", CASES, ids=IDS)
def test_structure(name, max_leaf, stride):
    sc = L.lookup(name)
    tree = twin(name, max_leaf, stride)
    nodes, order, info = tree
    n_all = D.n_prims(sc)
    n_tree = n_all - info["n_unbounded"]
    assert info["node_stride"] == stride and info["max_leaf_param"] == max_leaf and info["width"] == 2
    assert nodes.size == info["node_bytes"] == info["n_nodes"] * stride
    assert sorted(order.tolist()) == list(range(n_all)), "prim_order is not a permutation"
    rng, depth, bfs, (lo, hi, first, cnt) = B.walk(tree, n_tree)
    # child ranges are contiguous, partition the parent's and are adjacent; the root covers the tree
    assert np.array_equal(rng[:, 0, 1], rng[:, 1, 0])
    assert rng[0, 0, 0] == 0 and rng[0, 1, 1] == n_tree
    both_leaves = (cnt[:, 0] > 0) & (cnt[:, 1] > 0)
    assert np.array_equal(first[both_leaves, 1], first[both_leaves, 0] + cnt[both_leaves, 0]), "sibling leaves are not adjacent"
    assert cnt.max() <= max_leaf
    # a leaf's parent holds more than max_leaf (the root-leaf form aside)
    if info["n_nodes"] > 1 or cnt[0, 1] > 0:
        assert ((rng[:, 1, 1] - rng[:, 0, 0]) > max_leaf).all()
    # breadth-first: by level, within a level by the start of the range
    assert bfs == list(range(info["n_nodes"])), "numbering is not breadth-first"
    start = rng[:, 0, 0]
    for k in range(1, info["n_nodes"]):
        assert (depth[k - 1], start[k - 1]) < (depth[k], start[k])
    leaves = int((cnt > 0).sum())
    assert info["n_leaves"] == leaves and info["max_leaf_size"] == int(cnt.max())
    assert info["max_depth"] == int(depth.max()) + 1
    assert info["max_depth"] + 1 <= 63, "stack_need"
    assert int(cnt.sum()) == n_tree
    again = build_bvh_lbvh(sc, max_leaf, stride)
    assert np.array_equal(again[0], nodes) and np.array_equal(again[1], order) and again[2] == info


def spread10(v):
    v = v.astype(np.uint64) & 0x3FF
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def numpy_order(sc, tree_prims):
    """rrt_bvh_lbvh.h's sort key restated: the leaf order of the tree's primitives (source order in)."""
    plo, phi = B.prim_boxes(sc)
    c = 0.5 * (plo[tree_prims] + phi[tree_prims])
    code = np.zeros(len(tree_prims), np.uint64)
    with np.errstate(all="ignore"):
        for a in range(3):
            cmin, cmax = c[:, a].min(), c[:, a].max()

            def bin16(x):
                v = (x - cmin) * (16.0 / (cmax - cmin))
                return 15 if not v < 16.0 else (int(v) if v > 0.0 else 0)

            usable = cmax > cmin and bin16(cmax) > bin16(cmin)
            cell = np.zeros(len(c), np.uint64)
            if usable:
                x = (c[:, a] - cmin) * (1024.0 / (cmax - cmin))
                cell = np.where(~(x < 1024.0), 1023, np.where(x > 0.0, np.floor(x), 0.0)).astype(np.uint64)
            code |= spread10(cell) << np.uint64(2 - a)
    key = (code << np.uint64(32)) | np.arange(len(tree_prims), dtype=np.uint64)
    return np.asarray(tree_prims)[np.argsort(key, kind="stable")]


@pytest.mark.parametrize("name", [n for n, ml, st in CASES if (ml, st) == (1, 32)])
def test_leaf_order_is_the_sorted_key(name):
    sc = L.lookup(name)
    for max_leaf, stride in SHAPES:  # one order whatever the shape
        nodes, order, info = twin(name, max_leaf, stride)
        n_tree = D.n_prims(sc) - info["n_unbounded"]
        tree_prims = np.sort(order[:n_tree])
        assert np.array_equal(order[:n_tree], numpy_order(sc, tree_prims))
        assert (order[n_tree:] >= len(sc.spheres) + (0 if sc.quads is None else len(sc.quads))).all()  # the unbounded media


@pytest.mark.parametrize("name,max_leaf,stride", CASES, ids=IDS)
def test_stored_boxes(name, max_leaf, stride):
    sc = L.lookup(name)
    tree = twin(name, max_leaf, stride)
    nodes, order, info = tree
    n_tree = D.n_prims(sc) - info["n_unbounded"]
    rng, depth, bfs, (lo, hi, first, cnt) = B.walk(tree, n_tree)
    plo, phi = B.prim_boxes(sc)
    plo, phi = plo[order], phi[order]
    for k in range(info["n_nodes"]):
        for c in range(2):
            a, b = rng[k, c]
            if a < b:
                assert (lo[k, c].astype(np.float64) <= plo[a:b].min(axis=0)).all() and (hi[k, c].astype(np.float64) >= phi[a:b].max(axis=0)).all()
    # a build is its own refit
    r_nodes, r_order, r_info, sah = refit_bvh_lbvh_world(sc, sc, max_leaf, stride)
    assert np.array_equal(r_nodes, nodes) and np.array_equal(r_order, order) and r_info == info
    assert np.isfinite(sah) and sah > 0.0


_twin_render = {}


def twin_render(name):
    if name not in _twin_render:
        _twin_render[name] = oracle.render(D.scene(name), oracle.TWIN, threads=8)
    return _twin_render[name]


@pytest.mark.parametrize("max_leaf,stride", SHAPES)
@pytest.mark.parametrize("name", ["C2", "C5", "NW1"])
def test_walking_the_twin_tree_renders_the_linear_scan(name, max_leaf, stride):
    sc = D.scene(name)
    nodes, order, info = twin(name, max_leaf, stride)
    kacc, _, _ = oracle.render_kbvh(sc, nodes, order, info, threads=8)
    assert np.array_equal(kacc, twin_render(name)[0])


def test_equal_codes_sort_by_index_and_split_by_index_bits():
    nodes, order, info = twin("one_centre64", 1, 32)
    assert np.array_equal(order, np.arange(64))
    assert info["max_depth"] == 6 and info["n_nodes"] == 63
    nodes, order, info = twin("one_centre64", 3, 80)  # leaves of 2: the pairs of the level above
    assert info["max_depth"] == 5 and info["n_nodes"] == 31 and info["max_leaf_size"] == 2


def test_two_unusable_axes_sort_along_the_third():
    nodes, order, info = twin("line65", 1, 32)
    assert np.array_equal(order, np.arange(65))  # the spheres are given by increasing x


def test_root_leaf_form():
    for name, n in (("spheres2", 2), ("spheres3", 3), ("fog2", 2)):
        nodes, order, info = twin(name, 3, 80)
        assert (info["n_nodes"], info["n_leaves"], info["max_depth"], info["max_leaf_size"]) == (1, 1, 1, n)
        # the binned builder's form: child 0 = the leaf of all n, child 1 the never-hit box with link 0
        assert nodes.view(np.uint32)[18:20].tolist() == [n << 28, 0]
        assert (nodes.view(np.float32)[9:18] >= np.float32(9e29)).all()
        nodes, order, info = twin(name, 1, 32)
        assert info["n_nodes"] == n - 1 and info["max_leaf_size"] == 1
    assert twin("fog2", 1, 32)[2]["n_unbounded"] == 1


# Primitive tests per ray of the oracle's walk at 64x36x8, the LBVH twin's (1, 32) tree over the
# binned twin's: the measured ratios plus 0.05. Leaves of 1 leave little room in
# primitive tests, so this is a tripwire for a broken interleave, not a quality claim.
QUALITY = {"C2": 0.9756 + 0.05, "C5": 0.9595 + 0.05, "NW9": 1.0334 + 0.05}


@pytest.mark.parametrize("name", sorted(QUALITY))
def test_quality_against_the_binned_tree(name):
    kw = dict(image_width=64, samples_per_pixel=8)
    sc = rrt.config_scene(name, **kw) if name.startswith("C") else rrt.next_week_scene(9, kw)
    nodes, order, info = build_bvh_lbvh(sc, 1, 32)
    b_nodes, b_order, b_info = build_bvh_binned(sc, 1, 2.0, 32)
    _, rays, tests = oracle.render_kbvh(sc, nodes, order, info, threads=8)
    _, b_rays, b_tests = oracle.render_kbvh(sc, b_nodes, b_order, b_info, threads=8)
    ratio = (tests / rays) / (b_tests / b_rays)
    print(f"{name}: primitive tests per ray {tests / rays:.4f} (lbvh) vs {b_tests / b_rays:.4f} (binned), ratio {ratio:.4f}")
    assert ratio <= QUALITY[name]


def test_abi_flag_and_exports():
    header = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert re.search(r"#define\s+RRT_FLAG_FAST_BVH\s+0x40u\b", header)
    assert re.search(r"RRT_BUILDER_BINNED\s*=\s*0\s*,\s*RRT_BUILDER_LBVH\s*=\s*1", header)
    assert _lib.FLAG_FAST_BVH == 0x40 and _lib.BUILDERS == {"binned": 0, "lbvh": 1}
    lib = _lib.load()
    for name in ("rrt_build_bvh_lbvh", "rrt_refit_bvh_lbvh_world", "rrt_scene_set_builder",
                 "rrt_testing_scene_build_stats", "rrt_testing_lbvh_form"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.rrt_hip_abi_version() == 11
    assert ctypes.sizeof(_lib.RrtSceneBuildStats) == 40


def test_bad_arguments_are_refused(monkeypatch):
    sc = D.scene("C2")
    for ml, st in ((0, 80), (8, 80), (3, 64), (3, 0)):
        with pytest.raises(rrt.RrtError):
            build_bvh_lbvh(sc, ml, st)
        with pytest.raises(rrt.RrtError):
            refit_bvh_lbvh_world(sc, sc, ml, st)
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    n = len(sc.spheres)
    assert lib.rrt_build_bvh_lbvh(None, n, None, 3, 80, None, 0, None, ctypes.byref(info)) == -1  # null spheres
    assert lib.rrt_refit_bvh_lbvh_world(_lib.ptr(sc.spheres), n, None, 3, 80, None, None, None, 0, None, ctypes.byref(info), None) == -1
    # the sizing call, then a buffer one byte short and a null order
    assert lib.rrt_build_bvh_lbvh(_lib.ptr(sc.spheres), n, None, 3, 80, None, 0, None, ctypes.byref(info)) == 0
    assert info.node_bytes == info.n_nodes * 80 and info.n_nodes > 1
    nodes, order = np.zeros(info.node_bytes, np.uint8), np.zeros(n, np.uint32)
    assert lib.rrt_build_bvh_lbvh(_lib.ptr(sc.spheres), n, None, 3, 80, _lib.ptr(nodes), nodes.size - 1, _lib.ptr(order), None) == -1
    assert lib.rrt_build_bvh_lbvh(_lib.ptr(sc.spheres), n, None, 3, 80, _lib.ptr(nodes), nodes.size, None, None) == -1
    assert lib.rrt_build_bvh_lbvh(_lib.ptr(sc.spheres), n, None, 3, 80, _lib.ptr(nodes), nodes.size, _lib.ptr(order), None) == 0
    assert np.array_equal(nodes, twin("C2", 3, 80)[0])
    # a medium whose boundary range leaves the boundary quads
    fog = L.scene("fog2")
    bad = fog.media.copy()
    bad["boundary_kind"][0], bad["first"][0], bad["count"][0] = 1, 0, 6
    with pytest.raises(rrt.RrtError):
        build_bvh_lbvh(dataclasses.replace(fog, media=bad), 3, 80)
    monkeypatch.setenv("RRT_BVH_WIDTH", "4")
    with pytest.raises(rrt.RrtError, match="RRT_BVH_WIDTH"):
        build_bvh_lbvh(sc, 3, 80)
    with pytest.raises(rrt.RrtError, match="RRT_BVH_WIDTH"):
        refit_bvh_lbvh_world(sc, sc, 3, 80)
