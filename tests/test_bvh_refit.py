"""The host twin of the device BVH refit (rrt_refit_bvh_binned; rrt_bvh_binned.h refit_raw is the
algorithm both sides compile). No GPU: the twin defines the feature, and tests/test_gpu_scene_refit.py
holds the device to its bytes. Checked here: a refit over unchanged spheres reproduces the builder's
tree (the key-ordered union, and the builder's boxes are tight); after a move the tree keeps links
and order, its stored boxes follow the numpy specification of tests/test_bvh_binned.py over the new
primitive boxes, and the oracle walking it renders what a linear scan of the moved scene renders;
the SAH cost equals a numpy restatement of its definition. Nothing compares with a tolerance."""
import ctypes
import os
import re

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned, decode_bvh2, refit_bvh_binned

import books64_book2_scenes as B
import device_bvh_scenes as D
from test_bvh_binned import f16_outward, f32_outward, prim_boxes, walk
from test_gpu_scene_update import jittered, with_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt_hip.h")
NODE_COST = 2.0

PROTOTYPES = (
    "int32_t rrt_scene_refit_spheres(RrtScene *scene, const RrtSphere *spheres, uint32_t n_spheres, "
    "const float *motion, void *stream);",
    "int32_t rrt_scene_tree_cost(RrtScene *scene, RrtTreeCost *out);",
    "int32_t rrt_refit_bvh_binned(const RrtSphere *built_spheres, uint32_t n_spheres, const RrtSceneExt *built_ext, "
    "uint32_t max_leaf, double node_cost, uint32_t node_stride, const RrtSphere *new_spheres, const float *new_motion, "
    "void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out, RrtBvhInfo *info, double *sah_out);",
    "int32_t rrt_testing_scene_refit_stats(const RrtScene *scene, RrtSceneRefitStats *out);",
    "int32_t rrt_testing_refit_form(int32_t form);",
)

_scenes = {}


def scene(name):
    if name == "mixed":
        if name not in _scenes:
            _scenes[name] = B.mixed_scene(rrt.next_week_scene(1, D.KW))
        return _scenes[name]
    return D.scene(name)


# ---- 1. exports and the null scene ---------------------------------------------------------------
def test_entry_points_are_exported_with_the_headers_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    lib = _lib.load()
    for proto in PROTOTYPES:
        assert proto in flat, proto
        name = re.search(r"(rrt_\w+)\(", proto).group(1)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "typedef struct RrtTreeCost { double sah; double sah_at_build; uint64_t refits_since_build; } RrtTreeCost;" in flat
    assert ctypes.sizeof(_lib.RrtTreeCost) == 24 and ctypes.sizeof(_lib.RrtSceneRefitStats) == 32
    assert lib.rrt_hip_abi_version() == 11


def test_null_scene_is_refused_without_a_device():
    lib = _lib.load()
    sp = np.zeros(2, _lib.SPHERE_DTYPE)
    cost, st = _lib.RrtTreeCost(), _lib.RrtSceneRefitStats()
    calls = {
        "rrt_scene_refit_spheres": lambda: lib.rrt_scene_refit_spheres(None, _lib.ptr(sp), 2, None, None),
        "rrt_scene_tree_cost": lambda: lib.rrt_scene_tree_cost(None, ctypes.byref(cost)),
        "rrt_testing_scene_refit_stats": lambda: lib.rrt_testing_scene_refit_stats(None, ctypes.byref(st)),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = lib.rrt_hip_last_error().decode()
        assert name in msg and "null scene" in msg, msg


def test_refit_form_takes_minus_one_zero_and_one():
    for form in (0, 1, -1):
        _lib.refit_form(form)
    with pytest.raises(rrt.RrtError):
        _lib.refit_form(2)
    _lib.refit_form(-1)


def test_bad_arguments_are_refused_like_the_builders():
    sc = D.scene("C2")
    for ml, st in ((0, 80), (8, 80), (3, 64)):
        with pytest.raises(rrt.RrtError):
            refit_bvh_binned(sc, sc.spheres, None, ml, NODE_COST, st)


# ---- 2. identity ---------------------------------------------------------------------------------
IDENTITY = ["spheres2", "spheres3", "spheres4", "spheres5", "spheres64", "spheres65", "spheres1025", "C2", "C5", "NW1",
            "coincident40", "concentric40", "big_among_small", "mixed"]


@pytest.mark.parametrize("max_leaf,stride", D.SHAPES)
@pytest.mark.parametrize("name", IDENTITY)
def test_refit_over_unchanged_spheres_is_the_built_tree(name, max_leaf, stride):
    sc = scene(name)
    built = build_bvh_binned(sc, max_leaf, NODE_COST, stride)
    nodes, order, info, sah = refit_bvh_binned(sc, sc.spheres, sc.motion, max_leaf, NODE_COST, stride)
    assert info == built[2]
    assert np.array_equal(order, built[1])
    assert nodes.tobytes() == built[0].tobytes()
    assert np.isfinite(sah) and sah > 0.0


# ---- 3. stored boxes after a move ----------------------------------------------------------------
MOVED = [("spheres5", 3, 80), ("spheres65", 3, 80), ("C2", 3, 80), ("C5", 1, 32), ("NW1", 3, 80), ("mixed", 3, 80)]
JITTERS = [(11, 0.05), (12, 0.4)]


def child_unions(tree, sc):
    """Per node and child the f64 union of its primitives' boxes, bottom-up as the refit forms it
    (test_bvh_binned.py::test_stored_boxes' specification); also the walk."""
    nodes, order, info = tree[:3]
    n_tree = D.n_prims(sc) - info["n_unbounded"]
    rng, depth, bfs, (lo, hi, first, cnt) = walk((nodes, order, info), n_tree)
    plo, phi = prim_boxes(sc)
    plo, phi = plo[order], phi[order]  # leaf order
    n = info["n_nodes"]
    ulo, uhi = np.zeros((n, 2, 3)), np.zeros((n, 2, 3))
    for k in range(n - 1, -1, -1):  # children carry larger numbers than their parents
        for c in range(2):
            a, b = rng[k, c]
            if cnt[k, c] > 0:
                ulo[k, c], uhi[k, c] = plo[a:b].min(axis=0), phi[a:b].max(axis=0)
            elif a < b:
                ch = int(first[k, c])
                ulo[k, c], uhi[k, c] = ulo[ch].min(axis=0), uhi[ch].max(axis=0)
    real = rng[:, :, 1] > rng[:, :, 0]  # not the never-hit slot of a root leaf
    root = (plo[:n_tree].min(axis=0), phi[:n_tree].max(axis=0))
    return ulo, uhi, real, root, (lo, hi, first, cnt)


@pytest.mark.parametrize("seed,scale", JITTERS)
@pytest.mark.parametrize("name,max_leaf,stride", MOVED)
def test_stored_boxes_after_a_move(name, max_leaf, stride, seed, scale):
    sc = scene(name)
    built = build_bvh_binned(sc, max_leaf, NODE_COST, stride)
    moved = with_spheres(sc, jittered(sc, seed, scale), sc.motion)
    tree = refit_bvh_binned(sc, moved.spheres, moved.motion, max_leaf, NODE_COST, stride)
    nodes, order, info, _ = tree
    assert info == built[2] and np.array_equal(order, built[1])
    b_first, b_cnt = decode_bvh2(built[0], stride)[2:]
    ulo, uhi, real, (root_lo, root_hi), (lo, hi, first, cnt) = child_unions(tree, moved)
    assert np.array_equal(first, b_first) and np.array_equal(cnt, b_cnt), "the refit changed a link"
    assert nodes.tobytes() != built[0].tobytes(), "the move did not change a box"
    o = np.maximum(np.abs(root_lo), np.abs(root_hi))
    grow = lambda p: 4.0 * 2.0 ** -24 * (2.0 * np.abs(p) + 3.0 * o)
    want_lo, want_hi = f32_outward(ulo - grow(ulo), uhi + grow(uhi))
    if stride == 32:
        want_lo, want_hi = f16_outward(want_lo, False), f16_outward(want_hi, True)
    assert np.array_equal(lo[real], want_lo[real]) and np.array_equal(hi[real], want_hi[real])
    # hence every stored box contains its primitives' new boxes
    assert (lo[real].astype(np.float64) <= ulo[real]).all() and (hi[real].astype(np.float64) >= uhi[real]).all()


# ---- 4. the refit tree renders the moved scene ---------------------------------------------------
@pytest.mark.parametrize("seed,scale", JITTERS)
@pytest.mark.parametrize("name,max_leaf,stride", [("C2", 3, 80), ("C5", 1, 32), ("NW1", 3, 80)])
def test_walking_the_refit_tree_renders_the_linear_scan(name, max_leaf, stride, seed, scale):
    sc = scene(name)
    moved = with_spheres(sc, jittered(sc, seed, scale), sc.motion)
    nodes, order, info, _ = refit_bvh_binned(sc, moved.spheres, moved.motion, max_leaf, NODE_COST, stride)
    kacc, krays, _ = oracle.render_kbvh(moved, nodes, order, info, threads=8)
    tacc, trays, _ = oracle.render(moved, oracle.TWIN, threads=8)
    assert np.array_equal(kacc, tacc)
    assert krays == trays


# ---- 5. cost -------------------------------------------------------------------------------------
def numpy_sah(tree, sc, node_cost):
    """The definition of RrtTreeCost.sah: t_k = w0 A(box0) + w1 A(box1), A = 2 (a c1 + a c2 + c1 c2)
    in that order, w = the leaf's count or node_cost; summed for k = 0 .. n-1 sequentially in f64 and
    divided by the area of the root box (the union of node 0's child boxes)."""
    ulo, uhi, real, _, (lo, hi, first, cnt) = child_unions(tree, sc)

    def area(mn, mx):
        a, c1, c2 = (np.float64(mx[j]) - np.float64(mn[j]) for j in range(3))
        return np.float64(2.0) * (a * c1 + a * c2 + c1 * c2)

    total = np.float64(0.0)
    for k in range(len(ulo)):
        w = [np.float64(cnt[k, c]) if cnt[k, c] > 0 else np.float64(node_cost if real[k, c] else 0.0) for c in range(2)]
        a = [area(ulo[k, c], uhi[k, c]) if real[k, c] else np.float64(0.0) for c in range(2)]
        total = total + (w[0] * a[0] + w[1] * a[1])
    kids = [c for c in range(2) if real[0, c]]
    root_lo = np.min([ulo[0, c] for c in kids], axis=0)
    root_hi = np.max([uhi[0, c] for c in kids], axis=0)
    return float(total / area(root_lo, root_hi))


@pytest.mark.parametrize("name", IDENTITY)
def test_cost_of_the_identity_refit_is_the_definition(name):
    sc = scene(name)
    max_leaf, stride = (1, 32) if name == "C5" else (3, 80)
    tree = refit_bvh_binned(sc, sc.spheres, sc.motion, max_leaf, NODE_COST, stride)
    want = numpy_sah(tree, sc, NODE_COST)
    assert np.float64(tree[3]).tobytes() == np.float64(want).tobytes(), (tree[3], want)


@pytest.mark.parametrize("name,max_leaf,stride", [("C2", 3, 80), ("C5", 1, 32)])
def test_cost_after_a_move_is_the_definition_and_grows_on_c5(name, max_leaf, stride):
    sc = scene(name)
    at_build = refit_bvh_binned(sc, sc.spheres, sc.motion, max_leaf, NODE_COST, stride)[3]
    moved = with_spheres(sc, jittered(sc, 12, 0.4), sc.motion)
    tree = refit_bvh_binned(sc, moved.spheres, moved.motion, max_leaf, NODE_COST, stride)
    assert np.float64(tree[3]).tobytes() == np.float64(numpy_sah(tree, moved, NODE_COST)).tobytes()
    print(f"{name}: sah {tree[3]:.4f} after the 0.4 jitter, {at_build:.4f} at build, ratio {tree[3] / at_build:.4f}")
    if name == "C5":
        assert tree[3] > at_build
