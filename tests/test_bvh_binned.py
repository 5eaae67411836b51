"""The host twin of the device BVH builder (rrt_build_bvh_binned; rustraytrace_amd/csrc/rrt_bvh_binned.h
is the algorithm both sides compile). No GPU: the twin is the specification the device builder is
held to (tests/test_gpu_device_bvh.py), so its trees are checked here for structure, for their stored
boxes against a numpy restatement of the pipeline (union -> slack -> outward f32 -> outward f16), for
being conservative in use (the oracle walking them renders what a linear scan renders) and for
quality against the sweep builder's trees."""
import os
import re

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh, build_bvh_binned, decode_bvh2

import device_bvh_scenes as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, ml, st) for name in D.SCENES for ml, st in D.SHAPES]
IDS = [f"{n}-leaf{ml}-{st}B" for n, ml, st in CASES]

_trees = {}


def twin(name, max_leaf, stride):
    key = (name, max_leaf, stride)
    if key not in _trees:
        _trees[key] = build_bvh_binned(D.scene(name), max_leaf, 2.0, stride)
    return _trees[key]


# ---- the padded f64 primitive boxes (rrt_host.cpp prim_boxes), restated ---------------------------
def _pad(lo, hi):
    small = (hi - lo) < 0.0001
    return np.where(small, lo - 0.0001 / 2.0, lo), np.where(small, hi + 0.0001 / 2.0, hi)


def _quad_boxes(q):
    a, u, v = (q[k][:, :3].astype(np.float64) for k in ("q", "u", "v"))
    corners = np.stack([a, a + u + v, a + u, a + v])
    return _pad(corners.min(axis=0), corners.max(axis=0))


def prim_boxes(sc):
    cr = sc.spheres["center_radius"]
    c, r = cr[:, :3].astype(np.float64), np.maximum(cr[:, 3].astype(np.float64), 0.0)[:, None]
    lo, hi = c - r, c + r
    if sc.motion is not None:
        c2 = (cr[:, :3] + sc.motion[:, :3].astype(np.float32)).astype(np.float64)  # the f32 sum, then widened
        lo, hi = np.minimum(lo, c2 - r), np.maximum(hi, c2 + r)
    los, his = [_pad(lo, hi)[0]], [_pad(lo, hi)[1]]
    if sc.quads is not None:
        qlo, qhi = _quad_boxes(sc.quads)
        los.append(qlo), his.append(qhi)
    if sc.media is not None:
        blo, bhi = _quad_boxes(sc.boundary_quads) if sc.boundary_quads is not None else (None, None)
        for m in sc.media:
            if m["boundary_kind"] == 0:
                mc, mr = m["sphere"][:3].astype(np.float64), max(float(m["sphere"][3]), 0.0)
                mlo, mhi = _pad(mc - mr, mc + mr)
            else:
                f, n = int(m["first"]), int(m["count"])
                mlo, mhi = _pad(blo[f:f + n].min(axis=0), bhi[f:f + n].max(axis=0))
            los.append(mlo[None]), his.append(mhi[None])
    return np.concatenate(los), np.concatenate(his)


def f32_outward(lo, hi):
    def step(d, up):
        f = d.astype(np.float32)
        wrong = (f.astype(np.float64) < d) if up else (f.astype(np.float64) > d)
        return np.where(wrong, np.nextafter(f, np.float32(np.inf if up else -np.inf)), f)

    return step(lo, False), step(hi, True)


def f16_outward(x, up):
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    wrong = (h.astype(np.float32) < x) if up else (h.astype(np.float32) > x)
    h = np.where(wrong, np.nextafter(h, np.float16(np.inf if up else -np.inf)), h)
    sub = (np.abs(h) > 0) & (np.abs(h) < np.float16(2.0 ** -14))
    tiny = np.float16(2.0 ** -14)
    pushed = np.where(h > 0, tiny if up else np.float16(0.0), np.float16(-0.0) if up else -tiny)
    return np.where(sub, pushed, h).astype(np.float32)


def walk(tree, n_tree):
    """Per node and child: the leaf-order range it covers; checks links on the way. Returns (ranges
    [n, 2, 2], depth per node, breadth-first order of the internal nodes)."""
    nodes, order, info = tree
    lo, hi, first, cnt = decode_bvh2(nodes, info["node_stride"])
    n = info["n_nodes"]
    rng = np.zeros((n, 2, 2), np.int64)
    depth = np.zeros(n, np.int64)
    bfs = [0]
    for k in bfs:  # grows while iterating: breadth-first, left to right
        for c in range(2):
            if cnt[k, c] == 0 and not (n == 1 and c == 1):
                child = int(first[k, c])
                assert 0 < child < n
                depth[child] = depth[k] + 1
                bfs.append(child)
    assert len(bfs) == n and len(set(bfs)) == n
    for k in reversed(bfs):
        for c in range(2):
            if cnt[k, c] > 0:
                rng[k, c] = (first[k, c], first[k, c] + cnt[k, c])
            elif n == 1 and c == 1:
                rng[k, c] = (n_tree, n_tree) if cnt[k, 0] else (0, 0)  # the never-hit slot
            else:
                ch = int(first[k, c])
                assert rng[ch, 0, 1] == rng[ch, 1, 0]
                rng[k, c] = (rng[ch, 0, 0], rng[ch, 1, 1])
    return rng, depth, bfs, (lo, hi, first, cnt)


@pytest.mark.parametrize("name,max_leaf,stride", CASES, ids=IDS)
def test_structure(name, max_leaf, stride):
    sc = D.scene(name)
    tree = twin(name, max_leaf, stride)
    nodes, order, info = tree
    n_all = D.n_prims(sc)
    n_tree = n_all - info["n_unbounded"]
    assert info["node_stride"] == stride and info["max_leaf_param"] == max_leaf and info["width"] == 2
    assert nodes.size == info["node_bytes"] == info["n_nodes"] * stride
    assert sorted(order.tolist()) == list(range(n_all)), "prim_order is not a permutation"
    rng, depth, bfs, (lo, hi, first, cnt) = walk(tree, n_tree)
    # child ranges partition the parent's and are adjacent; the root covers the tree
    assert np.array_equal(rng[:, 0, 1], rng[:, 1, 0])
    assert rng[0, 0, 0] == 0 and rng[0, 1, 1] == n_tree
    both_leaves = (cnt[:, 0] > 0) & (cnt[:, 1] > 0)
    assert np.array_equal(first[both_leaves, 1], first[both_leaves, 0] + cnt[both_leaves, 0])
    assert cnt.max() <= max_leaf or (info["n_nodes"] == 1 and cnt[0, 0] <= max_leaf)
    assert bfs == list(range(info["n_nodes"])), "numbering is not breadth-first"
    # info matches the walk
    leaves = int((cnt > 0).sum())
    assert info["n_leaves"] == leaves and info["max_leaf_size"] == int(cnt.max())
    assert info["max_depth"] == int(depth.max()) + 1
    assert int(cnt.sum()) == n_tree
    if name == "coincident40":
        assert info["max_depth"] <= 8
    again = build_bvh_binned(sc, max_leaf, 2.0, stride)
    assert np.array_equal(again[0], nodes) and np.array_equal(again[1], order) and again[2] == info


@pytest.mark.parametrize("name,max_leaf,stride", CASES, ids=IDS)
def test_stored_boxes(name, max_leaf, stride):
    sc = D.scene(name)
    tree = twin(name, max_leaf, stride)
    nodes, order, info = tree
    n_tree = D.n_prims(sc) - info["n_unbounded"]
    rng, depth, bfs, (lo, hi, first, cnt) = walk(tree, n_tree)
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
    root_lo, root_hi = plo[:n_tree].min(axis=0), phi[:n_tree].max(axis=0)
    o = np.maximum(np.abs(root_lo), np.abs(root_hi))
    grow = lambda p: 4.0 * 2.0 ** -24 * (2.0 * np.abs(p) + 3.0 * o)
    want_lo, want_hi = f32_outward(ulo - grow(ulo), uhi + grow(uhi))
    if stride == 32:
        want_lo, want_hi = f16_outward(want_lo, False), f16_outward(want_hi, True)
    assert np.array_equal(lo[real], want_lo[real]) and np.array_equal(hi[real], want_hi[real])
    # hence every stored box contains its primitives' boxes
    assert (lo[real].astype(np.float64) <= ulo[real]).all() and (hi[real].astype(np.float64) >= uhi[real]).all()


_twin_render = {}


def twin_render(name):
    if name not in _twin_render:
        _twin_render[name] = oracle.render(D.scene(name), oracle.TWIN, threads=8)
    return _twin_render[name]


@pytest.mark.parametrize("max_leaf,stride", D.SHAPES)
@pytest.mark.parametrize("name", ["C2", "C5", "NW1"])
def test_walking_the_twin_tree_renders_the_linear_scan(name, max_leaf, stride):
    sc = D.scene(name)
    nodes, order, info = twin(name, max_leaf, stride)
    kacc, _, _ = oracle.render_kbvh(sc, nodes, order, info, threads=8)
    assert np.array_equal(kacc, twin_render(name)[0])


@pytest.mark.parametrize("max_leaf,stride", D.SHAPES)
@pytest.mark.parametrize("name", ["NW7", "NW9"])
def test_walking_the_twin_tree_renders_the_sweep_trees_pixels(name, max_leaf, stride):
    """Pixels only: exact ties make ray counts depend on the tree in these scenes."""
    sc = D.scene(name)
    nodes, order, info = twin(name, max_leaf, stride)
    kacc, _, _ = oracle.render_kbvh(sc, nodes, order, info, threads=8)
    s_nodes, s_order, s_info = build_bvh(sc)
    sacc, _, _ = oracle.render_kbvh(sc, s_nodes, s_order, s_info, threads=8)
    assert np.array_equal(kacc, sacc)


# Primitive tests per ray of the oracle's walk, twin tree / sweep tree in the shape scene creation
# keeps for the sweep tree, at 64x36x8: measured ratios plus 0.02, a regression guard.
QUALITY = {"C2": 0.8107 + 0.02, "C5": 1.0268 + 0.02, "NW9": 0.9940 + 0.02}


@pytest.mark.parametrize("name", sorted(QUALITY))
def test_quality_against_the_sweep_tree(name):
    kw = dict(image_width=64, samples_per_pixel=8)
    sc = rrt.config_scene(name, **kw) if name.startswith("C") else rrt.next_week_scene(9, kw)
    s_nodes, s_order, s_info = build_bvh(sc)
    shape = (3, 80) if s_info["node_stride"] == 80 else (1, 32)
    nodes, order, info = build_bvh_binned(sc, shape[0], 2.0, shape[1])
    _, rays, tests = oracle.render_kbvh(sc, nodes, order, info, threads=8)
    _, s_rays, s_tests = oracle.render_kbvh(sc, s_nodes, s_order, s_info, threads=8)
    ratio = (tests / rays) / (s_tests / s_rays)
    print(f"{name}: primitive tests per ray {tests / rays:.4f} (binned) vs {s_tests / s_rays:.4f} (sweep), ratio {ratio:.4f}")
    assert ratio <= QUALITY[name]


def test_abi_flag_and_exports():
    header = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert re.search(r"#define\s+RRT_FLAG_DEVICE_BVH\s+0x10u\b", header)
    assert _lib.FLAG_DEVICE_BVH == 0x10
    lib = _lib.load()
    for name in ("rrt_build_bvh_binned", "rrt_scene_read_bvh"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.rrt_hip_abi_version() == 11


def test_bad_arguments_are_refused():
    sc = D.scene("C2")
    for ml, st in ((0, 80), (8, 80), (3, 64)):
        with pytest.raises(rrt.RrtError):
            build_bvh_binned(sc, ml, 2.0, st)
