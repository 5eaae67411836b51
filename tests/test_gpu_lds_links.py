"""GPU: the f32 node step on staged scenes whose inner links, t.node and stack entries are LDS byte
offsets (rrt_internal.h lds_node_link), with the stack behind the staged scene, and the leaf decode
by mask logic — bit for bit against the oracle on tiny frames (48 x 27 x 2 spp or smaller).

Each case compares the f32 frame with the oracle's TWIN mode (its own tree) and its walk of the
kernel's tree (KBVH), the ray count with both, the counting kernel's sphere tests with KBVH's (every
primitive of a visited leaf range is one test, so a wrong count field in a postponed range shows),
box tests = 2 x node visits, and the node visits with NODE_VISITS: the counts of the kernel before
the links became offsets, recorded on one MI355X from the same scenes (the oracle reports no node
count). The cases:

  tiny        1, 2 and 3 spheres at one primitive per leaf: the root's links are leaves (or the
              never-hit child's 0), or one inner link; offset 0 is the root
  rtow        the RTOW generator at the largest grid_half the 40 KB budget stages (11; 12 is read from
              global memory), and a field at one primitive per leaf: 318 nodes, offsets up to 25,360
  ladder      tests/deep_scenes.py's ladder in the LDS class (26 live stack entries behind the scene),
              and its cluster whose block passes 64 KiB with the limit raised: stack addresses beyond
              16 bits, node offsets still small; the ladder on the f64 kernel too (its leaf decode)
  twin7       two sibling leaves of 7 primitives each, overlapping so that rays hit both boxes: the
              postponed range is first0 | 14 << 28, the 4-bit field's largest value
  classes     a diffuse-only scene (C4's class) and a staged book-2 scene
"""
import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S
from rustraytrace_amd.render import build_bvh, decode_bvh2

import deep_scenes as D
from test_gpu_books64 import _check, _gpu_f64
from test_gpu_parity import _book1_scene, assert_bit_exact, gpu_tile
from test_launch_plan import KIB64, scene_query

pytestmark = pytest.mark.gpu

# node visits of the parent kernel (index links, stack first), one MI355X
NODE_VISITS = {
    "tiny1": 2731, "tiny2": 2890, "tiny3": 3827, "rtow11": 61005, "field316": 103761, "ladder": 336653,
    "cluster64": 121229, "twin7": 6098, "diffuse": 9468, "book2": 51471,
}


def _mats():
    return np.concatenate([S._material(0, (0.5, 0.5, 0.5)), S._material(1, (0.7, 0.6, 0.5), fuzz=0.1)])


def tiny(n):
    """n unit-spaced spheres (Lambertian, metal, Lambertian) under the sky: C2's kernel class."""
    sph = np.concatenate([S._sphere((-1.1 + 1.1 * i, 0.0, 0.0), 0.5, i % 2) for i in range(n)])
    cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=48, samples_per_pixel=2, max_depth=8, vfov=40.0,
                        lookfrom=(0.0, 0.5, 4.0), lookat=(0.0, 0.0, 0.0), seed=7, n_spheres=n)
    return S.SceneData(cam, sph, _mats(), name=f"tiny{n}")


def twin7():
    """A ground sphere and two groups of 7 overlapping metal spheres (r = 1, centres within 0.05 of
    (-0.6, 1, 0) and (0.6, 1, 0)): at 7 primitives per leaf the groups are sibling leaves."""
    rng = np.random.default_rng(2)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0)]
    for g in range(2):
        for _ in range(7):
            sph.append(S._sphere(np.array([-0.6 + 1.2 * g, 1.0, 0.0]) + rng.uniform(-0.05, 0.05, 3), 1.0, 1))
    sph = np.concatenate(sph)
    cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=48, samples_per_pixel=2, max_depth=8, vfov=30.0,
                        lookfrom=(6.0, 2.5, 8.0), lookat=(0.0, 0.5, 0.0), seed=7, n_spheres=len(sph))
    return S.SceneData(cam, sph, _mats(), name="twin7")


def _compare(key, scene, nodes, order, info, twin_rays=True):
    """Frame, rays and work counts of one staged scene against the oracle and the parent's node visits."""
    assert info["node_stride"] == 80, "the scene must be staged in LDS (80-B nodes)"
    gpu, idx, ctr, work = gpu_tile(scene, count=True)
    assert len(idx) == scene.height and np.all(gpu[..., 3] == scene.spp)
    kref, krays, ktests = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    assert_bit_exact(gpu, kref, scene.spp)
    tref, trays, _ = oracle.render(scene, oracle.TWIN, threads=16)
    assert_bit_exact(gpu, tref, scene.spp)
    print(f"{key}: rays {ctr['rays']} (KBVH {krays}, TWIN {trays}), work {work}, KBVH sphere tests {ktests}")
    assert ctr["rays"] == krays == work["rays"]
    if twin_rays:
        assert trays == krays
    assert work["sphere_tests"] == ktests
    assert work["box_tests"] == 2 * work["node_visits"]
    assert work["node_visits"] == NODE_VISITS[key]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_trees(monkeypatch, n):
    monkeypatch.setenv("RRT_MAX_LEAF", "1")
    scene = tiny(n)
    nodes, order, info = build_bvh(scene)
    _, _, first, count = decode_bvh2(nodes, 80)
    assert info["n_nodes"] == (2 if n == 3 else 1)
    inner = [(i, c) for i in range(len(count)) for c in range(2) if count[i, c] == 0 and first[i, c] != 0]
    assert inner == ([(0, 1)] if n == 3 else [])  # 3 spheres: the root's second link is the only inner one
    assert int(count.sum()) == n  # one primitive per leaf
    _compare(f"tiny{n}", scene, nodes, order, info)


def test_rtow_at_the_largest_staged_grid():
    """grid_half 11 (486 spheres, 40,608 B of nodes and primitives) is staged; 12 no longer fits 40 KB."""
    scene = rrt.rtow(image_width=48, samples_per_pixel=2, max_depth=8, grid_half=11)
    nodes, order, info = build_bvh(scene)
    assert info["node_bytes"] + 48 * len(order) <= 40 * 1024
    _, _, info12 = build_bvh(rrt.rtow(image_width=48, samples_per_pixel=2, max_depth=8, grid_half=12))
    assert info12["node_stride"] == 32
    _compare("rtow11", scene, nodes, order, info)


def test_highest_node_offsets(monkeypatch):
    """One primitive per leaf: 319 primitives in 318 nodes, 40,752 B of the 40,960 B budget, the last
    node at offset 25,360 (three more field spheres and the scene is read from global memory)."""
    monkeypatch.setenv("RRT_MAX_LEAF", "1")
    scene = D.cluster(2, 316, 1)
    nodes, order, info = build_bvh(scene)
    assert info["n_nodes"] == 318 and (info["n_nodes"] - 1) * 80 == 25360
    _, _, info3 = build_bvh(D.cluster(2, 319, 1))
    assert info3["node_stride"] == 32
    _compare("field316", scene, nodes, order, info)


def test_ladder_stack_behind_the_scene(monkeypatch):
    """The ladder in C2's class (512 x 6 after the fallback): 26 live entries of a stack that starts
    behind the staged scene."""
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    scene, nodes, order, info = D.built(None, "ladder", 1)
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["scene_in_lds"] == 1 and (plan["threads"], plan["waves"]) == (512, 6)
    _compare("ladder", scene, nodes, order, info)


def test_stack_addresses_beyond_16_bits(monkeypatch):
    """64 coincident spheres: the block's 74,496 B of LDS need the raised limit, so stack entries sit
    at addresses above 65,535 while they hold node offsets of at most 5,280. The coincident spheres tie, so
    the ray count is compared with the kernel's tree alone (they share a material: equal frames)."""
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    scene, nodes, order, info = D.built(None, "cluster", 64, 10, 1)
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["scene_in_lds"] == 1 and plan["raise_limit"] == 1 and plan["lds_bytes"] > KIB64
    _compare("cluster64", scene, nodes, order, info, twin_rays=False)


def test_ladder_on_the_f64_kernel(monkeypatch):
    """The f64 kernel's leaf decode (the same mask logic) on the ladder, against BOOKS."""
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    scene = D.ladder(1)
    gpu, gpu32, gpu_rays = _gpu_f64(scene)
    books, books_rays, _ = oracle.render(scene, oracle.BOOKS, threads=16)
    assert gpu_rays == books_rays
    _check(scene, gpu, books, "ladder f64")
    assert np.array_equal(gpu32, gpu.astype(np.float32))


def test_two_sibling_leaves_of_seven(monkeypatch):
    monkeypatch.setenv("RRT_MAX_LEAF", "7")
    scene = twin7()
    nodes, order, info = build_bvh(scene)
    _, _, first, count = decode_bvh2(nodes, 80)
    both = [i for i in range(len(count)) if count[i, 0] == 7 and count[i, 1] == 7]
    assert len(both) == 1 and first[both[0], 1] == first[both[0], 0] + 7  # one range of 14: first0 | 14 << 28
    _compare("twin7", scene, nodes, order, info)


def test_diffuse_class(monkeypatch):
    monkeypatch.setenv("RRT_SCENE_IN_LDS", "1")
    scene = _book1_scene((0, 4), False)
    nodes, order, info = build_bvh(scene)
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["kernel_class"] == -2 and plan["scene_in_lds"] == 1
    _compare("diffuse", scene, nodes, order, info)


def test_book2_staged_class(monkeypatch):
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    scene, nodes, order, info = D.built(None, "moving_cluster", 4, 60)
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["kernel_class"] == 1 and plan["scene_in_lds"] == 1
    _compare("book2", scene, nodes, order, info, twin_rays=False)
