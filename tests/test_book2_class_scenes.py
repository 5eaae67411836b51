"""Conditions on the scenes of tests/book2_class_scenes.py, on the oracle and the launch plan alone
(no device): what tests/test_gpu_book2_classes.py assumes of them when it renders every book-2/3
instantiation of the f32 kernel.

For every scene and placement the GPU test uses: the launch plan names the intended instantiation
(class, placement of scene and Perlin tables, stack width, LDS limit), the oracle's walk of the host
tree (KBVH) is finite and equals its own tree's frame (TWIN) bit for bit, with equal ray counts where
no coincident cluster is in the scene, the noise material and the media change the frame (so a frame
cannot match without the branch under test), and the trees of classes 2 to 4 mix primitive kinds in
their leaves. A red GPU test is then the kernel's fault, and a green one means the named cell ran.
"""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned, decode_bvh2

import book2_class_scenes as B
from test_launch_plan import KIB64, check_f32_plan, scene_query

PLACEMENTS = [None, "0"]  # RRT_SCENE_IN_LDS: unset (staged when it fits), "0" (read from global memory)
PLACEMENT_IDS = ["lds", "global"]
DEEP = (False, 250, 60)  # composite(cls, *DEEP): 250 field spheres and a chain of 60 coincident ones


def place(monkeypatch, in_lds, perlin_in_lds=None):
    """Set the two placement overrides scene creation reads (None: unset)."""
    for name, value in (("RRT_SCENE_IN_LDS", in_lds), ("RRT_PERLIN_IN_LDS", perlin_in_lds)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def plan_of(scene, info, order):
    """(query, plan) of a built scene, under the overrides the caller has set."""
    q = scene_query(scene, info, len(order))
    return q, _lib.launch_plan(**q)


def check_cell(scene, info, order, cls, noise, in_lds, perlin_in_lds=None, min_depth=7):
    """A composite of 60 field spheres lands in the cell (class, noise, placement) it is named for:
    16-bit stack, default LDS limit, a tree of 30 to 80 nodes, at least min_depth deep (the sweep
    builder's trees; the device builder's binned trees are flatter). perlin_in_lds "0": the tables
    stay in global memory although they would fit."""
    q, plan = plan_of(scene, info, order)
    if perlin_in_lds is None:
        check_f32_plan(q, plan)  # the layout formula restated in tests/test_launch_plan.py
    assert plan["ok"] == 1 and plan["kernel_class"] == cls
    assert plan["scene_in_lds"] == (1 if in_lds is None else 0)
    assert info["node_stride"] == (80 if in_lds is None else 32)
    assert q["n_perlin"] == (1 if noise else 0)
    assert plan["perlin_in_lds"] == (1 if noise and perlin_in_lds is None else 0)
    assert (plan["stack_bytes"], plan["threads"], plan["raise_limit"]) == (2, 256, 0)
    assert 30 <= info["n_nodes"] <= 80 and len(order) >= 62 and info["max_depth"] >= min_depth
    return plan


def check_deep(scene, info, order, cls, in_lds):
    """composite(cls, *DEEP): a stack of more than 60 entries. Staged, the 256-thread block passes
    64 KiB and the launch raises the limit; read from global memory it is about 32 KiB of stack."""
    q, plan = plan_of(scene, info, order)
    check_f32_plan(q, plan)
    assert plan["ok"] == 1 and plan["kernel_class"] == cls and (plan["stack_bytes"], plan["threads"]) == (2, 256)
    assert q["stack_depth"] > 60 and plan["scene_in_lds"] == (1 if in_lds is None else 0)
    if in_lds is None:
        assert plan["raise_limit"] == 1 and plan["lds_bytes"] > KIB64
        assert plan["lds_bytes"] < KIB64 + 6 * 1024  # some 40 more primitives still stage: a margin
    else:
        assert plan["raise_limit"] == 0 and info["node_stride"] == 32
        assert plan["lds_bytes"] == q["stack_depth"] * 256 * 2 > 30 * 1024
    return plan


def check_wide(scene, info, order, cls):
    """moving_wide(cls): more than 65,535 nodes, 4-byte stack entries in 512-thread blocks."""
    q, plan = plan_of(scene, info, order)
    check_f32_plan(q, plan)
    assert info["n_nodes"] > 65535 and plan["ok"] == 1 and plan["kernel_class"] == cls
    assert (plan["stack_bytes"], plan["threads"], plan["scene_in_lds"], plan["raise_limit"]) == (4, 512, 0, 0)
    return plan


@functools.lru_cache(maxsize=None)
def kbvh(in_lds, name, *args):
    """(frame, rays) of the oracle's walk of the host tree of B.built(in_lds, name, *args); read-only."""
    scene, nodes, order, info = B.built(in_lds, name, *args)
    frame, rays, _ = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    frame.setflags(write=False)
    return frame, rays


@functools.lru_cache(maxsize=None)
def twin(name, *args):
    """(frame, rays) of the oracle's own books-structured tree; read-only."""
    frame, rays, _ = oracle.render(getattr(B, name)(*args), oracle.TWIN, threads=16)
    frame.setflags(write=False)
    return frame, rays


def assert_oracles_agree(in_lds, name, *args, rays=True):
    k, krays = kbvh(in_lds, name, *args)
    t, trays = twin(name, *args)
    assert np.isfinite(k).all()
    assert np.array_equal(k, t), f"{int((k != t).any(-1).sum())} pixels differ between KBVH and TWIN"
    if rays:
        assert krays == trays


# ---- the 16 cells, and the same with the Perlin tables left in global memory ----------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("cls", B.CLASSES)
def test_composite_cells(monkeypatch, cls, noise, in_lds):
    place(monkeypatch, in_lds)
    scene, nodes, order, info = B.built(in_lds, "composite", cls, noise)
    assert scene.width <= 48 and scene.height <= 36 and scene.spp == 4
    plan = check_cell(scene, info, order, cls, noise, in_lds)
    print(f"{scene.name} in_lds={in_lds}: {len(order)} primitives, {info['n_nodes']} nodes, depth {info['max_depth']}, "
          f"{plan['lds_bytes']} B of LDS")
    assert_oracles_agree(in_lds, "composite", cls, noise)
    if noise:  # RRT_PERLIN_IN_LDS=0: the same tree, the tables outside LDS
        place(monkeypatch, in_lds, "0")
        off = check_cell(scene, info, order, cls, noise, in_lds, "0")
        assert off["lds_bytes"] == plan["lds_bytes"] - 5120


@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("cls", B.CLASSES)
def test_device_builder_cells(monkeypatch, cls, in_lds):
    """The trees RRT_FLAG_DEVICE_BVH keeps for the noise composites, by the device builder's host twin
    (tests/test_gpu_device_bvh.py holds the builder to it): the same cells, and a walk TWIN agrees with."""
    place(monkeypatch, in_lds)
    scene = B.composite(cls, True)
    nodes, order, info = build_bvh_binned(scene, *((3, 2.0, 80) if in_lds is None else (1, 2.0, 32)))
    check_cell(scene, info, order, cls, True, in_lds, min_depth=0)
    k, krays, _ = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    t, trays = twin("composite", cls, True)
    assert np.array_equal(k, t) and krays == trays


def test_a_misnamed_cell_is_caught(monkeypatch):
    """check_cell fails on a scene of another cell: another placement, class, or noise build."""
    place(monkeypatch, "0")
    scene, _, order, info = B.built("0", "composite", 2, True)
    for wrong in ((2, True, None), (3, True, "0"), (2, False, "0")):
        with pytest.raises(AssertionError):
            check_cell(scene, info, order, *wrong)
    with pytest.raises(AssertionError):  # the tables are staged unless the override says otherwise
        check_cell(scene, info, order, 2, True, "0", "0")
    check_cell(scene, info, order, 2, True, "0")


# ---- deep stacks, the 32-bit stack ----------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("cls", [2, 3, 4])
def test_deep_composites(monkeypatch, cls, in_lds):
    place(monkeypatch, in_lds)
    scene, nodes, order, info = B.built(in_lds, "composite", cls, *DEEP)
    plan = check_deep(scene, info, order, cls, in_lds)
    print(f"{scene.name} in_lds={in_lds}: {info['n_nodes']} nodes, depth {info['max_depth']}, {plan['lds_bytes']} B")
    # the coincident spheres tie, and the two trees test them in different orders: pixels only
    assert_oracles_agree(in_lds, "composite", cls, *DEEP, rays=False)


@pytest.mark.parametrize("cls", [1, 2, 3])
def test_moving_wide(monkeypatch, cls):
    """KBVH only (tests/test_gpu_launch_shapes.py test_32_bit_stack_kernel: TWIN meets a tie between
    tiny spheres). The quad and the medium are seen: the frames of classes 2 and 3 differ from class 1's."""
    place(monkeypatch, None)
    scene, nodes, order, info = B.built(None, "moving_wide", cls)
    assert (scene.width, scene.height, scene.spp) == (16, 9, 2)
    check_wide(scene, info, order, cls)
    frame, rays = kbvh(None, "moving_wide", cls)
    assert np.isfinite(frame).all() and rays > 0
    still = B.D.built(None, "wide")  # the book-1 scene it was made from
    base, _, _ = oracle.render_kbvh(*still, threads=16)
    assert not np.array_equal(frame, base)
    if cls > 1:
        assert not np.array_equal(frame, kbvh(None, "moving_wide", 1)[0])


# ---- the branches under test are reached ----------------------------------------------------------
@pytest.mark.parametrize("cls", B.CLASSES)
def test_noise_material_is_seen(cls):
    """The same geometry with a plain Lambertian in the noise material's place gives another frame."""
    noisy, _ = twin("composite", cls, True)
    plain, _ = twin("composite", cls, True, 60, 0, True)
    n = int((noisy != plain).any(-1).sum())
    print(f"class {cls}: the noise material shows in {n} pixels")
    assert n >= 4


def test_media_are_seen():
    for noise in (False, True):
        scene = B.composite(3, noise)
        assert len(scene.media) == 2
        bare, _, _ = oracle.render(B.without_media(scene), oracle.TWIN, threads=16)
        assert int((twin("composite", 3, noise)[0] != bare).any(-1).sum()) > 100


def test_moving_spheres_are_seen():
    """Every class's composite has moving field spheres, and stopping them changes the frame."""
    for cls in B.CLASSES:
        scene = B.composite(cls, False)
        assert np.count_nonzero(scene.motion[:, 1]) == 15
        still = dataclasses.replace(scene, motion=np.zeros_like(scene.motion))
        frame, _, _ = oracle.render(still, oracle.TWIN, threads=16)
        assert not np.array_equal(frame, twin("composite", cls, False)[0])


@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("cls", [2, 3, 4])
def test_leaves_mix_primitive_kinds(monkeypatch, cls, in_lds):
    """Some leaf holds more than one primitive kind (sphere, quad, medium), or two sibling leaves hold
    different kinds: the leaf loop changes kind within a batch."""
    place(monkeypatch, in_lds)
    scene, nodes, order, info = B.built(in_lds, "composite", cls, True)
    ns, nq = len(scene.spheres), len(scene.quads)
    kind = np.where(order < ns, 0, np.where(order < ns + nq, 1, 2))
    assert set(kind) == ({0, 1, 2} if cls == 3 else {0, 1})
    _, _, first, count = decode_bvh2(nodes, info["node_stride"])
    mixed = 0
    for f, c in zip(first, count):
        kinds = [set(kind[f[k]:f[k] + c[k]]) for k in (0, 1) if c[k]]
        mixed += any(len(s) > 1 for s in kinds) or (len(kinds) == 2 and kinds[0] != kinds[1])
    assert mixed >= 1
