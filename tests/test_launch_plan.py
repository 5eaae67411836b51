"""The render launch's shape (rrt_internal.h LaunchPlan, through the test-only export
rrt_testing_launch_plan) on the host: no device needed.

A block's dynamic LDS is its traversal stack (stack_depth x threads x 2 or 4 B) plus whatever is
staged beside it (nodes, primitives, Perlin tables). rrt_scene_create accepts any tree whose walk
needs at most 64 stack entries and stages any scene of up to 40 KB, so a deep tree in a 1024- or
512-thread block asks for more than the 64 KiB a launch may declare by default, and at 1024 threads
for more than the 160 KiB a gfx950 block can have at all. The launch used to pick its block without
looking at that size (`tuned_shape` below restates that choice). The plan keeps the tuned shape
whenever it fits 64 KiB (the pinned table: no benchmarked config moves), else falls back to a smaller
instantiated block of the class, else raises the kernel's dynamic-LDS limit, never past 160 KiB.

The layout formula is restated here in Python (`layout_bytes`), independently of the library.
"""
import itertools

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh

import deep_scenes as D

KIB64 = 64 * 1024
BLOCK_MAX = 160 * 1024  # 163,840 B: the LDS of a gfx950 CU, all of which one block may declare
MAX_STACK = 64          # rrt_internal.h kMaxStackDepth
PERLIN_BYTES = 256 * 16 + 256 * 4  # GPerlin: 256 float4 vectors + 256 packed permutation words


def ceil16(n):
    return (n + 15) // 16 * 16


def scene_query(scene, info, n_prims, f64=False):
    """The RrtLaunchPlanQuery of a scene built with build_bvh."""
    k = scene.materials["kind"]
    book2 = (scene.motion is not None or scene.quads is not None or scene.media is not None
             or np.isin(k, (5, 6, 7)).any())
    return dict(n_nodes=info["n_nodes"], n_prims=n_prims, stack_depth=info["max_depth"] + 1,
                node_stride=info["node_stride"], book=3 if scene.flags & _lib.FLAG_BOOK3 else 2 if book2 else 0,
                specular=int(np.isin(k, (1, 2)).any()), image_tex=int((k == 3).any()),
                n_perlin=0 if scene.perlin is None else len(scene.perlin),
                n_media=0 if scene.media is None else len(scene.media),
                n_quads=0 if scene.quads is None else len(scene.quads), f64=int(f64))


def f32_class(q):
    if q["book"] == 3:
        return 4
    if q["book"] == 2:
        return 3 if q.get("n_media") else 2 if q.get("n_quads") else 1
    if not q["specular"] and q["node_stride"] == 80:
        return -2
    return 0 if q["image_tex"] else -1


def staged_bytes(q):
    """Nodes + primitive records (sphere + material, + motion in the book-2/3 classes) of a staged scene."""
    if q["node_stride"] != 80:
        return 0
    return q["n_nodes"] * 80 + q["n_prims"] * (48 + (16 if q["book"] else 0))


def layout_bytes(q, threads, stack_bytes, perlin_in_lds):
    """The f32 kernels' block: the stack rounded up to 16 B, the staged scene, the Perlin tables."""
    return (ceil16(q["stack_depth"] * threads * stack_bytes) + (staged_bytes(q) if stack_bytes == 2 else 0)
            + (q.get("n_perlin", 0) * PERLIN_BYTES if perlin_in_lds else 0))


def tuned_shape(q):
    """(threads, waves, waves of the noise-free kernel, stack bytes): the shape the launch picked
    before it looked at the LDS size (launch_width at the default knobs), which is the tuned shape of
    every benchmarked config."""
    cls, lds = f32_class(q), q["node_stride"] == 80
    if q["n_nodes"] > 65535:
        return 512, 1, 1, 4
    if cls == 4:
        return 256, 5, 5, 2
    if cls > 0:
        return 256, 5, (6 if cls <= 2 else 5), 2
    if lds:
        return {-1: (1024, 8, 8, 2), -2: (256, 8, 8, 2), 0: (512, 6, 6, 2)}[cls]
    return 256, 7, 7, 2


def check_f32_plan(q, plan):
    """The invariants of every f32 plan; returns the tuned shape's bytes."""
    assert plan["ok"] == 1 and plan["f64"] == 0
    assert plan["kernel_class"] == f32_class(q)
    wide_stack = q["n_nodes"] > 65535
    assert plan["stack_bytes"] == (4 if wide_stack else 2)
    assert plan["scene_in_lds"] == (1 if q["node_stride"] == 80 and not wide_stack else 0)
    assert plan["threads"] in (256, 512, 1024)
    assert plan["lds_bytes"] == layout_bytes(q, plan["threads"], plan["stack_bytes"], plan["perlin_in_lds"])
    assert plan["lds_bytes"] <= BLOCK_MAX
    assert plan["raise_limit"] == (1 if plan["lds_bytes"] > KIB64 else 0)
    if plan["perlin_in_lds"]:  # the tables are staged only where they cost no raise
        assert q["n_perlin"] > 0 and q["book"] and plan["lds_bytes"] <= KIB64
    elif q.get("n_perlin") and q["book"]:
        assert layout_bytes(q, plan["threads"], plan["stack_bytes"], True) > KIB64
    t, w, wnf, sb = tuned_shape(q)
    tuned = layout_bytes(q, t, sb, plan["perlin_in_lds"])
    if tuned <= KIB64:  # unchanged shapes
        assert (plan["threads"], plan["waves"], plan["waves_noise_free"], plan["stack_bytes"]) == (t, w, wnf, sb)
        assert plan["lds_bytes"] == tuned and not plan["raise_limit"]
    else:  # a smaller block of the class; the limit is raised only when that does not fit either
        assert plan["threads"] <= t and plan["lds_bytes"] <= tuned
        if plan["raise_limit"]:
            assert plan["threads"] == min(t, 512), "raised although a smaller block exists"
    return tuned


# ---- pinned shapes: the benchmarked configs at their default sizes -----------------------------
# (class, threads, waves, noise-free waves, scene in LDS, Perlin in LDS, LDS bytes); derived from
# launch_width's rules before the plan existed: C2 1024 x 8 at 63,136 B (11 x 1024 x 2 of stack +
# 17,280 of nodes + 486 x 48), C5 256 x 7 from L2, books 2 / 3 256 x 5 (noise-free classes 1-2: x 6).
PINNED = {
    "C1": (-2, 256, 8, 8, 1, 0, 1248),
    "C2": (-1, 1024, 8, 8, 1, 0, 63136),
    "C4": (-2, 256, 8, 8, 1, 0, 1200),
    "C5": (-1, 256, 7, 7, 0, 0, 8704),
    "NW1": (1, 256, 5, 6, 0, 0, 6656),
    "NW2": (1, 256, 5, 6, 1, 0, 1232),
    "NW3": (-2, 256, 8, 8, 1, 0, 1152),
    "NW4": (1, 256, 5, 6, 1, 1, 6352),
    "NW5": (2, 256, 5, 6, 1, 0, 1424),
    "NW6": (2, 256, 5, 6, 1, 1, 6480),
    "NW7": (2, 256, 5, 6, 1, 0, 5536),
    "NW8": (3, 256, 5, 5, 1, 0, 2800),
    "NW9": (3, 256, 5, 5, 0, 1, 13312),
    "NW10": (3, 256, 5, 5, 0, 1, 13312),
    "B3": (4, 256, 5, 5, 1, 0, 4464),
}


@pytest.mark.parametrize("name", list(PINNED))
def test_benchmarked_configs_keep_their_shape(name):
    scene = rrt.named_scene(name)
    _, order, info = build_bvh(scene)
    q = scene_query(scene, info, len(order))
    plan = _lib.launch_plan(**q)
    tuned = check_f32_plan(q, plan)
    got = (plan["kernel_class"], plan["threads"], plan["waves"], plan["waves_noise_free"], plan["scene_in_lds"],
           plan["perlin_in_lds"], plan["lds_bytes"])
    assert got == PINNED[name]
    assert plan["raise_limit"] == 0 and plan["stack_bytes"] == 2 and tuned == plan["lds_bytes"]


# ---- the deep scenes ---------------------------------------------------------------------------
# generator, arguments, and the tuned shape's LDS bytes with the scene staged (over 65,536 in eight
# of the ten; 167,744 is over the 160 KiB a block can have at all)
DEEP = [
    ("ladder", (1,), 79088), ("ladder", (0,), 36080), ("ladder", (1, True), 50416),
    ("cluster", (14, 470, 1), 79712), ("cluster", (40, 10, 1), 87808), ("cluster", (64, 10, 1), 140032),
    ("cluster", (60, 400, 1), 167744), ("cluster", (60, 400, 0), 72512), ("cluster", (40, 400, 1, True), 83888),
    ("moving_cluster", (60, 300), 70448),
]


@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
@pytest.mark.parametrize("gen,args,tuned_lds", DEEP, ids=[f"{g}{a}" for g, a, _ in DEEP])
def test_deep_scene_plans(monkeypatch, gen, args, tuned_lds, in_lds):
    if in_lds is None:
        monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    else:
        monkeypatch.setenv("RRT_SCENE_IN_LDS", in_lds)
    scene, _, order, info = D.built(in_lds, gen, *args)
    assert info["node_stride"] == (80 if in_lds is None else 32)
    q = scene_query(scene, info, len(order))
    plan = _lib.launch_plan(**q)
    tuned = check_f32_plan(q, plan)
    print(f"{gen}{args} in_lds={in_lds}: stack_need {q['stack_depth']} scene {staged_bytes(q)} B, tuned shape "
          f"{tuned_shape(q)[0]} thr {tuned} B -> plan {plan['threads']} x {plan['waves']} {plan['lds_bytes']} B "
          f"raise {plan['raise_limit']}")
    if in_lds is None:
        assert tuned == tuned_lds
    if gen != "moving_cluster":  # book 1: the f64 kernel's plan for the same counts
        q64 = dict(q, f64=1)
        check_f64_plan(q64, _lib.launch_plan(**q64))


def test_over_limit_rows_fall_back_or_raise(monkeypatch):
    """The rows of the table whose tuned shape is over 64 KiB, spelt out: what the plan does instead."""
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    want = {  # (threads, waves, LDS bytes, raise)
        ("ladder", (1,)): (512, 6, 50416, 0),
        ("cluster", (14, 470, 1)): (512, 6, 60256, 0),
        ("cluster", (40, 10, 1)): (512, 6, 46848, 0),
        ("cluster", (64, 10, 1)): (512, 6, 74496, 1),
        ("cluster", (60, 400, 1)): (512, 6, 104256, 1),
        ("cluster", (60, 400, 0)): (256, 8, 72512, 1),
        ("cluster", (40, 400, 1, True)): (512, 6, 83888, 1),
        ("moving_cluster", (60, 300)): (256, 5, 70448, 1),
    }
    for (gen, args), shape in want.items():
        scene, _, order, info = D.built(None, gen, *args)
        plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
        assert (plan["threads"], plan["waves"], plan["lds_bytes"], plan["raise_limit"]) == shape, (gen, args)


@pytest.mark.parametrize("gen", ["wide", "wide_deep"])
def test_wide_scene_plans(monkeypatch, gen):
    """More than 65,535 nodes: the 32-bit stack in 512-thread blocks, 2 KiB per stack entry."""
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    scene, _, order, info = D.built(None, gen)
    q = scene_query(scene, info, len(order))
    assert q["n_nodes"] > 65535 and q["node_stride"] == 32
    plan = _lib.launch_plan(**q)
    check_f32_plan(q, plan)
    assert (plan["threads"], plan["stack_bytes"], plan["scene_in_lds"]) == (512, 4, 0)
    assert plan["lds_bytes"] == q["stack_depth"] * 2048
    if gen == "wide_deep":
        assert q["stack_depth"] >= 33 and plan["raise_limit"] == 1  # the 32-bit stack past 64 KiB
    else:
        assert plan["raise_limit"] == 0
    assert _lib.launch_plan(**dict(q, f64=1))["ok"] == 0  # RRT_FLAG_F64: at most 65,535 nodes


# ---- the f64 kernel's plan ---------------------------------------------------------------------
def f64_min_bytes(q):
    """The staged f64 scene in its smallest form (112-B nodes, f32 sphere records): the host stages an
    f64 scene only when this fits 64 KiB (rrt_books64.hip f64_lds_min_bytes)."""
    return ceil16(q["stack_depth"] * 512 * 2) + q["n_nodes"] * 112 + q["n_prims"] * 16


def check_f64_plan(q, plan):
    staged = q["node_stride"] == 80
    if staged and f64_min_bytes(q) > KIB64:
        assert plan["ok"] == 0  # the host builds the global-memory tree for such a scene instead
        return
    assert plan["ok"] == 1 and plan["f64"] == 1
    assert plan["kernel_class"] == (2 if not q["specular"] else 0 if q["image_tex"] else 1)
    assert (plan["threads"], plan["stack_bytes"], plan["scene_in_lds"]) == (512, 2, int(staged))
    want = ceil16(q["stack_depth"] * 512 * 2)
    if staged:
        wide = plan["shape"] == 2
        assert plan["shape"] in (1, 2) and (wide or not plan["rec32_in_lds"])
        want += q["n_nodes"] * 112 + q["n_prims"] * ((32 if wide else 16) + (8 if plan["inv_r_in_lds"] else 0)
                                                     + (16 if plan["rec32_in_lds"] else 0))
        want += 8 if plan["inv_r_in_lds"] else 0
    else:
        assert plan["shape"] == 0
    assert plan["lds_bytes"] == want <= KIB64 and plan["raise_limit"] == 0


# ---- sweep -------------------------------------------------------------------------------------
# (n_nodes, n_prims) of a staged scene of about 0, 20 and 40 KB, per bytes of a primitive record
SIZES = {48: [(1, 1), (100, 250), (200, 520)], 64: [(1, 1), (100, 190), (200, 390)]}
CLASSES = [  # query fields of each kernel class
    dict(book=0, specular=0, image_tex=0), dict(book=0, specular=0, image_tex=1),  # -2 when staged, else -1 / 0
    dict(book=0, specular=1, image_tex=0), dict(book=0, specular=1, image_tex=1),  # -1, 0
    dict(book=2), dict(book=2, n_quads=3), dict(book=2, n_quads=3, n_media=1), dict(book=3, n_quads=3),
]


def test_sweep_every_accepted_shape_has_a_plan():
    n = raised = 0
    for cls, stride, wide_stack, size, perlin in itertools.product(CLASSES, (80, 32), (False, True), range(3),
                                                                   (0, 1, 2)):
        if wide_stack and stride == 80:
            continue  # more than 65,535 nodes never fit the 40 KB budget
        if perlin and not cls["book"]:
            continue  # noise materials make a scene a book-2 scene
        n_nodes, n_prims = SIZES[64 if cls["book"] else 48][size]
        if wide_stack:
            n_nodes, n_prims = 70000 + n_nodes, 70001 + n_prims
        for depth in range(1, MAX_STACK + 1):
            q = dict(cls, n_nodes=n_nodes, n_prims=n_prims, stack_depth=depth, node_stride=stride, n_perlin=perlin)
            assert staged_bytes(q) <= 40 * 1024
            plan = _lib.launch_plan(**q)
            check_f32_plan(q, plan)
            n += 1
            raised += plan["raise_limit"]
            if not cls["book"] and not wide_stack:
                q64 = dict(q, f64=1)
                check_f64_plan(q64, _lib.launch_plan(**q64))
        # what rrt_scene_create rejects has no plan, and no size either
        for bad in (dict(stack_depth=MAX_STACK + 1), dict(stack_depth=1000), dict(stack_depth=MAX_STACK + 1, f64=1)):
            plan = _lib.launch_plan(**dict(q, **bad))
            assert plan["ok"] == 0 and plan["lds_bytes"] == 0 and plan["threads"] == 0
        if cls["book"] or wide_stack:  # RRT_FLAG_F64: book-1 scenes of at most 65,535 nodes
            plan = _lib.launch_plan(**dict(q, f64=1, stack_depth=8))
            assert plan["ok"] == 0 and plan["lds_bytes"] == 0
    assert n > 5000 and 0 < raised < n
    # the launch knobs' other arms (RRT_MIN_WAVES, RRT_GLOBAL_WAVES): 512-thread blocks, same invariants
    for mw, gw, stride in itertools.product((4, 6), (4, 6, 7), (80, 32)):
        for depth in (1, 33, 64):
            q = dict(book=0, specular=1, image_tex=0, n_nodes=200, n_prims=520, stack_depth=depth, node_stride=stride)
            plan = _lib.launch_plan(**dict(q, min_waves=mw, global_waves=gw))
            assert plan["ok"] == 1 and plan["lds_bytes"] == layout_bytes(q, plan["threads"], 2, 0) <= BLOCK_MAX
            assert plan["raise_limit"] == (plan["lds_bytes"] > KIB64)
    with pytest.raises(rrt.RrtError):
        _lib.launch_plan(n_nodes=1, n_prims=1, stack_depth=1, node_stride=64)


# ---- the reference reaches the deep slots -------------------------------------------------------
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
def test_oracle_walk_of_the_ladder_goes_deep(monkeypatch, in_lds):
    """Conditions on the reference alone: the KBVH walk of the ladder holds at least 24 live stack
    entries (measured: 26 of a stack_need of 28 staged, 27 of 29 from global memory), so a GPU render
    that matches it has written and read that many slots."""
    if in_lds is None:
        monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    else:
        monkeypatch.setenv("RRT_SCENE_IN_LDS", in_lds)
    for kind in (1, 0):
        scene, nodes, order, info = D.built(in_lds, "ladder", kind)
        oracle.kbvh_stack_peak()
        k, _, _ = oracle.render_kbvh(scene, nodes, order, info)
        peak = oracle.kbvh_stack_peak()
        print(f"ladder({kind}) in_lds={in_lds}: stack_need {info['max_depth'] + 1}, oracle peak {peak}")
        assert 24 <= peak <= info["max_depth"] + 1
        assert oracle.kbvh_stack_peak() == 0  # read and reset
        assert np.isfinite(k).all()


def test_oracle_walk_of_the_wide_scenes_goes_deep(monkeypatch):
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    for gen in ("wide", "wide_deep"):
        scene, nodes, order, info = D.built(None, gen)
        oracle.kbvh_stack_peak()
        oracle.render_kbvh(scene, nodes, order, info, threads=16)
        peak = oracle.kbvh_stack_peak()
        print(f"{gen}: {info['n_nodes']} nodes, stack_need {info['max_depth'] + 1}, oracle peak {peak}")
        assert info["n_nodes"] > 65535 and 20 <= peak <= info["max_depth"] + 1
    assert info["max_depth"] + 1 >= 33  # wide_deep: the 32-bit stack of 512 threads past 64 KiB
