"""GPU: the launch shapes at the LDS limits and the deep stack slots (tests/deep_scenes.py), bit for
bit against the oracle's walk of the kernel's own tree (KBVH), with equal ray counts.

The other GPU suites render shallow, balanced trees: no walk of theirs holds more than about ten
stack entries, no block asks for more than 64 KiB of LDS, and no scene has the 65,536 nodes that
select the 32-bit-stack kernel. Here: walks that hold 24-27 live entries (the oracle's own peak is
asserted in tests/test_launch_plan.py), in every book-1 class, staged and read from global memory;
launches that fall back to a smaller block or raise the kernel's dynamic-LDS limit (asserted through
the launch plan); the 32-bit stack; and the f64 kernel on the same scenes against BOOKS.
"""
import numpy as np
import pytest

from oracle import oracle
from rustraytrace_amd import _lib

import deep_scenes as D
from test_gpu_books64 import _check, _gpu_f64
from test_gpu_parity import assert_bit_exact, gpu_tile
from test_launch_plan import KIB64, scene_query

pytestmark = pytest.mark.gpu


def _place(monkeypatch, in_lds):
    if in_lds is None:
        monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    else:
        monkeypatch.setenv("RRT_SCENE_IN_LDS", in_lds)


def _plan(scene, info, order, **kw):
    return _lib.launch_plan(**dict(scene_query(scene, info, len(order)), **kw))


def _render_and_compare(scene, nodes, order, info, twin=False, threads=1):
    gpu, idx, ctr, _ = gpu_tile(scene)
    assert len(idx) == scene.height
    ref, rays, _ = oracle.render_kbvh(scene, nodes, order, info, threads=threads)
    assert_bit_exact(gpu, ref, scene.spp)
    assert ctr["rays"] == rays
    assert np.all(gpu[..., 3] == scene.spp)
    if twin:  # the independent books-structured tree finds the same closest hits
        tw, trays, _ = oracle.render(scene, oracle.TWIN, threads=threads)
        assert_bit_exact(gpu, tw, scene.spp)
        assert trays == rays


# ---- deep pushes, f32 --------------------------------------------------------------------------
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
@pytest.mark.parametrize("kind", [1, 0], ids=["specular", "diffuse"])
def test_ladder_deep_pushes(monkeypatch, kind, in_lds):
    """26 (staged) / 27 (global) live stack entries. Staged: kind 1 is C2's class, whose 1024-thread
    block would need 79,088 B and falls back to 512 x 6; kind 0 the diffuse class at 256 x 8. From
    global memory: 256 x 7."""
    _place(monkeypatch, in_lds)
    scene, nodes, order, info = D.built(in_lds, "ladder", kind)
    plan = _plan(scene, info, order)
    assert (plan["threads"], plan["waves"]) == ((256, 7) if in_lds else (512, 6) if kind else (256, 8))
    _render_and_compare(scene, nodes, order, info, twin=True)


def test_ladder_textured_full_class(monkeypatch):
    """The earth texture on material 0: the full book-1 class (0), 512 x 6."""
    _place(monkeypatch, None)
    scene, nodes, order, info = D.built(None, "ladder", 1, True)
    plan = _plan(scene, info, order)
    assert (plan["kernel_class"], plan["threads"], plan["waves"]) == (0, 512, 6)
    _render_and_compare(scene, nodes, order, info, twin=True)


def test_ladder_from_l2_in_512_thread_blocks(monkeypatch):
    """RRT_GLOBAL_WAVES=6: scenes read from global memory in 512 x 6 blocks."""
    _place(monkeypatch, "0")
    monkeypatch.setenv("RRT_GLOBAL_WAVES", "6")
    scene, nodes, order, info = D.built("0", "ladder", 1)
    plan = _plan(scene, info, order, global_waves=6)
    assert (plan["threads"], plan["waves"], plan["scene_in_lds"]) == (512, 6, 0)
    _render_and_compare(scene, nodes, order, info, twin=True)


# ---- LDS limits, f32 ---------------------------------------------------------------------------
LIMITS = [  # generator arguments, (threads, raise the dynamic-LDS limit)
    ((14, 470, 1), (512, 0)),        # 79,712 B at 1024 threads -> 60,256 at 512
    ((40, 10, 1), (512, 0)),         # 87,808 -> 46,848
    ((64, 10, 1), (512, 1)),         # the stack cap: 140,032 -> 74,496, raised
    ((60, 400, 1), (512, 1)),        # 167,744 (over a block's 160 KiB) -> 104,256, raised
    ((60, 400, 0), (256, 1)),        # diffuse class: 72,512 at its 256 threads, raised
    ((40, 400, 1, True), (512, 1)),  # full class with the earth texture: 83,888 at 512, raised
]


@pytest.mark.parametrize("args,shape", LIMITS, ids=[str(a) for a, _ in LIMITS])
def test_cluster_at_the_lds_limits(monkeypatch, args, shape):
    _place(monkeypatch, None)
    scene, nodes, order, info = D.built(None, "cluster", *args)
    plan = _plan(scene, info, order)
    assert plan["scene_in_lds"] == 1 and (plan["threads"], plan["raise_limit"]) == shape
    assert (plan["lds_bytes"] > KIB64) == bool(shape[1])
    _render_and_compare(scene, nodes, order, info)


def test_book2_cluster_over_64k(monkeypatch):
    """A moving sphere makes the scene a book-2 scene (class 1, 256 x 5, 64 B per primitive): 62 stack
    entries and 38,704 B of scene are 70,448 B, over the default limit."""
    _place(monkeypatch, None)
    scene, nodes, order, info = D.built(None, "moving_cluster", 60, 300)
    plan = _plan(scene, info, order)
    assert (plan["kernel_class"], plan["threads"], plan["scene_in_lds"], plan["raise_limit"]) == (1, 256, 1, 1)
    _render_and_compare(scene, nodes, order, info)


# ---- the 32-bit stack --------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["wide", "wide_deep"])
def test_32_bit_stack_kernel(monkeypatch, gen):
    """More than 65,535 nodes. wide_deep's stack_need of 33 or more puts the 512-thread block's 32-bit
    stack past 64 KiB. TWIN differs from KBVH by one ray on these scenes (a tie between tiny spheres
    that the two trees visit in different orders), so KBVH alone is the reference."""
    _place(monkeypatch, None)
    scene, nodes, order, info = D.built(None, gen)
    plan = _plan(scene, info, order)
    assert info["n_nodes"] > 65535 and (plan["stack_bytes"], plan["threads"]) == (4, 512)
    assert plan["raise_limit"] == (1 if gen == "wide_deep" else 0)
    _render_and_compare(scene, nodes, order, info, threads=16)


# ---- f64 ---------------------------------------------------------------------------------------
F64 = [("ladder", (1,)), ("ladder", (0,)), ("cluster", (40, 10, 1))]


@pytest.mark.parametrize("gen,args", F64, ids=[f"{g}{a}" for g, a in F64])
def test_f64_kernel_on_deep_scenes(monkeypatch, gen, args):
    """The f64 kernel's own stack code on the same scenes, against BOOKS: every sum bit for bit,
    equal closest-hit query counts."""
    _place(monkeypatch, None)
    scene = getattr(D, gen)(*args)
    gpu, gpu32, gpu_rays = _gpu_f64(scene)
    books, books_rays, _ = oracle.render(scene, oracle.BOOKS, threads=16)
    assert gpu_rays == books_rays
    _check(scene, gpu, books, f"{gen}{args} f64")
    assert np.array_equal(gpu32, gpu.astype(np.float32))
