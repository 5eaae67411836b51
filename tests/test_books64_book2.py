"""CPU tests of the f64 books path for book 2 (RRT_FLAG_F64_BOOK2: moving spheres, quads, checker
textures): the additive ABI, scene creation's refusals (they come before any device call), the launch
plan of the kernel's book-2 class, and the conditions on the reference that make bit-equality a fair
bar for tests/test_gpu_books64_book2.py.

BOOKS finds the closest hit in its own tree; an exact t-tie between two primitives is won by tree
order, and no f64 mode of the oracle walks the kernel's tree. So the GPU tests compare bits only on
frames where BOOKS does not depend on the primitive order: each frame of books64_book2_scenes.py must
give the same bits and ray counts with its quad list and its sphere list reversed.
"""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib

import books64_book2_scenes as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt_hip.h")
CLI = os.path.join(ROOT, "rustraytrace_amd", "rrt")
KIB64 = 64 * 1024
BLOCK_MAX = 160 * 1024
MAX_STACK = 64


# ---- additive ABI ------------------------------------------------------------------------------
def test_flag_value_in_header_and_bindings():
    src = open(HEADER).read()
    m = re.search(r"#define\s+RRT_FLAG_F64_BOOK2\s+(0x[0-9a-fA-F]+)u", src)
    assert m and int(m.group(1), 16) == 0x20 == _lib.FLAG_F64_BOOK2
    assert _lib.FLAG_F64_BOOK2 & (_lib.FLAG_RAY_TIME | _lib.FLAG_QUIET | _lib.FLAG_BOOK3 | _lib.FLAG_F64
                                  | _lib.FLAG_DEVICE_BVH) == 0


def test_ex_entries_exported_and_abi_version_unchanged():
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("rrt_hip_render_f64_ex", "rrt_hip_render_f64_rgb8_ex"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        decl = re.search(name + r"\s*\(([^)]*)\)", src)
        assert decl and len(decl.group(1).split(",")) == 12 == len(getattr(lib, name).argtypes)
        # the one-shot without _ex, plus the RrtSceneExt pointer
        assert len(getattr(lib, name[:-3]).argtypes) == 11
    assert lib.rrt_hip_abi_version() == 11
    assert "There is no _ex form" not in open(HEADER).read()
    assert _lib.DEVICE_OPS64["QUAD64"] == (10, 9, 2) and _lib.DEVICE_OPS64["CHECKER64"] == (11, 4, 1)
    assert ctypesizeof_query() == 64


def ctypesizeof_query():
    import ctypes

    return ctypes.sizeof(_lib.RrtLaunchPlanQuery)


# ---- refusals, with no device ------------------------------------------------------------------
SMALL = dict(image_width=32, samples_per_pixel=4, max_depth=4)


@pytest.mark.parametrize("which,item", [(4, "Perlin"), (8, "media"), ("book3", "RRT_FLAG_BOOK3")])
def test_scene_creation_refuses_what_the_class_does_not_cover(which, item):
    sc = rrt.rest_of_your_life_scene(SMALL) if which == "book3" else rrt.next_week_scene(which, SMALL)
    with pytest.raises(rrt.RrtError) as e:
        rrt.DeviceScene(sc, device=0, f64=True, f64_book2=True)
    assert e.value.code == -1  # RRT_E_INVALID
    assert "RRT_FLAG_F64_BOOK2" in str(e.value) and item in str(e.value)
    with pytest.raises(rrt.RrtError) as e:  # the flag alone implies RRT_FLAG_F64: the same refusal
        rrt.DeviceScene(sc, device=0, f64_book2=True)
    assert e.value.code == -1 and "RRT_FLAG_F64_BOOK2" in str(e.value)


def test_kind6_and_kind7_materials_are_named():
    sc = rrt.next_week_scene(1, SMALL)
    for kind, word in ((6, "kind 6"), (7, "kind 7")):
        mats = sc.materials.copy()
        mats["kind"][len(mats) - 1] = kind
        bad = rrt.SceneData(sc.camera, sc.spheres, mats, flags=sc.flags, motion=sc.motion)
        with pytest.raises(rrt.RrtError, match="RRT_FLAG_F64_BOOK2") as e:
            rrt.DeviceScene(bad, device=0, f64_book2=True)
        assert e.value.code == -1 and word in str(e.value)


def test_f64_alone_keeps_todays_refusal():
    sc = rrt.next_week_scene(1, SMALL)
    with pytest.raises(rrt.RrtError, match="RRT_FLAG_F64 renders book-1 scenes") as e:
        rrt.DeviceScene(sc, device=0, f64=True)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="book-1"):
        rrt.render_f64(sc)
    with pytest.raises(ValueError, match="book-1"):
        rrt.render_f64_rgb8(sc)


def test_cli_refuses_noise_scene_before_any_device_call():
    r = subprocess.run([CLI, "the_next_week", "4", "--books-f64-book2", "--image_width", "32", "--samples_per_pixel", "4"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "HIP render failed: RRT_FLAG_F64_BOOK2" in r.stderr
    assert r.stdout == ""


# ---- launch plan -------------------------------------------------------------------------------
THREADS = 256  # the class's block: 143-149 VGPRs, 3 waves per SIMD, three blocks per CU


def ceil16(n):
    return (n + 15) // 16 * 16


def staged_layout(q, inv_r):
    """The book-2 class's block as this test states it: the 16-bit stack of its 256-thread block rounded
    up to 16 B; for a staged scene the nodes re-laid as 112 B each, one 16-B f32 record per primitive
    (a sphere's (center1, r), a quad's (q, tag)), and the f64 1/r table (8 B per primitive, + 8 B of
    alignment) when it still fits 64 KiB. Motion rows and the 128-B quad records stay in global memory."""
    n = ceil16(q["stack_depth"] * THREADS * 2)
    if q["node_stride"] == 80:
        n += q["n_nodes"] * 112 + q["n_prims"] * (16 + (8 if inv_r else 0)) + (8 if inv_r else 0)
    return n


def host_stages(q):
    """Scene creation's staging rule for every f64 scene (rrt_books64.hip f64_lds_min_bytes): the smallest
    staged form under a 512-thread block's stack within 64 KiB, whatever block the class launches."""
    return ceil16(q["stack_depth"] * 512 * 2) + q["n_nodes"] * 112 + q["n_prims"] * 16 <= KIB64


def test_launch_plan_of_the_book2_class():
    n = 0
    sizes = [(1, 1), (100, 250), (200, 520), (300, 700), (520, 1400)]
    for (n_nodes, n_prims), stride, n_quads, depth in itertools.product(sizes, (80, 32), (0, 3), range(1, MAX_STACK + 1)):
        q = dict(book=2, f64=1, f64_book2=1, n_nodes=n_nodes, n_prims=n_prims, stack_depth=depth, node_stride=stride,
                 n_quads=n_quads, specular=1, image_tex=1)
        plan = _lib.launch_plan(**q)
        if stride == 80 and not host_stages(q):
            # scene creation builds the global-memory tree for such a scene; the plan itself refuses
            # only what does not fit its own block
            assert plan["ok"] == int(staged_layout(q, False) <= KIB64)
            continue
        assert plan["ok"] == 1 and plan["f64"] == 1 and plan["kernel_class"] == 3
        assert (plan["threads"], plan["waves"], plan["stack_bytes"], plan["scene_in_lds"]) == (THREADS, 3, 2, int(stride == 80))
        assert plan["shape"] == (1 if stride == 80 else 0) and plan["rec32_in_lds"] == 0
        if stride == 80:
            assert plan["inv_r_in_lds"] == int(staged_layout(q, True) <= KIB64)
        assert plan["lds_bytes"] == staged_layout(q, plan["inv_r_in_lds"])
        assert plan["lds_bytes"] <= BLOCK_MAX and (plan["lds_bytes"] <= KIB64 or plan["raise_limit"])
        n += 1
        for bad in (dict(n_perlin=1), dict(n_media=1), dict(stack_depth=MAX_STACK + 1), dict(n_nodes=70000),
                    dict(book=3)):
            assert _lib.launch_plan(**dict(q, **bad))["ok"] == 0
        # with the word 0 every answer is today's: refused
        assert _lib.launch_plan(**dict(q, f64_book2=0))["ok"] == 0
    assert n > 400
    # a book-1 scene with the word set plans as RRT_FLAG_F64 alone
    q1 = dict(book=0, f64=1, n_nodes=100, n_prims=250, stack_depth=12, node_stride=80, specular=1, image_tex=0)
    assert _lib.launch_plan(**dict(q1, f64_book2=1)) == _lib.launch_plan(**q1)
    # and without f64 the word means nothing
    q2 = dict(book=2, n_nodes=100, n_prims=190, stack_depth=12, node_stride=80)
    assert _lib.launch_plan(**dict(q2, f64_book2=1)) == _lib.launch_plan(**q2)


# ---- conditions on the reference alone ---------------------------------------------------------
@pytest.mark.parametrize("name", B.FRAMES)
def test_books_does_not_depend_on_primitive_order(name):
    scene = B.frame(name)
    ref, rays, _ = oracle.render(scene, oracle.BOOKS, threads=16)
    assert np.isfinite(ref).all() and np.all(ref[..., 3] == scene.spp) and ref[..., :3].max() > 0
    ran = 0
    for what in ("quads", "spheres"):
        other = B.reordered(scene, what)
        if other is None:
            continue
        out, rays2, _ = oracle.render(other, oracle.BOOKS, threads=16)
        ndiff = int((out[..., :3] != ref[..., :3]).sum())
        print(f"{name}: {what} reversed: {ndiff} channels differ, rays {rays2} vs {rays}")
        assert ndiff == 0 and rays2 == rays
        ran += 1
    assert ran >= 1


def test_mixed_frame_exercises_every_addition():
    """Each of the four quads and the earth sphere changes the mixed frame: every branch is reached."""
    scene = B.frame("mixed")
    ref, _, _ = oracle.render(scene, oracle.BOOKS, threads=16)
    nq = len(scene.quads)
    for drop in range(nq + 1):
        sc = rrt.SceneData(scene.camera.copy(), scene.spheres, scene.materials, textures=scene.textures,
                           flags=scene.flags, motion=scene.motion, quads=scene.quads)
        if drop < nq:
            sc.quads = np.ascontiguousarray(np.delete(scene.quads, drop))
        else:
            sc.spheres, sc.motion = scene.spheres[:-1], scene.motion[:-1]
            sc.camera["params_u"][0, 2] = len(sc.spheres)
        out, _, _ = oracle.render(sc, oracle.BOOKS, threads=16)
        changed = int((out[..., :3] != ref[..., :3]).any(axis=-1).sum())
        print(f"mixed without {'quad %d' % drop if drop < nq else 'the earth sphere'}: {changed} pixels change")
        assert changed > 100
