"""rrt_scene_refit_spheres and rrt_scene_tree_cost on the GPU.

The yardstick for the tree is the host twin (rrt_refit_bvh_binned over the scene the tree was built
from and the newest spheres): equal node bytes, the kept leaf order, unchanged info. The yardstick for
the per-primitive tables is a fresh DeviceScene of the new inputs, its rows gathered through the kept
leaf order. f32 frames equal the oracle walking the tree read back; f64 frames equal BOOKS, which
reads no tree. No tolerance anywhere: bytes and bits. Frames are 32x18x4.
"""
import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import refit_bvh_binned

import books64_book2_scenes as B
import device_bvh_scenes as D
from test_gpu_device_bvh import assert_same_tree
from test_gpu_scene_update import (TABLES, _b3, assert_equals_fresh, fresh, frame_of, jittered, open_scene, snapshot,
                                   with_spheres)

pytestmark = pytest.mark.gpu

_scenes = {}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def scene(name):
    """D.scene's scenes, the mixed book-2 scene, and G70: RTOW with grid_half 70 (19,603 nodes), the
    smallest of this file's trees over the single workgroup's bound of 16,384 nodes."""
    if name in ("mixed", "G70"):
        if name not in _scenes:
            _scenes[name] = (B.mixed_scene(rrt.next_week_scene(1, D.KW)) if name == "mixed" else
                             rrt.rtow(grid_half=70, max_depth=8, **D.KW))
        return _scenes[name]
    return D.scene(name)


def twin_refit(built, new, info, f64=False):
    """The twin's refit for the shape the scene keeps (test_gpu_device_bvh.twin_of's node prices)."""
    cost = 1.5 if (f64 and info["node_stride"] == 80) else 2.0
    return refit_bvh_binned(built, new.spheres, new.motion, info["max_leaf_param"], cost, info["node_stride"])


def assert_tables_through_kept_order(got, want):
    """got: the refitted scene's snapshot; want: a fresh scene's of the same inputs (another leaf order)."""
    kept, fresh_order = got["tree"][1], want["tree"][1]
    at = np.empty(len(fresh_order), np.int64)
    at[fresh_order] = np.arange(len(fresh_order))  # primitive -> its row in the fresh scene
    for t in TABLES:
        g, w = got["tables"][t], want["tables"][t]
        assert g.shape == w.shape, t
        if not g.size:
            continue
        if t == "boxes":  # primitive order
            assert g.tobytes() == w.tobytes(), "boxes differ"
            continue
        rows = w.reshape(len(fresh_order), -1)[at[kept]]
        assert g.reshape(len(kept), -1).tobytes() == rows.tobytes(), f"table {t} differs"


# ---- 1. device equals twin -----------------------------------------------------------------------
# the form of the bottom-up pass each tree takes: 1 = the single workgroup, 0 = one launch per level
FORMS = {"spheres2": 1, "spheres3": 1, "spheres65": 1, "spheres1025": 1, "C2": 1, "C5": 1, "NW1": 1, "mixed": 1, "G70": 0}
assert set(FORMS.values()) == {0, 1}


@pytest.mark.parametrize("name", list(FORMS))
def test_three_refits_equal_the_twin_f32(name):
    sc = scene(name)
    original = fresh(sc)
    ds = open_scene(sc)
    info = original["tree"][2]
    steps = [jittered(sc, 11), jittered(sc, 12, scale=0.4), sc.spheres]
    for step, spheres in enumerate(steps):
        new = with_spheres(sc, spheres, sc.motion)
        ds.refit_spheres(spheres, sc.motion)
        got = snapshot(ds, frame=step == 2)
        twin = twin_refit(sc, new, info)
        assert got["tree"][2] == info, "a refit changed the info"
        assert_same_tree(got["tree"], twin[:3])
        assert np.array_equal(got["tree"][1], original["tree"][1]), "a refit changed the leaf order"
        if step < 2:
            assert_tables_through_kept_order(got, fresh(new, frame=False))
            assert got["tree"][0].tobytes() != original["tree"][0].tobytes()
        else:
            assert_equals_fresh(got, original)
        st = ds.refit_stats()
        assert st["refits"] == step + 1 and st["last_form"] == FORMS[name] and st["last_launches"] >= 4
        assert (info["n_nodes"] <= 16384) == bool(FORMS[name])
    assert ds.update_stats()["updates"] == 0
    ds.close()


# ---- 2. both forms, same bytes -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spheres65", "C2"])
def test_both_forms_write_the_same_bytes(name):
    sc = scene(name)
    sp = jittered(sc, 12, scale=0.4)
    trees = {}
    try:
        for form in (0, 1):
            _lib.refit_form(form)
            ds = open_scene(sc)
            ds.refit_spheres(sp, sc.motion)
            trees[form] = ds.read_bvh()
            assert ds.refit_stats()["last_form"] == form
            ds.close()
    finally:
        _lib.refit_form(-1)
    assert_same_tree(trees[0], trees[1])
    info = trees[0][2]
    assert_same_tree(trees[0], twin_refit(sc, with_spheres(sc, sp, sc.motion), info)[:3])


def test_forcing_the_single_workgroup_over_its_bound_is_refused():
    sc = scene("G70")
    ds = open_scene(sc)
    before = snapshot(ds)
    try:
        _lib.refit_form(1)
        with pytest.raises(rrt.RrtError) as e:
            ds.refit_spheres(jittered(sc, 11))
        assert e.value.code == -1 and "rrt_testing_refit_form" in str(e.value)
    finally:
        _lib.refit_form(-1)
    assert ds.refit_stats()["refits"] == 0
    assert_equals_fresh(snapshot(ds), before)
    ds.close()


# ---- 3. frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C5", "NW1"])
def test_f32_frame_is_the_oracles_walk_of_the_refitted_tree(name):
    sc = scene(name)
    sp = jittered(sc, 12, scale=0.4)
    moved = with_spheres(sc, sp, sc.motion)
    ds = open_scene(sc)
    before = frame_of(ds)
    ds.refit_spheres(sp, sc.motion)
    frame, rays = frame_of(ds)
    nodes, order, info = ds.read_bvh()
    ds.close()
    kacc, krays, _ = oracle.render_kbvh(moved, nodes, order, info, threads=16)
    assert frame.tobytes() != before[0].tobytes()
    assert np.array_equal(frame, kacc)
    assert rays == krays


@pytest.mark.parametrize("name", ["spheres64", "C5", "mixed"])
def test_f64_frame_is_books_and_a_fresh_scenes(name):
    sc = scene(name)
    kw = dict(f64=True, f64_book2=True) if name == "mixed" else dict(f64=True)
    sp = jittered(sc, 12, scale=0.4)
    moved = with_spheres(sc, sp, sc.motion)
    ds = open_scene(sc, **kw)
    info = ds.bvh_info()
    ds.refit_spheres(sp, sc.motion)
    got = snapshot(ds)
    ds.close()
    assert_same_tree(got["tree"], twin_refit(sc, moved, info, f64=True)[:3])
    want = fresh(moved, **kw)
    assert_tables_through_kept_order(got, want)
    books, books_rays, _ = oracle.render(moved, oracle.BOOKS, threads=16)  # BOOKS reads no tree
    assert np.array_equal(got["frame"], books) and got["rays"] == books_rays
    assert got["frame"].tobytes() == want["frame"].tobytes() and got["rays"] == want["rays"]


# ---- 4. stream order -----------------------------------------------------------------------------
def test_refit_is_ordered_on_its_stream_without_a_wait():
    torch = _torch()
    sc = scene("C2")
    sp = jittered(sc, 81, scale=0.5)
    old = fresh(sc)
    ds = open_scene(sc)
    ds.refit_spheres(sc.spheres)  # the first refit allocates and may wait; the ones below do neither
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device="cuda:0")
    first = frame_of(ds, stream)
    rows = sp.copy()
    ds.refit_spheres(rows, stream_ptr=stream.cuda_stream)
    rows["center_radius"][:] = 0.0  # the caller's array is free as soon as the call returns
    second = frame_of(ds, stream)
    stream.synchronize()
    torch.cuda.synchronize()
    assert ds.refit_stats()["last_allocations"] == 0
    after, _ = frame_of(ds)  # the refitted scene's frame, taken afterwards
    ds.close()
    assert first.cpu().numpy().tobytes() == old["frame"].tobytes()
    assert second.cpu().numpy().tobytes() == after.tobytes()
    assert after.tobytes() != old["frame"].tobytes()


# ---- 5. allocation -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C5", "NW1"])
def test_second_refit_allocates_nothing(name):
    sc = scene(name)
    ds = open_scene(sc)
    assert ds.refit_stats() == {"refits": 0, "last_allocations": 0, "last_launches": 0, "last_form": 0}
    ds.refit_spheres(jittered(sc, 61), sc.motion)
    assert ds.refit_stats()["last_allocations"] > 0
    for seed in (62, 63):
        ds.refit_spheres(jittered(sc, seed, scale=0.5), sc.motion)
        assert ds.refit_stats()["last_allocations"] == 0
    ds.update_spheres(jittered(sc, 64), sc.motion)  # an update after a refit: shared buffers, its own reserve
    ds.update_spheres(jittered(sc, 65), sc.motion)
    assert ds.update_stats()["last_allocations"] == 0
    ds.refit_spheres(jittered(sc, 66), sc.motion)  # a refit after an update
    assert ds.refit_stats()["last_allocations"] == 0
    ds.close()
    ds = open_scene(sc)  # the other way round: the update first
    ds.update_spheres(jittered(sc, 67), sc.motion)
    ds.refit_spheres(jittered(sc, 68), sc.motion)
    ds.update_spheres(jittered(sc, 69), sc.motion)
    assert ds.update_stats()["last_allocations"] == 0
    ds.refit_spheres(jittered(sc, 70), sc.motion)
    assert ds.refit_stats()["last_allocations"] == 0
    ds.close()


# ---- 6. a rebuild resets -------------------------------------------------------------------------
def test_update_after_refit_equals_fresh_and_resets_the_cost():
    sc = scene("C2")
    sp = jittered(sc, 12, scale=0.4)
    ds = open_scene(sc)
    ds.refit_spheres(sp)
    cost = ds.tree_cost()
    assert cost["refits_since_build"] == 1 and cost["sah"] != cost["sah_at_build"]
    ds.update_spheres(sp)
    assert_equals_fresh(snapshot(ds), fresh(with_spheres(sc, sp)))
    cost = ds.tree_cost()
    assert cost["refits_since_build"] == 0 and cost["sah"] == cost["sah_at_build"]
    ds.close()


# ---- 7. refusals ---------------------------------------------------------------------------------
def _refusals():
    c2 = D.scene("C2")
    bad_index = c2.spheres.copy()
    bad_index["material_index"][3] = len(c2.materials)
    motion = np.zeros((len(c2.spheres), 4), np.float32)
    motion[7, 1] = 0.25
    one = D.first_spheres(1)
    return {
        "count": (c2, dict(device_bvh=True), lambda ds: ds.refit_spheres(c2.spheres[:-1]), "n_spheres"),
        "null": (c2, dict(device_bvh=True),
                 lambda ds: _lib.check(ds._lib.rrt_scene_refit_spheres(ds._h, None, len(c2.spheres), None, None)), "null spheres"),
        "material": (c2, dict(device_bvh=True), lambda ds: ds.refit_spheres(bad_index), "material_index"),
        "flag": (c2, dict(device_bvh=False), lambda ds: ds.refit_spheres(c2.spheres), "RRT_FLAG_DEVICE_BVH"),
        "media": (D.scene("NW9"), dict(device_bvh=True),
                  lambda ds: ds.refit_spheres(D.scene("NW9").spheres, D.scene("NW9").motion), "media"),
        "book3": (_b3(), dict(device_bvh=True), lambda ds: ds.refit_spheres(ds.scene.spheres), "RRT_FLAG_BOOK3"),
        "root_leaf": (one, dict(device_bvh=True), lambda ds: ds.refit_spheres(one.spheres), "fewer than 2 primitives"),
        "motion": (c2, dict(device_bvh=True), lambda ds: ds.refit_spheres(c2.spheres, motion), "book-2 world"),
    }


@pytest.mark.parametrize("case", ["count", "null", "material", "flag", "media", "book3", "root_leaf", "motion"])
def test_refusals_leave_the_scene_untouched(case):
    sc, kw, call, reason = _refusals()[case]
    ds = open_scene(sc, **kw)
    before = snapshot(ds)
    with pytest.raises(rrt.RrtError) as e:
        call(ds)
    assert e.value.code == -1 and reason in str(e.value) and "rrt_scene_refit_spheres" in str(e.value), str(e.value)
    after = snapshot(ds)
    assert ds.refit_stats()["refits"] == 0
    ds.close()
    assert_equals_fresh(after, before)


# ---- 8. cost -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C5"])
def test_tree_cost_equals_the_twins(name):
    sc = scene(name)
    ds = open_scene(sc)
    info = ds.bvh_info()
    at_build = twin_refit(sc, sc, info)[3]
    for n, (seed, scale) in enumerate([(11, 0.05), (12, 0.4)]):
        sp = jittered(sc, seed, scale)
        ds.refit_spheres(sp)
        cost = ds.tree_cost()
        want = twin_refit(sc, with_spheres(sc, sp), info)[3]
        assert np.float64(cost["sah"]).tobytes() == np.float64(want).tobytes(), (cost, want)
        # taken lazily, after the first refit had already changed the boxes: still the build's
        assert np.float64(cost["sah_at_build"]).tobytes() == np.float64(at_build).tobytes(), (cost, at_build)
        assert cost["refits_since_build"] == n + 1
    ds.close()
