"""The fast device builder (RRT_FLAG_FAST_BVH: rustraytrace_amd/csrc/rrt_bvh_lbvh.h, the LBVH kernels of
rrt_bvh_build.hip) on the GPU.

The builder is held to its sequential host twin (rrt_build_bvh_lbvh, the same header): equal node bytes,
leaf order and info in both of its forms (one launch per phase; the single workgroup), for every scene
of tests/device_bvh_scenes.py, the edge shapes of tests/lbvh_scenes.py and a 10^5-sphere scene. Renders
are checked the way every render here is: bit for bit against the oracle walking the tree the scene
holds, and for the f64 kernel against BOOKS. Updates are compared with a fresh flagged scene of the new
inputs, refits with the refit twin (rrt_refit_bvh_lbvh_world), rrt_scene_set_builder with fresh scenes
of either builder. No tolerance anywhere. Frames are 32x18x4 unless a test says otherwise.
"""
import subprocess

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh, build_bvh_lbvh, refit_bvh_lbvh_world

import device_bvh_scenes as D
import geometry_scenes as G
import lbvh_scenes as L
import media_scenes as M
from test_gpu_device_bvh import CLI, assert_same_tree, scale_scene
from test_gpu_scene_geometry import assert_equals_fresh_g, snapshot_g
from test_gpu_scene_media import assert_equals_fresh_w, snapshot_w
from test_gpu_scene_update import assert_equals_fresh, frame_of, jittered, open_scene, snapshot, with_spheres

pytestmark = pytest.mark.gpu

ALL = list(D.SCENES) + [k for k in L.SCENES if k not in D.SCENES]
BOOK1 = D.BOOK1 + [k for k in L.BOOK1 if k not in D.SCENES]
SMALL_MAX = 2048  # primitives the single workgroup takes (rrt_bvh_build.hip kLbvhSmallMax)


def n_tree_of(sc):
    nodes, order, info = build_bvh_lbvh(sc, 1, 32)
    return D.n_prims(sc) - info["n_unbounded"]


def twin_of(sc, info):
    return build_bvh_lbvh(sc, info["max_leaf_param"], info["node_stride"])


@pytest.fixture
def form():
    """Forces a form for one test and restores the automatic choice."""
    yield _lib.lbvh_form
    _lib.lbvh_form(-1)


def device_tree(sc, **kw):
    ds = rrt.DeviceScene(sc, device=0, fast_bvh=True, **kw)
    tree, stats = ds.read_bvh(), ds.build_stats()
    ds.close()
    return tree, stats


# ---- 1. device equals twin ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_device_equals_twin_f32_in_both_forms(name, form):
    sc = L.lookup(name)
    trees = []
    for f in (0, 1):
        if f == 1 and n_tree_of(sc) > SMALL_MAX:
            continue
        form(f)
        tree, stats = device_tree(sc)
        assert stats["builder"] == "lbvh" and stats["form"] == f and stats["blocking_reads"] == 1
        assert_same_tree(tree, twin_of(sc, tree[2]))
        trees.append(tree)
    if len(trees) == 2:
        assert_same_tree(trees[0], trees[1])


@pytest.mark.parametrize("name", BOOK1)
def test_device_equals_twin_f64(name):
    sc = L.lookup(name)
    tree, stats = device_tree(sc, f64=True)
    assert stats["builder"] == "lbvh"
    assert_same_tree(tree, twin_of(sc, tree[2]))


def test_forcing_the_single_workgroup_over_its_bound_fails_the_build(form):
    sc = D.scene("C5")
    form(1)
    with pytest.raises(rrt.RrtError) as e:
        rrt.DeviceScene(sc, device=0, fast_bvh=True)
    assert e.value.code != 0 and "fast build" in str(e.value)


# The launches an LBVH build counts in its launch-per-phase form (rrt_bvh_build.hip lbvh_build,
# lbvh_finish; a rocPRIM sort counts once): init, bounds, keys, sort, topology, levels, sort = 7 before
# the read; flags and scan (leaves over 1 only), ids, links = 4 after it; the box pass is one launch per
# level plus the slack over 16,384 nodes, else 1. The pack of emit is not the builder's.
LAUNCH_CONSTANT = 7 + 4 + 1


def test_device_equals_twin_at_1e5_spheres():
    sc = scale_scene()
    ds = rrt.DeviceScene(sc, device=0, fast_bvh=True)
    tree, stats = ds.read_bvh(), ds.build_stats()
    ds.close()
    assert tree[2]["node_stride"] == 32 and tree[2]["max_leaf_size"] == 1
    assert_same_tree(tree, twin_of(sc, tree[2]))
    assert stats["builder"] == "lbvh" and stats["form"] == 0 and stats["blocking_reads"] == 1 and stats["shape_attempts"] == 1
    assert stats["launches"] <= LAUNCH_CONSTANT + tree[2]["max_depth"], stats
    gpu = rrt.render(sc, fast_bvh=True)
    assert np.all(gpu[..., 3] == sc.spp) and np.isfinite(gpu).all()


def test_build_stats_of_c2():
    ds = rrt.DeviceScene(D.scene("C2"), device=0, fast_bvh=True)
    stats = ds.build_stats()
    ds.close()
    assert stats == {"builder": "lbvh", "launches": 1, "blocking_reads": 1, "form": 1, "shape_attempts": 1}
    ds = rrt.DeviceScene(D.scene("C2"), device=0, device_bvh=True)
    binned = ds.build_stats()
    levels = ds.bvh_info()["max_depth"]
    ds.close()
    assert binned["builder"] == "binned" and binned["form"] == 0
    assert binned["blocking_reads"] >= 1 + levels and binned["launches"] >= 2 + 9 * levels


@pytest.mark.parametrize("name", ["C2", "C5"])
def test_default_path_untouched(name):
    sc = D.scene(name)
    ds = rrt.DeviceScene(sc, device=0)
    nodes, order, info = ds.read_bvh()
    ds.close()
    h_nodes, h_order, h_info = build_bvh(sc)
    assert np.array_equal(nodes, h_nodes) and np.array_equal(order, h_order)
    assert info == h_info


# ---- 2. frames ------------------------------------------------------------------------------------
def flagged_frame(sc, **kw):
    ds = open_scene(sc, fast_bvh=True, **kw)
    frame, rays = frame_of(ds)
    tree = ds.read_bvh()
    ds.close()
    return frame, rays, tree


@pytest.mark.parametrize("name", ALL)
def test_frame_is_the_oracles_walk_of_the_scenes_tree(name):
    sc = L.lookup(name)
    gpu, rays, (nodes, order, info) = flagged_frame(sc)
    kref, krays, _ = oracle.render_kbvh(sc, nodes, order, info, threads=16)
    assert np.array_equal(gpu.astype(np.float64), kref), "flagged render differs from the oracle over its own tree"
    assert rays == krays


@pytest.mark.parametrize("name", ["C2", "C5", "spheres65", "line65"])
def test_f64_frame_is_books(name):
    sc = L.lookup(name)
    gpu, rays, _ = flagged_frame(sc, f64=True)
    books, books_rays, _ = oracle.render(sc, oracle.BOOKS, threads=16)
    assert np.array_equal(gpu, books)
    assert rays == books_rays


# ---- 3. updates -----------------------------------------------------------------------------------
def fresh_of(sc, snap, **kw):
    ds = open_scene(sc, **kw)
    got = snap(ds)
    ds.close()
    return got


def test_sphere_updates_equal_fresh_flagged_scenes():
    sc = D.scene("C2")
    ds = open_scene(sc, fast_bvh=True)
    for step, spheres in enumerate([jittered(sc, 11), jittered(sc, 12, scale=0.4)]):
        new = with_spheres(sc, spheres)
        ds.update_spheres(spheres)
        got = snapshot(ds)
        assert_equals_fresh(got, fresh_of(new, snapshot, fast_bvh=True))
        assert_same_tree(got["tree"], twin_of(new, got["tree"][2]))
        assert ds.build_stats()["builder"] == "lbvh"
        if step == 1:
            assert ds.update_stats()["last_allocations"] == 0
    ds.close()


def test_geometry_updates_equal_fresh_flagged_scenes():
    sc = G.scene("B3")  # quads with a light list
    ds = open_scene(sc, fast_bvh=True)
    for step, seed in enumerate((21, 22)):
        spheres, quads, lights = G.moved(sc, seed)
        new = G.with_geometry(sc, spheres, sc.motion, quads, lights)
        ds.update_geometry(spheres=spheres, motion=sc.motion, quads=quads, lights=lights)
        got = snapshot_g(ds)
        assert_equals_fresh_g(got, fresh_of(new, snapshot_g, fast_bvh=True))
        assert_same_tree(got["tree"], twin_of(new, got["tree"][2]))
        if step == 1:
            assert ds.update_stats()["last_allocations"] == 0
    ds.close()


def test_world_updates_equal_fresh_flagged_scenes():
    sc = M.scene("fog")
    ds = open_scene(sc, fast_bvh=True)
    for step, new in enumerate((M.moved(sc, 31), M.sphere0_far(sc), M.moved(sc, 32))):  # the second flips the classification
        M.change(ds, "update_world", new)
        got = snapshot_w(ds)
        assert_equals_fresh_w(got, fresh_of(new, snapshot_w, fast_bvh=True))
        assert_same_tree(got["tree"], twin_of(new, got["tree"][2]))
        if step >= 1:
            assert ds.update_stats()["last_allocations"] == 0
    ds.close()


# ---- 4. refits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C5", "fog"])
def test_refits_equal_the_lbvh_refit_twin(name):
    sc = M.scene("fog") if name == "fog" else D.scene(name)
    ds = open_scene(sc, fast_bvh=True)
    built = ds.read_bvh()
    info = built[2]

    def refit(new):
        if name == "fog":
            M.change(ds, "refit_world", new)
        else:
            ds.refit_spheres(new.spheres)

    refit(sc)  # unchanged inputs: the build's bytes
    assert_same_tree(ds.read_bvh(), built)
    for seed in (41, 42):
        new = M.moved(sc, seed) if name == "fog" else with_spheres(sc, jittered(sc, seed, 0.05))
        refit(new)
        want = refit_bvh_lbvh_world(sc, new, info["max_leaf_param"], info["node_stride"])
        got = ds.read_bvh()
        assert_same_tree(got, want[:3])
        assert not np.array_equal(got[0], built[0])
        cost = ds.tree_cost()
        assert np.float64(cost["sah"]).tobytes() == np.float64(want[3]).tobytes(), (cost, want[3])
        at_build = refit_bvh_lbvh_world(sc, sc, info["max_leaf_param"], info["node_stride"])[3]
        assert np.float64(cost["sah_at_build"]).tobytes() == np.float64(at_build).tobytes()
    assert ds.refit_stats()["last_allocations"] == 0
    ds.close()


# ---- 5. set_builder -------------------------------------------------------------------------------
def test_set_builder_switches_the_next_updates_builder():
    sc = D.scene("C5")
    ds = open_scene(sc)  # the binned builder
    assert ds.build_stats()["builder"] == "binned"
    steps = [("binned", jittered(sc, 51)), ("lbvh", jittered(sc, 52)), ("binned", jittered(sc, 53))]
    for step, (builder, spheres) in enumerate(steps):
        new = with_spheres(sc, spheres)
        ds.set_builder(builder)
        ds.update_spheres(spheres)
        assert ds.build_stats()["builder"] == builder
        assert_equals_fresh(snapshot(ds), fresh_of(new, snapshot, fast_bvh=builder == "lbvh"))
        if step == 2:
            assert ds.update_stats()["last_allocations"] == 0
    ds.refit_spheres(sc.spheres)  # a refit follows the current (binned) build
    ds.set_builder("lbvh")
    ds.update_spheres(sc.spheres)
    assert ds.update_stats()["last_allocations"] == 0
    assert_equals_fresh(snapshot(ds), fresh_of(sc, snapshot, fast_bvh=True))
    with pytest.raises(ValueError):
        ds.set_builder("sweep")
    assert _lib.load().rrt_scene_set_builder(ds._h, 2) == -1
    ds.close()
    host = rrt.DeviceScene(sc, device=0)
    with pytest.raises(rrt.RrtError):
        host.set_builder("lbvh")
    with pytest.raises(rrt.RrtError):
        host.build_stats()
    host.close()


# ---- 6. one-shots, CLI, refusals --------------------------------------------------------------------
def test_one_shot_entries_equal_the_device_scene_route():
    sc = D.scene("NW9")
    accum, _, _ = flagged_frame(sc)
    assert np.array_equal(rrt.render(sc, fast_bvh=True), accum)  # rrt_hip_render_ex, one worker
    lib = _lib.load()
    lib.rrt_testing_device_wrap(1)
    try:
        two = rrt.render(sc, n_gpus=2, fast_bvh=True)
    finally:
        lib.rrt_testing_device_wrap(0)
    assert np.array_equal(two, accum)
    assert np.array_equal(rrt.render_rgb8(sc, fast_bvh=True), rrt.quantize_accum(sc.width, sc.height, accum, sc.spp))
    c5 = D.scene("C5")
    accum64, _, _ = flagged_frame(c5, f64=True)
    assert np.array_equal(rrt.render_f64(c5, fast_bvh=True), accum64)


def test_cli_fast_bvh_equals_python(tmp_path):
    path = tmp_path / "nw9.ppm"
    r = subprocess.run([CLI, "--backend", "hip", "the_next_week", "9", "--image_width", "32", "--samples_per_pixel", "4",
                        "--fast-bvh", "-o", str(path)], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    sc = D.scene("NW9")
    acc = rrt.render(sc, fast_bvh=True)
    assert path.read_bytes() == rrt.format_ppm_from_accum(sc.width, sc.height, acc, sc.spp)


def test_width_4_is_refused_with_the_flag(monkeypatch):
    monkeypatch.setenv("RRT_BVH_WIDTH", "4")
    with pytest.raises(rrt.RrtError) as e:
        rrt.DeviceScene(D.scene("C2"), device=0, fast_bvh=True)
    assert e.value.code == -1 and "RRT_FLAG_FAST_BVH" in str(e.value)
