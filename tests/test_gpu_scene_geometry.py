"""rrt_scene_update_geometry and rrt_scene_refit_geometry on the GPU: quads and book-3 light lists
changed in place.

The yardstick is tests/test_gpu_scene_update.py's, extended with the geometry tables (the GQuad or
GQuad64 records, the quads' table rows, the GLight records): a fresh DeviceScene(device_bvh=True) of
the new inputs. An updated scene holds its bytes everywhere and renders its frame with its ray count.
A refitted scene holds the tree of the host twin (rrt_refit_bvh_binned_ex), the fresh scene's tables
gathered through the kept leaf order and its geometry tables as they are; an f64 frame is the fresh
scene's bit for bit, an f32 frame the oracle's walk of the refitted tree read back (the assertion of
tests/test_gpu_scene_refit.py). No tolerance anywhere. Every refused input is rejected on the host.
Frames are 32 x 18 x 4; book 3 renders its square frames at 4 spp.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import refit_bvh_binned

import device_bvh_scenes as D
import geometry_scenes as G
from test_gpu_device_bvh import assert_same_tree
from test_gpu_scene_refit import assert_tables_through_kept_order
from test_gpu_scene_update import assert_equals_fresh, frame_of, jittered, open_scene, snapshot

pytestmark = pytest.mark.gpu

GEOMETRY_TABLES = tuple(_lib.SCENE_GEOMETRY_TABLES)
F64 = dict(f64=True, f64_book2=True)


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def snapshot_g(ds, frame=True):
    snap = snapshot(ds, frame)
    snap["geometry"] = {t: ds.read_table(t) for t in GEOMETRY_TABLES}
    return snap


_fresh = {}


def fresh_g(sc, frame=True, key=None, **kw):
    """A fresh scene's snapshot; `key` caches it (the unchanged scenes, asked for by several tests)."""
    if key is not None and (key, frame) in _fresh:
        return _fresh[(key, frame)]
    ds = open_scene(sc, **kw)
    snap = snapshot_g(ds, frame)
    ds.close()
    if key is not None:
        _fresh[(key, frame)] = snap
    return snap


def assert_geometry_equal(got, want):
    for t in GEOMETRY_TABLES:
        assert got["geometry"][t].shape == want["geometry"][t].shape, t
        assert got["geometry"][t].tobytes() == want["geometry"][t].tobytes(), f"table {t} differs"


def assert_equals_fresh_g(got, want):
    assert_equals_fresh(got, want)
    assert_geometry_equal(got, want)


def change(ds, how, sc, spheres, quads, lights, **kw):
    getattr(ds, how)(spheres=spheres, motion=sc.motion, quads=quads, lights=lights, **kw)


# ---- 1. update: three updates equal a fresh scene ---------------------------------------------------
CASES = {"NW5": {}, "NW7": {}, "mixed": {}, "mixed_f64": F64, "B3": {}, "multi_light": {}}


@pytest.mark.parametrize("case", list(CASES))
def test_three_updates_equal_fresh(case):
    name, kw = case.split("_f64")[0], CASES[case]
    sc = G.scene(name)
    original = fresh_g(sc, key=case, **kw)
    held = [t for t in GEOMETRY_TABLES if original["geometry"][t].size]
    assert "quad_rows" in held and ("gquads64" if kw else "gquads") in held and ("gquads" in held) != bool(kw)
    assert ("glights" in held) == (sc.lights is not None)
    ds = open_scene(sc, **kw)
    # a jitter, a larger move that changes the tree, back to the original
    steps = [G.moved(sc, 11, 0.01), G.moved(sc, 12, 0.3), (sc.spheres, sc.quads, sc.lights)]
    for step, (spheres, quads, lights) in enumerate(steps):
        new = G.with_geometry(sc, spheres, sc.motion, quads, lights)
        change(ds, "update_geometry", sc, spheres, quads, lights)
        got = snapshot_g(ds)
        want = original if step == 2 else fresh_g(new, **kw)
        assert_equals_fresh_g(got, want)
        assert ds.scene.quads.tobytes() == new.quads.tobytes()
        if step < 2:  # the update did change the scene
            assert got["geometry"]["quad_rows"].tobytes() != original["geometry"]["quad_rows"].tobytes()
            assert got["frame"].tobytes() != original["frame"].tobytes()
            if sc.lights is not None:
                assert got["geometry"]["glights"].tobytes() != original["geometry"]["glights"].tobytes()
            assert got["tree"][0].tobytes() != original["tree"][0].tobytes()
    st = ds.update_stats()
    assert st["updates"] == 3 and st["last_allocations"] == 0
    ds.close()


@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
def test_update_of_300_quads_and_40_spheres(monkeypatch, in_lds):
    # 340 primitives fit the LDS budget; RRT_SCENE_IN_LDS=0 (read at every build) gives the
    # global-memory shape: 32-B nodes, the leaf size of that shape
    if in_lds is not None:
        monkeypatch.setenv("RRT_SCENE_IN_LDS", in_lds)
    sc = G.scene("big")
    assert len(sc.quads) == 300 and len(sc.spheres) == 40  # two 256-lane blocks of quads
    ds = open_scene(sc)
    assert ds.bvh_info()["node_stride"] == (80 if in_lds is None else 32)
    spheres, quads, _ = G.moved(sc, 21, 0.2)
    change(ds, "update_geometry", sc, spheres, quads, None)
    got = snapshot_g(ds)
    ds.close()
    assert_equals_fresh_g(got, fresh_g(G.with_geometry(sc, spheres, None, quads)))


def test_a_material_permutation_changes_prim_mtl():
    sc = G.scene("NW7")
    quads = sc.quads.copy()
    quads["material_index"] = np.roll(quads["material_index"], 5)
    assert not np.array_equal(quads["material_index"], sc.quads["material_index"])
    before = fresh_g(sc, key="NW7")
    ds = open_scene(sc)
    ds.update_geometry(quads=quads)
    got = snapshot_g(ds)
    ds.close()
    assert got["tables"]["prim_mtl"].tobytes() != before["tables"]["prim_mtl"].tobytes()
    assert got["geometry"]["gquads"].tobytes() == before["geometry"]["gquads"].tobytes()
    assert_equals_fresh_g(got, fresh_g(G.with_geometry(sc, quads=quads)))


def test_null_quads_keep_the_scenes_quads():
    sc = G.scene("mixed")
    sp = jittered(sc, 31)
    ds = open_scene(sc)
    ds.update_geometry(spheres=sp, motion=sc.motion)
    got = snapshot_g(ds)
    ds.close()
    assert_equals_fresh_g(got, fresh_g(G.with_geometry(sc, sp, sc.motion)))


# ---- 2. refit ---------------------------------------------------------------------------------------
def twin_refit(built, new, info, f64=False):
    cost = 1.5 if (f64 and info["node_stride"] == 80) else 2.0  # test_gpu_device_bvh.twin_of's node prices
    return refit_bvh_binned(built, new.spheres, new.motion, info["max_leaf_param"], cost, info["node_stride"],
                            new_quads=new.quads)


def assert_refitted(got, built, new, original, want, f64):
    info = original["tree"][2]
    assert got["tree"][2] == info, "a refit changed the info"
    assert_same_tree(got["tree"], twin_refit(built, new, info, f64)[:3])
    assert np.array_equal(got["tree"][1], original["tree"][1]), "a refit changed the leaf order"
    assert_tables_through_kept_order(got, want)
    assert_geometry_equal(got, want)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("case", ["NW5", "NW7", "mixed", "mixed_f64", "B3", "big"])
def test_refit_equals_the_twin_and_a_fresh_scenes_tables(case, form):
    torch = _torch()
    name, kw = case.split("_f64")[0], (F64 if case.endswith("_f64") else {})
    sc = G.scene(name)
    original = fresh_g(sc, key=case, **kw)
    spheres, quads, lights = G.moved(sc, 11, 0.01)
    new = G.with_geometry(sc, spheres, sc.motion, quads, lights)
    want = fresh_g(new, **kw)
    try:
        _lib.refit_form(form)
        ds = open_scene(sc, **kw)
        change(ds, "refit_geometry", sc, sc.spheres, sc.quads, sc.lights)  # the first refit allocates and may wait
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device="cuda:0")
        change(ds, "refit_geometry", sc, spheres, quads, lights, stream_ptr=stream.cuda_stream)
        buf = frame_of(ds, stream)  # enqueued behind the refit: no host synchronisation in between
        stream.synchronize()
        torch.cuda.synchronize()
        st = ds.refit_stats()
        assert st["refits"] == 2 and st["last_form"] == form and st["last_allocations"] == 0
        got = snapshot_g(ds)
        ds.close()
    finally:
        _lib.refit_form(-1)
    assert buf.cpu().numpy().tobytes() == got["frame"].tobytes()
    assert_refitted(got, sc, new, original, want, bool(kw))
    assert got["tree"][0].tobytes() != original["tree"][0].tobytes()
    if kw:  # f64: a fresh scene's frame bit for bit
        assert got["frame"].tobytes() == want["frame"].tobytes() and got["rays"] == want["rays"]
    else:  # f32: the oracle's walk of the refitted tree
        kacc, krays, _ = oracle.render_kbvh(new, got["tree"][0], got["tree"][1], got["tree"][2], threads=16)
        assert np.array_equal(got["frame"], kacc)
        assert got["rays"] == krays


def test_refits_and_updates_interleave_without_allocating():
    sc = G.scene("mixed")
    ds = open_scene(sc)
    original = fresh_g(sc, key="mixed")

    def moved(seed):
        spheres, quads, _ = G.moved(sc, seed, 0.02)
        return spheres, quads, G.with_geometry(sc, spheres, sc.motion, quads)

    sp, q, _ = moved(41)
    ds.refit_geometry(spheres=sp, motion=sc.motion, quads=q)
    assert ds.refit_stats()["last_allocations"] > 0
    for seed in (42, 43):
        sp, q, _ = moved(seed)
        ds.refit_geometry(spheres=sp, motion=sc.motion, quads=q)
        assert ds.refit_stats()["last_allocations"] == 0
    sp44 = jittered(sc, 44)
    ds.refit_spheres(sp44, sc.motion)  # a sphere refit between geometry refits: the quads stay
    assert ds.refit_stats()["last_allocations"] == 0
    new = G.with_geometry(sc, sp44, sc.motion, q)
    got = snapshot_g(ds, frame=False)
    assert_refitted(got, sc, new, original, fresh_g(new, frame=False), False)
    assert ds.tree_cost()["refits_since_build"] == 4
    sp, q, new = moved(45)
    ds.update_geometry(spheres=sp, motion=sc.motion, quads=q)  # the first geometry update: its own reserve
    assert_equals_fresh_g(snapshot_g(ds), fresh_g(new))
    cost = ds.tree_cost()
    assert cost["refits_since_build"] == 0 and cost["sah"] == cost["sah_at_build"]
    sp, q, new = moved(46)
    ds.update_geometry(spheres=sp, motion=sc.motion, quads=q)
    assert ds.update_stats()["last_allocations"] == 0
    built = new  # the tree the refits below keep
    after_update = snapshot_g(ds, frame=False)
    sp, q, new = moved(47)
    ds.refit_geometry(spheres=sp, motion=sc.motion, quads=q)
    assert ds.refit_stats()["last_allocations"] == 0
    got = snapshot_g(ds, frame=False)
    assert_refitted(got, built, new, after_update, fresh_g(new, frame=False), False)
    cost = ds.tree_cost()
    assert cost["refits_since_build"] == 1
    want = twin_refit(built, new, got["tree"][2])[3]
    assert np.float64(cost["sah"]).tobytes() == np.float64(want).tobytes(), (cost, want)
    ds.update_spheres(sc.spheres, sc.motion)  # the sphere update after geometry changes: the quads stay
    assert ds.update_stats()["last_allocations"] == 0
    assert_equals_fresh_g(snapshot_g(ds), fresh_g(G.with_geometry(sc, sc.spheres, sc.motion, q)))
    ds.close()


def test_first_geometry_refit_after_sphere_refits_grows_the_staging_once():
    sc = G.scene("mixed")
    ds = open_scene(sc)
    ds.refit_spheres(jittered(sc, 51), sc.motion)
    ds.refit_spheres(jittered(sc, 52), sc.motion)
    assert ds.refit_stats()["last_allocations"] == 0
    spheres, quads, _ = G.moved(sc, 53, 0.02)
    ds.refit_geometry(spheres=spheres, motion=sc.motion, quads=quads)
    assert ds.refit_stats()["last_allocations"] > 0  # the quads' device rows, the larger pinned buffer
    spheres, quads, _ = G.moved(sc, 54, 0.02)
    ds.refit_geometry(spheres=spheres, motion=sc.motion, quads=quads)
    assert ds.refit_stats()["last_allocations"] == 0
    new = G.with_geometry(sc, spheres, sc.motion, quads)
    got = snapshot_g(ds, frame=False)
    ds.close()
    assert_refitted(got, sc, new, fresh_g(sc, key="mixed"), fresh_g(new, frame=False), False)


def test_one_scene_through_all_three_tiers_equals_the_geometry_entries_alone():
    """Sphere, geometry and world entries on one media-free scene, against a second scene taken through
    the same inputs by the geometry entries alone: every table and the tree bit for bit, and without
    media the world tier needs no more staging than the geometry tier has allocated."""
    sc = G.scene("mixed")
    tiers, plain = open_scene(sc), open_scene(sc)

    def same():
        assert_equals_fresh_g(snapshot_g(tiers, frame=False), snapshot_g(plain, frame=False))
        for t in _lib.SCENE_MEDIA_TABLES:
            assert tiers.read_table(t).tobytes() == plain.read_table(t).tobytes(), f"table {t} differs"
        assert tiers.refit_stats()["last_allocations"] == 0

    sp = jittered(sc, 61)
    tiers.refit_spheres(sp, sc.motion)
    plain.refit_geometry(spheres=sp, motion=sc.motion)
    sp, q, _ = G.moved(sc, 62, 0.02)
    tiers.refit_geometry(spheres=sp, motion=sc.motion, quads=q)
    plain.refit_geometry(spheres=sp, motion=sc.motion, quads=q)
    sp, q, _ = G.moved(sc, 63, 0.02)
    tiers.refit_world(spheres=sp, motion=sc.motion, quads=q, media=None)
    plain.refit_geometry(spheres=sp, motion=sc.motion, quads=q)
    same()
    sp, q, _ = G.moved(sc, 64, 0.3)
    tiers.update_world(spheres=sp, motion=sc.motion, quads=q)
    plain.update_geometry(spheres=sp, motion=sc.motion, quads=q)
    sp = jittered(sc, 65)
    tiers.refit_spheres(sp, sc.motion)
    plain.refit_geometry(spheres=sp, motion=sc.motion)
    same()
    assert tiers.refit_stats()["refits"] == 4 and tiers.update_stats()["updates"] == 1
    tiers.close()
    plain.close()


# ---- 3. refusals ------------------------------------------------------------------------------------
def _geometry_call(entry, **fields):
    """The C entry with an RrtSceneGeometry filled field by field (arrays the caller keeps alive)."""
    def call(ds):
        g = _lib.RrtSceneGeometry()
        sc = ds.scene
        g.spheres, g.n_spheres = (sc.spheres.ctypes.data if len(sc.spheres) else None), len(sc.spheres)
        for k, v in fields.items():
            setattr(g, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        _lib.check(getattr(ds._lib, entry)(ds._h, ctypes.byref(g), None))
    return call


def _refusals(entry):
    how = "update_geometry" if "update" in entry else "refit_geometry"
    c2, nw7, nw9, mixed, b3 = D.scene("C2"), G.scene("NW7"), D.scene("NW9"), G.scene("mixed"), G.scene("B3")
    one = D.first_spheres(1)
    bad_sphere = c2.spheres.copy()
    bad_sphere["material_index"][3] = len(c2.materials)
    motion = np.zeros((len(c2.spheres), 4), np.float32)
    motion[7, 1] = 0.25

    def quads_with(sc, j, **fields):
        q = sc.quads.copy()
        for k, v in fields.items():
            q[k][j] = v
        return q

    textured = int(np.flatnonzero(mixed.materials["kind"] == 3)[0])
    other_kind = b3.lights.copy()
    other_kind["kind"][0] = 1 - other_kind["kind"][0]
    do = lambda **kw: (lambda ds: getattr(ds, how)(**kw))
    on = dict(device_bvh=True)
    return {
        # check_change's list for the sphere entries but for RRT_FLAG_BOOK3
        "sphere_count": (c2, on, do(spheres=c2.spheres[:-1]), "n_spheres"),
        "null_spheres": (c2, on, _geometry_call(entry, spheres=None), "null spheres"),
        "sphere_material": (c2, on, do(spheres=bad_sphere), "material_index"),
        "flag": (c2, dict(device_bvh=False), do(), "RRT_FLAG_DEVICE_BVH"),
        "root_leaf": (one, on, do(), "fewer than 2 primitives"),
        "motion": (c2, on, do(motion=motion), "book-2 world"),
        "null_geometry": (c2, on, lambda ds: _lib.check(getattr(ds._lib, entry)(ds._h, None, None)), "null geometry"),
        # media and boundary quads
        "media": (nw9, on, do(motion=nw9.motion), "media"),
        # counts and kinds
        "quad_count": (nw7, on, do(quads=nw7.quads[:-1]), "n_quads"),
        "light_count": (b3, on, do(lights=b3.lights[:-1]), "n_lights"),
        "light_kind": (b3, on, do(lights=other_kind), "differs from the scene's entry"),
        "lights_missing": (b3, on, _geometry_call(entry), "lights are missing"),
        "lights_on_book2": (nw7, on, do(lights=b3.lights), "lights are given"),
        # quad materials
        "quad_material": (nw7, on, do(quads=quads_with(nw7, 4, material_index=len(nw7.materials))), "material_index out of range"),
        "quad_textured": (mixed, on, do(motion=mixed.motion, quads=quads_with(mixed, 2, material_index=textured)),
                          "image textures on quads"),
        # degenerate quads
        "u_equals_v": (nw7, on, do(quads=quads_with(nw7, 3, v=nw7.quads["u"][3])), "quad 3 is degenerate"),
        "u_zero": (nw7, on, do(quads=quads_with(nw7, 17, u=0.0)), "quad 17 is degenerate"),
        "nan_in_q": (nw7, on, do(quads=quads_with(nw7, 0, q=(np.nan, 0.0, 0.0, 0.0))), "quad 0 is degenerate"),
    }


REFUSALS = ["sphere_count", "null_spheres", "sphere_material", "flag", "root_leaf", "motion", "null_geometry", "media",
            "quad_count", "light_count", "light_kind", "lights_missing", "lights_on_book2", "quad_material",
            "quad_textured", "u_equals_v", "u_zero", "nan_in_q"]


@pytest.mark.parametrize("entry", ["rrt_scene_update_geometry", "rrt_scene_refit_geometry"])
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_the_scene_untouched(case, entry):
    sc, kw, call, reason = _refusals(entry)[case]
    ds = open_scene(sc, **kw)
    before = snapshot_g(ds, frame=False)
    with pytest.raises(rrt.RrtError) as e:
        call(ds)
    assert e.value.code == -1 and reason in str(e.value) and entry in str(e.value), str(e.value)
    after = snapshot_g(ds, frame=False)
    assert ds.update_stats()["updates"] == 0 and ds.refit_stats()["refits"] == 0
    ds.close()
    assert_equals_fresh_g(after, before)


def test_boundary_quads_are_refused_by_name():
    # boundary quads come with media, whose refusal comes first; alone they are refused too:
    # cornell_smoke (the_next_week 8) created without its two media
    nw8 = rrt.next_week_scene(8, D.KW)
    assert nw8.media is not None and nw8.boundary_quads is not None and len(nw8.boundary_quads) == 12
    sc = dataclasses.replace(nw8, media=None)
    ds = open_scene(sc)
    before = snapshot_g(ds, frame=False)
    for how in ("update_geometry", "refit_geometry"):
        with pytest.raises(rrt.RrtError) as e:
            getattr(ds, how)(motion=sc.motion)
        assert e.value.code == -1 and "boundary quads" in str(e.value), str(e.value)
    assert_equals_fresh_g(snapshot_g(ds, frame=False), before)
    ds.close()


def test_update_spheres_on_book3_is_still_refused_with_the_old_message():
    sc = G.scene("B3")
    ds = open_scene(sc)
    for how in ("update_spheres", "refit_spheres"):
        with pytest.raises(rrt.RrtError) as e:
            getattr(ds, how)(sc.spheres)
        assert e.value.code == -1 and "RRT_FLAG_BOOK3 scenes are not updated (their light list restates geometry)" in str(e.value)
    ds.close()


# ---- 4. unchanged paths -----------------------------------------------------------------------------
def test_update_geometry_with_spheres_only_is_update_spheres():
    sc = D.scene("C2")
    sp = jittered(sc, 61, scale=0.3)
    a, b = open_scene(sc), open_scene(sc)
    a.update_geometry(spheres=sp)
    b.update_spheres(sp)
    got, want = snapshot_g(a), snapshot_g(b)
    assert a.update_stats() == b.update_stats()
    a.close(), b.close()
    assert_equals_fresh_g(got, want)
