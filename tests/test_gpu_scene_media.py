"""rrt_scene_update_world and rrt_scene_refit_world on the GPU: scenes with constant media changed in
place.

The yardstick is tests/test_gpu_scene_geometry.py's, extended with the GMedium records: a fresh
DeviceScene(device_bvh=True) of the new inputs. An updated scene holds its bytes everywhere — the
classification of the media (n_unbounded, the tail of the leaf order) included — and renders its frame
with its ray count. A refitted scene keeps the classification and the leaf order of its last build and
holds the tree of the host twin (rrt_refit_bvh_binned_world), the fresh scene's tables gathered through
the kept leaf order, its quad and medium records as they are, and renders the oracle's walk of the
refitted tree read back. No tolerance anywhere. Every refused input is rejected on the host.
Frames are 32 x 18 x 4; book 3 renders its square frame at 4 spp.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd import world as W
from rustraytrace_amd.render import decode_bvh2, refit_bvh_binned_world

import device_bvh_scenes as D
import geometry_scenes as G
import media_scenes as M
from test_gpu_device_bvh import assert_same_tree
from test_gpu_scene_geometry import assert_equals_fresh_g, assert_geometry_equal, snapshot_g
from test_gpu_scene_refit import assert_tables_through_kept_order
from test_gpu_scene_update import frame_of, jittered, open_scene

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def snapshot_w(ds, frame=True):
    snap = snapshot_g(ds, frame)
    snap["gmedia"] = ds.read_table("gmedia")
    return snap


_fresh = {}


def fresh_w(sc, frame=True, key=None):
    """A fresh scene's snapshot; `key` caches it (the unchanged scenes, asked for by several tests)."""
    if key is not None and (key, frame) in _fresh:
        return _fresh[(key, frame)]
    ds = open_scene(sc)
    snap = snapshot_w(ds, frame)
    ds.close()
    if key is not None:
        _fresh[(key, frame)] = snap
    return snap


def assert_equals_fresh_w(got, want):
    assert_equals_fresh_g(got, want)
    assert got["gmedia"].shape == want["gmedia"].shape
    assert got["gmedia"].tobytes() == want["gmedia"].tobytes(), "table gmedia differs"


def n_tree_of(snap):
    """Primitives under the tree read back: the sum of its leaves' counts."""
    nodes, _, info = snap["tree"]
    return int(decode_bvh2(nodes, info["node_stride"])[3].sum())


# ---- 1. update: three updates equal a fresh scene ---------------------------------------------------
@pytest.mark.parametrize("name", ["NW8", "NW9", "B3media", "fog"])
def test_three_updates_equal_fresh(name):
    sc = M.scene(name)
    original = fresh_w(sc, key=name)
    assert original["gmedia"].size == 8 * len(sc.media)
    assert original["geometry"]["quad_rows"].size == 8 * len(sc.quads)  # the source-order tables of a media scene
    ds = open_scene(sc)
    # a jitter, a larger move that changes the tree, back to the original
    for step, new in enumerate([M.moved(sc, 11, 0.01), M.moved(sc, 12, 0.3), sc]):
        M.change(ds, "update_world", new)
        got = snapshot_w(ds)
        want = original if step == 2 else fresh_w(new)
        assert_equals_fresh_w(got, want)
        assert ds.scene.media.tobytes() == new.media.tobytes()
        if step < 2:  # the update did change the scene
            assert got["gmedia"].tobytes() != original["gmedia"].tobytes()
            assert got["tree"][0].tobytes() != original["tree"][0].tobytes()
            assert got["frame"].tobytes() != original["frame"].tobytes()
            assert got["geometry"]["gquads"].tobytes() != original["geometry"]["gquads"].tobytes()
    st = ds.update_stats()
    assert st["updates"] == 3 and st["last_allocations"] == 0
    ds.close()


# ---- 2. the classification flips ----------------------------------------------------------------------
def test_the_classification_flips_both_ways_without_allocating():
    fog = M.scene("fog")
    far, small = M.sphere0_far(fog), M.fog_radius(fog, 1.0)
    n_prims = D.n_prims(fog)
    want = {"fog": fresh_w(fog, key="fog"), "far": fresh_w(far), "small": fresh_w(small)}
    assert [want[k]["tree"][2]["n_unbounded"] for k in ("fog", "far", "small")] == [1, 0, 0]
    ds = open_scene(fog)
    steps = [
        ("far", lambda: ds.update_world(spheres=far.spheres, motion=fog.motion)),  # sphere 0 to x = 60: 1 -> 0
        ("fog", lambda: ds.update_world(spheres=fog.spheres, motion=fog.motion)),  # back: 0 -> 1
        ("small", lambda: ds.update_world(motion=fog.motion, media=small.media)),  # the media argument alone
        ("fog", lambda: ds.update_world(motion=fog.motion, media=fog.media)),
    ]
    for k, (state, call) in enumerate(steps):
        call()
        got = snapshot_w(ds)
        assert_equals_fresh_w(got, want[state])
        unb = want[state]["tree"][2]["n_unbounded"]
        assert ds.bvh_info()["n_unbounded"] == unb and n_tree_of(got) == n_prims - unb  # the tree gains / loses the fog
        if k >= 1:
            assert ds.update_stats()["last_allocations"] == 0
    assert ds.update_stats()["updates"] == 4
    ds.close()


def test_fog5_keeps_four_media_outside_the_tree_through_an_update():
    sc = M.scene("fog5")
    ds = open_scene(sc)
    assert ds.bvh_info()["n_unbounded"] == 4
    new = M.with_world(sc, G.jitter_spheres(sc.spheres, 21, 0.2), sc.motion)
    ds.update_world(spheres=new.spheres, motion=new.motion)
    got = snapshot_w(ds)
    ds.close()
    assert got["tree"][2]["n_unbounded"] == 4 and n_tree_of(got) == D.n_prims(sc) - 4
    first_medium = len(sc.spheres) + len(sc.quads)
    assert list(got["tree"][1][-4:]) == [first_medium + m for m in (2, 3, 4, 5)]
    assert_equals_fresh_w(got, fresh_w(new))


# ---- 3. refit -----------------------------------------------------------------------------------------
def twin_refit(built, new, info):
    return refit_bvh_binned_world(built, new, info["max_leaf_param"], 2.0, info["node_stride"])


def assert_refitted(got, built, new, original, want):
    info = original["tree"][2]
    assert got["tree"][2] == info, "a refit changed the info"
    assert_same_tree(got["tree"], twin_refit(built, new, info)[:3])
    assert np.array_equal(got["tree"][1], original["tree"][1]), "a refit changed the leaf order"
    assert_tables_through_kept_order(got, want)
    assert_geometry_equal(got, want)
    assert got["gmedia"].tobytes() == want["gmedia"].tobytes(), "table gmedia differs"


def assert_renders_the_oracles_walk(got, new):
    """The f32 frame and ray count equal the oracle's walk of the tree read back. A moved book-3 scene
    has NaN sums (the light pdf at a hit point inside a light sphere, tests/test_gpu_book3_scenes.py):
    the same channels are NaN on both sides, and every other channel is equal."""
    kacc, krays, _ = oracle.render_kbvh(new, got["tree"][0], got["tree"][1], got["tree"][2], threads=16)
    nan = np.isnan(kacc)
    assert np.array_equal(np.isnan(got["frame"]), nan)
    assert not nan.any() or new.lights is not None
    assert np.array_equal(got["frame"][~nan], kacc[~nan])
    assert got["rays"] == krays


@pytest.mark.parametrize("name", ["NW8", "NW9", "fog", "B3media"])
def test_refit_equals_the_twin_and_a_fresh_scenes_tables(name):
    torch = _torch()
    sc = M.scene(name)
    original = fresh_w(sc, key=name)
    new = M.moved(sc, 11, 0.01)  # a jitter of everything
    want = fresh_w(new)
    assert want["tree"][2]["n_unbounded"] == original["tree"][2]["n_unbounded"]
    ds = open_scene(sc)
    M.change(ds, "refit_world", sc)  # the first refit allocates and may wait
    assert ds.refit_stats()["last_allocations"] > 0
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device="cuda:0")
    M.change(ds, "refit_world", new, stream_ptr=stream.cuda_stream)
    buf = frame_of(ds, stream)  # enqueued behind the refit: no host synchronisation in between
    stream.synchronize()
    torch.cuda.synchronize()
    st = ds.refit_stats()
    assert st["refits"] == 2 and st["last_allocations"] == 0
    got = snapshot_w(ds)
    cost = ds.tree_cost()
    ds.close()
    assert buf.cpu().numpy().tobytes() == got["frame"].tobytes()
    assert_refitted(got, sc, new, original, want)
    assert got["tree"][0].tobytes() != original["tree"][0].tobytes()
    assert got["gmedia"].tobytes() != original["gmedia"].tobytes()
    assert_renders_the_oracles_walk(got, new)
    sah = twin_refit(sc, new, got["tree"][2])[3]
    assert cost["refits_since_build"] == 2
    assert np.float64(cost["sah"]).tobytes() == np.float64(sah).tobytes(), (cost, sah)


def test_refits_keep_the_classification_compose_and_an_update_restores_it():
    fog = M.scene("fog")
    far = M.sphere0_far(fog)
    original = fresh_w(fog, key="fog")
    ds = open_scene(fog)
    # sphere 0 leaves the fog's sphere: a build would take the fog into the tree, the refit keeps it outside
    ds.refit_world(spheres=far.spheres, motion=fog.motion)
    got = snapshot_w(ds)
    assert got["tree"][2]["n_unbounded"] == 1 and fresh_w(far, frame=False)["tree"][2]["n_unbounded"] == 0
    assert got["tree"][2] == original["tree"][2] and np.array_equal(got["tree"][1], original["tree"][1])
    assert_same_tree(got["tree"], twin_refit(fog, far, got["tree"][2])[:3])
    assert_renders_the_oracles_walk(got, far)
    # a second refit composes: the tree is the twin's of the build and the newest inputs
    new = M.moved(fog, 13, 0.02)
    M.change(ds, "refit_world", new)
    assert ds.refit_stats()["last_allocations"] == 0
    got = snapshot_w(ds)
    assert_refitted(got, fog, new, original, fresh_w(new, frame=False))
    assert_renders_the_oracles_walk(got, new)
    cost = ds.tree_cost()
    assert cost["refits_since_build"] == 2
    assert np.float64(cost["sah"]).tobytes() == np.float64(twin_refit(fog, new, got["tree"][2])[3]).tobytes()
    # the media argument alone, the rest kept
    md = new.media.copy()
    md["sphere"][0, :3] += np.float32(0.3)
    M_new = M.with_world(new, motion=new.motion, media=md)
    ds.refit_world(spheres=new.spheres, motion=new.motion, media=md)
    assert ds.refit_stats()["last_allocations"] == 0
    got = snapshot_w(ds, frame=False)
    assert_refitted(got, fog, M_new, original, fresh_w(M_new, frame=False))
    # a later update: the fresh scene again, the fog in the tree
    M.change(ds, "update_world", far)
    got = snapshot_w(ds)
    assert_equals_fresh_w(got, fresh_w(far))
    cost = ds.tree_cost()
    assert got["tree"][2]["n_unbounded"] == 0 and cost["refits_since_build"] == 0 and cost["sah"] == cost["sah_at_build"]
    # and a refit of that build keeps its classification, with nothing allocated
    back = M.moved(far, 14, 0.02)
    after_update = got
    M.change(ds, "update_world", far)
    assert ds.update_stats()["last_allocations"] == 0
    M.change(ds, "refit_world", back)
    assert ds.refit_stats()["last_allocations"] == 0
    got = snapshot_w(ds, frame=False)
    ds.close()
    assert_refitted(got, far, back, after_update, fresh_w(back, frame=False))


# ---- 4. stream order ------------------------------------------------------------------------------------
def test_refit_world_is_ordered_on_its_stream_without_a_wait():
    torch = _torch()
    sc = M.scene("fog")
    new = M.moved(sc, 81, 0.3)
    old = fresh_w(sc, key="fog")
    ds = open_scene(sc)
    M.change(ds, "refit_world", sc)  # the first refit allocates and may wait; the ones below do neither
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device="cuda:0")
    first = frame_of(ds, stream)
    rows = {k: getattr(new, k).copy() for k in ("spheres", "quads", "media", "boundary_quads")}
    ds.refit_world(spheres=rows["spheres"], motion=new.motion, quads=rows["quads"], media=rows["media"],
                   boundary_quads=rows["boundary_quads"], stream_ptr=stream.cuda_stream)
    for a in rows.values():  # the caller's arrays are free as soon as the call returns
        a.view(np.uint8)[:] = 0
    second = frame_of(ds, stream)
    stream.synchronize()
    torch.cuda.synchronize()
    assert ds.refit_stats()["last_allocations"] == 0
    after, _ = frame_of(ds)  # the refitted scene's frame, taken afterwards
    ds.close()
    assert first.cpu().numpy().tobytes() == old["frame"].tobytes()
    assert second.cpu().numpy().tobytes() == after.tobytes()
    assert after.tobytes() != old["frame"].tobytes()


# ---- 5. media=None keeps the media ----------------------------------------------------------------------
def test_null_media_keep_the_scenes_media():
    sc = M.scene("NW9")
    sp = jittered(sc, 31)
    ds = open_scene(sc)
    ds.update_world(spheres=sp, motion=sc.motion)
    got = snapshot_w(ds)
    ds.close()
    assert_equals_fresh_w(got, fresh_w(M.with_world(sc, sp, sc.motion)))
    assert got["gmedia"].tobytes() == fresh_w(sc, key="NW9")["gmedia"].tobytes()


def test_boundary_quads_without_media_are_accepted_and_re_formed():
    # cornell_smoke (the_next_week 8) created without its two media: 12 boundary quads no medium names
    nw8 = M.scene("NW8")
    sc = dataclasses.replace(nw8, media=None)
    new = M.moved(sc, 41, 0.05)
    assert new.media is None and new.boundary_quads.tobytes() != sc.boundary_quads.tobytes()
    original = fresh_w(sc)
    assert original["gmedia"].size == 0
    n_quads = len(sc.quads)
    ds = open_scene(sc)
    ds.update_world(motion=sc.motion, quads=new.quads, boundary_quads=new.boundary_quads)
    got = snapshot_w(ds)
    assert_equals_fresh_w(got, fresh_w(new))
    mine = got["geometry"]["gquads"].view(_lib.GQUAD_DTYPE)[n_quads:]
    assert mine.tobytes() == _lib.quad_records(new.boundary_quads)[1].tobytes()  # they follow the new rows
    assert mine.tobytes() != original["geometry"]["gquads"].view(_lib.GQUAD_DTYPE)[n_quads:].tobytes()
    ds.refit_world(motion=sc.motion, boundary_quads=sc.boundary_quads)  # and the refit puts the old ones back
    back = snapshot_w(ds, frame=False)
    ds.close()
    assert back["geometry"]["gquads"].view(_lib.GQUAD_DTYPE)[n_quads:].tobytes() == \
        original["geometry"]["gquads"].view(_lib.GQUAD_DTYPE)[n_quads:].tobytes()


def test_a_scene_without_media_takes_the_world_entries_like_the_geometry_ones():
    sc = G.scene("NW7")
    spheres, quads, _ = G.moved(sc, 11, 0.05)
    a, b = open_scene(sc), open_scene(sc)
    a.update_world(spheres=spheres, quads=quads)
    b.update_geometry(spheres=spheres, quads=quads)
    got, want = snapshot_w(a), snapshot_w(b)
    assert a.update_stats() == b.update_stats()
    a.close(), b.close()
    assert_equals_fresh_w(got, want)


# ---- 6. refusals ------------------------------------------------------------------------------------------
def _world_call(entry, media=None, **fields):
    """The C entry with an RrtSceneGeometry (and RrtSceneMedia) filled field by field (arrays the
    caller keeps alive)."""
    def call(ds):
        g = _lib.RrtSceneGeometry()
        sc = ds.scene
        g.spheres, g.n_spheres = (sc.spheres.ctypes.data if len(sc.spheres) else None), len(sc.spheres)
        if sc.motion is not None:
            g.sphere_motion = sc.motion.ctypes.data
        for k, v in fields.items():
            setattr(g, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        wm = None
        if media is not None:
            wm = _lib.RrtSceneMedia()
            for k, v in media.items():
                setattr(wm, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        _lib.check(getattr(ds._lib, entry)(ds._h, ctypes.byref(g), None if wm is None else ctypes.byref(wm), None))
    return call


@pytest.fixture(scope="module")
def lonely():
    """One sphere and two small sphere media: a tree of three primitives which two all-holding media would
    leave with one."""
    white = W.Lambertian((0.7, 0.7, 0.7))
    objs = [W.Sphere((0.0, 0.0, 0.0), 0.5, white),
            W.ConstantMedium(W.Sphere((1.5, 0.0, 0.0), 0.4, white), 0.5, (0.9, 0.9, 0.9)),
            W.ConstantMedium(W.Sphere((-1.5, 0.0, 0.0), 0.4, white), 0.5, (0.9, 0.9, 0.9))]
    cam = W.Camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=40.0,
                   lookfrom=(0.0, 1.0, 8.0), lookat=(0.0, 0.0, 0.0))
    return W.build(W.HittableList(objs), cam, book=2, seed=7, name="lonely")


def _refusals(entry):
    how = "update_world" if "update" in entry else "refit_world"
    c2, nw7, mixed, b3, fog = D.scene("C2"), G.scene("NW7"), G.scene("mixed"), M.scene("B3media"), M.scene("fog")
    one = D.first_spheres(1)
    bad_sphere = fog.spheres.copy()
    bad_sphere["material_index"][3] = len(fog.materials)
    motion = np.zeros((len(c2.spheres), 4), np.float32)
    motion[7, 1] = 0.25

    def quads_with(sc, j, **fields):
        q = sc.quads.copy()
        for k, v in fields.items():
            q[k][j] = v
        return q

    def media_with(m, **fields):
        md = fog.media.copy()
        for k, v in fields.items():
            md[k][m] = v
        return md

    def bquads_with(j, **fields):
        q = fog.boundary_quads.copy()
        for k, v in fields.items():
            q[k][j] = v
        return q

    textured = int(np.flatnonzero(mixed.materials["kind"] == 3)[0])
    lambertian = int(np.flatnonzero(fog.materials["kind"] != 7)[0])
    other_kind = b3.lights.copy()
    other_kind["kind"][0] = 1 - other_kind["kind"][0]
    do = lambda **kw: (lambda ds: getattr(ds, how)(**{"motion": ds.scene.motion, **kw}))
    on = dict(device_bvh=True)
    return {
        # what the geometry entries refuse, but for media and boundary quads
        "sphere_count": (fog, on, do(spheres=fog.spheres[:-1], motion=None), "n_spheres"),
        "null_spheres": (fog, on, _world_call(entry, spheres=None), "null spheres"),
        "sphere_material": (fog, on, do(spheres=bad_sphere), "material_index"),
        "flag": (fog, dict(device_bvh=False), do(), "RRT_FLAG_DEVICE_BVH"),
        "root_leaf": (one, on, do(), "fewer than 2 primitives"),
        "motion": (c2, on, do(motion=motion), "book-2 world"),
        "motion_f64": (c2, dict(device_bvh=True, f64=True), do(motion=motion), "book-2 world"),
        "null_geometry": (fog, on, lambda ds: _lib.check(getattr(ds._lib, entry)(ds._h, None, None, None)), "null geometry"),
        "quad_count": (fog, on, do(quads=fog.quads[:-1]), "n_quads"),
        "light_count": (b3, on, do(lights=b3.lights[:-1]), "n_lights"),
        "light_kind": (b3, on, do(lights=other_kind), "differs from the scene's entry"),
        "lights_missing": (b3, on, _world_call(entry), "lights are missing"),
        "lights_on_book2": (fog, on, do(lights=b3.lights), "lights are given"),
        "quad_material": (fog, on, do(quads=quads_with(fog, 2, material_index=len(fog.materials))), "material_index out of range"),
        "quad_textured": (mixed, on, do(quads=quads_with(mixed, 2, material_index=textured)), "image textures on quads"),
        "quad_u_zero": (nw7, on, do(quads=quads_with(nw7, 17, u=0.0)), "quad 17 is degenerate"),
        "quad_nan": (fog, on, do(quads=quads_with(fog, 0, q=(np.nan, 0.0, 0.0, 0.0))), "quad 0 is degenerate"),
        # the media's own
        "media_count": (fog, on, do(media=fog.media[:-1]), "n_media is 2"),
        "bquad_count": (fog, on, do(boundary_quads=fog.boundary_quads[:-1]), "n_boundary_quads is 5"),
        "medium_kind": (fog, on, do(media=media_with(0, boundary_kind=1)), "medium 0: boundary_kind, first or count"),
        "medium_first": (fog, on, do(media=media_with(1, first=1)), "medium 1: boundary_kind, first or count"),
        "medium_count": (fog, on, do(media=media_with(1, count=5)), "medium 1: boundary_kind, first or count"),
        "medium_material_range": (fog, on, do(media=media_with(2, material_index=len(fog.materials))),
                                  "medium 2: material_index must name an RRT_MAT_ISOTROPIC material"),
        "medium_material_kind": (fog, on, do(media=media_with(0, material_index=lambertian)),
                                 "medium 0: material_index must name an RRT_MAT_ISOTROPIC material"),
        "density_zero": (fog, on, do(media=media_with(1, density=0.0)), "medium 1: density must be positive and finite"),
        "density_negative": (fog, on, do(media=media_with(0, density=-0.5)), "medium 0: density must be positive and finite"),
        "density_inf": (fog, on, do(media=media_with(2, density=np.inf)), "medium 2: density must be positive and finite"),
        "density_nan": (fog, on, do(media=media_with(2, density=np.nan)), "medium 2: density must be positive and finite"),
        "medium_sphere_nan": (fog, on, do(media=media_with(0, sphere=(0.0, np.nan, 0.0, 1.0))), "medium 0: the sphere row must be finite"),
        "medium_radius_inf": (fog, on, do(media=media_with(2, sphere=(0.0, 0.0, 0.0, np.inf))), "medium 2: the sphere row must be finite"),
        "bquad_u_equals_v": (fog, on, do(boundary_quads=bquads_with(3, v=fog.boundary_quads["u"][3])), "boundary quad 3 is degenerate"),
        "bquad_nan": (fog, on, do(boundary_quads=bquads_with(5, q=(0.0, 0.0, np.nan, 0.0))), "boundary quad 5 is degenerate"),
    }


REFUSALS = ["sphere_count", "null_spheres", "sphere_material", "flag", "root_leaf", "motion", "motion_f64", "null_geometry",
            "quad_count", "light_count", "light_kind", "lights_missing", "lights_on_book2", "quad_material", "quad_textured",
            "quad_u_zero", "quad_nan", "media_count", "bquad_count", "medium_kind", "medium_first", "medium_count",
            "medium_material_range", "medium_material_kind", "density_zero", "density_negative", "density_inf",
            "density_nan", "medium_sphere_nan", "medium_radius_inf", "bquad_u_equals_v", "bquad_nan"]


@pytest.mark.parametrize("entry", ["rrt_scene_update_world", "rrt_scene_refit_world"])
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_the_scene_untouched(case, entry):
    sc, kw, call, reason = _refusals(entry)[case]
    f64 = bool(kw.get("f64"))
    ds = open_scene(sc, **kw)
    before = snapshot_w(ds, frame=False)
    with pytest.raises(rrt.RrtError) as e:
        call(ds)
    assert e.value.code == -1 and reason in str(e.value) and entry in str(e.value), str(e.value)
    after = snapshot_w(ds, frame=False)
    assert ds.update_stats()["updates"] == 0 and ds.refit_stats()["refits"] == 0
    assert ds.f64 == f64
    ds.close()
    assert_equals_fresh_w(after, before)


def test_a_classification_that_leaves_a_tree_of_one_is_refused_by_the_update(lonely):
    md = lonely.media.copy()
    md["sphere"][:] = (0.0, 0.0, 0.0, 100.0)  # each holds the other and the sphere: both would leave the tree
    ds = open_scene(lonely)
    before = snapshot_w(ds, frame=False)
    assert before["tree"][2]["n_unbounded"] == 0
    with pytest.raises(rrt.RrtError) as e:
        ds.update_world(motion=lonely.motion, media=md)
    assert e.value.code == -1 and "rrt_scene_update_world" in str(e.value), str(e.value)
    assert "fewer than 2 primitives in the tree" in str(e.value)
    assert ds.update_stats()["updates"] == 0
    assert_equals_fresh_w(snapshot_w(ds, frame=False), before)
    # a refit classifies nothing: it keeps both in the tree and accepts the rows
    ds.refit_world(motion=lonely.motion, media=md)
    got = snapshot_w(ds)
    ds.close()
    new = M.with_world(lonely, motion=lonely.motion, media=md)
    assert got["tree"][2]["n_unbounded"] == 0
    assert_same_tree(got["tree"], twin_refit(lonely, new, got["tree"][2])[:3])
    assert_renders_the_oracles_walk(got, new)


def test_the_older_entries_still_refuse_media_with_their_messages():
    sc = M.scene("fog")
    ds = open_scene(sc)
    for how in ("update_spheres", "refit_spheres"):
        with pytest.raises(rrt.RrtError) as e:
            getattr(ds, how)(sc.spheres, sc.motion)
        assert "scenes with constant media are not updated" in str(e.value)
    for how in ("update_geometry", "refit_geometry"):
        with pytest.raises(rrt.RrtError) as e:
            getattr(ds, how)(motion=sc.motion)
        assert "scenes with constant media are not updated" in str(e.value)
    ds.close()
