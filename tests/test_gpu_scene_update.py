"""rrt_scene_set_camera and rrt_scene_update_spheres on the GPU.

The yardstick throughout is a fresh DeviceScene(..., device_bvh=True) of the new inputs: an updated
scene must hold the same node bytes, leaf order and info, the same bytes in every per-primitive table
(the boxes too: the fresh scene's are formed on the host, the updated scene's on the device), and
render the same frame with the same ray count. No tolerance anywhere: everything is compared as
bytes. Frames are 32x18x4 unless a test says otherwise.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S

import books64_book2_scenes as B
import device_bvh_scenes as D
from test_gpu_device_bvh import assert_same_tree, scale_scene, twin_of

pytestmark = pytest.mark.gpu

TABLES = tuple(_lib.SCENE_TABLES)


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def frame_of(ds, stream=None):
    """The scene's whole frame and its ray count, rendered now (or enqueued on `stream`: the buffer)."""
    torch = _torch()
    sc = ds.scene
    f64 = bool(ds.f64)
    tile = ds.tile(16, 0, 1, 0, sc.spp)
    buf = torch.full((ds.tile_rows(tile), sc.width, 4), float("nan"), dtype=torch.float64 if f64 else torch.float32,
                     device="cuda:0")
    render = ds.render_tile_f64_async if f64 else ds.render_tile_async
    if stream is not None:
        render(tile, buf.data_ptr(), stream.cuda_stream)
        return buf
    ds.reset_counters()
    render(tile, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), int(ds.counters()["rays"])


def open_scene(sc, device_bvh=True, **kw):
    ds = rrt.DeviceScene(sc, device=0, device_bvh=device_bvh, **kw)
    ds.f64 = bool(kw.get("f64") or kw.get("f64_book2"))
    return ds


def snapshot(ds, frame=True):
    snap = {"tree": ds.read_bvh(), "tables": {t: ds.read_table(t) for t in TABLES}}
    if frame:
        snap["frame"], snap["rays"] = frame_of(ds)
    return snap


def fresh(sc, frame=True, **kw):
    ds = open_scene(sc, **kw)
    snap = snapshot(ds, frame)
    ds.close()
    return snap


def assert_equals_fresh(got, want):
    assert got["tree"][2] == want["tree"][2], "info dict differs"
    assert_same_tree(got["tree"], want["tree"])
    for t in TABLES:
        assert got["tables"][t].shape == want["tables"][t].shape, t
        assert got["tables"][t].tobytes() == want["tables"][t].tobytes(), f"table {t} differs"
    if "frame" in want:
        assert got["frame"].shape == want["frame"].shape
        assert got["frame"].tobytes() == want["frame"].tobytes(), "frame differs"
        assert got["rays"] == want["rays"]


def with_spheres(sc, spheres, motion=None):
    return dataclasses.replace(sc, spheres=np.ascontiguousarray(spheres), motion=motion)


def jittered(sc, seed, scale=0.05):
    """A seeded jitter of the centers plus a permutation of material_index."""
    rng = np.random.default_rng(seed)
    sp = sc.spheres.copy()
    sp["center_radius"][:, :3] += rng.normal(0.0, scale, (len(sp), 3)).astype(np.float32)
    sp["material_index"] = rng.permutation(sp["material_index"])
    return sp


# ---- 1. f32 book 1 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,stride", [("spheres64", 80), ("C2", None), ("C5", 32)])
def test_three_updates_equal_fresh_f32(name, stride):
    sc = D.scene(name)
    original = fresh(sc)
    assert stride is None or original["tree"][2]["node_stride"] == stride  # the LDS shape and the global one
    ds = open_scene(sc)
    for step, spheres in enumerate([jittered(sc, 11), jittered(sc, 12, scale=0.4), sc.spheres]):
        new = with_spheres(sc, spheres)
        ds.update_spheres(spheres)
        got = snapshot(ds)
        want = original if step == 2 else fresh(new)
        assert_equals_fresh(got, want)
        assert_same_tree(got["tree"], twin_of(new, got["tree"][2]))
        if step < 2:  # the update did change the scene
            assert got["tables"]["prim_cr"].tobytes() != original["tables"]["prim_cr"].tobytes()
            assert got["frame"].tobytes() != original["frame"].tobytes()
    assert ds.update_stats()["updates"] == 3
    ds.close()


# ---- 2. shape change without a size change ----------------------------------------------------
def test_tree_shape_changes_both_ways():
    spread = D.scene("big_among_small")
    assert len(spread.spheres) == 201
    together = spread.spheres.copy()
    together["center_radius"][:] = (3.0, 1.0, -2.0, 0.25)
    clumped = with_spheres(spread, together)
    want = {"spread": fresh(spread), "clumped": fresh(clumped)}
    a, b = want["spread"]["tree"][2], want["clumped"]["tree"][2]
    assert a["n_nodes"] != b["n_nodes"] and a["max_depth"] != b["max_depth"]
    for first in ("spread", "clumped"):  # either tree may be the larger previous one
        ds = open_scene(spread if first == "spread" else clumped)
        other = "clumped" if first == "spread" else "spread"
        for step in (other, first, other):
            ds.update_spheres(together if step == "clumped" else spread.spheres)
            assert_equals_fresh(snapshot(ds), want[step])
        ds.close()


# ---- 3. edge radii ----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"f64": True}], ids=["f32", "f64"])
def test_zero_and_negative_radius(kw):
    sc = D.scene("spheres64")
    sp = sc.spheres.copy()
    sp["center_radius"][5, 3] = 0.0
    sp["center_radius"][9, 3] = -0.5
    sp["center_radius"][11, 3] = -0.0
    ds = open_scene(sc, **kw)
    ds.update_spheres(sp)
    got, want = snapshot(ds), fresh(with_spheres(sc, sp), **kw)
    ds.close()
    assert_equals_fresh(got, want)
    if not kw:  # the book-1 layout carries r * r and, in b.w, 1 / r = +inf at r = 0
        order = got["tree"][1]
        row = int(np.flatnonzero(order == 5)[0])
        assert got["tables"]["prim_cr"].reshape(-1, 4)[row, 3] == 0.0
        assert got["tables"]["prim_mtl"].reshape(-1, 8)[row, 7] == 0x7F800000


# ---- 4. book 2, f32 ---------------------------------------------------------------------------
def moved_nw1(sc, seed):
    rng = np.random.default_rng(seed)
    sp = jittered(sc, seed)
    motion = (sc.motion * np.float32(0.5)).astype(np.float32)
    motion[:, :3] += np.where(sc.motion[:, :3] != 0, rng.normal(0, 0.02, (len(sp), 3)), 0.0).astype(np.float32)
    assert np.any(motion[:, :3] != 0)
    return sp, motion


def test_book2_moving_spheres():
    sc = D.scene("NW1")
    assert sc.motion is not None
    ds = open_scene(sc)
    for seed in (21, 22):
        sp, motion = moved_nw1(sc, seed)
        ds.update_spheres(sp, motion)
        assert_equals_fresh(snapshot(ds), fresh(with_spheres(sc, sp, motion)))
    ds.update_spheres(sc.spheres, sc.motion)
    assert_equals_fresh(snapshot(ds), fresh(sc))
    ds.close()


def quads_and_spheres():
    """Three quads (two with NW1's checker material) and 20 spheres over four materials."""
    nw1 = D.scene("NW1")
    checker = nw1.materials[np.flatnonzero(nw1.materials["kind"] == 5)[:1]]
    mats = np.concatenate([checker, S._material(0, (0.6, 0.3, 0.2)), S._material(1, (0.8, 0.8, 0.9), fuzz=0.1),
                           S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5)])
    rng = np.random.default_rng(31)
    sph = np.concatenate([S._sphere((rng.uniform(-4, 4), rng.uniform(0.3, 2.0), rng.uniform(-4, 4)),
                                    rng.uniform(0.2, 0.6), 1 + k % 3) for k in range(20)])
    quads = np.concatenate([B._quad((-6, 0, -6), (12, 0, 0), (0, 0, 12), 0), B._quad((-6, 0, -6), (12, 0, 0), (0, 6, 0), 0),
                            B._quad((-6, 0, -6), (0, 0, 12), (0, 6, 0), 1)])
    cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=40.0,
                        lookfrom=(5.0, 4.0, 12.0), lookat=(0.0, 1.0, 0.0), n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, flags=nw1.flags, name="quads_and_spheres", quads=quads)


def test_book2_quads_keep_their_rows():
    sc = quads_and_spheres()
    n = len(sc.spheres)
    ds = open_scene(sc)
    before = snapshot(ds)
    sp = jittered(sc, 32, scale=0.3)
    ds.update_spheres(sp)
    got = snapshot(ds)
    ds.close()
    assert_equals_fresh(got, fresh(with_spheres(sc, sp)))
    assert got["tables"]["prim_motion"].size, "a book-2 world holds motion rows"
    for t in TABLES:
        if not got["tables"][t].size:
            continue
        for j in range(len(sc.quads)):
            rows = []
            for snap in (before, got):
                table = snap["tables"][t].reshape(n + len(sc.quads), -1)
                at = j + n if t == "boxes" else int(np.flatnonzero(snap["tree"][1] == n + j)[0])
                rows.append(table[at].tobytes())
            assert rows[0] == rows[1], f"quad {j}'s row of {t} changed"


# ---- 5. f64 -----------------------------------------------------------------------------------
def _mixed32():
    return B.mixed_scene(rrt.next_week_scene(1, D.KW))


@pytest.mark.parametrize("name", ["spheres64", "C5", "mixed"])
def test_f64_update_equals_fresh_and_books(name):
    sc = _mixed32() if name == "mixed" else D.scene(name)
    kw = dict(f64=True, f64_book2=True) if name == "mixed" else dict(f64=True)
    ds = open_scene(sc, **kw)
    if name == "mixed":
        sp, motion = moved_nw1(sc, 41)
    else:
        sp, motion = jittered(sc, 41), None
    new = with_spheres(sc, sp, motion)
    ds.update_spheres(sp, motion)
    got = snapshot(ds)
    ds.close()
    assert_equals_fresh(got, fresh(new, **kw))
    assert got["tables"]["prim_inv_r64"].size and got["tables"]["prim_diel64"].size
    books, books_rays, _ = oracle.render(new, oracle.BOOKS, threads=16)  # BOOKS reads no tree
    assert np.array_equal(got["frame"], books)
    assert got["rays"] == books_rays


# ---- 6. scale ---------------------------------------------------------------------------------
def test_update_at_1e5_spheres():
    sc = scale_scene()  # 32 wide, 1 spp
    sp = jittered(sc, 51)
    new = with_spheres(sc, sp)
    ds = open_scene(sc)
    ds.update_spheres(sp)
    got = snapshot(ds)
    ds.close()
    assert got["tree"][2]["node_stride"] == 32
    assert_same_tree(got["tree"], twin_of(new, got["tree"][2]))
    assert_equals_fresh(got, fresh(new))


# ---- 7. no steady-state allocation ------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C5", "NW1"])
def test_second_update_allocates_nothing(name):
    sc = D.scene(name)
    ds = open_scene(sc)
    assert ds.update_stats() == {"updates": 0, "last_allocations": 0, "last_levels": 0}
    motion = sc.motion
    ds.update_spheres(jittered(sc, 61), motion)
    first = ds.update_stats()
    assert first["updates"] == 1 and first["last_allocations"] > 0 and first["last_levels"] > 0
    for seed in (62, 63):  # other spheres, another tree
        ds.update_spheres(jittered(sc, seed, scale=0.5), motion)
        assert ds.update_stats()["last_allocations"] == 0
    assert ds.update_stats()["updates"] == 3
    ds.close()


# ---- 8. camera --------------------------------------------------------------------------------
def _b3(**ov):
    return rrt.rest_of_your_life_scene(dict(D.KW, **ov))


CAMERA_CASES = {
    "C2": (lambda **ov: rrt.build_in_one_weekend_scene({**D.KW, "max_depth": 100, **ov}), dict(device_bvh=True),
           (10.0, 3.0, 5.0)),
    "C2_f64": (lambda **ov: rrt.build_in_one_weekend_scene({**D.KW, "max_depth": 100, **ov}),
               dict(device_bvh=True, f64=True), (10.0, 3.0, 5.0)),
    "NW9": (lambda **ov: rrt.next_week_scene(9, dict(D.KW, **ov)), dict(device_bvh=False), (400.0, 300.0, -500.0)),
    "B3": (_b3, dict(device_bvh=False), (278.0, 300.0, -700.0)),
}


@pytest.mark.parametrize("name", list(CAMERA_CASES))
def test_set_camera_equals_fresh(name):
    build, kw, lookfrom = CAMERA_CASES[name]
    ds = open_scene(build(), **kw)
    for ov in (dict(lookfrom=lookfrom, max_depth=7), dict(lookfrom=lookfrom, max_depth=7, image_width=48)):
        new = build(**ov)
        new.camera["params_u"][0, 1] = 0xC0FFEE  # another seed
        ds.set_camera(new.camera)
        assert (ds.scene.width, ds.scene.height) == (new.width, new.height)
        assert_equals_fresh(snapshot(ds), fresh(new, **kw))
    ds.close()


def test_set_camera_refuses_a_non_square_spp_on_book3():
    sc = _b3()
    ds = open_scene(sc, device_bvh=False)
    before = frame_of(ds)
    cam = _b3(lookfrom=(278.0, 300.0, -700.0)).camera
    cam["params_f"][0, 3] = 5.0
    with pytest.raises(rrt.RrtError) as e:
        ds.set_camera(cam)
    assert e.value.code == -1 and "square" in str(e.value)
    after = frame_of(ds)
    ds.close()
    assert before[0].tobytes() == after[0].tobytes() and before[1] == after[1]


def test_set_camera_then_update_spheres():
    sc = D.scene("C2")
    new_cam = rrt.build_in_one_weekend_scene(dict(D.KW, max_depth=9, lookfrom=(9.0, 4.0, 6.0))).camera
    sp = jittered(sc, 71)
    ds = open_scene(sc)
    ds.set_camera(new_cam)
    ds.update_spheres(sp)
    got = snapshot(ds)
    ds.close()
    assert_equals_fresh(got, fresh(dataclasses.replace(sc, camera=new_cam, spheres=sp)))


# ---- 9. refusals ------------------------------------------------------------------------------
def _refusals():
    c2 = D.scene("C2")
    bad_index = c2.spheres.copy()
    bad_index["material_index"][3] = len(c2.materials)
    motion = np.zeros((len(c2.spheres), 4), np.float32)
    motion[7, 1] = 0.25
    one = D.first_spheres(1)
    return {
        "count": (c2, dict(device_bvh=True), lambda ds: ds.update_spheres(c2.spheres[:-1]), "n_spheres"),
        "null": (c2, dict(device_bvh=True),
                 lambda ds: _lib.check(ds._lib.rrt_scene_update_spheres(ds._h, None, len(c2.spheres), None, None)), "null spheres"),
        "material": (c2, dict(device_bvh=True), lambda ds: ds.update_spheres(bad_index), "material_index"),
        "flag": (c2, dict(device_bvh=False), lambda ds: ds.update_spheres(c2.spheres), "RRT_FLAG_DEVICE_BVH"),
        "media": (D.scene("NW9"), dict(device_bvh=True),
                  lambda ds: ds.update_spheres(D.scene("NW9").spheres, D.scene("NW9").motion), "media"),
        "book3": (_b3(), dict(device_bvh=True), lambda ds: ds.update_spheres(ds.scene.spheres), "RRT_FLAG_BOOK3"),
        "root_leaf": (one, dict(device_bvh=True), lambda ds: ds.update_spheres(one.spheres), "fewer than 2 primitives"),
        "motion": (c2, dict(device_bvh=True), lambda ds: ds.update_spheres(c2.spheres, motion), "book-2 world"),
    }


@pytest.mark.parametrize("case", ["count", "null", "material", "flag", "media", "book3", "root_leaf", "motion"])
def test_refusals_leave_the_scene_untouched(case):
    sc, kw, call, reason = _refusals()[case]
    ds = open_scene(sc, **kw)
    before = snapshot(ds)
    with pytest.raises(rrt.RrtError) as e:
        call(ds)
    assert e.value.code == -1 and reason in str(e.value), str(e.value)
    after = snapshot(ds)
    assert ds.update_stats()["updates"] == 0
    ds.close()
    assert_equals_fresh(after, before)


# ---- 10. ordering -----------------------------------------------------------------------------
def test_update_is_ordered_after_the_streams_work():
    torch = _torch()
    sc = D.scene("C2")
    sp = jittered(sc, 81, scale=0.5)
    old, new = fresh(sc), fresh(with_spheres(sc, sp))
    assert old["frame"].tobytes() != new["frame"].tobytes()
    ds = open_scene(sc)
    stream = torch.cuda.Stream(device="cuda:0")
    first = frame_of(ds, stream)
    ds.update_spheres(sp, stream_ptr=stream.cuda_stream)
    second = frame_of(ds, stream)
    stream.synchronize()
    torch.cuda.synchronize()
    ds.close()
    assert first.cpu().numpy().tobytes() == old["frame"].tobytes()
    assert second.cpu().numpy().tobytes() == new["frame"].tobytes()
