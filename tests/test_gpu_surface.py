"""Surface records of a created scene (rrt_scene_surface_async, rrt_scene_surface,
rrt_scene_primary_surface_async) against tests/surface_cases.py.

Two questions. Which primitive the walk answers: on the scenes the plain query accepts, the query's own
answer bit for bit; on scenes with constant media, the linear scan of their surfaces alone
(ray_query_cases.check_hits) and the same scene created without its media. What the record says about
that primitive: surface_cases.expected from the reported (prim, t), every field of every ray bit for bit,
the misses and the padding too. No tolerance anywhere.
"""
import os

import numpy as np
import pytest

import rustraytrace_amd as rrt
from rustraytrace_amd import _lib
from oracle import oracle

import book2_class_scenes as B
import ray_query_cases as Q
import surface_cases as SC
from test_gpu_scene_update import frame_of, open_scene

pytestmark = pytest.mark.gpu

NO, MISS = _lib.NO_PRIM, _lib.SURFACE_MISS
PLACEMENTS = {"lds": None, "global": "0"}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_open = {}


def device_scene(name, placement="lds", **kw):
    """The scene `name` (surface_cases.scene; "<name>-media": without its media) on the device, created
    once per (name, placement, flags) under the placement's RRT_SCENE_IN_LDS; closed with the module."""
    flags = dict(kw)
    device_bvh = flags.pop("device_bvh", False)
    key = (name, placement, device_bvh, tuple(sorted(flags.items())))
    if key not in _open:
        sc = B.without_media(SC.scene(name[:-6])) if name.endswith("-media") else SC.scene(name)
        old = os.environ.pop("RRT_SCENE_IN_LDS", None)
        try:
            if PLACEMENTS[placement] is not None:
                os.environ["RRT_SCENE_IN_LDS"] = PLACEMENTS[placement]
            ds = open_scene(sc, device_bvh=device_bvh, **flags)
        finally:
            os.environ.pop("RRT_SCENE_IN_LDS", None)
            if old is not None:
                os.environ["RRT_SCENE_IN_LDS"] = old
        stride = ds.bvh_info()["node_stride"]
        if placement == "global":
            assert stride == 32, (name, stride)
        elif name in BOTH and not device_bvh:  # staged: the two placements of these scenes run different kernels
            # (the device builders' trees of RTOW need not fit the staging budget: they run as created)
            assert stride == 80, (name, stride)
        _open[key] = ds
    return _open[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _open.values():
        ds.close()
    _open.clear()


def n_prims(name):
    return Q.geometry(SC.scene(name)).n_prims


# Every case in its placements. The existing cases as tests/test_gpu_ray_query.py places them, and the
# tiny trees and book 3 read from global memory too; the bouncing spheres and the_next_week 10 are past
# the staging budget and read from global memory whatever is asked (one placement, as created).
BOTH = ("rtow", "comp1", "comp2", "one_sphere", "two_spheres", "quad_sphere", "book3", "comp1n", "earth", "comp3n")
AS_CREATED = ("nw1", "wide1", "final10")
OLD = [(n, s, t) for n, s, t in Q.CASES if n != "rtow_moved"]
PLACED = [(n, s, t, p) for n, s, t in OLD + SC.NEW_CASES for p in (("lds", "global") if n in BOTH else ("lds",))]
PLACED_IDS = [f"{n}-{s}-{t:.2f}-{p}" for n, s, t, p in PLACED]
MEDIA = {n for n, _, _ in SC.MEDIA_CASES}

_answers = {}


def answers(name, ray_set, time, placement):
    """surface() of a case, once per module."""
    key = (name, ray_set, time, placement)
    if key not in _answers:
        got = device_scene(name, placement).surface(SC.rays(name, ray_set, time))
        got.setflags(write=False)
        _answers[key] = got
    return _answers[key]


def as_hits(rec):
    h = np.zeros(len(rec), _lib.HIT_DTYPE)
    h["t"], h["prim"] = rec["t"], rec["prim"]
    return h


# ---- 1. the walk -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ray_set,time,placement", PLACED, ids=PLACED_IDS)
def test_walk(name, ray_set, time, placement):
    r = SC.rays(name, ray_set, time)
    got = answers(name, ray_set, time, placement)
    if name in MEDIA:  # the plain query refuses the scene: the scan of its surfaces alone
        sc = SC.case_scan(name, ray_set, time)
        decided = Q.check_hits(sc, r, as_hits(got), n_prims(name))
        print(f"{name} {ray_set} {placement}: {decided} of {len(r)} rays decided, {int((got['prim'] != NO).sum())} hits")
        assert decided >= (1.0 - Q.UNDECIDED_CAP) * len(r)
    else:
        assert as_hits(got).tobytes() == device_scene(name, placement).query(r).tobytes()
    if name == "wide1":
        assert device_scene(name, placement).bvh_info()["n_nodes"] > 65535  # the 32-bit stack


# ---- 2. the records ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ray_set,time,placement", PLACED, ids=PLACED_IDS)
def test_records(name, ray_set, time, placement):
    r = SC.rays(name, ray_set, time)
    got = answers(name, ray_set, time, placement)
    want = SC.expected(SC.scene(name), r, got["prim"], got["t"])
    SC.assert_records_equal(got, want, f"{name} {ray_set} {placement}")
    hit = got["prim"] != NO
    assert (got["kind"][~hit] == MISS).all() and (got["kind"][hit] < 7).all() and (got["_pad"] == 0).all()
    kinds = {int(k): int((got["kind"][hit] == k).sum()) for k in np.unique(got["kind"][hit])}
    print(f"{name} {ray_set} {placement}: {int(hit.sum())} hits by kind {kinds}, {int((got['front_face'][hit] == 0).sum())} from inside")


@pytest.mark.parametrize("flag", ["device_bvh", "fast_bvh"])
def test_records_on_a_device_built_tree(flag):
    ds = device_scene("rtow", "lds", device_bvh=True, fast_bvh=flag == "fast_bvh")
    r = Q.rays("rtow", "camera", 0.0)
    got = ds.surface(r)
    assert as_hits(got).tobytes() == ds.query(r).tobytes()
    SC.assert_records_equal(got, SC.expected(Q.scene("rtow"), r, got["prim"], got["t"]), flag)


# ---- 3. media are invisible ----------------------------------------------------------------------------------
def _through_media(sc, r, t_surface):
    """Rays that cross a boundary quad of the scene's media before their closest surface (or at all, for
    a miss): the f32 quad test of every boundary quad over [0.001, t]."""
    bq = np.ascontiguousarray(sc.boundary_quads, dtype=_lib.QUAD_DTYPE)
    n, nq = len(r), len(bq)
    rows = np.empty((n, nq, 9), np.float32)
    rows[:, :, 0:3], rows[:, :, 3:6] = r["o"][:, None, :], r["d"][:, None, :]
    rows[:, :, 6] = Q.T_MIN
    rows[:, :, 7] = np.where(t_surface > 0, t_surface, np.inf).astype(np.float32)[:, None]
    rows[:, :, 8] = np.arange(nq, dtype=np.float32)[None, :]
    h, _ = oracle.quad_hit_f32(bq, rows.reshape(-1, 9))
    return (h.reshape(n, nq) != 0).any(axis=1)


@pytest.mark.parametrize("name,ray_set", [(n, s) for n, s, _ in SC.MEDIA_CASES if n != "final10"])
@pytest.mark.parametrize("placement", ["lds", "global"])
def test_media_are_invisible(name, ray_set, placement):
    sc = SC.scene(name)
    r = SC.rays(name, ray_set, SC.TIME)
    got = answers(name, ray_set, SC.TIME, placement)
    bare = device_scene(name + "-media", placement).surface(r)
    SC.assert_records_equal(got, bare, f"{name} against the scene without its media")
    # rays through the smoke boxes report what lies behind them: a wall, a light or a field sphere, or the miss
    through = _through_media(sc, r, got["t"])
    behind = through & (got["prim"] != NO)
    assert behind.sum() >= 64, int(behind.sum())
    ns = len(sc.spheres)
    walls = behind & (got["prim"] >= ns)
    assert walls.sum() >= 64 and (got["prim"][walls] < ns + len(sc.quads)).all()
    assert (got["kind"][behind] != 7).all()


def test_unbounded_medium_is_passed_over():
    ds = device_scene("final10")
    info = ds.bvh_info()
    assert info["n_unbounded"] > 0  # the_next_week 10's fog around the whole scene: tested after the walk by the render
    r = SC.rays("final10", "inside_hi", SC.TIME)
    got = answers("final10", "inside_hi", SC.TIME, "lds")
    bare = device_scene("final10-media").surface(r)
    assert device_scene("final10-media").bvh_info()["n_unbounded"] == 0
    SC.assert_records_equal(got, bare, "final10 against the scene without its media")
    with pytest.raises(rrt.RrtError) as e:  # the plain query still refuses the scene
        ds.query(r[:64])
    assert e.value.code == -1 and "media" in str(e.value)


def test_medium_in_a_wide_tree():
    """moving_wide(3): a sphere-bounded medium in a tree of more than 65,535 nodes (the 32-bit stack)."""
    sc = B.moving_wide(3)
    r = Q.rays("wide1", "camera", SC.TIME)
    # towards the medium's bounding sphere too
    c = sc.media["sphere"][0, :3]
    o = np.tile(np.float32([-1.0, 0.0, 0.0]), (32, 1))
    d = (c + np.random.default_rng(Q.SEED).uniform(-0.05, 0.05, (32, 3))).astype(np.float32) - o
    r = np.concatenate([r, Q.make_rays(o, d, np.inf, SC.TIME)])
    ds, bare = open_scene(sc, device_bvh=False), open_scene(B.without_media(sc), device_bvh=False)
    try:
        assert ds.bvh_info()["n_nodes"] > 65535
        got = ds.surface(r)
        SC.assert_records_equal(got, bare.surface(r), "moving_wide(3) against the scene without its medium")
        SC.assert_records_equal(got, SC.expected(sc, r, got["prim"], got["t"]), "moving_wide(3)")
        assert (got["prim"] != NO).sum() >= 16
    finally:
        ds.close()
        bare.close()


# ---- 4. the G-buffer -------------------------------------------------------------------------------------------
def camera_rays(cam, time=0.0):
    """The primary entries' rays: ((pixel00 + du * x) + dv * y) - origin, every operation rounded to f32."""
    c = cam[0] if cam.ndim else cam
    w, h = int(c["params_f"][1]), int(c["params_f"][2])
    org, p00, du, dv = (np.asarray(c[k][:3], dtype=np.float32) for k in ("origin", "pixel00", "pixel_delta_u", "pixel_delta_v"))
    x = np.arange(w, dtype=np.float32)[None, :, None]
    y = np.arange(h, dtype=np.float32)[:, None, None]
    d = ((p00 + (du * x).astype(np.float32)).astype(np.float32) + (dv * y).astype(np.float32)).astype(np.float32) - org
    return Q.make_rays(np.broadcast_to(org, (h * w, 3)), d.reshape(-1, 3).astype(np.float32), np.inf, time), (h, w)


def _g_scene(name):
    """comp3n: 36 x 36, the camera's background colour, constant media; rtow48: RTOW at 48 x 27 under the sky."""
    return rrt.rtow(image_width=48, **Q._SMALL) if name == "rtow48" else SC.scene(name)


@pytest.mark.parametrize("name,shape,bg_mode", [("comp3n", (36, 36), 1), ("rtow48", (27, 48), 0)])
def test_g_buffer(name, shape, bg_mode):
    sc = _g_scene(name)
    assert int(sc.camera["params_u"][0, 3]) == bg_mode
    ds = open_scene(sc, device_bvh=False)
    try:
        r, hw = camera_rays(sc.camera, SC.TIME)
        assert hw == shape and (shape[0] % 8 != 0 or shape[1] % 8 != 0)  # partial 8 x 8 tiles
        got = ds.primary_surface(SC.TIME)
        assert got.shape == shape and got.dtype == _lib.SURFACE_DTYPE
        flat = got.reshape(-1)
        SC.assert_records_equal(flat, ds.surface(r), f"{name}: primary_surface against surface() of the camera rays")
        SC.assert_records_equal(flat, SC.expected(sc, r, flat["prim"], flat["t"]), f"{name}: primary_surface")
        hit = flat["prim"] != NO
        assert hit.sum() > flat.size // 4
        if name == "rtow48":  # the sky above the horizon; the plain entry accepts the scene
            assert (~hit).sum() > 16 and (flat["albedo"][~hit] > 0.49).all()
            assert as_hits(flat).tobytes() == ds.primary_hits(SC.TIME).reshape(-1).tobytes()
        else:
            with pytest.raises(rrt.RrtError):
                ds.primary_hits(SC.TIME)
    finally:
        ds.close()


# ---- 5. order and edges ------------------------------------------------------------------------------------------
FILL = 0x7FC0DEAD


def _buffers(r):
    torch = _torch()
    d_r = torch.from_numpy(np.frombuffer(r.tobytes() or b"\0" * 32, dtype=np.float32).copy()).to("cuda:0")
    d_o = torch.full((max(len(r), 1) * 16 + 16,), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return d_r, d_o


def _device_surface(ds, r, stream=None, buffers=None):
    """surface_async through torch buffers; returns the records and what lies behind them in the buffer."""
    torch = _torch()
    n = len(r)
    d_r, d_o = buffers or _buffers(r)
    s = stream or torch.cuda.current_stream()
    ds.surface_async(d_r.data_ptr(), n, d_o.data_ptr(), s.cuda_stream)
    s.synchronize()
    out = d_o.cpu().numpy()
    return out[: 16 * n].view(_lib.SURFACE_DTYPE).copy(), out[16 * n:]


@pytest.mark.parametrize("flag", ["device_bvh", "fast_bvh"])
def test_records_follow_updates_and_refits(flag):
    torch = _torch()
    sc, moved = Q.scene("rtow"), Q.scene("rtow_moved")
    r = Q.rays("rtow", "camera", 0.0)
    ds = open_scene(sc, device_bvh=True, fast_bvh=flag == "fast_bvh")
    try:
        first = ds.surface(r)  # the first query of the scene
        SC.assert_records_equal(first, SC.expected(sc, r, first["prim"], first["t"]), "before the update")
        ds.update_spheres(moved.spheres)
        got = ds.surface(r)
        Q.check_hits(Q.case_scan("rtow_moved", "camera", 0.0), r, as_hits(got), len(sc.spheres))
        SC.assert_records_equal(got, SC.expected(moved, r, got["prim"], got["t"]), "after update_spheres")
        assert got.tobytes() != first.tobytes()
        ds.update_spheres(sc.spheres)
        ds.refit_spheres(moved.spheres)  # the first refit allocates its staging
        ds.refit_spheres(sc.spheres)
        torch.cuda.synchronize()
        # a refit and the records behind it on one stream, no synchronisation between
        stream = torch.cuda.Stream(device="cuda:0")
        buffers = _buffers(r)
        ds.refit_spheres(moved.spheres, stream_ptr=stream.cuda_stream)
        got, tail = _device_surface(ds, r, stream=stream, buffers=buffers)
        assert (tail == FILL).all()
        Q.check_hits(Q.case_scan("rtow_moved", "camera", 0.0), r, as_hits(got), len(sc.spheres))
        SC.assert_records_equal(got, SC.expected(moved, r, got["prim"], got["t"]), "after a refit on the same stream")
    finally:
        ds.close()


def test_batch_edges_and_intervals_that_find_nothing():
    ds = device_scene("quad_sphere")
    sc = SC.scene("quad_sphere")
    r0 = Q.rays("quad_sphere", "camera", 0.0)
    base = ds.surface(r0)
    assert (base["prim"] != NO).sum() >= 64
    _, tail = _device_surface(ds, r0[:0])  # n = 0 enqueues nothing
    assert (tail == FILL).all()
    ds.surface_async(0, 0, 0)
    assert len(ds.surface(r0[:0])) == 0
    for n in (1, 63, 65):  # a partial group, device arrays against host arrays
        dev, tail = _device_surface(ds, np.ascontiguousarray(r0[:n]))
        assert dev.tobytes() == base[:n].tobytes() and (tail == FILL).all()
    for tmax in (np.nan, 0.001, 0.0, -1.0):
        r = r0.copy()
        r["tmax"] = tmax
        got = ds.surface(r)
        assert (got["prim"] == NO).all() and (got["kind"] == MISS).all()
        SC.assert_records_equal(got, SC.expected(sc, r, got["prim"], got["t"]), f"tmax = {tmax}")
        assert (got["albedo"] > 0).all()  # the sky


def _refused(call, word):
    with pytest.raises(rrt.RrtError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)


def test_refusals_leave_the_scene_rendering():
    torch = _torch()
    r = Q.rays("rtow", "camera", 0.0)[:64]
    smoke = open_scene(SC.scene("smoke"), device_bvh=False)
    f64 = open_scene(Q.scene("rtow"), device_bvh=False, f64=True)
    plain = open_scene(Q.scene("rtow"), device_bvh=True)
    try:
        before = [frame_of(ds)[0].tobytes() for ds in (smoke, f64, plain)]
        rays = torch.zeros(64 * 8, dtype=torch.float32, device="cuda:0")
        out = torch.zeros(64 * 16 + 16, dtype=torch.int32, device="cuda:0")
        _refused(lambda: f64.surface(r), "RRT_FLAG_F64")
        _refused(lambda: f64.primary_surface(), "RRT_FLAG_F64")
        _refused(lambda: plain.surface_async(rays.data_ptr(), 64, 0), "null surface records")
        _refused(lambda: plain.surface_async(rays.data_ptr(), 64, out.data_ptr() + 8), "surface records must be 16-byte aligned")
        _refused(lambda: plain.surface_async(0, 64, out.data_ptr()), "null rays")
        _refused(lambda: plain.surface_async(rays.data_ptr() + 4, 64, out.data_ptr()), "rays must be 16-byte aligned")
        _refused(lambda: plain.primary_surface_async(0), "null surface records")
        _refused(lambda: plain.primary_surface_async(out.data_ptr() + 4), "16-byte aligned")
        torch.cuda.synchronize()
        assert (out == 0).all()  # nothing was enqueued
        _refused(lambda: smoke.query(r), "media")  # the existing entries still refuse media
        _refused(lambda: smoke.primary_hits(), "media")
        assert (smoke.surface(r)["kind"] != 7).all()
        # a scene left invalid by a change that failed midway (the test hook stands in for the device error)
        smoke2 = open_scene(SC.scene("smoke"), device_bvh=True)
        try:
            for ds in (plain, smoke2):  # the media scene too: invalid is refused whatever the entry accepts
                assert "rrt_testing_scene_fail_update" in ds.testing_fail_update()
                for call in (lambda: ds.surface(r), lambda: ds.surface_async(rays.data_ptr(), 64, out.data_ptr()),
                             lambda: ds.primary_surface(), lambda: ds.primary_surface_async(out.data_ptr())):
                    _refused(call, "invalid since a change of it failed (rrt_testing_scene_fail_update")
            _refused(lambda: plain.query(r), "invalid")
        finally:
            smoke2.close()
        torch.cuda.synchronize()
        assert (out == 0).all()  # nothing was enqueued
        plain.update_spheres(Q.scene("rtow").spheres)  # a later update that succeeds: valid again
        got = plain.surface(r)
        SC.assert_records_equal(got, SC.expected(Q.scene("rtow"), r, got["prim"], got["t"]), "after the scene is valid again")
        after = [frame_of(ds)[0].tobytes() for ds in (smoke, f64, plain)]
        assert before == after
    finally:
        for ds in (smoke, f64, plain):
            ds.close()
