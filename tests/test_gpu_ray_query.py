"""Ray queries on a created scene (rrt_scene_query_async, rrt_scene_query, rrt_scene_primary_hits_async)
against the linear scans of tests/ray_query_cases.py.

The query kernel runs the render's own node step and leaf tests (trav_node, trav_leaves) on caller
rays, so this is also the ray-by-ray check of the render's closest hit. The rules (ray_query_cases.
check_hits): every reported hit names a primitive whose own f32 test accepts the ray, with that test's
t bit for bit; every DECIDED ray (the module's rules (a)-(d); tests/test_ray_query_cases.py caps the
undecided ones at 2 % per set) has the scan's primitive and t, bit for bit. No tolerance anywhere.
"""
import os

import numpy as np
import pytest

import rustraytrace_amd as rrt
from rustraytrace_amd import _lib

import ray_query_cases as Q
from test_gpu_scene_update import frame_of, open_scene

pytestmark = pytest.mark.gpu

NO = _lib.NO_PRIM
PLACEMENTS = {"lds": None, "global": "0"}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_open = {}


def device_scene(name, placement="lds", **kw):
    """The scene `name` on the device, created once per (name, placement, flags) under the placement's
    RRT_SCENE_IN_LDS; closed when the module is done."""
    key = (name, placement, tuple(sorted(kw.items())))
    if key not in _open:
        old = os.environ.pop("RRT_SCENE_IN_LDS", None)
        try:
            if PLACEMENTS[placement] is not None:
                os.environ["RRT_SCENE_IN_LDS"] = PLACEMENTS[placement]
            ds = open_scene(Q.scene(name), device_bvh=kw.pop("device_bvh", False), **kw)
        finally:
            os.environ.pop("RRT_SCENE_IN_LDS", None)
            if old is not None:
                os.environ["RRT_SCENE_IN_LDS"] = old
        stride = ds.bvh_info()["node_stride"]
        assert stride == (32 if placement == "global" else 80), (name, placement, stride)
        _open[key] = ds
    return _open[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _open.values():
        ds.close()
    _open.clear()


def n_prims(name):
    return Q.geometry(Q.scene(name)).n_prims


# every case in its placements: staged and read from global memory for RTOW and the two composites; the
# stock Cornell box, book 3 and the tiny trees as created (staged); the wide tree reads 32-B nodes through
# the 32-bit stack. Bouncing spheres (the_next_week 1: 485 primitives of 64 B and their nodes) are past
# the 40 KB a scene may stage, so the library reads them from global memory whatever is asked: one
# placement (test_bouncing_spheres_do_not_stage); the staged radius-and-motion kernel runs on comp1.
PLACED = [(n, s, t, p) for n, s, t in Q.CASES if n != "rtow_moved"
          for p in (("lds", "global") if n in ("rtow", "comp1", "comp2") else ("global",) if n in ("wide1", "nw1") else ("lds",))]
PLACED_IDS = [f"{n}-{s}-{t:.2f}-{p}" for n, s, t, p in PLACED]


# ---- 1 and 6. against the scan (the tiny trees are among the cases) --------------------------------
@pytest.mark.parametrize("name,ray_set,time,placement", PLACED, ids=PLACED_IDS)
def test_closest_equals_the_scan(name, ray_set, time, placement):
    ds = device_scene(name, placement)
    if name == "wide1":
        assert ds.bvh_info()["n_nodes"] > 65535  # the 32-bit stack
    r = Q.rays(name, ray_set, time)
    sc = Q.case_scan(name, ray_set, time)
    hits = ds.query(r)
    decided = Q.check_hits(sc, r, hits, n_prims(name))
    print(f"{name} {ray_set} {placement}: {decided} of {len(r)} rays decided, {int((hits['prim'] != NO).sum())} hits")
    assert decided >= (1.0 - Q.UNDECIDED_CAP) * len(r)


def test_bouncing_spheres_do_not_stage():
    ds = rrt.DeviceScene(Q.scene("nw1"))
    try:
        assert ds.bvh_info()["node_stride"] == 32
    finally:
        ds.close()


def test_wide_tree_through_the_cloud():
    """The rays that cross wide1's 66,000 tiny spheres (rule (c) leaves a tenth of them undecided): the
    per-primitive rules for all, the scan's answer for the decided ones."""
    ds = device_scene("wide1", "global")
    r = Q.rays("wide1", "through", 0.37)
    sc = Q.scan(Q.geometry(Q.scene("wide1")), r)
    hits = ds.query(r)
    Q.check_hits(sc, r, hits, n_prims("wide1"))
    assert (hits["prim"] != NO).sum() >= 16


# ---- 2. any-hit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ray_set,time,placement", PLACED, ids=PLACED_IDS)
def test_any_hit_finds_a_hit_exactly_when_closest_does(name, ray_set, time, placement):
    ds = device_scene(name, placement)
    r = Q.rays(name, ray_set, time)
    closest, anyh = ds.query(r), ds.query(r, mode="any")
    assert np.array_equal(anyh["prim"] != NO, closest["prim"] != NO)
    Q.check_hits(Q.case_scan(name, ray_set, time), r, anyh, n_prims(name), decided=False)
    assert (anyh["t"] >= closest["t"]).all()  # never closer than the closest


# ---- 3. batch shapes ---------------------------------------------------------------------------------
FILL = 0x7FC0DEAD


def _buffers(r):
    """(rays, hits) of a device query in torch buffers, the hits pre-filled; the device is idle on return."""
    torch = _torch()
    d_r = torch.from_numpy(np.frombuffer(r.tobytes() or b"\0" * 32, dtype=np.float32).copy()).to("cuda:0")
    d_h = torch.full((max(len(r), 1) * 2,), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return d_r, d_h


def _device_query(ds, r, mode="closest", stream=None, buffers=None):
    """query_async through torch buffers; returns the hits and what lies behind them in the buffer."""
    torch = _torch()
    n = len(r)
    d_r, d_h = buffers or _buffers(r)
    s = stream or torch.cuda.current_stream()
    ds.query_async(d_r.data_ptr(), n, d_h.data_ptr(), mode, s.cuda_stream)
    s.synchronize()
    out = d_h.cpu().numpy()
    return out[: 2 * n].view(_lib.HIT_DTYPE).copy(), out[2 * n:]


@pytest.mark.parametrize("placement", ["lds", "global"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_batch_shapes(n, placement):
    ds = device_scene("rtow", placement)
    full = Q.rays("rtow", "camera", 0.0)
    want = ds.query(full)
    pick = np.arange(n) % len(full) if n <= len(full) else np.concatenate([np.arange(len(full)), [17]])
    if 1 < n <= 65:
        pick = (pick * 61 + 5) % len(full)  # other neighbours than in the full batch
    r = np.ascontiguousarray(full[pick])
    host = ds.query(r)
    dev, tail = _device_query(ds, r)
    assert host.tobytes() == want[pick].tobytes()
    assert dev.tobytes() == host.tobytes()
    if n == 0:
        assert (tail == FILL).all()  # nothing was written


# ---- 4. intervals --------------------------------------------------------------------------------------
def test_interval_ends():
    ds = device_scene("quad_sphere")
    r0 = Q.rays("quad_sphere", "camera", 0.0)
    sc = Q.case_scan("quad_sphere", "camera", 0.0)
    base = ds.query(r0)
    ok = ~sc.undecided & (base["prim"] != NO)
    on_sphere, on_quad = ok & (base["prim"] == 0), ok & (base["prim"] == 1)
    assert on_sphere.sum() >= 16 and on_quad.sum() >= 16
    t = base["t"]
    up = np.nextafter(t, np.float32(np.inf))
    for tmax, keeps_sphere, keeps_quad in ((np.full_like(t, np.inf), True, True), (t, False, True), (up, True, True),
                                           (np.full_like(t, 0.001), False, False), (np.zeros_like(t), False, False),
                                           (np.full_like(t, -1.0), False, False), (np.full_like(t, np.nan), False, False)):
        r = r0.copy()
        r["tmax"] = tmax
        got = ds.query(r)
        for sel, keeps in ((on_sphere, keeps_sphere), (on_quad, keeps_quad)):
            if keeps:  # the same hit: the open bound above t, the quad's closed bound at t
                assert got[sel].tobytes() == base[sel].tobytes()
            else:      # lost, and nothing else lies before it
                assert (got["prim"][sel] == NO).all() and (got["t"][sel].view(np.uint32) == 0).all()
        # and the per-primitive rules for every ray at this tmax
        Q.check_hits(Q.scan(Q.geometry(Q.scene("quad_sphere")), r), r, got, 2, decided=False)


# ---- 5. edge rays --------------------------------------------------------------------------------------
def edge_rays(name):
    """256 rays: zero, NaN and infinite directions, one and two zero components, origins in and on spheres."""
    g = Q.geometry(Q.scene(name))
    rng = np.random.default_rng(Q.SEED)
    o = rng.uniform(-3.0, 3.0, (256, 3)).astype(np.float32)
    d = rng.standard_normal((256, 3)).astype(np.float32)
    d[0:8] = 0.0
    k = 8
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            d[k:k + 8, axis] = bad
            k += 8
    for axis in range(3):  # one component exactly 0, then -0
        d[k:k + 8, axis] = 0.0
        d[k + 8:k + 16, axis] = -0.0
        k += 16
    for axis in range(3):  # two components exactly 0: axis-parallel rays
        d[k:k + 16] = 0.0
        d[k:k + 16, axis] = np.where(np.arange(16) % 2, -1.0, 1.0)
        k += 16
    ns = len(g.centres)
    pick = rng.integers(0, ns, 40)
    o[k:k + 20] = g.centres[pick[:20]] + (0.3 * g.radii[pick[:20], None] * rng.uniform(-1, 1, (20, 3))).astype(np.float32)
    k += 20
    u = rng.standard_normal((20, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[k:k + 20] = (g.centres[pick[20:]] + g.radii[pick[20:], None] * u).astype(np.float32)  # on the surface
    k += 20
    assert k <= 256
    return Q.make_rays(o, d)


@pytest.mark.parametrize("name,placement", [("rtow", "lds"), ("rtow", "global"), ("comp2", "lds"), ("comp2", "global")])
def test_edge_rays(name, placement):
    ds = device_scene(name, placement)
    r = edge_rays(name)
    sc = Q.scan(Q.geometry(Q.scene(name)), r)
    for mode in ("closest", "any"):
        hits = ds.query(r, mode=mode)  # returns RRT_OK (no exception)
        Q.check_hits(sc, r, hits, n_prims(name), decided=False)
    assert (ds.query(r)["prim"] != NO).sum() >= 32  # the set does hit things


# ---- 7. primary hits -----------------------------------------------------------------------------------
def camera_rays(cam, time=0.0):
    """The path tracer's camera rays at zero jitter, no defocus: ((pixel00 + du * x) + dv * y) - origin in f32."""
    c = cam[0] if cam.ndim else cam
    w, h = int(c["params_f"][1]), int(c["params_f"][2])
    org, p00, du, dv = (np.asarray(c[k][:3], dtype=np.float32) for k in ("origin", "pixel00", "pixel_delta_u", "pixel_delta_v"))
    x = np.arange(w, dtype=np.float32)[None, :, None]
    y = np.arange(h, dtype=np.float32)[:, None, None]
    d = ((p00 + (du * x).astype(np.float32)).astype(np.float32) + (dv * y).astype(np.float32)).astype(np.float32) - org
    return Q.make_rays(np.broadcast_to(org, (h * w, 3)), d.reshape(-1, 3).astype(np.float32), np.inf, time), (h, w)


@pytest.mark.parametrize("name,shape", [("rtow", (36, 64)), ("cornell", (32, 32))])
def test_primary_hits_equal_the_query_of_the_camera_rays(name, shape):
    ds = rrt.DeviceScene(Q.scene(name))
    try:
        r, hw = camera_rays(ds.scene.camera)
        assert hw == shape
        got = ds.primary_hits()
        assert got.shape == shape
        assert got.reshape(-1).tobytes() == ds.query(r).tobytes()
        assert (got["prim"] != NO).sum() > got.size // 4
        if name == "rtow":  # another camera, a frame that is no multiple of the 8 x 8 tile
            cam = rrt.rtow(image_width=20, samples_per_pixel=1, max_depth=4).camera
            ds.set_camera(cam)
            r2, hw2 = camera_rays(ds.scene.camera, time=0.25)
            assert hw2 == (11, 20)
            got2 = ds.primary_hits(time=0.25)
            assert got2.shape == hw2 and got2.reshape(-1).tobytes() == ds.query(r2).tobytes()
    finally:
        ds.close()


# ---- 8. after a change ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["device_bvh", "fast_bvh"])
def test_queries_follow_updates_and_refits(flag):
    torch = _torch()
    sc, moved = Q.scene("rtow"), Q.scene("rtow_moved")
    r = Q.rays("rtow", "camera", 0.0)
    ds = open_scene(sc, device_bvh=True, fast_bvh=flag == "fast_bvh")
    fresh = open_scene(moved, device_bvh=True, fast_bvh=flag == "fast_bvh")
    try:
        Q.check_hits(Q.case_scan("rtow", "camera", 0.0), r, ds.query(r), len(sc.spheres))  # the first query
        ds.update_spheres(moved.spheres)
        assert ds.query(r).tobytes() == fresh.query(r).tobytes()  # another tree, another leaf order
        assert ds.query(r, mode="any").tobytes() == fresh.query(r, mode="any").tobytes()
        ds.update_spheres(sc.spheres)
        ds.refit_spheres(moved.spheres)  # the first refit allocates its staging
        ds.refit_spheres(sc.spheres)
        torch.cuda.synchronize()
        # a refit and the query behind it on one stream, no synchronisation between
        stream = torch.cuda.Stream(device="cuda:0")
        buffers = _buffers(r)
        ds.refit_spheres(moved.spheres, stream_ptr=stream.cuda_stream)
        hits, _ = _device_query(ds, r, stream=stream, buffers=buffers)
        assert ds.refit_stats()["last_allocations"] == 0
        Q.check_hits(Q.case_scan("rtow_moved", "camera", 0.0), r, hits, len(sc.spheres))
        ds.update_spheres(sc.spheres)
        assert ds.update_stats()["last_allocations"] == 0
        Q.check_hits(Q.case_scan("rtow", "camera", 0.0), r, ds.query(r), len(sc.spheres))
    finally:
        ds.close()
        fresh.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------
def _refused(call, word):
    with pytest.raises(rrt.RrtError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)


def test_refusals_leave_the_scene_rendering():
    torch = _torch()
    r = Q.rays("rtow", "camera", 0.0)[:64]
    smoke = open_scene(rrt.next_week_scene(8, dict(image_width=32, samples_per_pixel=2, max_depth=4)), device_bvh=False)
    f64 = open_scene(Q.scene("rtow"), device_bvh=False, f64=True)
    plain = open_scene(Q.scene("rtow"), device_bvh=False)
    try:
        before = [frame_of(ds)[0].tobytes() for ds in (smoke, f64, plain)]
        buf = torch.zeros(64 * 8, dtype=torch.float32, device="cuda:0")
        _refused(lambda: smoke.query(r), "media")
        _refused(lambda: smoke.primary_hits(), "media")
        _refused(lambda: f64.query(r), "RRT_FLAG_F64")
        _refused(lambda: plain.query(r, mode=7), "mode")
        _refused(lambda: plain.query_async(buf.data_ptr(), 64, 0), "hits")
        _refused(lambda: plain.query_async(0, 64, buf.data_ptr()), "rays")
        _refused(lambda: plain.primary_hits_async(0), "hits")
        plain.query_async(0, 0, 0)  # n = 0 enqueues nothing
        after = [frame_of(ds)[0].tobytes() for ds in (smoke, f64, plain)]
        assert before == after
    finally:
        for ds in (smoke, f64, plain):
            ds.close()


# ---- 10. counters --------------------------------------------------------------------------------------
def test_queries_leave_counters_and_renders_alone():
    ds = open_scene(Q.scene("rtow"), device_bvh=False)
    try:
        frame, rays = frame_of(ds)
        counters = ds.counters()
        r = Q.rays("rtow", "inside", 0.0)
        for i in range(10):
            ds.query(r, mode="any" if i % 2 else "closest")
        ds.primary_hits()
        assert ds.counters() == counters
        frame2, rays2 = frame_of(ds)
        assert frame2.tobytes() == frame.tobytes() and rays2 == rays
    finally:
        ds.close()
