"""The f64 books path for book 2 (RRT_FLAG_F64_BOOK2, rrt_books64.hip class kF64Book2: moving
spheres, quads, checker textures) against the oracle's f64 BOOKS restatement.

Every frame of books64_book2_scenes.py renders through DeviceScene(f64=True, f64_book2=True) and must
give BOOKS' f64 sums bit for bit, w = spp, the same number of closest-hit queries, the f32 entry equal
to the sums rounded, and the same PPM bytes. tests/test_books64_book2.py shows on the reference alone
that these frames do not depend on the primitive order (no exact t-tie decides a pixel), so no test
here carries a tolerance. A box wrongly pruned (rrt_box32.h, on a quad's closed interval or a sphere
between its two end positions) would show as a ray-count or bit mismatch.

The kernel's quad test and checker parity are also checked pointwise (RRT_OP_QUAD64, RRT_OP_CHECKER64)
against the oracle's f64 Quad::hit and CheckerTexture, at the edges of each comparison.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib

import books64_book2_scenes as B
from test_gpu_books64 import _check

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustraytrace_amd", "rrt")


@functools.lru_cache(maxsize=None)
def _books(name):
    """BOOKS' sequential f64 sums and ray count of a frame (computed once, read-only)."""
    acc, rays, _ = oracle.render(B.frame(name), oracle.BOOKS, threads=16)
    acc.setflags(write=False)
    return acc, rays


def _gpu(scene, device_bvh=False, f64_book2=True):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ds = rrt.DeviceScene(scene, device=0, f64=True, f64_book2=f64_book2, device_bvh=device_bvh)
    tile = ds.tile(16, 0, 1, 0, scene.spp)
    n_rows = ds.tile_rows(tile)
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((n_rows, scene.width, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    ds.reset_counters()
    ds.render_tile_f64_async(tile, buf.data_ptr(), stream)
    torch.cuda.synchronize()
    rays = int(ds.counters()["rays"])
    buf32 = torch.full((n_rows, scene.width, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    ds.render_tile_async(tile, buf32.data_ptr(), stream)
    torch.cuda.synchronize()
    out, out32 = buf.cpu().numpy(), buf32.cpu().numpy()
    info = ds.bvh_info()
    ds.close()
    return out, out32, rays, info


def _frame_against_books(name, label, **kw):
    scene = B.frame(name)
    books, books_rays = _books(name)
    gpu, gpu32, rays, info = _gpu(scene, **kw)
    print(f"{label}: {rays} closest-hit queries (BOOKS {books_rays}), node stride {info['node_stride']}")
    assert np.all(gpu[..., 3] == scene.spp)
    assert rays == books_rays, f"{label}: {rays} closest-hit queries vs BOOKS {books_rays}"
    _check(scene, gpu, books, label)  # bits; implies within 1e-4 and equal bytes, both checked too
    assert np.array_equal(gpu32, gpu.astype(np.float32))
    q = rrt.quantize_accum_books_f64(scene.width, scene.height, gpu, scene.spp)
    qb = rrt.quantize_accum_books_f64(scene.width, scene.height, np.ascontiguousarray(books), scene.spp)
    assert rrt.format_pnm_from_rgb8(scene.width, scene.height, q) == rrt.format_pnm_from_rgb8(scene.width, scene.height, qb)
    return info


# ---- frames against BOOKS ----------------------------------------------------------------------
@pytest.mark.parametrize("name", B.FRAMES)
def test_frame_matches_books_path(monkeypatch, name):
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    _frame_against_books(name, name)


@pytest.mark.parametrize("name", ["s1d50", "s7", "mixed"])
def test_frame_from_global_memory(monkeypatch, name):
    monkeypatch.setenv("RRT_SCENE_IN_LDS", "0")
    info = _frame_against_books(name, f"{name} from global memory")
    assert info["node_stride"] == 32


@pytest.mark.parametrize("name", ["s1d50", "s7", "mixed"])
def test_frame_with_device_bvh(monkeypatch, name):
    monkeypatch.delenv("RRT_SCENE_IN_LDS", raising=False)
    _frame_against_books(name, f"{name} device BVH", device_bvh=True)


# ---- other paths -------------------------------------------------------------------------------
def test_count_work_counts_books_rays():
    import torch

    scene = B.frame("mixed")
    ds = rrt.DeviceScene(scene, device=0, f64=True, f64_book2=True)
    work = ds.count_work(ds.tile(16, 0, 1, 0, scene.spp))
    ds.close()
    torch.cuda.synchronize()
    assert int(work["rays"]) == _books("mixed")[1]


def test_book1_scene_with_the_flag_renders_f64_bits():
    scene = rrt.config_scene("C1", image_width=64, samples_per_pixel=16)
    a, a32, rays_a, info_a = _gpu(scene, f64_book2=True)
    b, b32, rays_b, info_b = _gpu(scene, f64_book2=False)
    assert rays_a == rays_b and info_a == info_b
    assert np.array_equal(a, b) and np.array_equal(a32, b32)


def test_sample_schedules_are_bit_identical(monkeypatch):
    """300 samples, more than rrt_accum_chunk(): the prefix chunk, the tail units and
    rrt_fold_samples64 all run; the same bits with the partial budget of RRT_PARTIAL_MB=1."""
    assert 300 > _lib.load().rrt_accum_chunk()
    scene = rrt.next_week_scene(1, dict(image_width=48, samples_per_pixel=300, max_depth=8))
    books, books_rays, _ = oracle.render(scene, oracle.BOOKS, threads=16)
    gpu, _, rays, _ = _gpu(scene)
    assert rays == books_rays
    _check(scene, gpu, books, "s1 48 wide x 300 spp")
    monkeypatch.setenv("RRT_PARTIAL_MB", "1")
    again, _, rays2, _ = _gpu(scene)
    assert rays2 == rays and np.array_equal(again, gpu)


def test_one_shots_equal_the_tile_render():
    scene = B.frame("mixed")
    tile, _, _, _ = _gpu(scene)
    accum = rrt.render_f64(scene, book2=True)
    assert np.array_equal(accum, tile)
    lib = _lib.load()
    lib.rrt_testing_device_wrap(1)
    try:
        two = rrt.render_f64(scene, n_gpus=2, book2=True)
    finally:
        lib.rrt_testing_device_wrap(0)
    assert np.array_equal(two, tile)
    rgb8 = rrt.render_f64_rgb8(scene, book2=True)
    assert np.array_equal(rgb8, rrt.quantize_accum_books_f64(scene.width, scene.height, accum, scene.spp))


def test_cli_books_f64_book2(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    args = [CLI, "--backend", "hip", "the_next_week", "7", "--books-f64-book2", "--image_width", "32",
            "--samples_per_pixel", "4", "--max_depth", "10"]
    outs = {}
    for name, extra in [("dev", []), ("host", ["--host-quantise"]), ("p6", ["--p6"])]:
        path = tmp_path / f"{name}.ppm"
        r = subprocess.run(args + extra + ["-o", str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[name] = path.read_bytes()
    scene = rrt.next_week_scene(7, dict(image_width=32, samples_per_pixel=4, max_depth=10))
    rgb8 = rrt.render_f64_rgb8(scene, book2=True)
    assert outs["dev"] == rrt.format_pnm_from_rgb8(scene.width, scene.height, rgb8)
    assert outs["host"] == outs["dev"]
    assert outs["p6"] == rrt.format_pnm_from_rgb8(scene.width, scene.height, rgb8, binary=True)
    r = subprocess.run([CLI, "the_next_week", "7", "--books-f64", "--image_width", "32", "--samples_per_pixel", "4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "RRT_FLAG_F64 renders book-1 scenes" in r.stderr


# ---- RRT_OP_QUAD64 -----------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
# q = (0, 0, -2), u = (2, 0, 0), v = (0, 2, 0): normal (0, 0, 1), D = -2, w = (0, 0, 1/4), so for a ray
# with d.x = d.y = 0 the plane coordinates are exact: alpha = o.x / 2, beta = o.y / 2, t = (-2 - o.z) / d.z
AXIS = ((0.0, 0.0, -2.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))
OBLIQUE = ((-1.25, 0.5, -3.0), (2.5, 0.75, -0.5), (-0.25, 1.75, 1.0))  # every value an f32


def _quad_rows():
    up, dn = np.nextafter, np.nextafter
    rows = []

    def row(o, d, tmin=0.001, closest=INF, j=0):
        rows.append([*o, *d, tmin, closest, float(j)])

    # |denom| one f64 step below, at and above 1e-8, both signs; t ~ 1, inside
    for s in (1.0, -1.0):
        for dz in (dn(1e-8, 0.0), 1e-8, up(1e-8, 1.0)):
            row((1.0, 1.0, -2.0 - s * dz), (0.0, 0.0, s * dz))
    # t = RN(2 / 2000) = the f64 0.001 = tmin: accepted (closed interval); one step below: rejected
    row((1.0, 1.0, 0.0), (0.0, 0.0, -2000.0))
    row((1.0, 1.0, 0.0), (0.0, 0.0, -2000.0), tmin=up(0.001, 1.0))
    row((1.0, 1.0, 0.0), (0.0, 0.0, up(-2000.0, -3000.0)))
    # t = 2 exactly, against closest = 2 (accepted), one step below (rejected), tmin = 2 and above
    row((1.0, 1.0, 0.0), (0.0, 0.0, -1.0), closest=2.0)
    row((1.0, 1.0, 0.0), (0.0, 0.0, -1.0), closest=dn(2.0, 0.0))
    row((1.0, 1.0, 0.0), (0.0, 0.0, -1.0), tmin=2.0, closest=2.0)
    row((1.0, 1.0, 0.0), (0.0, 0.0, -1.0), tmin=up(2.0, 3.0))
    # corners and edges (alpha or beta exactly 0 or 1), and one step outside each
    for x in (0.0, 2.0, 1.0, dn(0.0, -1.0), up(2.0, 3.0), -0.0):
        for y in (0.0, 2.0, 1.0, dn(0.0, -1.0), up(2.0, 3.0)):
            row((x, y, 0.0), (0.0, 0.0, -1.0))
    # along an edge, in the plane (denom = 0) and nearly so
    row((-1.0, 0.0, -2.0), (1.0, 0.0, 0.0))
    row((-1.0, 0.0, -2.0), (1.0, 0.0, 1e-9))
    row((-1.0, 0.0, -1.0), (1.0, 0.0, -1.0))  # meets the edge y = 0 at x = 0: the corner
    # origin on the plane: t = -0 (accepted only from tmin <= 0)
    for tmin in (0.001, 0.0, -0.0, -1.0):
        row((1.0, 1.0, -2.0), (0.0, 0.0, -1.0), tmin=tmin)
        row((1.0, 1.0, -2.0), (0.0, 0.0, 1.0), tmin=tmin)
    # NaN and infinities in every column
    base = [1.0, 1.0, 0.0, 0.25, -0.125, -1.0, 0.001, INF]
    for col in range(8):
        for bad in (NAN, INF, -INF):
            r = list(base)
            r[col] = bad
            rows.append([*r, 0.0])
            rows.append([*r, 1.0])
    # ordinary rays at both quads
    rng = np.random.default_rng(64)
    for j, (q, u, v) in enumerate((AXIS, OBLIQUE)):
        q, u, v = (np.asarray(x) for x in (q, u, v))
        for _ in range(120):
            o = rng.uniform(-4, 4, 3)
            a, b = rng.uniform(-0.3, 1.3, 2)
            d = (q + a * u + b * v) - o
            row(o, d * rng.choice([1.0, -1.0, 0.5, 3.0]), closest=rng.choice([INF, 1.0, 0.9]), j=j)
    return np.array(rows, dtype=np.float64)


def test_quad64_matches_oracle_quad_hit():
    rows = _quad_rows()
    quads = np.zeros(2, dtype=_lib.QUAD_DTYPE)
    for j, (q, u, v) in enumerate((AXIS, OBLIQUE)):
        quads["q"][j, :3], quads["u"][j, :3], quads["v"][j, :3] = q, u, v
    out = _lib.device_ops64("QUAD64", rows, quads=quads)
    hits = 0
    for r, (hit, tbits) in zip(rows, out):
        q, u, v = (AXIS, OBLIQUE)[int(r[8])]
        want = oracle.quad_hit(q, u, v, r[0:3], r[3:6], tmin=r[6], tmax=r[7], f32=False)
        assert bool(hit) == (want is not None), f"row {r.tolist()}: kernel {hit}, oracle {want}"
        if want is not None:
            hits += 1
            assert np.uint64(tbits) == np.float64(want[0]).view(np.uint64), f"row {r.tolist()}: t bits differ"
        else:
            assert tbits == 0
    assert 40 < hits < len(rows) - 40
    # the edges named above, by their known answers
    first = dict(zip(["below", "at", "above"], out[:3, 0]))
    assert (first["below"], first["at"], first["above"]) == (0, 1, 1)
    assert list(out[6:13, 0]) == [1, 0, 0, 1, 0, 1, 0]


# ---- RRT_OP_CHECKER64 --------------------------------------------------------------------------
def _checker_cases():
    up = np.nextafter
    cases = {}
    inv = 1.0 / 0.32  # bouncing_spheres' ground
    pts = []
    for k in (-3, -2, -1, 0, 1, 2, 3, 7):  # cell boundaries and one step either side
        x = k * 0.32
        pts += [(x, 0.5, 0.5), (up(x, -INF), 0.5, 0.5), (up(x, INF), 0.5, 0.5), (0.1, x, -x), (x, x, x)]
    pts += [(-0.0, 0.0, -0.0), (-1e-300, 1e-300, 0.0), (-5.3, -2.2, -9.9), (NAN, 0.5, 0.5), (0.5, NAN, NAN),
            (INF, 0.5, 0.5), (-INF, 0.5, 0.5), (INF, -INF, NAN)]
    rng = np.random.default_rng(5)
    pts += [tuple(p) for p in rng.uniform(-20, 20, (100, 3))]
    cases[inv] = pts
    # inv_scale * p beyond +-2^31: the cast saturates; sums that wrap
    big = 2.0 ** 31
    cases[1.0] = [(big, 0.0, 0.0), (big - 1.0, 0.0, 0.0), (big - 0.5, 0.0, 0.0), (-big, 0.0, 0.0), (-big - 1.0, 0.0, 0.0),
                  (-big + 0.5, 0.0, 0.0), (1e300, 1.0, 0.0), (-1e300, 0.0, 0.0), (big, big, 0.0), (big, big, big),
                  (big - 1.0, 1.0, 0.0), (big - 1.0, big - 1.0, 2.0), (-big, -big, -big), (-big, -1.0, 0.0),
                  (2147483646.0, 1.0, 1.0), (2147483646.5, 1.0, 1.0)]
    cases[1e10] = [(0.3, -0.3, 0.0), (1.0, 1.0, 1.0), (-1.0, 1e-10, 2e-10), (0.2, 0.2, 1e-11)]
    cases[NAN] = [(1.0, 2.0, 3.0)]
    cases[-2.5] = [tuple(p) for p in rng.uniform(-3, 3, (20, 3))]
    return cases


def test_checker64_matches_oracle_checker():
    table = np.zeros(1, dtype=_lib.PERLIN_DTYPE)
    n = 0
    for inv, pts in _checker_cases().items():
        pts = np.array(pts, dtype=np.float64)
        rows = np.concatenate([np.full((len(pts), 1), inv), pts], axis=1)
        out = _lib.device_ops64("CHECKER64", rows)[:, 0]
        want = oracle.book2_textures(table, pts, inv_scale=inv, f32=False)[2]
        bad = np.flatnonzero(out.astype(bool) != want)
        assert len(bad) == 0, f"inv_scale {inv}: rows {rows[bad].tolist()} kernel {out[bad]} oracle {want[bad]}"
        n += len(pts)
        if inv == 1.0:  # the saturating casts and wrapping sums give both parities
            assert set(out.tolist()) == {0, 1}
    assert n > 150
