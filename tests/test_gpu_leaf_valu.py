"""GPU: the leaf iteration's root code after its issue-slot cut — one tmin compare, the discriminant's own
square-root entry, the far root behind a ballot — on 36 x 36 x 4 frames, bit for bit against the oracle's
walk of the kernel's tree (KBVH), with KBVH's ray and sphere-test counts from the counting kernel, box
tests = 2 x node visits, and the node visits of the kernel before the change (NODE_VISITS, recorded on
one MI355X from these scenes with the parent commit's library; the oracle reports no node count).

  tangent  a discriminant of exactly 0 in a lane among ordinary lanes. A ray along -z from the origin and a
           unit sphere at (1, 0, -5): h = 5, a = 1, c = 25, disc = 0, root 5 — all exact. The leaf loop now
           sends such a lane (and, with it, the wave) through the library square root. A camera ray carries
           its pixel's jitter, so no frame holds an exactly tangent ray: this one case is pointwise, through
           the SPHERE op of rrt_testing_device_ops (test_range over a one-record range, both record forms),
           row i at lane i % 64, the tangent rows and rays that start inside their sphere in the even
           waves only: the odd waves hold ordinary lanes and take neither cold arm
  shells   nested dielectric shells (glass, an air bubble, a glass core) on a ground sphere, seen from
           inside a large glass sphere: every camera ray starts inside that sphere (near root below tmin,
           the far root accepted), a refracted ray starts on the sphere it entered, and the lanes of the
           same wave that test the other spheres take the near root; a wave of sky rays takes the far
           root in no lane
  ranges   clusters of 1, 2, 3 and 3 + 3 overlapping metal spheres at three primitives per leaf: leaf
           ranges of 1, 2, 3 and two sibling leaves of 3. A ray scattered by a cluster sphere starts on
           it, so its first range holds the skipped primitive at that sphere's place in its leaf — first,
           middle or last (every sphere of a leaf of three is seen; where the skipped primitive falls is
           not reported by any interface, so it is not asserted)
  and shells and ranges read from global memory (RRT_SCENE_IN_LDS=0), and tests/book2_class_scenes.py's
  class-2 composite (moving spheres, quads, dielectric field spheres: the book-2 record form of test_prim).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S
from rustraytrace_amd.render import build_bvh, decode_bvh2

import book2_class_scenes as B
import device_ops_cases as C
from test_book2_class_scenes import place
from test_gpu_device_ops import accepted, assert_same, u32
from test_gpu_leaf_arms import _exact_disc
from test_gpu_leaf_ranges import _has_hits, _leaf_env, range_lengths
from test_gpu_parity import assert_bit_exact, gpu_tile
from test_launch_plan import scene_query

F = np.float32

# node visits of the parent commit's kernel, one MI355X
NODE_VISITS = {
    "shells-lds": 91866, "shells-global": 115924, "ranges-lds": 28298, "ranges-global": 32818,
    "composite2-lds": 224151, "composite2-global": 302017,
}


# ---- the scenes ---------------------------------------------------------------------------------------
def shells():
    """Material 0 ground, 1 glass (1.5), 2 the air bubble inside glass (1 / 1.5), 3 metal."""
    rng = np.random.default_rng(11)
    lookfrom = (0.0, 2.0, 7.0)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0), S._sphere(lookfrom, 1.25, 1)]
    for i in range(9):
        c = np.array([2.2 * (i % 3) - 2.2, 0.75, 2.2 * (i // 3) - 2.2]) + rng.uniform(-0.1, 0.1, 3)
        sph += [S._sphere(c, 0.75, 1), S._sphere(c, 0.6, 2), S._sphere(c, 0.3, 1 if i % 2 else 3)]
    sph = np.concatenate(sph)
    mats = np.concatenate([S._material(0, (0.5, 0.5, 0.5)), S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5),
                           S._material(2, (1.0, 1.0, 1.0), ref_idx=1.0 / 1.5), S._material(1, (0.8, 0.6, 0.2), fuzz=0.0)])
    cam = S.make_camera(aspect_ratio=1.0, image_width=36, samples_per_pixel=4, max_depth=8, vfov=50.0,
                        lookfrom=lookfrom, lookat=(0.0, 0.5, 0.0), seed=5, n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, name="shells")


RANGE_CLUSTERS = (1, 2, 3, 6, 6, 3, 2, 1, 6)


def ranges():
    """Clusters of L overlapping metal spheres for L in RANGE_CLUSTERS (6: two clusters of 3 side by side),
    on a 3 x 3 grid over a Lambertian ground sphere."""
    rng = np.random.default_rng(3)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0)]
    for i, length in enumerate(RANGE_CLUSTERS):
        cx, cz = 3.0 * (i % 3) - 3.0, 3.0 * (i // 3) - 3.0
        for g, n in ((0, length),) if length <= 3 else ((0, 3), (1, length - 3)):
            for _ in range(n):
                sph.append(S._sphere(np.array([cx + g, 0.45, cz]) + rng.uniform(-0.05, 0.05, 3), 0.45, 1))
    sph = np.concatenate(sph)
    mats = np.concatenate([S._material(0, (0.5, 0.5, 0.5)), S._material(1, (0.7, 0.6, 0.5), fuzz=0.1)])
    cam = S.make_camera(aspect_ratio=1.0, image_width=36, samples_per_pixel=4, max_depth=8, vfov=40.0,
                        lookfrom=(0.0, 11.0, 9.0), lookat=(0.0, 0.0, 0.0), seed=7, n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, name="ranges")


TANGENT = [0, 0, 0, 0, 0, -1, 1, 0, -5, 1, np.inf]  # (o, d, c, r, closest)
SPECIAL_LANES = (0, 7, 31, 32, 50, 63)


def tangent_rows():
    """(rows, is_special, is_tangent): 32 waves of 64 rows; the even waves hold, at SPECIAL_LANES, the
    tangent ray (with `closest` beyond and before its root 5) and device_ops_cases' rays that start inside
    or on their sphere, among ordinary rows; the odd waves hold ordinary rows alone."""
    sc = C.sphere_cases()
    tang = C.f32([TANGENT, TANGENT[:10] + [6.0], TANGENT[:10] + [5.0], TANGENT[:10] + [4.0]])
    special = np.concatenate([tang, sc["inside"], sc["on_surface"][:2]])
    rows = sc["random"][:32 * 64].copy()
    assert len(rows) == 32 * 64
    is_special = np.zeros(len(rows), bool)
    is_tangent = np.zeros(len(rows), bool)
    k = 0
    for w in range(0, 32, 2):
        for lane in SPECIAL_LANES:
            rows[64 * w + lane] = special[k % len(special)]
            is_special[64 * w + lane] = True
            is_tangent[64 * w + lane] = k % len(special) < len(tang)
            k += 1
    return rows, is_special, is_tangent


# ---- on the CPU: the cases are what the GPU tests assume ----------------------------------------------
def test_tangent_rows_have_a_zero_discriminant():
    rows, is_special, is_tangent = tangent_rows()
    assert is_tangent.sum() >= 16 and (is_special & ~is_tangent).sum() >= 16
    for row in rows[is_tangent]:
        assert _exact_disc(row) == 0
    hit, root = oracle.sphere_hit_f32(rows[is_tangent])
    closest = rows[is_tangent][:, 10]
    assert np.array_equal(hit[:, 2] != 0, closest > F(5)), "the twin accepts the root 5 where `closest` is beyond it"
    assert (root[hit[:, 2] != 0, 2] == F(5)).all() and (root[:, 0] == F(5)).all()
    with np.errstate(all="ignore"):
        ordinary = [_exact_disc(r) for r in rows[~is_special][:300]]
    assert all(x < 0 or x > Fraction(1, 2 ** 60) for x in ordinary), "ordinary rows: the straight-line square root"
    assert sum(x > 0 for x in ordinary) > 30
    for w in range(32):
        assert is_special[64 * w:64 * w + 64].sum() == (len(SPECIAL_LANES) if w % 2 == 0 else 0)


def test_shells_camera_starts_inside_a_sphere():
    scene = shells()
    cr = scene.spheres["center_radius"]
    eye = np.array([0.0, 2.0, 7.0])
    inside = np.linalg.norm(cr[:, :3] - eye, axis=1) < cr[:, 3]
    assert inside.sum() == 1 and inside[1] and scene.materials["kind"][scene.spheres["material_index"][1]] == 2
    frame, rays, _ = oracle.render(scene, oracle.TWIN, threads=16)
    assert _has_hits(scene, rays) and np.isfinite(frame).all()


def test_ranges_tree_holds_the_leaf_ranges(monkeypatch):
    _leaf_env(monkeypatch, None, 3)
    scene = ranges()
    nodes, _, info = build_bvh(scene)
    assert info["node_stride"] == 80 and {1, 2, 3, 6} <= range_lengths(nodes, 80)
    _, _, first, count = decode_bvh2(nodes, 80)
    assert any(c0 == 3 and c1 == 3 and f1 == f0 + 3 for (c0, c1), (f0, f1) in zip(count, first)), "two sibling leaves of 3"
    frame, rays, _ = oracle.render(scene, oracle.TWIN, threads=16)
    assert _has_hits(scene, rays)


# ---- on the GPU ---------------------------------------------------------------------------------------
def _compare(key, scene, nodes, order, info, cls, in_lds):
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["kernel_class"] == cls and plan["scene_in_lds"] == (1 if in_lds is None else 0)
    assert scene.width <= 36 and scene.height <= 36 and scene.spp == 4
    gpu, idx, ctr, work = gpu_tile(scene, count=True)
    assert len(idx) == scene.height and np.all(gpu[..., 3] == scene.spp)
    kref, krays, ktests = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    assert _has_hits(scene, krays)
    print(f'    "{key}": {work["node_visits"]},  # rays {ctr["rays"]} (KBVH {krays}), work {work}, KBVH tests {ktests}')
    assert_bit_exact(gpu, kref, scene.spp)
    assert ctr["rays"] == krays == work["rays"]
    assert work["sphere_tests"] == ktests
    assert work["box_tests"] == 2 * work["node_visits"]
    assert work["node_visits"] == NODE_VISITS[key]


@pytest.mark.gpu
def test_zero_discriminant_among_ordinary_lanes():
    """The leaf loop's decision and root for every row are the f32 twin's, in both record forms: the
    tangent lanes' root is 5 from the library square root's 0, and the ordinary lanes of their waves, which
    take that arm with them, keep their roots."""
    rows, is_special, is_tangent = tangent_rows()
    out = _lib.device_ops("SPHERE", rows)
    hit, t = oracle.sphere_hit_f32(rows)
    closest = u32(np.ascontiguousarray(rows[:, 10]))
    for b, book in enumerate(("book 1", "book 2")):
        w = out[:, 6 * b:6 * b + 6]
        h_inf, t_inf = hit[:, b] != 0, u32(np.ascontiguousarray(t[:, b]))
        h_c, t_c = hit[:, 2 + b], u32(np.ascontiguousarray(t[:, 2 + b]))
        assert np.array_equal(accepted(w[:, 0]), h_inf), f"{book} exact_root: acceptance differs from the twin's hit"
        assert_same(f"SPHERE {book} exact_root", w[h_inf, 0], t_inf[h_inf], rows[h_inf])
        want = np.stack([h_c, np.where(h_c != 0, t_c, closest)], axis=1)  # a miss leaves `closest` as it was
        assert_same(f"SPHERE {book} test_range, special lanes", w[is_special, 2:4], want[is_special], rows[is_special])
        assert_same(f"SPHERE {book} test_range, ordinary lanes", w[~is_special, 2:4], want[~is_special], rows[~is_special])
        assert_same(f"SPHERE {book} tangent roots", w[is_tangent, 0], np.full(is_tangent.sum(), F(5)), rows[is_tangent])
        assert np.array_equal(w[is_tangent, 2] == 1, rows[is_tangent][:, 10] > F(5))


@pytest.mark.gpu
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
def test_rays_that_start_inside_spheres(monkeypatch, in_lds):
    _leaf_env(monkeypatch, in_lds, 3)
    scene = shells()
    nodes, order, info = build_bvh(scene)
    _compare(f"shells-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, -1, in_lds)


@pytest.mark.gpu
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
def test_short_leaf_ranges(monkeypatch, in_lds):
    _leaf_env(monkeypatch, in_lds, 3)
    scene = ranges()
    nodes, order, info = build_bvh(scene)
    _compare(f"ranges-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, -1, in_lds)


@pytest.mark.gpu
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
def test_book2_composite(monkeypatch, in_lds):
    place(monkeypatch, in_lds)
    monkeypatch.delenv("RRT_MAX_LEAF", raising=False)
    scene, nodes, order, info = B.built(in_lds, "composite", 2, False)
    _compare(f"composite2-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, 2, in_lds)
