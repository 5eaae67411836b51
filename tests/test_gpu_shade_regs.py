"""GPU: the shading pass after the path state left scratch — the state word (bounce index, need_ray, has),
the next origin and direction stored before the path-ending arms, T * att formed ahead of the roulette
split, ray_consts' one ballot over the three slopes — on 36 x 36 x 4
frames at max_depth 12, bit for bit against the oracle's walk of the kernel's tree (KBVH), with KBVH's ray
and sphere-test counts, the oracle's path count, box tests = 2 x node visits, and the node visits of the
kernel before the change (NODE_VISITS, recorded on one MI355X from these scenes with the parent commit's
library; the oracle reports no node count).

  mix        a Lambertian ground, Lambertian, metal (fuzz 0.2: some scattered rays are absorbed) and
             dielectric spheres under the sky, defocus on: the untextured book-1 class; with the earth
             texture on one sphere the textured class
  diffuse    Lambertian spheres and an emitter under a background colour (bg_mode 1): the diffuse-only
             class when staged, the untextured one when read from global memory
  composite  tests/book2_class_scenes.py's class-2 composite (moving spheres, quads, dielectrics)
  each staged in LDS and read from global memory (RRT_SCENE_IN_LDS=0). At depth 12 a path passes bounce
  5, so the roulette arm and both throughput updates run (the CPU test below: more rays than at depth 5).

Pointwise, through rrt_testing_device_ops, rows at lane i % 64. Direction components of +-0, subnormal,
+-2^-126, >= 2^126, +-inf and NaN sit at SPECIAL_LANES of the even waves among ordinary rows; the odd waves
hold ordinary rows only, so a wave takes ray_consts' cold arm beside hot lanes and its neighbour does not
take it; two more waves hold a special component in every lane.
  SLOPES  reads ray_consts' fields out: inv must equal clamped_slope of each component (the form before
          the change, run on the device beside it) bit for bit, and numpy's clamp of the IEEE 1 / s wherever
          clamped_slope claims it (|s| < 2^126, NaN, zero and subnormal included); oi, the plane-pair
          offsets and the packed rotations follow from inv. This is the check of slope_normal, the class
          mask and the cold arm's select.
  SPHERE  the sphere tests behind ray_consts (they read rk.a and rk.ra, not the slopes): the special
          directions through div_by_a's and the square root's guarded arms, as the issue asks.
  VEC     unit() on the same special components. unit() is not changed here; the rows pin its values for
          the directions the other two ops use.
"""
import numpy as np
import pytest

from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S
from rustraytrace_amd.render import build_bvh

import book2_class_scenes as B
import device_ops_cases as C
from test_book2_class_scenes import place
from test_gpu_device_ops import assert_same
from test_gpu_leaf_ranges import _has_hits
from test_gpu_parity import assert_bit_exact, gpu_tile
from test_launch_plan import scene_query

F = np.float32

# node visits of the parent commit's kernel, one MI355X
NODE_VISITS = {
    "diffuse-lds": 41719, "diffuse-global": 50274, "mix-lds": 54079, "mix-global": 69829,
    "mix-textured-lds": 53945, "mix-textured-global": 69647, "composite2-lds": 224151, "composite2-global": 302017,
}


# ---- the scenes ---------------------------------------------------------------------------------------
def mix(textured, max_depth=12):
    """Material 0 ground, 1 Lambertian, 2 metal, 3 glass, 4 the air inside glass, 5 the earth texture (or a
    second Lambertian)."""
    rng = np.random.default_rng(29)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0), S._sphere((-2.2, 1.0, 0.0), 1.0, 5),
           S._sphere((0.0, 1.0, 0.0), 1.0, 3), S._sphere((0.0, 1.0, 0.0), 0.8, 4), S._sphere((2.2, 1.0, 0.0), 1.0, 2)]
    for i in range(24):
        c = np.array([1.1 * (i % 6) - 2.75, 0.25, 1.6 + 0.7 * (i // 6)]) + rng.uniform(-0.1, 0.1, 3) * (1, 0, 1)
        sph.append(S._sphere(c, 0.25, 1 + i % 3))
    sph = np.concatenate(sph)
    mats = np.concatenate([S._material(0, (0.5, 0.5, 0.5)), S._material(0, (0.8, 0.3, 0.2)),
                           S._material(1, (0.8, 0.7, 0.6), fuzz=0.2), S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5),
                           S._material(2, (1.0, 1.0, 1.0), ref_idx=1.0 / 1.5),
                           S._material(3 if textured else 0, (0.4, 0.6, 0.8), tex=0)])
    cam = S.make_camera(aspect_ratio=1.0, image_width=36, samples_per_pixel=4, max_depth=max_depth, vfov=35.0,
                        lookfrom=(1.5, 2.5, 9.0), lookat=(0.0, 0.7, 0.0), defocus_angle=0.5, focus_dist=9.0,
                        seed=13, n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, textures=[S.earth_texture()] if textured else [],
                       name="mix-textured" if textured else "mix")


def diffuse(max_depth=12):
    """Lambertian spheres and one emitter under a dim background colour."""
    rng = np.random.default_rng(31)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0), S._sphere((0.0, 3.2, 0.0), 1.0, 3)]
    for i in range(20):
        c = np.array([1.3 * (i % 5) - 2.6, 0.5, 1.3 * (i // 5) - 2.0]) + rng.uniform(-0.15, 0.15, 3) * (1, 0, 1)
        sph.append(S._sphere(c, 0.5, 1 + i % 2))
    sph = np.concatenate(sph)
    mats = np.concatenate([S._material(0, (0.6, 0.6, 0.6)), S._material(0, (0.9, 0.8, 0.7)),
                           S._material(0, (0.2, 0.4, 0.9)), S._material(4, (4.0, 4.0, 3.0))])
    cam = S.make_camera(aspect_ratio=1.0, image_width=36, samples_per_pixel=4, max_depth=max_depth, vfov=40.0,
                        lookfrom=(0.0, 4.0, 9.0), lookat=(0.0, 0.8, 0.0), background=(0.1, 0.15, 0.2),
                        seed=17, n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, name="diffuse")


SCENES = {"mix": lambda **kw: mix(False, **kw), "mix-textured": lambda **kw: mix(True, **kw), "diffuse": diffuse}
# kernel class staged in LDS / read from global memory
CLASSES = {"mix": (-1, -1), "mix-textured": (0, 0), "diffuse": (-2, -1)}

SPECIAL = [0.0, -0.0, 2.0 ** -140, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126), 2.0 ** 126, -(2.0 ** 127),
           1.5 * 2.0 ** 127, np.inf, -np.inf, np.nan]
SPECIAL_LANES = (0, 7, 31, 32, 50, 63)
WAVES = 16


def special_rows(ordinary, first_col):
    """(rows, is_special): WAVES waves of 64 rows of `ordinary`; in the even waves the rows at SPECIAL_LANES
    have one of the three components from column `first_col` on replaced by a SPECIAL value (every value in
    every component), the odd waves stay ordinary."""
    rows = np.array(ordinary[:WAVES * 64], dtype=F)
    assert len(rows) == WAVES * 64
    is_special = np.zeros(len(rows), bool)
    k = 0
    for w in range(0, WAVES, 2):
        for lane in SPECIAL_LANES:
            rows[64 * w + lane, first_col + k % 3] = F(SPECIAL[(k // 3) % len(SPECIAL)])
            is_special[64 * w + lane] = True
            k += 1
    assert k >= 3 * len(SPECIAL)
    return rows, is_special


def sphere_rows():
    return special_rows(C.sphere_cases()["random"], 3)  # (o, d, c, r, closest): d


def slope_rows():
    """(o, d) of sphere_rows, then two waves whose every lane holds a special component (lane l: SPECIAL
    value l % 12 in component l % 3, the next value in the next component for the second wave's lanes)."""
    rows, is_special = sphere_rows()
    rows = rows[:, :6]
    extra = np.array(C.sphere_cases()["random"][WAVES * 64:WAVES * 64 + 128], dtype=F)[:, :6]
    assert len(extra) == 128
    for i in range(128):
        extra[i, 3 + i % 3] = F(SPECIAL[i % len(SPECIAL)])
        if i >= 64:
            extra[i, 3 + (i + 1) % 3] = F(SPECIAL[(i + 5) % len(SPECIAL)])
    return np.concatenate([rows, extra]), np.concatenate([is_special, np.ones(128, bool)])


def vec_rows():
    rng = np.random.default_rng(0x5AD3)
    v, n = rng.normal(size=(WAVES * 64, 3)), rng.normal(size=(WAVES * 64, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    e = rng.choice([1 / 1.5, 1.5, 1.0], (len(v), 1))
    cosine = rng.uniform(0, 1, (len(v), 1))
    r0 = ((1 - e) / (1 + e)) ** 2
    return special_rows(np.concatenate([v, n, e, cosine, r0], axis=1).astype(F), 0)  # (v, n, e, cosine, r0): v


# ---- on the CPU: the cases are what the GPU tests assume ----------------------------------------------
@pytest.fixture(scope="module")
def twin_rays():
    """Rays the oracle traces through each frame scene at depths 12 and 5 (computed once)."""
    return {name: tuple(oracle.render(make(max_depth=d), oracle.TWIN, threads=16)[1] for d in (12, 5))
            for name, make in SCENES.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_paths_pass_the_roulette_depth(twin_rays, name):
    deep, shallow = twin_rays[name]
    print(f"{name}: {deep} rays at depth 12, {shallow} at depth 5")
    assert deep > shallow, "paths reach bounce 5: the roulette arm and both throughput updates run"
    assert _has_hits(SCENES[name](), deep)


def test_mix_holds_every_book1_kind():
    for textured in (False, True):
        scene = mix(textured)
        kinds = set(scene.materials["kind"][scene.spheres["material_index"]].tolist())
        assert kinds == ({0, 1, 2, 3} if textured else {0, 1, 2})
    scene = diffuse()
    assert set(scene.materials["kind"].tolist()) == {0, 4} and int(scene.camera["params_u"][0, 3]) == 1


def test_special_rows_sit_in_the_even_waves():
    for (rows, is_special), col in ((sphere_rows(), 3), (vec_rows(), 0)):
        for w in range(WAVES):
            assert is_special[64 * w:64 * w + 64].sum() == (len(SPECIAL_LANES) if w % 2 == 0 else 0)
        assert np.isfinite(rows[~is_special, col:col + 3]).all()
    rows, is_special = sphere_rows()
    d = rows[is_special, 3:6]
    a = np.abs(d)
    tiny = F(2.0 ** -126)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            col = d[:, c]
            assert (col == 0).any() and ((a[:, c] > 0) & (a[:, c] < tiny)).any() and (a[:, c] == tiny).any()
            assert ((a[:, c] >= F(2.0 ** 126)) & np.isfinite(col)).any() and np.isinf(col).any() and np.isnan(col).any()
    normal = np.abs(rows[~is_special, 3:6])
    assert (normal >= tiny).all(), "ordinary rows stay on ray_consts' straight-line path"


# ---- on the GPU ---------------------------------------------------------------------------------------
def _compare(key, scene, nodes, order, info, cls, in_lds):
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["kernel_class"] == cls and plan["scene_in_lds"] == (1 if in_lds is None else 0)
    assert scene.width <= 36 and scene.height <= 36 and scene.spp == 4
    gpu, idx, ctr, work = gpu_tile(scene, count=True)
    assert len(idx) == scene.height and np.all(gpu[..., 3] == scene.spp)
    kref, krays, ktests = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    assert _has_hits(scene, krays)
    print(f'    "{key}": {work["node_visits"]},  # rays {ctr["rays"]} (KBVH {krays}), paths {ctr["paths"]}, work {work}, '
          f'KBVH tests {ktests}')
    assert_bit_exact(gpu, kref, scene.spp)
    assert ctr["rays"] == krays == work["rays"]
    assert ctr["paths"] == scene.width * scene.height * scene.spp  # the oracle's: one path per sample
    assert work["sphere_tests"] == ktests
    assert work["box_tests"] == 2 * work["node_visits"]
    assert work["node_visits"] == NODE_VISITS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_book1_classes_at_depth_12(monkeypatch, name, in_lds):
    place(monkeypatch, in_lds)
    monkeypatch.delenv("RRT_MAX_LEAF", raising=False)
    scene = SCENES[name]()
    assert scene.max_depth == 12
    nodes, order, info = build_bvh(scene)
    _compare(f"{name}-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info,
             CLASSES[name][0 if in_lds is None else 1], in_lds)


@pytest.mark.gpu
@pytest.mark.parametrize("in_lds", [None, "0"], ids=["lds", "global"])
def test_book2_composite(monkeypatch, in_lds):
    place(monkeypatch, in_lds)
    monkeypatch.delenv("RRT_MAX_LEAF", raising=False)
    scene, nodes, order, info = B.built(in_lds, "composite", 2, False)
    _compare(f"composite2-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, 2, in_lds)


def expected_slopes(d):
    """(clamp of numpy's IEEE 1 / s to +-2^64 with a NaN giving +2^64 and |s| < 2^-126 the signed bound,
    where clamped_slope claims that value): per component of d."""
    big = F(2.0 ** 64)
    with np.errstate(all="ignore"):
        q = F(1) / d
        want = np.where(np.isnan(q), big, np.minimum(np.maximum(q, -big), big)).astype(F)
        want = np.where(np.abs(d) < F(2.0 ** -126), np.copysign(big, d), want).astype(F)
        claimed = ~(np.abs(d) >= F(2.0 ** 126)) | np.isinf(d)
    return want, claimed


def test_expected_slopes_on_known_values():
    d = np.array([2.0, -0.5, 0.0, -0.0, 2.0 ** -140, -(2.0 ** -126), np.inf, -np.inf, np.nan, 2.0 ** -70], F)
    want, claimed = expected_slopes(d)
    big = 2.0 ** 64
    assert claimed.all()
    assert np.array_equal(want.view(np.uint32), np.array([0.5, -2.0, big, -big, big, -big, 0.0, -0.0, big, big], F).view(np.uint32))
    assert not expected_slopes(np.array([2.0 ** 126, -(2.0 ** 127)], F))[1].any()


@pytest.mark.gpu
def test_ray_consts_slopes_cold_arm_beside_hot_lanes():
    rows, is_special = slope_rows()
    out = _lib.device_ops("SLOPES", rows)
    o, d = rows[:, :3], rows[:, 3:6]
    inv = np.ascontiguousarray(out[:, 0:3]).view(F)
    for sel, what in ((is_special, "special lanes"), (~is_special, "ordinary lanes")):
        assert_same(f"SLOPES inv against clamped_slope per component, {what}", out[sel, 0:3], out[sel, 9:12], rows[sel])
    want, claimed = expected_slopes(d)
    assert claimed[~is_special].all() and claimed.sum() > 3 * len(rows) - 3 * 128
    got = np.where(claimed, inv, want).astype(F)  # unclaimed components (|s| >= 2^126, finite) pass through
    assert_same("SLOPES inv against the clamped IEEE reciprocal", got, want, rows)
    with np.errstate(all="ignore"):
        assert_same("SLOPES oi = o * inv", out[:, 3:6], (o * inv).astype(F), rows)
    neg = inv < 0
    offs = np.stack([np.where(neg[:, 0], 4, 0), np.where(neg[:, 1], 16, 12), np.where(neg[:, 2], 28, 24)], axis=1)
    assert np.array_equal(out[:, 6:9], offs.astype(np.uint32)), "plane-pair offsets of a staged node"
    packed = neg[:, 0] * 16 + neg[:, 1] * (16 << 5) + neg[:, 2] * (16 << 10)
    assert np.array_equal(out[:, 12], packed.astype(np.uint32)), "packed rotations of the f16 nodes"
    assert neg[~is_special].any() and (~neg[~is_special]).any()


@pytest.mark.gpu
def test_sphere_tests_of_special_directions():
    """Every word of the SPHERE op equals the f32 twin's, special and ordinary lanes alike (the twin's
    acceptance, roots and test_range results; NaNs equal as a class)."""
    rows, is_special = sphere_rows()
    out = _lib.device_ops("SPHERE", rows)
    hit, t = oracle.sphere_hit_f32(rows)
    closest = np.ascontiguousarray(rows[:, 10]).view(np.uint32)
    for b, book in enumerate(("book 1", "book 2")):
        w = out[:, 6 * b:6 * b + 6]
        h_c, t_c = hit[:, 2 + b], np.ascontiguousarray(t[:, 2 + b]).view(np.uint32)
        want = np.stack([h_c, np.where(h_c != 0, t_c, closest)], axis=1)  # a miss leaves `closest` as it was
        for sel, what in ((is_special, "special lanes"), (~is_special, "ordinary lanes")):
            assert_same(f"SPHERE {book} test_range, {what}", w[sel, 2:4], want[sel], rows[sel])
            assert_same(f"SPHERE {book} test_range by the per-ray reciprocal, {what}", w[sel, 4:6], want[sel], rows[sel])
    assert_same("SPHERE sphere_root", out[:, 12], hit[:, 4], rows)


@pytest.mark.gpu
def test_unit_of_special_directions():
    rows, is_special = vec_rows()
    out, want = _lib.device_ops("VEC", rows), oracle.vec_f32(rows)
    for sel, what in ((is_special, "special lanes"), (~is_special, "ordinary lanes")):
        assert_same(f"VEC unit, {what}", out[sel, :3], want[sel, :3], rows[sel])
    assert_same("VEC, ordinary lanes", out[~is_special], want[~is_special], rows[~is_special])
