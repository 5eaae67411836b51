"""GPU: the leaf loop over ranges of every length on 36 x 36 x 4 frames — bit for bit against the oracle's
walk of the kernel's tree (KBVH) and its own tree (TWIN), with the ray count of both, KBVH's sphere-test
count from the counting kernel, box tests = 2 x node visits, and the node visits of the kernel before
the loop's accept became two selects and the counting variant counted a range at once (NODE_VISITS,
recorded on one MI355X from these scenes; the oracle reports no node count).

The loop leaves the skipped primitive (exit_skip: the sphere a scattered ray leaves) out by an index
gap and accepts a root by two selects on one mask. What these frames can and cannot show of the gap:
testing the skipped record anyway changes neither a frame nor a count (its root is rejected, and the
counting kernel counts it either way), so they constrain the index stepping through wrong-neighbour
effects only — a record tested twice or never changes the hit or the tie's winner; a read past the
range's end meets another leaf's primitive. Where in a range the skipped primitive falls is not
asserted: no interface reports it. The scenes:

  clusters sibling clusters of a and b overlapping spheres for every a + b = 2 ... 14 (a = b or b - 1) on a
           ground sphere. Staged at 7 primitives per leaf the clusters are sibling leaves, and the ranges
           a walk postpones hold 1 to 14 primitives (test_trees_hold_every_range_length; at 3 per leaf
           1 to 6; read from global memory the builder keeps one primitive per leaf whatever the limit:
           1 and 2, one case). A ray scattered by a cluster sphere starts on it with the others around
           it, so its first range holds the skipped primitive, at the sphere's place in its leaf;
           camera rays skip none. Metal: the untextured specular class (C2's kernel), staged and read
           from global memory; Lambertian: the diffuse class (a staged class only)
  pairs    spheres in coincident pairs (equal centre and radius) whose two members carry different
           albedos: the root ties, the strict `<` keeps the earlier primitive in leaf order, and the
           other member's albedo would change the frame. TWIN's own tree orders a pair its own way,
           so this scene is held to KBVH alone
  media    tests/book2_class_scenes.py's class-3 composite (quads, media, moving spheres), staged and
           read from global memory: test_range's quad / medium arm beside the sphere arm
"""
import numpy as np
import pytest

from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S
from rustraytrace_amd.render import build_bvh, decode_bvh2

import book2_class_scenes as B
from test_book2_class_scenes import place
from test_gpu_parity import assert_bit_exact, gpu_tile
from test_launch_plan import scene_query

PLACEMENTS = [None, "0"]
PLACEMENT_IDS = ["lds", "global"]

# node visits of the parent kernel (branchy accept), one MI355X
NODE_VISITS = {
    "clusters1-7-lds": 35054, "clusters1-7-global": 47964, "clusters1-3-lds": 38844, "clusters0-7-lds": 34492,
    "pairs-2-lds": 45916, "pairs-2-global": 55384, "pairs-4-lds": 42455, "media-lds": 205879, "media-global": 265434,
}


def _camera(n):
    return S.make_camera(aspect_ratio=1.0, image_width=36, samples_per_pixel=4, max_depth=8, vfov=30.0,
                         lookfrom=(6.0, 2.5, 8.0), lookat=(0.0, 0.5, 0.0), seed=7, n_spheres=n)


def clusters(kind):
    """Sibling clusters of a and b = L - a overlapping spheres (a = L // 2) for L = 2 ... 14, on a 4 x 4 grid
    over a ground sphere, seen from above. kind 1: metal clusters on a Lambertian ground (class -1),
    0: Lambertian throughout (class -2)."""
    rng = np.random.default_rng(2)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0)]
    for length in range(2, 15):
        i, a = length - 2, length // 2
        cx, cz = 3.0 * (i % 4) - 4.5, 3.0 * (i // 4) - 4.5
        for g, n in ((0, a), (1, length - a)):
            for _ in range(n):
                sph.append(S._sphere(np.array([cx + g, 0.45, cz]) + rng.uniform(-0.05, 0.05, 3), 0.45, 1))
    sph = np.concatenate(sph)
    mats = np.concatenate([S._material(0, (0.5, 0.5, 0.5)), S._material(kind, (0.7, 0.6, 0.5), fuzz=0.1)])
    cam = S.make_camera(aspect_ratio=1.0, image_width=36, samples_per_pixel=4, max_depth=8, vfov=40.0,
                        lookfrom=(0.0, 14.0, 12.0), lookat=(0.0, 0.0, 0.0), seed=7, n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, name=f"clusters{kind}")


def pairs():
    """A ground sphere and 9 coincident pairs on it: member 0 of a pair red metal, member 1 blue Lambertian."""
    rng = np.random.default_rng(4)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0)]
    for i in range(9):
        c, r = (-2.0 + 2.0 * (i % 3) + rng.uniform(-0.2, 0.2), 0.0, -2.0 + 2.0 * (i // 3) + rng.uniform(-0.2, 0.2)), rng.uniform(0.5, 0.9)
        c = (c[0], r, c[2])
        sph += [S._sphere(c, r, 1), S._sphere(c, r, 2)]
    sph = np.concatenate(sph)
    mats = np.concatenate([S._material(0, (0.5, 0.5, 0.5)), S._material(1, (0.9, 0.1, 0.1), fuzz=0.0),
                           S._material(0, (0.1, 0.1, 0.9))])
    return S.SceneData(_camera(len(sph)), sph, mats, name="pairs")


def range_lengths(nodes, stride):
    """The lengths of the leaf ranges a walk of this tree can postpone: a leaf child alone, or both
    leaf children of one node."""
    _, _, _, count = decode_bvh2(nodes, stride)
    out = set()
    for c0, c1 in count:
        out |= {int(c) for c in (c0, c1) if c} | ({int(c0 + c1)} if c0 and c1 else set())
    return out


def _leaf_env(monkeypatch, in_lds, max_leaf):
    place(monkeypatch, in_lds)
    monkeypatch.setenv("RRT_MAX_LEAF", str(max_leaf))


def _has_hits(scene, rays):
    """More than three rays for every two camera rays: the frame is not sky alone."""
    return 2 * rays > 3 * scene.width * scene.height * scene.spp


def _compare(key, scene, nodes, order, info, cls, in_lds, use_twin=True):
    plan = _lib.launch_plan(**scene_query(scene, info, len(order)))
    assert plan["kernel_class"] == cls and plan["scene_in_lds"] == (1 if in_lds is None else 0)
    assert info["node_stride"] == (80 if in_lds is None else 32)
    assert (scene.width, scene.height, scene.spp) == (36, 36, 4)
    gpu, idx, ctr, work = gpu_tile(scene, count=True)
    assert len(idx) == scene.height and np.all(gpu[..., 3] == scene.spp)
    kref, krays, ktests = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    assert _has_hits(scene, krays)
    print(f'    "{key}": {work["node_visits"]},  # rays {ctr["rays"]} (KBVH {krays}), work {work}, KBVH tests {ktests}')
    assert_bit_exact(gpu, kref, scene.spp)
    assert ctr["rays"] == krays == work["rays"]
    if use_twin:
        tref, trays, _ = oracle.render(scene, oracle.TWIN, threads=16)
        assert_bit_exact(gpu, tref, scene.spp)
        assert trays == krays
    assert work["sphere_tests"] == ktests
    assert work["box_tests"] == 2 * work["node_visits"]
    assert work["node_visits"] == NODE_VISITS[key]


# ---- on the CPU: the scenes are what the GPU cases assume -------------------------------------------
def test_trees_hold_every_range_length(monkeypatch):
    """Staged at 7 primitives per leaf, the clusters are sibling leaves: ranges of 1 to 14. Trees read
    from global memory are built at one primitive per leaf whatever the limit: ranges of 1 and 2."""
    _leaf_env(monkeypatch, None, 7)
    nodes, _, info = build_bvh(clusters(1))
    assert info["node_stride"] == 80 and range_lengths(nodes, 80) == set(range(1, 15))
    _, _, first, count = decode_bvh2(nodes, 80)
    assert any(c0 == 7 and c1 == 7 and f1 == f0 + 7 for (c0, c1), (f0, f1) in zip(count, first)), "two sibling leaves of 7"
    _leaf_env(monkeypatch, None, 3)
    nodes, _, info = build_bvh(clusters(1))
    assert range_lengths(nodes, info["node_stride"]) == set(range(1, 7))
    _leaf_env(monkeypatch, "0", 7)
    nodes, _, info = build_bvh(clusters(1))
    assert info["node_stride"] == 32 and range_lengths(nodes, 32) == {1, 2}


def test_oracle_frames_have_hits(monkeypatch):
    _leaf_env(monkeypatch, None, 7)
    for scene in (clusters(1), clusters(0), pairs()):
        frame, rays, _ = oracle.render(scene, oracle.TWIN, threads=16)
        assert _has_hits(scene, rays) and np.isfinite(frame).all(), scene.name
    place(monkeypatch, None)
    monkeypatch.delenv("RRT_MAX_LEAF", raising=False)
    scene = B.built(None, "composite", 3, False)[0]
    _, rays, _ = oracle.render(scene, oracle.TWIN, threads=16)
    assert _has_hits(scene, rays)


def test_pairs_tie_and_the_winner_shows(monkeypatch):
    """Each pair shares centre and radius; swapping the members' albedos changes the oracle's frame, so
    the frame depends on which member of a tie wins."""
    _leaf_env(monkeypatch, None, 4)
    scene = pairs()
    cr = scene.spheres["center_radius"]
    assert all(np.array_equal(cr[1 + 2 * i], cr[2 + 2 * i]) for i in range(9))
    nodes, order, info = build_bvh(scene)
    a, _, _ = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    import dataclasses

    mats = scene.materials.copy()
    mats[[1, 2]] = mats[[2, 1]]
    b, _, _ = oracle.render_kbvh(dataclasses.replace(scene, materials=mats), nodes, order, info, threads=16)
    assert not np.array_equal(a, b)


# ---- on the GPU ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_leaf,in_lds", [(7, None), (3, None), (7, "0")], ids=["7-lds", "3-lds", "7-global"])
def test_specular_ranges(monkeypatch, max_leaf, in_lds):
    _leaf_env(monkeypatch, in_lds, max_leaf)
    scene = clusters(1)
    nodes, order, info = build_bvh(scene)
    _compare(f"clusters1-{max_leaf}-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, -1, in_lds)


@pytest.mark.gpu
def test_diffuse_ranges(monkeypatch):
    """Staged only: read from global memory a diffuse scene runs the specular class's kernel."""
    _leaf_env(monkeypatch, None, 7)
    scene = clusters(0)
    nodes, order, info = build_bvh(scene)
    _compare("clusters0-7-lds", scene, nodes, order, info, -2, None)


@pytest.mark.gpu
@pytest.mark.parametrize("max_leaf,in_lds", [(2, None), (4, None), (2, "0")], ids=["2-lds", "4-lds", "2-global"])
def test_coincident_pairs_keep_the_earlier_primitive(monkeypatch, max_leaf, in_lds):
    _leaf_env(monkeypatch, in_lds, max_leaf)
    scene = pairs()
    nodes, order, info = build_bvh(scene)
    _compare(f"pairs-{max_leaf}-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, -1, in_lds,
             use_twin=False)


@pytest.mark.gpu
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
def test_quads_and_media(monkeypatch, in_lds):
    place(monkeypatch, in_lds)
    monkeypatch.delenv("RRT_MAX_LEAF", raising=False)
    scene, nodes, order, info = B.built(in_lds, "composite", 3, False)
    _compare(f"media-{'lds' if in_lds is None else 'global'}", scene, nodes, order, info, 3, in_lds)
