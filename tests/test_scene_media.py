"""Constant media in the world-change entries, without a GPU: the classification the GPU tests assume
(rrt_build_bvh_binned's n_unbounded), rrt_testing_medium_records (the host compilation of
rrt_medium_form.h, the one definition of what a medium contributes) against numpy, and
rrt_refit_bvh_binned_world, the host twin that defines rrt_scene_refit_world's tree. Nothing compares
with a tolerance."""
import ctypes
import os
import re

import numpy as np
import pytest

import rustraytrace_amd as rrt
from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned, decode_bvh2, refit_bvh_binned_world

import device_bvh_scenes as D
import media_scenes as M
from test_bvh_binned import _pad, _quad_boxes, f32_outward, prim_boxes
from test_bvh_refit import child_unions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt_hip.h")
NODE_COST = 2.0

PROTOTYPES = (
    "int32_t rrt_scene_update_world(RrtScene *scene, const RrtSceneGeometry *geometry, const RrtSceneMedia *media, "
    "void *stream);",
    "int32_t rrt_scene_refit_world(RrtScene *scene, const RrtSceneGeometry *geometry, const RrtSceneMedia *media, "
    "void *stream);",
    "int32_t rrt_refit_bvh_binned_world(const RrtSphere *built_spheres, uint32_t n_spheres, const RrtSceneExt *built_ext, "
    "uint32_t max_leaf, double node_cost, uint32_t node_stride, const RrtSphere *new_spheres, const RrtSceneExt *new_ext, "
    "void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out, RrtBvhInfo *info, double *sah_out);",
    "int32_t rrt_testing_medium_records(const RrtMedium *media, uint32_t n_media, const RrtQuad *boundary_quads, "
    "uint32_t n_boundary_quads, uint32_t n_quads, double *boxes6, void *gmedium);",
)


# ---- 0. the ABI ----------------------------------------------------------------------------------
def test_entry_points_are_exported_with_the_headers_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    lib = _lib.load()
    for proto in PROTOTYPES:
        assert proto in flat, proto
        name = re.search(r"(rrt_\w+)\(", proto).group(1)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert ("typedef struct RrtSceneMedia { const RrtMedium *media; uint32_t n_media; uint32_t n_boundary_quads; "
            "const RrtQuad *boundary_quads; } RrtSceneMedia;") in flat
    assert ctypes.sizeof(_lib.RrtSceneMedia) == 24
    assert re.search(r"RRT_TABLE_GMEDIA = 10\b", flat) and _lib.SCENE_MEDIA_TABLES["gmedia"][0] == 10
    assert "gmedia" not in _lib.SCENE_GEOMETRY_TABLES
    assert lib.rrt_hip_abi_version() == 11


def test_null_scene_is_refused_without_a_device():
    lib = _lib.load()
    g = _lib.RrtSceneGeometry()
    for name in ("rrt_scene_update_world", "rrt_scene_refit_world"):
        assert getattr(lib, name)(None, ctypes.byref(g), None, None) == -1, name
        msg = lib.rrt_hip_last_error().decode()
        assert name in msg and "null scene" in msg, msg


# ---- 1. the classification the GPU tests assume ---------------------------------------------------
def n_unbounded(sc):
    return build_bvh_binned(sc, 3, NODE_COST, 80)[2]["n_unbounded"]


def test_the_scenes_classify_as_the_gpu_tests_assume():
    fog, fog5 = M.scene("fog"), M.scene("fog5")
    assert (len(fog.spheres), len(fog.quads), len(fog.media), len(fog.boundary_quads)) == (24, 4, 3, 6)
    assert np.count_nonzero(np.abs(fog.motion[:, :3]).sum(axis=1)) == 6
    assert len(fog5.media) == 7 and (fog5.media["sphere"][2:] == (0.0, 0.0, 0.0, M.FOG_RADIUS)).all()
    assert (fog5.media["boundary_kind"][2:] == 0).all() and len(set(fog5.media["density"][2:])) == 1
    assert n_unbounded(fog) == 1
    nodes, order, info = build_bvh_binned(fog5, 3, NODE_COST, 80)
    first_medium = len(fog5.spheres) + len(fog5.quads)
    assert info["n_unbounded"] == 4  # the kMaxUnbounded cap
    assert list(order[-4:]) == [first_medium + m for m in (2, 3, 4, 5)] and first_medium + 6 in order[:-4]
    assert n_unbounded(M.sphere0_far(fog)) == 0
    assert n_unbounded(M.fog_radius(fog, 1.0)) == 0
    nw8, nw9, b3 = M.scene("NW8"), M.scene("NW9"), M.scene("B3media")
    assert (len(nw8.quads), len(nw8.media), len(nw8.boundary_quads)) == (6, 2, 12) and n_unbounded(nw8) == 0
    assert (len(nw9.spheres), len(nw9.quads), len(nw9.media)) == (1006, 2401, 2) and n_unbounded(nw9) == 1
    assert sorted(b3.media["boundary_kind"]) == [0, 1] and b3.lights is not None


# ---- 2. rrt_testing_medium_records against numpy ---------------------------------------------------
def medium(sphere=(0, 0, 0, 0), kind=0, first=0, count=0, mat=0, density=1.0):
    r = np.zeros(1, dtype=_lib.MEDIUM_DTYPE)
    r["sphere"][0], r["boundary_kind"][0], r["first"][0], r["count"][0] = sphere, kind, first, count
    r["material_index"][0], r["density"][0] = mat, density
    return r


def numpy_medium_boxes(media, bquads):
    """A sphere boundary: [c - max(r, 0), c + max(r, 0)] in f64, padded (aabb.rs:104-115: an axis
    thinner than 1e-4 grows by 5e-5 on either side). A quad boundary: the boundary quads' padded boxes
    folded in range order from the empty box, the pad applied after every fold as Aabb::from_boxes
    does — so the thin axis of an axis-aligned face, whose own pad leaves it a rounding short of 1e-4,
    is padded once more by the first fold."""
    qlo, qhi = _quad_boxes(bquads) if bquads is not None else (None, None)
    out = np.zeros((len(media), 6))
    for m, md in enumerate(media):
        if md["boundary_kind"] == 0:
            c, r = md["sphere"][:3].astype(np.float64), max(np.float64(md["sphere"][3]), 0.0)
            lo, hi = _pad(c - r, c + r)
        else:
            lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
            for k in range(int(md["first"]), int(md["first"]) + int(md["count"])):
                lo, hi = _pad(np.minimum(lo, qlo[k]), np.maximum(hi, qhi[k]))
        out[m, :3], out[m, 3:] = lo, hi
    return out


@pytest.mark.parametrize("name", ["fog", "NW8", "NW9", "B3media"])
def test_medium_boxes_are_the_numpy_specification(name):
    sc = M.scene(name)
    boxes, _ = _lib.medium_records(sc.media, sc.boundary_quads, len(sc.quads))
    assert boxes.tobytes() == numpy_medium_boxes(sc.media, sc.boundary_quads).tobytes()
    if name in ("NW8", "NW9"):  # tests/test_bvh_binned.py's specification, exact for spheres and rotated boxes
        plo, phi = prim_boxes(sc)
        first = len(sc.spheres) + len(sc.quads)
        assert boxes[:, :3].tobytes() == plo[first:].tobytes() and boxes[:, 3:].tobytes() == phi[first:].tobytes()
    assert {int(k) for k in sc.media["boundary_kind"]} == ({1} if name == "NW8" else {0} if name == "NW9" else {0, 1})


def test_medium_boxes_are_padded_and_clamp_the_radius():
    bq = np.concatenate([G_quad((1, 2, 3), (2, 0, 0), (0, 0.5, 0)), G_quad((1, 2, 3), (0, 0, 0.25), (2, 0, 0))])
    md = np.concatenate([medium((1, 2, 3, 0.0)), medium((1, 2, 3, -4.0)), medium((0.5, 0, 0, 2.0)),
                         medium(kind=1, first=0, count=1), medium(kind=1, first=0, count=2)])
    boxes, _ = _lib.medium_records(md, bq)
    d = 0.0001 / 2.0
    point = [1 - d, 2 - d, 3 - d, 1 + d, 2 + d, 3 + d]
    assert boxes[0].tolist() == point and boxes[1].tolist() == point  # r = 0 and max(r, 0): padded on every axis
    assert boxes[2].tolist() == [-1.5, -2.0, -2.0, 2.5, 2.0, 2.0]
    # a flat quad: padded along its normal, and once more by the fold ((3 + d) - (3 - d) rounds below 1e-4)
    assert (3 + d) - (3 - d) < 0.0001
    assert boxes[3].tolist() == [1.0, 2.0, 3 - d - d, 3.0, 2.5, 3 + d + d]
    assert boxes[4].tolist() == [1.0, 2 - d, 3 - d - d, 3.0, 2.5, 3.25]  # the union keeps what each fold padded
    assert boxes.tobytes() == numpy_medium_boxes(md, bq).tobytes()


def G_quad(q, u, v):
    r = np.zeros(1, dtype=_lib.QUAD_DTYPE)
    r["q"][0, :3], r["u"][0, :3], r["v"][0, :3] = q, u, v
    return r


def test_medium_records_are_the_numpy_specification():
    densities = np.array([0.01, 0.0001, 1.0, 3.0, 0.7, 1e-30, 3e38, 0.008], np.float32)
    md = np.concatenate([medium((k, -k, 0.5 * k, k - 2.0), kind=k % 2, first=3 * k, count=(k % 2) * 6, density=d)
                         for k, d in enumerate(densities)])
    bq = np.concatenate([G_quad((j, 0, 0), (1, 0, 0), (0, 1, 0)) for j in range(30)])
    for n_quads in (0, 7, 2401):
        _, g = _lib.medium_records(md, bq, n_quads)
        assert g.dtype == _lib.GMEDIUM_DTYPE
        want_sphere = md["sphere"].copy()
        want_sphere[:, 3] = np.maximum(want_sphere[:, 3], np.float32(0.0))
        assert g["sphere"].tobytes() == want_sphere.tobytes()
        assert np.array_equal(g["kind"], md["boundary_kind"]) and np.array_equal(g["count"], md["count"])
        assert np.array_equal(g["first"], n_quads + md["first"])
        want = np.array([np.float32(-1.0 / np.float64(d)) for d in densities], np.float32)
        assert g["neg_inv_density"].tobytes() == want.tobytes()


def test_medium_records_refuse_a_range_outside_the_boundary_quads():
    bq = G_quad((0, 0, 0), (1, 0, 0), (0, 1, 0))
    for bad in (medium(kind=1, first=0, count=2), medium(kind=1, first=1, count=1), medium(kind=1, count=0), medium(kind=2)):
        with pytest.raises(rrt.RrtError) as e:
            _lib.medium_records(bad, bq)
        assert e.value.code == -1 and "rrt_testing_medium_records" in str(e.value)


@pytest.mark.parametrize("name", ["NW8", "NW9"])
def test_medium_boxes_are_the_builders_stored_leaf_boxes(name):
    """With single-primitive leaves every medium of the tree is a leaf of its own, whose stored box is
    the medium's box grown by the slab test's slack and rounded outward to f32 (tests/test_bvh_refit.py's
    specification of a stored box)."""
    sc = M.scene(name)
    boxes, _ = _lib.medium_records(sc.media, sc.boundary_quads, len(sc.quads))
    tree = build_bvh_binned(sc, 1, NODE_COST, 80)
    nodes, order, info = tree
    _, _, _, (root_lo, root_hi), (lo, hi, first, cnt) = child_unions(tree, sc)
    o = np.maximum(np.abs(root_lo), np.abs(root_hi))
    grow = lambda p: 4.0 * 2.0 ** -24 * (2.0 * np.abs(p) + 3.0 * o)
    first_medium = len(sc.spheres) + len(sc.quads)
    n_tree = len(order) - info["n_unbounded"]
    seen = 0
    for m in range(len(sc.media)):
        at = np.flatnonzero(order[:n_tree] == first_medium + m)
        if not len(at):  # tested after the walk: final_scene's fog
            assert name == "NW9" and first_medium + m in order[n_tree:]
            continue
        k, c = np.argwhere((cnt == 1) & (first == at[0]))[0]
        want_lo, want_hi = f32_outward(boxes[m, :3] - grow(boxes[m, :3]), boxes[m, 3:] + grow(boxes[m, 3:]))
        assert np.array_equal(lo[k, c], want_lo) and np.array_equal(hi[k, c], want_hi)
        seen += 1
    assert seen == len(sc.media) - info["n_unbounded"] and seen >= 1


# ---- 3. rrt_refit_bvh_binned_world ----------------------------------------------------------------
SCENES = ["fog", "fog5", "NW8", "NW9", "B3media"]


@pytest.mark.parametrize("max_leaf,stride", D.SHAPES)
@pytest.mark.parametrize("name", SCENES)
def test_refit_over_unchanged_inputs_is_the_built_tree(name, max_leaf, stride):
    sc = M.scene(name)
    built = build_bvh_binned(sc, max_leaf, NODE_COST, stride)
    nodes, order, info, sah = refit_bvh_binned_world(sc, sc, max_leaf, NODE_COST, stride)
    assert info == built[2]
    assert np.array_equal(order, built[1])
    assert nodes.tobytes() == built[0].tobytes()
    assert np.isfinite(sah) and sah > 0.0


@pytest.mark.parametrize("seed,amount", [(11, 0.01), (12, 0.3)])
@pytest.mark.parametrize("name", SCENES)
def test_stored_boxes_contain_the_moved_primitives(name, seed, amount):
    sc = M.scene(name)
    new = M.moved(sc, seed, amount)
    assert new.media.tobytes() != sc.media.tobytes()
    assert sc.boundary_quads is None or new.boundary_quads.tobytes() != sc.boundary_quads.tobytes()
    built = build_bvh_binned(sc, 3, NODE_COST, 80)
    at_build = refit_bvh_binned_world(sc, sc, 3, NODE_COST, 80)[3]
    tree = refit_bvh_binned_world(sc, new, 3, NODE_COST, 80)
    nodes, order, info, sah = tree
    assert info == built[2] and np.array_equal(order, built[1]), "a refit keeps the classification and the leaf order"
    b_first, b_cnt = decode_bvh2(built[0], 80)[2:]
    ulo, uhi, real, _, (lo, hi, first, cnt) = child_unions(tree, new)
    assert np.array_equal(first, b_first) and np.array_equal(cnt, b_cnt), "the refit changed a link"
    assert nodes.tobytes() != built[0].tobytes(), "the move did not change a box"
    assert (lo[real].astype(np.float64) <= ulo[real]).all() and (hi[real].astype(np.float64) >= uhi[real]).all()
    assert np.isfinite(sah) and sah != at_build


def test_a_moved_medium_alone_moves_its_leaf_box():
    sc = M.scene("fog")
    md = sc.media.copy()
    md["sphere"][0, :3] += np.float32(0.25)
    bq = sc.boundary_quads.copy()
    bq["q"][:, 1] += np.float32(0.5)
    for new in (M.with_world(sc, motion=sc.motion, media=md), M.with_world(sc, motion=sc.motion, boundary_quads=bq)):
        tree = refit_bvh_binned_world(sc, new, 3, NODE_COST, 80)
        ulo, uhi, real, _, (lo, hi, _, _) = child_unions(tree, new)
        assert tree[0].tobytes() != build_bvh_binned(sc, 3, NODE_COST, 80)[0].tobytes()
        assert (lo[real].astype(np.float64) <= ulo[real]).all() and (hi[real].astype(np.float64) >= uhi[real]).all()


@pytest.mark.parametrize("seed,amount", [(11, 0.01), (12, 0.3)])
@pytest.mark.parametrize("name", ["fog", "NW8"])
def test_walking_the_refit_tree_renders_the_linear_scan(name, seed, amount):
    sc = M.scene(name)
    new = M.moved(sc, seed, amount)
    nodes, order, info, _ = refit_bvh_binned_world(sc, new, 3, NODE_COST, 80)
    kacc, krays, _ = oracle.render_kbvh(new, nodes, order, info, threads=8)
    tacc, trays, _ = oracle.render(new, oracle.TWIN, threads=8)
    assert np.array_equal(kacc, tacc)
    assert krays == trays


def test_an_unbounded_medium_stays_outside_a_refitted_tree():
    sc = M.scene("fog")
    new = M.sphere0_far(sc)  # a fresh build would take the fog into the tree; the refit keeps it outside
    nodes, order, info, _ = refit_bvh_binned_world(sc, new, 3, NODE_COST, 80)
    assert info["n_unbounded"] == 1 and order[-1] == len(sc.spheres) + len(sc.quads) + 2
    kacc, krays, _ = oracle.render_kbvh(new, nodes, order, info, threads=8)
    tacc, trays, _ = oracle.render(new, oracle.TWIN, threads=8)
    assert np.array_equal(kacc, tacc) and krays == trays


@pytest.mark.parametrize("field,value", [("boundary_kind", 1), ("first", 1), ("count", 5)])
def test_a_changed_structure_is_refused(field, value):
    sc = M.scene("fog")
    md = sc.media.copy()
    m = 0 if field == "boundary_kind" else 1  # the sphere medium turned into quads; the box medium's range
    md[field][m] = value
    with pytest.raises(rrt.RrtError) as e:
        refit_bvh_binned_world(sc, M.with_world(sc, motion=sc.motion, media=md), 3, NODE_COST, 80)
    assert e.value.code == -1 and f"medium {m}" in str(e.value) and "boundary_kind, first or count" in str(e.value)


def test_other_counts_are_refused():
    sc = M.scene("fog")
    for new, what in ((M.with_world(sc, motion=sc.motion, media=sc.media[:-1]), "n_media"),
                      (M.with_world(sc, motion=sc.motion, boundary_quads=sc.boundary_quads[:-1]), "n_boundary_quads"),
                      (M.with_world(sc, motion=sc.motion, quads=sc.quads[:-1]), "n_quads")):
        with pytest.raises(rrt.RrtError) as e:
            refit_bvh_binned_world(sc, new, 3, NODE_COST, 80)
        assert e.value.code == -1 and what in str(e.value)
