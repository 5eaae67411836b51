"""rrt_testing_quad_records: the host compilation of rrt_quad_form.h, the one definition of what a quad
contributes to a scene (its padded f64 box, its GQuad64 and GQuad records) that scene creation calls on
the host and rrt_scene_update_geometry on the device. No GPU. The boxes are held to the leaf boxes
rrt_build_bvh_binned stores and to the numpy specification of tests/test_bvh_binned.py, the records to
a numpy restatement of quad.rs:21-37 in f64. Nothing compares with a tolerance: bits, and the stored
format's own outward rounding (slack 4 * 2^-24 * (2 |p| + 3 o) from the root box, then f32
rounded outward).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned, decode_bvh2

import geometry_scenes as G
from test_bvh_binned import _quad_boxes, f32_outward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt_hip.h")

PROTOTYPES = (
    "int32_t rrt_scene_update_geometry(RrtScene *scene, const RrtSceneGeometry *geometry, void *stream);",
    "int32_t rrt_scene_refit_geometry(RrtScene *scene, const RrtSceneGeometry *geometry, void *stream);",
    "int32_t rrt_refit_bvh_binned_ex(const RrtSphere *built_spheres, uint32_t n_spheres, const RrtSceneExt *built_ext, "
    "uint32_t max_leaf, double node_cost, uint32_t node_stride, const RrtSphere *new_spheres, const float *new_motion, "
    "const RrtQuad *new_quads, void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out, RrtBvhInfo *info, "
    "double *sah_out);",
    "int32_t rrt_testing_quad_records(const RrtQuad *quads, uint32_t n_quads, double *boxes6, void *gquad, void *gquad64);",
)


def with_extreme(name):
    """The scene's quads plus the quad with edges of 1e-3 and 1e3."""
    sc = G.scene(name)
    return G.with_geometry(sc, motion=sc.motion, quads=np.concatenate([sc.quads, G.EXTREME_QUAD]))


# ---- 1. exports ----------------------------------------------------------------------------------
def test_entry_points_are_exported_with_the_headers_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    lib = _lib.load()
    for proto in PROTOTYPES:
        assert proto in flat, proto
        name = re.search(r"(rrt_\w+)\(", proto).group(1)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert ("typedef struct RrtSceneGeometry { const RrtSphere *spheres; uint32_t n_spheres; const float *sphere_motion; "
            "const RrtQuad *quads; uint32_t n_quads; const RrtLight *lights; uint32_t n_lights; } RrtSceneGeometry;") in flat
    assert ctypes.sizeof(_lib.RrtSceneGeometry) == 56
    for code, name in enumerate(("GQUADS", "GQUADS64", "QUAD_ROWS", "GLIGHTS"), start=6):
        assert re.search(r"RRT_TABLE_%s = %d\b" % (name, code), flat), name
    assert sorted(c for c, _ in _lib.SCENE_GEOMETRY_TABLES.values()) == [6, 7, 8, 9]
    assert not set(_lib.SCENE_GEOMETRY_TABLES) & set(_lib.SCENE_TABLES)
    assert lib.rrt_hip_abi_version() == 11


def test_null_scene_and_null_geometry_are_refused_without_a_device():
    lib = _lib.load()
    g = _lib.RrtSceneGeometry()
    for name in ("rrt_scene_update_geometry", "rrt_scene_refit_geometry"):
        assert getattr(lib, name)(None, ctypes.byref(g), None) == -1
        msg = lib.rrt_hip_last_error().decode()
        assert name in msg and "null scene" in msg, msg
    assert lib.rrt_testing_quad_records(None, 3, None, None, None) == -1
    assert lib.rrt_testing_quad_records(None, 0, None, None, None) == 0  # every output may be NULL


# ---- 2. boxes ------------------------------------------------------------------------------------
def test_the_cases_the_boxes_must_cover_are_present():
    nw5, nw7 = G.scene("NW5"), G.scene("NW7")
    assert len(nw5.quads) == 5 and len(nw5.spheres) == 0 and len(nw7.quads) == 18
    flat = lambda q: ((q["u"][:, :3] == 0) & (q["v"][:, :3] == 0)).any(axis=1)  # a zero-extent axis: the pad branch
    assert flat(nw5.quads).all() and flat(nw7.quads).sum() >= 6
    rotated = ~flat(nw7.quads)  # RotateY'd box faces: no axis of zero extent
    assert rotated.sum() >= 4
    u, v = G.EXTREME_QUAD["u"][0, :3].astype(np.float64), G.EXTREME_QUAD["v"][0, :3].astype(np.float64)
    assert np.isclose(np.linalg.norm(u), 1e-3) and np.isclose(np.linalg.norm(v), 1e3)


@pytest.mark.parametrize("name", ["NW5", "NW7"])
def test_boxes_are_the_numpy_specification(name):
    sc = with_extreme(name)
    boxes, _, _ = _lib.quad_records(sc.quads)
    lo, hi = _quad_boxes(sc.quads)
    assert boxes[:, :3].tobytes() == np.ascontiguousarray(lo).tobytes()
    assert boxes[:, 3:].tobytes() == np.ascontiguousarray(hi).tobytes()
    width = boxes[:, 3:] - boxes[:, :3]
    assert (width > 0.0).all() and (width < 0.00011).any(), "no quad took the pad branch"


@pytest.mark.parametrize("name", ["NW5", "NW7"])
def test_boxes_are_the_leaf_boxes_the_builder_stores(name):
    sc = with_extreme(name)
    n_sph = len(sc.spheres)
    boxes, _, _ = _lib.quad_records(sc.quads)
    nodes, order, info = build_bvh_binned(sc, 1, 2.0, 80)
    lo, hi, first, cnt = decode_bvh2(nodes, 80)
    root_lo, root_hi = boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)  # these scenes hold quads only
    assert n_sph == 0
    o = np.maximum(np.abs(root_lo), np.abs(root_hi))
    grow = lambda p: 4.0 * 2.0 ** -24 * (2.0 * np.abs(p) + 3.0 * o)
    seen = set()
    for k in range(info["n_nodes"]):
        for c in range(2):
            if cnt[k, c] == 0:
                continue
            assert cnt[k, c] == 1, "max_leaf 1"
            j = int(order[first[k, c]]) - n_sph
            seen.add(j)
            mn, mx = boxes[j, :3], boxes[j, 3:]
            slo, shi = lo[k, c].astype(np.float64), hi[k, c].astype(np.float64)
            assert (slo <= mn).all() and (shi >= mx).all(), f"quad {j}: the stored box does not contain the f64 box"
            want_lo, want_hi = f32_outward(mn - grow(mn), mx + grow(mx))
            assert np.array_equal(lo[k, c], want_lo) and np.array_equal(hi[k, c], want_hi), f"quad {j}: beyond the slack"
    assert seen == set(range(len(sc.quads)))


# ---- 3. records ----------------------------------------------------------------------------------
def numpy_gquad64(q):
    """quad.rs:21-37 in f64 from the f32 inputs: n = cross(u, v), normal = n * (1 / sqrt(dot(n, n))),
    D = dot(normal, q), w = n * (1 / dot(n, n)), each sum left to right."""
    a, u, v = (q[k][:, :3].astype(np.float64) for k in ("q", "u", "v"))
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                  u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    nn = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
    normal = n * (1.0 / np.sqrt(nn))[:, None]
    w = n * (1.0 / nn)[:, None]
    d = normal[:, 0] * a[:, 0] + normal[:, 1] * a[:, 1] + normal[:, 2] * a[:, 2]
    return a, u, v, normal, w, d


@pytest.mark.parametrize("name", ["NW5", "NW7", "mixed"])
def test_gquad64_is_quad_rs_in_f64_and_gquad_its_f32_rounding(name):
    sc = with_extreme(name)
    _, g32, g64 = _lib.quad_records(sc.quads)
    a, u, v, normal, w, d = numpy_gquad64(sc.quads)
    for field, want in (("q", a), ("u", u), ("v", v), ("n", normal), ("w", w), ("D", d)):
        assert g64[field].tobytes() == np.ascontiguousarray(want).tobytes(), field
    assert np.isfinite(g64["n"]).all() and np.isfinite(g64["w"]).all() and np.isfinite(g64["D"]).all()
    for field in ("q", "u", "v"):  # the f32 inputs as they are; D in q's fourth slot, zeros elsewhere
        assert g32[field][:, :3].tobytes() == sc.quads[field][:, :3].tobytes(), field
    for field in ("n", "w"):
        assert g32[field][:, :3].tobytes() == g64[field].astype(np.float32).tobytes(), field
    assert g32["q"][:, 3].tobytes() == g64["D"].astype(np.float32).tobytes()
    assert not g32["u"][:, 3].any() and not g32["v"][:, 3].any() and not g32["n"][:, 3].any() and not g32["w"][:, 3].any()


def test_each_output_may_be_null():
    q = G.scene("NW7").quads
    boxes, g32, g64 = _lib.quad_records(q)
    lib = _lib.load()
    only = np.zeros_like(g64)
    _lib.check(lib.rrt_testing_quad_records(_lib.ptr(q), len(q), None, None, _lib.ptr(only)))
    assert only.tobytes() == g64.tobytes()
    only = np.zeros_like(boxes)
    _lib.check(lib.rrt_testing_quad_records(_lib.ptr(q), len(q), _lib.ptr(only), None, None))
    assert only.tobytes() == boxes.tobytes()
