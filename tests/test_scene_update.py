"""CPU tests of the scene-update interface (rrt_scene_set_camera, rrt_scene_update_spheres and their
test hooks): the exports carry the header's prototypes, a null scene is refused without a device,
and the sphere-box function the update runs on the device (rrt_sphere_box.h, here in its host
compilation) equals a numpy restatement of rrt_host.cpp prim_boxes + pad bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from rustraytrace_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrt_hip.h")

PROTOTYPES = (
    "int32_t rrt_scene_set_camera(RrtScene *scene, const RrtCamera *cam);",
    "int32_t rrt_scene_update_spheres(RrtScene *scene, const RrtSphere *spheres, uint32_t n_spheres, "
    "const float *motion, void *stream);",
    "int32_t rrt_testing_sphere_boxes(const RrtSphere *spheres, uint32_t n_spheres, const float *motion, double *out);",
    "int32_t rrt_testing_scene_read_table(RrtScene *scene, uint32_t what, void *out, size_t cap, size_t *bytes_out);",
    "int32_t rrt_testing_scene_update_stats(const RrtScene *scene, RrtSceneUpdateStats *out);",
)


def test_entry_points_are_exported_with_the_headers_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    lib = _lib.load()
    for proto in PROTOTYPES:
        assert proto in flat, proto
        name = re.search(r"(rrt_\w+)\(", proto).group(1)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.rrt_hip_abi_version() == 11


def test_null_scene_is_refused_without_a_device():
    lib = _lib.load()
    cam = np.zeros(1, _lib.CAMERA_DTYPE)
    sp = np.zeros(2, _lib.SPHERE_DTYPE)
    n = ctypes.c_size_t(0)
    st = _lib.RrtSceneUpdateStats()
    calls = {
        "rrt_scene_set_camera": lambda: lib.rrt_scene_set_camera(None, _lib.ptr(cam)),
        "rrt_scene_update_spheres": lambda: lib.rrt_scene_update_spheres(None, _lib.ptr(sp), 2, None, None),
        "rrt_testing_scene_read_table": lambda: lib.rrt_testing_scene_read_table(None, 1, None, 0, ctypes.byref(n)),
        "rrt_testing_scene_update_stats": lambda: lib.rrt_testing_scene_update_stats(None, ctypes.byref(st)),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = lib.rrt_hip_last_error().decode()
        assert name in msg and "null scene" in msg, msg
    with pytest.raises(_lib.RrtError):
        _lib.check(lib.rrt_testing_sphere_boxes(None, 3, None, None))


def numpy_boxes(cr, motion):
    """prim_boxes + pad (rrt_host.cpp; aabb.rs:104-115): r = max((double)r32, 0); per axis c -+ r in
    f64; with motion the union with the box at c2 = (double)(c32 + m32), an f32 sum; an axis whose
    size is < 1e-4 grows by delta / 2 on both sides."""
    cr = np.asarray(cr, np.float32)
    r = np.maximum(cr[:, 3].astype(np.float64), 0.0)[:, None]
    c = cr[:, :3].astype(np.float64)
    mn, mx = c - r, c + r
    if motion is not None:
        c2 = (cr[:, :3] + np.asarray(motion, np.float32)[:, :3]).astype(np.float64)  # float32 + float32
        mn, mx = np.where(mn <= c2 - r, mn, c2 - r), np.where(mx >= c2 + r, mx, c2 + r)
    thin = (mx - mn) < 0.0001
    mn, mx = np.where(thin, mn - 0.0001 / 2.0, mn), np.where(thin, mx + 0.0001 / 2.0, mx)
    return np.concatenate([mn, mx], axis=1)


def spheres_of(cr):
    sp = np.zeros(len(cr), _lib.SPHERE_DTYPE)
    sp["center_radius"] = np.asarray(cr, np.float32)
    return sp


EDGE = np.array([
    [0.0, 1.0, 2.0, 0.0],        # r = 0: every axis padded
    [1.0, -2.0, 3.0, -0.75],     # negative radius: r = 0
    [0.5, 0.25, -8.0, 4e-5],     # size 8e-5 < 1e-4: padded
    [0.5, 0.25, -8.0, 5e-5],     # the f32 nearest 5e-5 lies below it: size 9.9999997e-5, still padded
    [0.5, 0.25, -8.0, np.nextafter(np.float32(5e-5), np.float32(1))],  # one f32 step up: size > 1e-4, not padded
    [1e6, -1e6, 1e6, 0.3],       # a large center with a radius far below its f32 spacing
    [16777216.0, 3.0, -0.0, 1.0],
    [-0.0, 0.0, -0.0, -0.0],
], dtype=np.float32)


def test_sphere_boxes_equal_the_numpy_restatement_static():
    rng = np.random.default_rng(7)
    cr = np.concatenate([EDGE, rng.normal(0, 50, (500, 4)).astype(np.float32)])
    got = _lib.sphere_boxes(spheres_of(cr))
    want = numpy_boxes(cr, None)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the two sides of the pad threshold really are two sides
    for row in (2, 3):
        assert got[row, 0] == (0.5 - np.float64(EDGE[row, 3])) - 0.0001 / 2.0
    assert got[4, 0] == 0.5 - np.float64(EDGE[4, 3]) and got[4, 3] - got[4, 0] >= 0.0001
    assert got[0, 3] - got[0, 0] == (0.0 + 0.0001 / 2.0) - (0.0 - 0.0001 / 2.0)
    assert np.array_equal(got[1, :3], np.float64(EDGE[1, :3]) - 0.0001 / 2.0)


def test_sphere_boxes_equal_the_numpy_restatement_moving():
    rng = np.random.default_rng(8)
    cr = np.concatenate([EDGE, rng.normal(0, 50, (500, 4)).astype(np.float32)])
    motion = np.zeros((len(cr), 4), np.float32)
    motion[len(EDGE):, :3] = rng.normal(0, 1, (500, 3)).astype(np.float32)
    motion[0, :3] = (0.0, 0.5, 0.0)        # extends one axis only: x and z stay padded
    motion[1, :3] = (-0.0, -0.0, -0.0)     # a motion of -0.0
    motion[2, :3] = (0.0, 0.0, 1e-9)       # an f32 sum that rounds back to c
    motion[5, :3] = (0.03, -0.03, 0.0625)  # c + m rounds in f32 at 1e6 (ulp 0.0625)
    motion[7, :3] = (0.0, -0.0, 0.0)       # -0 + 0 sums
    motion[:, 3] = rng.normal(0, 1, len(cr)).astype(np.float32)  # the row's w is not read
    got = _lib.sphere_boxes(spheres_of(cr), motion)
    want = numpy_boxes(cr, motion)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert got[0, 1] == 1.0 and got[0, 4] == 1.5  # the moved axis is not padded, the other two are
    assert got[0, 0] == 0.0 - 0.0001 / 2.0 and got[0, 5] == 2.0 + 0.0001 / 2.0
    static = _lib.sphere_boxes(spheres_of(cr))
    assert np.array_equal(got[1].view(np.uint64), static[1].view(np.uint64))  # -0.0 moves nothing
    assert not np.array_equal(got[5], static[5])
