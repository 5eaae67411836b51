"""The frames of the f64 books path's book-2 tests (RRT_FLAG_F64_BOOK2), shared by
test_books64_book2.py (conditions on the reference alone) and test_gpu_books64_book2.py (the kernel
against BOOKS). Helper module: no tests.

  s1     the_next_week 1 (bouncing_spheres: moving spheres, checker ground) 64 wide, 4 spp, depth 8
  s1d50  the same, 96 wide, 8 spp, depth 50
  s2     the_next_week 2 (checkered_spheres) 64 wide, 8 spp, depth 10
  s5     the_next_week 5 (quads) 64 wide, 8 spp, depth 50
  s7     the_next_week 7 (cornell_box: quads, a light) 96 wide, 16 spp, depth 50
  mixed  s1d50 plus one static earth-textured sphere and four quads: metal, dielectric, light and the
         ground's checker material — every material branch on either primitive kind in one frame
"""
import copy
import functools

import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S

FRAMES = ("s1", "s1d50", "s2", "s5", "s7", "mixed")


def _nw(n, w, spp, depth):
    return rrt.next_week_scene(n, dict(image_width=w, samples_per_pixel=spp, max_depth=depth))


def _quad(q, u, v, mat):
    r = np.zeros(1, dtype=_lib.QUAD_DTYPE)
    r["q"][0, :3], r["u"][0, :3], r["v"][0, :3] = q, u, v
    r["material_index"][0] = mat
    return r


def mixed_scene(base=None):
    """`base` (default s1d50) with the earth sphere and the four quads of the module docstring."""
    sc = base if base is not None else _nw(1, 96, 8, 50)
    earth = _nw(3, 32, 1, 2)
    earth_mat = earth.materials[earth.spheres["material_index"][0]]
    assert int(earth_mat["kind"]) == 3 and len(earth.textures) == 1
    checker = int(np.flatnonzero(sc.materials["kind"] == 5)[0])  # the ground's
    nm = len(sc.materials)
    tex_mat = np.array([earth_mat], dtype=_lib.MATERIAL_DTYPE)
    tex_mat["_pad"][0, 0] = 0  # the frame's only texture
    mats = np.concatenate([sc.materials, tex_mat, S._material(1, (0.8, 0.85, 0.9), fuzz=0.05),
                           S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5), S._material(4, (4.0, 3.5, 3.0))])
    spheres = np.concatenate([sc.spheres, S._sphere((0.0, 1.0, 3.0), 1.0, nm)])
    motion = np.concatenate([sc.motion, np.zeros((1, 4), dtype=np.float32)])
    quads = np.concatenate([_quad((-6, 0, -3), (0, 0, 6), (0, 3, 0), nm + 1),
                            _quad((1, 0, 2.5), (2.5, 0, 0.7), (0, 2, 0), nm + 2),
                            _quad((-2, 5, -2), (4, 0, 0), (0, 0, 4), nm + 3),
                            _quad((3, 0.01, -4), (5, 0, 0), (0, 1.5, 3), checker)])
    cam = sc.camera.copy()
    cam["params_u"][0, 2] = len(spheres)
    return S.SceneData(cam, spheres, mats, textures=list(earth.textures), flags=sc.flags, name="mixed",
                       motion=motion, quads=quads)


@functools.lru_cache(maxsize=None)
def frame(name):
    """The frame `name` of FRAMES (built once; treat as read-only)."""
    if name == "s1":
        return _nw(1, 64, 4, 8)
    if name == "s1d50":
        return _nw(1, 96, 8, 50)
    if name == "s2":
        return _nw(2, 64, 8, 10)
    if name == "s5":
        return _nw(5, 64, 8, 50)
    if name == "s7":
        return _nw(7, 96, 16, 50)
    if name == "mixed":
        return mixed_scene()
    raise KeyError(name)


def reordered(scene, what):
    """`scene` with its quad list reversed (what = "quads") or its sphere list reversed, motion rows with
    it (what = "spheres"): the same world in another primitive order. None when the list has fewer than
    two entries (nothing to reorder)."""
    sc = copy.copy(scene)
    if what == "quads":
        if scene.quads is None or len(scene.quads) < 2:
            return None
        sc.quads = np.ascontiguousarray(scene.quads[::-1])
    elif what == "spheres":
        if len(scene.spheres) < 2:
            return None
        sc.spheres = np.ascontiguousarray(scene.spheres[::-1])
        if scene.motion is not None:
            sc.motion = np.ascontiguousarray(scene.motion[::-1])
    else:
        raise KeyError(what)
    return sc
