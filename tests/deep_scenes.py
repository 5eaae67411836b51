"""Scenes whose BVH walks go deep, for the launch-plan tests (tests/test_launch_plan.py, host only)
and the launch-shape tests (tests/test_gpu_launch_shapes.py).

The suite's other scenes have shallow, balanced trees: a walk of theirs never holds more than about
ten stack entries, and no block needs more LDS than the 64 KiB a launch may declare by default. A
BVH2 step pushes only when both children are inner nodes and both are hit, so depth alone (a chain
of coincident spheres, one child always a leaf) does not fill the stack either. These do:

  ladder      groups of four spheres at 1, 2, 4, ... 2^61 along +x, seen from -x: every ray down the
              axis hits both children at each level of the tree, and both are inner nodes
  cluster     a field of small spheres plus n coincident spheres (the SAH splits ties 1 | n - 1, a
              chain n deep): stack_need up to the kernels' 64, scene bytes up to the 40 KB LDS budget
  wide        the ladder plus 66,000 tiny spheres: more than 65,535 nodes, the 32-bit-stack kernel
  wide_deep   wide plus a coincident cluster: the 32-bit stack (512 threads x 4 B) past 64 KiB

All of them are built from scenes._sphere / _material / make_camera; frames are tiny (at most
32 x 18 x 4 samples).
"""
import dataclasses
import functools
import os

import numpy as np

from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S
from rustraytrace_amd.render import build_bvh

GREY = (0.5, 0.5, 0.5)
TINT = (0.7, 0.6, 0.5)


def _materials(kind, textured=False):
    """Material 0: Lambertian grey (the earth texture when `textured`); material 1: `kind` — 1 metal
    with fuzz 0.1, 0 Lambertian."""
    return np.concatenate([S._material(3 if textured else 0, GREY, tex=0), S._material(kind, TINT, fuzz=0.1)])


def _ladder_spheres():
    rng = np.random.default_rng(5)
    sph = []
    for i in range(62):
        s = 2.0 ** i
        for g in range(4):
            c = np.array([s, 0.0, 0.0]) + rng.uniform(-0.05, 0.05, 3) * s
            sph.append(S._sphere(c, 0.12 * s, (i + g) % 2))
    return sph


def _ladder_camera(n_spheres, image_width=32, samples_per_pixel=4):
    return S.make_camera(aspect_ratio=16.0 / 9.0, image_width=image_width, samples_per_pixel=samples_per_pixel,
                         max_depth=8, vfov=20.0, lookfrom=(-1.0, 0.0, 0.0), lookat=(1.0, 0.0, 0.0), seed=7,
                         n_spheres=n_spheres)


def ladder(kind, textured=False):
    """248 spheres, 32 x 18 x 4 spp. kind 1: the untextured-specular class (the full class when
    `textured`), kind 0: the diffuse class."""
    sph = np.concatenate(_ladder_spheres())
    return S.SceneData(_ladder_camera(len(sph)), sph, _materials(kind, textured),
                       textures=[S.earth_texture()] if textured else [], name=f"ladder{kind}")


def cluster(n_cluster, n_field, kind, textured=False):
    """A ground sphere, n_field small spheres (alternating materials) and n_cluster identical spheres
    ((0, 1, 0), r = 1), all of material 1, so whichever of them wins a tie the result is the same.
    Camera of test_gpu_parity._book1_scene (48 x 27 x 4 spp, defocus on)."""
    rng = np.random.default_rng(3)
    sph = [S._sphere((0.0, -1000.0, 0.0), 1000.0, 0)]
    for i in range(n_field):
        c = rng.uniform(-8.0, 8.0, 3) * np.array([1.0, 0.0, 1.0]) + np.array([0.0, 0.2, 0.0])
        sph.append(S._sphere(c, 0.2, i % 2))
    sph += [S._sphere((0.0, 1.0, 0.0), 1.0, 1) for _ in range(n_cluster)]
    sph = np.concatenate(sph)
    cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=48, samples_per_pixel=4, max_depth=12, vfov=30.0,
                        lookfrom=(6.0, 2.5, 8.0), lookat=(0.0, 0.5, 0.0), defocus_angle=0.6, focus_dist=9.0, seed=7,
                        n_spheres=len(sph))
    return S.SceneData(cam, sph, _materials(kind, textured), textures=[S.earth_texture()] if textured else [],
                       name=f"cluster{n_cluster}+{n_field}")


def moving_cluster(n_cluster, n_field):
    """cluster(n_cluster, n_field, 1) as a book-2 scene: the first field sphere moves (a motion row per
    sphere through RrtSceneExt, a time draw per camera ray), so the book-2 kernel class renders it and
    every primitive stages 16 B of motion too."""
    sc = cluster(n_cluster, n_field, 1)
    motion = np.zeros((len(sc.spheres), 4), np.float32)
    motion[1, :3] = (0.0, 0.3, 0.0)
    return dataclasses.replace(sc, motion=motion, flags=sc.flags | _lib.FLAG_RAY_TIME, name=sc.name + "+motion")


WIDE_DEEP_CLUSTER = 40  # coincident spheres of wide_deep()


def _wide(n_cluster):
    rng = np.random.default_rng(9)
    n = 66000
    c = rng.uniform(-0.4, 0.4, (n, 3))
    c[:, 0] = rng.uniform(-0.5, 0.5, n)
    tiny = np.zeros(n, dtype=_lib.SPHERE_DTYPE)
    tiny["center_radius"][:, :3] = c
    tiny["center_radius"][:, 3] = 0.002
    sph = np.concatenate(_ladder_spheres() + [tiny] + [S._sphere((0.5, 0.0, 0.0), 0.05, 1) for _ in range(n_cluster)])
    return S.SceneData(_ladder_camera(len(sph), image_width=16, samples_per_pixel=2), sph, _materials(1),
                       name=f"wide+{n_cluster}")


def wide():
    """ladder(1) plus 66,000 spheres of radius 0.002 around the camera's axis: more than 65,535 nodes
    (read from global memory), 16 x 9 x 2 spp."""
    return _wide(0)


def wide_deep():
    """wide() plus WIDE_DEEP_CLUSTER coincident spheres on the axis: a chain deep enough that the
    32-bit stack of a 512-thread block passes 64 KiB (stack_need >= 33)."""
    return _wide(WIDE_DEEP_CLUSTER)


@functools.lru_cache(maxsize=None)
def built(in_lds, name, *args):
    """(scene, nodes, order, info) of the generator `name`, built once per process, placement and
    arguments (the 66,000-sphere trees take seconds). in_lds: the RRT_SCENE_IN_LDS value the caller
    has set ("0": read from global memory), or None when it is unset. Callers leave all four unchanged."""
    assert os.environ.get("RRT_SCENE_IN_LDS") == in_lds
    scene = globals()[name](*args)
    return (scene,) + tuple(build_bvh(scene))
