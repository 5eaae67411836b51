"""Scenes for the book-2/3 classes of the f32 kernel (1 moving spheres, 2 quads, 3 media, 4 the book-3
integrator), shared by tests/test_book2_class_scenes.py (conditions on the oracle and the launch plan
alone) and tests/test_gpu_book2_classes.py (the kernel against the oracle). Helper module: no tests.

The stock book-2/3 scenes that stage in LDS walk trees of 1 to 10 nodes, and which of a class's
instantiations a scene selects (staged or read from global memory, with or without the noise path,
16- or 32-bit stack, default or raised LDS limit) is an accident of its size. These give every class
a tree of 30 to 80 nodes with spheres of every material among the base scene's own primitives:

  composite    a stock scene per class (the_next_week 2, 7, 8; the_rest_of_your_life) in a tiny frame,
               plus n_field small spheres cycling through Lambertian, metal, dielectric and (with
               `noise`) a Perlin-noise material, every fourth one moving, plus n_cluster coincident
               spheres (deep_scenes.cluster's chain: the SAH splits ties 1 | n - 1)
  moving_wide  deep_scenes.wide() (more than 65,535 nodes: the 32-bit stack) with one moving sphere,
               and a quad (class 2) or a sphere-bounded medium (class 3) off the axis

Frames are at most 48 x 27 x 4 samples. Generators are cached; callers leave their results unchanged.
"""
import dataclasses
import functools
import os

import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S
from rustraytrace_amd.render import build_bvh

import deep_scenes as D
from books64_book2_scenes import _quad

CLASSES = (1, 2, 3, 4)
LIGHT_SPHERE = ((190.0, 90.0, 190.0), 90.0)  # the book-3 scene's glass sphere, on its light list
# The field's seed per class. Chosen on the oracle alone, among a few hundred: no path of the frames the
# tests render meets an exact tie (the base scenes' box faces share edges and lie on the floor; a tie there
# goes to the first quad tested, so the oracle's walks of different trees — its own, the sweep builder's,
# the device builder's — would count different rays: about two in three of class 4's seeds do), and the
# noise spheres show in as many pixels as the tiny frames allow.
FIELD_SEED = {1: 111, 2: 213, 3: 115, 4: 199}
CLUSTER = {False: ((420.0, 400.0, 150.0), 30.0), True: ((1.0, 0.4, -2.5), 0.45)}  # Cornell units / class 1's


def _base(cls):
    """The class's stock scene in its small frame: 48 x 27 for class 1 (16:9), 36 x 36 for the Cornell
    boxes; 4 spp (a square, which book 3 needs), max_depth 10."""
    kw = dict(image_width=48 if cls == 1 else 36, samples_per_pixel=4, max_depth=10)
    return rrt.rest_of_your_life_scene(kw) if cls == 4 else rrt.next_week_scene({1: 2, 2: 7, 3: 8}[cls], kw)


def _field(cls, n_field):
    """(centres, radii) of the field spheres. Cornell boxes: centres uniform in [20, 535]^3, radii 4 to
    9; class 4 keeps 20 units clear of the light sphere (a hit point inside it makes the light pdf's
    sqrt(1 - r^2 / d^2) NaN). Class 1 (checkered_spheres: two r = 10 spheres seen from (13, 2, 3)):
    a slab around the origin, radii 0.12 to 0.3."""
    rng = np.random.default_rng(FIELD_SEED[cls])
    centres, radii = [], []
    while len(centres) < n_field:
        if cls == 1:
            c, r = rng.uniform((-4.0, -2.5, -5.0), (6.0, 2.5, 5.0)), rng.uniform(0.12, 0.3)
        else:
            c, r = rng.uniform(20.0, 535.0, 3), rng.uniform(4.0, 9.0)
        if cls == 4 and np.linalg.norm(c - np.array(LIGHT_SPHERE[0])) < LIGHT_SPHERE[1] + r + 20.0:
            continue
        centres.append(c)
        radii.append(r)
    return centres, radii


@functools.lru_cache(maxsize=None)
def composite(cls, noise, n_field=60, n_cluster=0, plain_noise=False):
    """The class's base scene plus n_field field spheres and n_cluster coincident ones.

    Field materials cycle through Lambertian, metal (fuzz 0.1), dielectric 1.5 and, with `noise`, the
    kind-6 material of the_next_week 4 with its one Perlin table (scale 0.05 in Cornell units, its own
    4 in class 1). Every fourth field sphere moves by (0, 15, 0) ((0, 0.4, 0) in class 1).
    plain_noise: the noise material's slot holds a plain Lambertian of its albedo instead (and no
    table) — the same geometry without the branch, for the preconditions test."""
    base = _base(cls)
    nm = len(base.materials)
    mats = [base.materials, S._material(0, (0.6, 0.3, 0.2)), S._material(1, (0.8, 0.85, 0.9), fuzz=0.1),
            S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5)]
    perlin = base.perlin
    if noise:
        nw4 = rrt.next_week_scene(4, dict(image_width=8, samples_per_pixel=1, max_depth=2))
        assert len(nw4.perlin) == 1 and base.perlin is None
        m = nw4.materials[nw4.materials["kind"] == 6][:1].copy()
        assert len(m) == 1 and int(m["_pad"][0, 0]) == 0
        if cls != 1:
            m["albedo_fuzz"][0, 3] = 0.05
        if plain_noise:
            m = S._material(0, tuple(m["albedo_fuzz"][0, :3]))
        else:
            perlin = nw4.perlin
        mats.append(m)
    mats = np.concatenate(mats)
    n_kinds = 4 if noise else 3
    centres, radii = _field(cls, n_field)
    field = [S._sphere(c, r, nm + i % n_kinds) for i, (c, r) in enumerate(zip(centres, radii))]
    cc, cr = CLUSTER[cls == 1]
    spheres = np.concatenate([base.spheres] + field + [S._sphere(cc, cr, nm) for _ in range(n_cluster)])
    motion = np.zeros((len(spheres), 4), np.float32)
    if base.motion is not None:
        motion[:len(base.spheres)] = base.motion
    motion[len(base.spheres):len(base.spheres) + n_field:4, 1] = 0.4 if cls == 1 else 15.0
    cam = base.camera.copy()
    cam["params_u"][0, 2] = len(spheres)
    name = f"composite{cls}{'n' if noise else ''}+{n_field}+{n_cluster}"
    return dataclasses.replace(base, camera=cam, spheres=spheres, materials=mats, motion=motion, perlin=perlin,
                               flags=base.flags | _lib.FLAG_RAY_TIME, name=name)


def without_media(scene):
    """`scene` without its constant media (and their boundary quads): a class-2 scene."""
    return dataclasses.replace(scene, media=None, boundary_quads=None, name=scene.name + "-media")


@functools.lru_cache(maxsize=None)
def moving_wide(cls):
    """deep_scenes.wide() (the ladder plus 66,000 tiny spheres, 16 x 9 x 2 spp) as a scene of class
    1, 2 or 3: the first ladder sphere moves; class 2 adds one Lambertian quad off the axis, class 3
    one small sphere-bounded medium off the axis. More than 65,535 nodes: the 32-bit-stack kernel.

    No class 4: the ladder's spheres reach 2^61, so the squared distances of book 3's light pdf
    overflow f32."""
    assert cls in (1, 2, 3)
    sc = D.wide()
    motion = np.zeros((len(sc.spheres), 4), np.float32)
    motion[0, :3] = (0.0, 0.05, 0.0)
    mats, quads, media = sc.materials, None, None
    if cls == 2:
        quads = _quad((0.5, 0.15, -0.2), (0.3, 0.05, 0.0), (0.0, 0.1, 0.3), 0)
    if cls == 3:
        mats = np.concatenate([mats, S._material(7, (0.9, 0.9, 0.9))])
        media = np.zeros(1, dtype=_lib.MEDIUM_DTYPE)
        media["sphere"][0] = (0.7, -0.12, 0.1, 0.08)
        media["material_index"][0] = len(mats) - 1
        media["density"][0] = 8.0
    return dataclasses.replace(sc, materials=mats, motion=motion, quads=quads, media=media,
                               flags=sc.flags | _lib.FLAG_RAY_TIME, name=f"moving_wide{cls}")


@functools.lru_cache(maxsize=None)
def built(in_lds, name, *args):
    """(scene, nodes, order, info) of the generator `name` for the placement the caller has set
    (in_lds: the RRT_SCENE_IN_LDS value, "0" = read from global memory, or None when it is unset),
    built once per process. Callers leave all four unchanged."""
    assert os.environ.get("RRT_SCENE_IN_LDS") == in_lds
    scene = globals()[name](*args)
    return (scene,) + tuple(build_bvh(scene))
