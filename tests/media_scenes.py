"""Scenes and moves for the world-change tests (rrt_scene_update_world, rrt_scene_refit_world,
rrt_refit_bvh_binned_world, rrt_testing_medium_records), shared by tests/test_scene_media.py and
tests/test_gpu_scene_media.py. Helper module: no tests. Generators are cached; callers leave their
results unchanged. Frames are 32 x 18 x 4; the book-3 scene renders its square frame at 4 spp.

  NW8      cornell_smoke: 6 quads, 2 box media, 12 boundary quads
  NW9      final_scene: 1006 spheres, 2401 quads, 2 sphere media, the r = 5000 fog unbounded
  B3media  book3_scenes.multi_light(): 5 lights, a sphere-bounded and a box-bounded medium
  fog      24 spheres inside [-2, 2]^3 (six moving), 4 quads, a small sphere medium inside the cluster, a
           box medium with 6 boundary quads, and a fog sphere of radius 50 about the origin, which holds
           everything else and so is tested outside the tree
  fog5     fog with five identical fog spheres: kMaxUnbounded = 4 of them outside the tree, the fifth in it
"""
import dataclasses
import functools

import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import world as W

import book3_scenes as B3
import device_bvh_scenes as D
import geometry_scenes as G

FOG_RADIUS = 50.0


def _fog(name, n_fogs):
    rng = np.random.default_rng(3)
    white = W.Lambertian((0.73, 0.73, 0.73))
    mats = [W.Lambertian((0.6, 0.3, 0.2)), W.Metal((0.8, 0.85, 0.9), 0.1), W.Dielectric(1.5), W.Lambertian((0.2, 0.5, 0.7))]
    objs = []
    for k in range(24):
        c = tuple(float(x) for x in rng.uniform(-1.4, 1.4, 3))
        r = float(rng.uniform(0.12, 0.3))
        mat = mats[k % len(mats)]
        objs.append(W.Sphere.moving(c, (c[0], c[1] + 0.2, c[2]), r, mat) if k % 4 == 0 else W.Sphere(c, r, mat))
    objs += [W.Quad((-2.0, -2.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), white),
             W.Quad((-2.0, -2.0, -2.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), W.Lambertian((0.65, 0.05, 0.05))),
             W.Quad((-2.0, -2.0, -2.0), (0.0, 0.0, 4.0), (0.0, 4.0, 0.0), W.Lambertian((0.12, 0.45, 0.15))),
             W.Quad((-0.6, 1.95, -0.6), (1.2, 0.0, 0.0), (0.0, 0.0, 1.2), W.DiffuseLight((7.0, 7.0, 7.0)))]
    objs += [W.ConstantMedium(W.Sphere((0.3, 0.2, -0.1), 0.6, white), 0.8, (0.9, 0.9, 0.9)),
             W.ConstantMedium(W.make_box((-1.5, -1.5, -1.5), (-0.5, -0.3, -0.6), white), 1.2, (0.2, 0.4, 0.9))]
    objs += [W.ConstantMedium(W.Sphere((0.0, 0.0, 0.0), FOG_RADIUS, white), 0.01, (1.0, 1.0, 1.0)) for _ in range(n_fogs)]
    cam = W.Camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=40.0,
                   lookfrom=(0.5, 1.0, 9.0), lookat=(0.0, 0.0, 0.0))
    return W.build(W.HittableList(objs), cam, book=2, seed=0x0F06, name=name)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "NW8":
        return rrt.next_week_scene(8, D.KW)
    if name == "NW9":
        return D.scene("NW9")
    if name == "B3media":
        return B3.multi_light()
    if name == "fog":
        return _fog("fog", 1)
    if name == "fog5":
        return _fog("fog5", 5)
    raise KeyError(name)


def with_world(sc, spheres=None, motion=None, quads=None, lights=None, media=None, boundary_quads=None):
    """`sc` with the given arrays replaced (None keeps; motion is always replaced, as update_world does)."""
    new = G.with_geometry(sc, spheres, motion, quads, lights)
    if media is not None:
        new = dataclasses.replace(new, media=np.ascontiguousarray(media))
    if boundary_quads is not None:
        new = dataclasses.replace(new, boundary_quads=np.ascontiguousarray(boundary_quads))
    return new


def moved(sc, seed, amount=0.01):
    """`sc` after a seeded move of everything: spheres, quads and a book-3 scene's lights as
    geometry_scenes.moved moves them; every medium's sphere centre by a normal of deviation `amount` x
    min(r, 10) and its density by a factor within 1 +- amount / 2 (so that every GMedium record changes,
    a quad-bounded medium's too); every quad-bounded medium's boundary quads by one vector per medium
    (the boundary stays closed), of deviation `amount` x its longest edge. Boundary quads no medium
    names move as a group of their own."""
    spheres, quads, lights = G.moved(sc, seed, amount)
    rng = np.random.default_rng(seed + 2000)
    media = None if sc.media is None else sc.media.copy()
    bquads = None if sc.boundary_quads is None else sc.boundary_quads.copy()
    owned = np.zeros(0 if bquads is None else len(bquads), bool)

    def shift(rows):
        ext = max(np.linalg.norm(bquads["u"][rows, :3], axis=1).max(), np.linalg.norm(bquads["v"][rows, :3], axis=1).max())
        bquads["q"][rows, :3] += (rng.normal(0.0, amount, 3) * ext).astype(np.float32)

    for m in range(0 if media is None else len(media)):
        media["density"][m] = np.float32(media["density"][m] * (1.0 + 0.5 * amount * rng.uniform(-1.0, 1.0)))
        if int(media["boundary_kind"][m]) == 0:
            r = min(max(float(media["sphere"][m, 3]), 0.0), 10.0)
            media["sphere"][m, :3] += (rng.normal(0.0, amount, 3) * r).astype(np.float32)
        else:
            rows = slice(int(media["first"][m]), int(media["first"][m]) + int(media["count"][m]))
            owned[rows] = True
            shift(rows)
    if bquads is not None and not owned.all():
        shift(np.flatnonzero(~owned))
    return with_world(sc, spheres, sc.motion, quads, lights, media, bquads)


def change(ds, how, new, **kw):
    """ds.update_world / ds.refit_world with every array of `new`."""
    getattr(ds, how)(spheres=new.spheres, motion=new.motion, quads=new.quads, lights=new.lights, media=new.media,
                     boundary_quads=new.boundary_quads, **kw)


def sphere0_far(sc):
    """`sc` with sphere 0 at x = 60: outside fog's r = 50 sphere, which then holds no longer everything."""
    sp = sc.spheres.copy()
    sp["center_radius"][0, 0] = 60.0
    return with_world(sc, sp, sc.motion)


def fog_radius(sc, r):
    """`sc` with its last medium's (the fog's) radius set to r."""
    md = sc.media.copy()
    md["sphere"][-1, 3] = r
    return with_world(sc, motion=sc.motion, media=md)
