"""Edge shapes for the fast builder's tests (tests/test_bvh_lbvh.py: the host twin rrt_build_bvh_lbvh;
tests/test_gpu_fast_bvh.py: the device builder behind RRT_FLAG_FAST_BVH): the smallest scenes at which
an LBVH's construction can go wrong. Helper module: no tests. Generators are cached; callers leave their
results unchanged. Frames are 32 x 18 x 4.

  spheres2, spheres3   n_tree = 2 and 3: the root-leaf form in the LDS shape
  one_centre64         64 spheres with one centre: every Morton code equal, the order is the index order
                       and the tree is the balanced one over the index bits, 6 deep
  line65               65 spheres on a line parallel to x: two unusable axes
  clusters             two clusters 10^6 apart and a third of the 90 primitives in one Morton cell
  spheres63 .. 257     around the wave size and over one 256-lane block
  quads                the_next_week 5: 5 quads, no sphere
  fog2                 two spheres inside a fog sphere: the medium is tested outside the tree of 2
"""
import functools

import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import world as W

import device_bvh_scenes as D
import geometry_scenes as G


def _line65():
    return D._custom("line65", [(-8.0 + 0.25 * k, 1.0, -2.0) for k in range(65)], [0.1] * 65)


def _clusters():
    rng = np.random.default_rng(11)
    one_cell = [(0.5 + 1e-3 * k, 1.0, 0.25) for k in range(30)]
    near = [tuple(x) for x in rng.uniform(-3.0, 3.0, (30, 3))]
    far = [tuple(x + np.array([1e6, 0.0, 0.0])) for x in rng.uniform(-3.0, 3.0, (30, 3))]
    return D._custom("clusters", one_cell + near + far, [0.2] * 90)


def _fog2():
    grey = W.Lambertian((0.6, 0.6, 0.6))
    objs = [W.Sphere((-0.6, 0.0, 0.0), 0.5, grey), W.Sphere((0.7, 0.1, -0.3), 0.4, W.Metal((0.8, 0.8, 0.9), 0.1)),
            W.ConstantMedium(W.Sphere((0.0, 0.0, 0.0), 50.0, grey), 0.01, (1.0, 1.0, 1.0))]
    cam = W.Camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=40.0,
                   lookfrom=(0.5, 1.0, 6.0), lookat=(0.0, 0.0, 0.0))
    return W.build(W.HittableList(objs), cam, book=2, seed=0x0F02, name="fog2")


SCENES = {
    "spheres2": lambda: D.scene("spheres2"),
    "spheres3": lambda: D.scene("spheres3"),
    "one_centre64": lambda: D.coincident(64),
    "line65": _line65,
    "clusters": _clusters,
    **{f"spheres{n}": (lambda n=n: D.first_spheres(n)) for n in (63, 257)},
    "spheres64": lambda: D.scene("spheres64"),
    "spheres65": lambda: D.scene("spheres65"),
    "quads": lambda: G.scene("NW5"),
    "fog2": _fog2,
}
BOOK1 = [k for k in SCENES if k not in ("quads", "fog2")]


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def lookup(name):
    """`name` among these scenes or device_bvh_scenes'."""
    return scene(name) if name in SCENES else D.scene(name)
