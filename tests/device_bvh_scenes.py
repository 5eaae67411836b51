"""Scenes shared by tests/test_bvh_binned.py (the host twin of the device BVH builder) and
tests/test_gpu_device_bvh.py (the device builder, RRT_FLAG_DEVICE_BVH): every scene at 32x18x4 unless
a test asks for another size. Not a test module."""
import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import scenes as S

KW = dict(image_width=32, samples_per_pixel=4)
# leaf size and node format of the three shapes scene creation can keep: LDS, global, the fallback
SHAPES = [(3, 80), (1, 32), (3, 32)]


def first_spheres(n):
    """The first n spheres of the 10,001-sphere RTOW scene (the r = 1000 ground sphere first)."""
    sc = rrt.config_scene("C5", **KW)
    sc.spheres = sc.spheres[:n].copy()
    sc.camera = sc.camera.copy()
    sc.camera["params_u"][0, 2] = n
    sc.name = f"spheres{n}"
    return sc


def _custom(name, centers, radii):
    mats = S._material(0, (0.5, 0.5, 0.5))
    sph = np.concatenate([S._sphere(c, r, 0) for c, r in zip(centers, radii)])
    cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=40.0,
                        lookfrom=(0.0, 2.0, 12.0), lookat=(0.0, 0.5, 0.0), n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, name=name)


def coincident(n=40):
    return _custom(f"coincident{n}", [(3.0, 1.0, -2.0)] * n, [0.25] * n)


def concentric(n=40):
    return _custom(f"concentric{n}", [(0.0, 1.0, 0.0)] * n, [0.1 * (k + 1) for k in range(n)])


def big_among_small(n=200, seed=5):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-6.0, 6.0, (n, 3))
    c[:, 1] = 0.2
    centers = [tuple(x) for x in c[: n // 2]] + [(0.0, -1000.0, 0.0)] + [tuple(x) for x in c[n // 2:]]
    return _custom("big_among_small", centers, [0.2] * (n // 2) + [1000.0] + [0.2] * (n - n // 2))


SCENES = {
    **{f"spheres{n}": (lambda n=n: first_spheres(n)) for n in (2, 3, 4, 5, 64, 65, 1025)},
    "C2": lambda: rrt.config_scene("C2", **KW),
    "C5": lambda: rrt.config_scene("C5", **KW),
    "NW1": lambda: rrt.next_week_scene(1, KW),
    "NW7": lambda: rrt.next_week_scene(7, KW),
    "NW9": lambda: rrt.next_week_scene(9, KW),
    "coincident40": coincident,
    "concentric40": concentric,
    "big_among_small": big_among_small,
}
BOOK1 = [k for k in SCENES if k not in ("NW1", "NW7", "NW9")]  # RRT_FLAG_F64 renders these

_cache = {}


def scene(name):
    """The named scene, built once per process (tests must not modify it)."""
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def n_prims(sc):
    return len(sc.spheres) + (0 if sc.quads is None else len(sc.quads)) + (0 if sc.media is None else len(sc.media))
