"""Scenes and moves for the geometry-change tests (rrt_scene_update_geometry, rrt_scene_refit_geometry,
rrt_refit_bvh_binned_ex, rrt_testing_quad_records), shared by tests/test_quad_form.py,
tests/test_bvh_refit_quads.py and tests/test_gpu_scene_geometry.py. Helper module: no tests.
Generators are cached; callers leave their results unchanged. Frames are 32 wide, 4 spp.
"""
import dataclasses
import functools

import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import _lib
from rustraytrace_amd import scenes as S

import book3_scenes as B3
import books64_book2_scenes as B
import device_bvh_scenes as D


@functools.lru_cache(maxsize=None)
def scene(name):
    """NW5 (5 quads, no sphere), NW7 (the Cornell box: 18 quads, 12 of them rotated box faces), mixed
    (moving spheres, an image texture and 4 quads), B3 (the stock book-3 scene), multi_light (5 lights,
    no media), big (300 quads and 40 spheres: two 256-lane blocks of quads, a global-memory tree)."""
    if name in ("NW5", "NW7"):
        return rrt.next_week_scene(int(name[2:]), D.KW)
    if name == "mixed":
        return B.mixed_scene(rrt.next_week_scene(1, D.KW))
    if name == "B3":
        return rrt.rest_of_your_life_scene(D.KW)
    if name == "multi_light":
        return B3.multi_light(media=False)
    if name == "big":
        return big_scene()
    raise KeyError(name)


def quad(q, u, v, mat=0):
    r = np.zeros(1, dtype=_lib.QUAD_DTYPE)
    r["q"][0, :3], r["u"][0, :3], r["v"][0, :3] = q, u, v
    r["material_index"][0] = mat
    return r


# a quad with edges of 1e-3 and 1e3 (|u x v|^2 = 1, but 1 / |n| scales components 10^6 apart)
EXTREME_QUAD = quad((0.5, -0.25, 3.0), (1e-3, 0.0, 0.0), (0.0, 6e2, 8e2))


def with_geometry(sc, spheres=None, motion=None, quads=None, lights=None):
    """`sc` with the given arrays replaced (None keeps; motion is always replaced, as update_geometry does)."""
    new = dataclasses.replace(sc, motion=motion)
    if spheres is not None:
        new = dataclasses.replace(new, spheres=np.ascontiguousarray(spheres))
    if quads is not None:
        new = dataclasses.replace(new, quads=np.ascontiguousarray(quads))
    if lights is not None:
        new = dataclasses.replace(new, lights=np.ascontiguousarray(lights))
    return new


def jitter_quads(quads, seed, scale=0.01):
    """A seeded jitter of q, u and v: normal, of deviation `scale` times the quad's longer edge."""
    rng = np.random.default_rng(seed)
    out = quads.copy()
    ext = np.maximum(np.linalg.norm(quads["u"][:, :3], axis=1), np.linalg.norm(quads["v"][:, :3], axis=1))[:, None]
    for k in ("q", "u", "v"):
        out[k][:, :3] += (rng.normal(0.0, scale, (len(out), 3)) * ext).astype(np.float32)
    return out


def jitter_spheres(spheres, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    out = spheres.copy()
    r = np.maximum(out["center_radius"][:, 3:4], 0.0)
    out["center_radius"][:, :3] += (rng.normal(0.0, scale, (len(out), 3)) * r).astype(np.float32)
    return out


def _same_parallelogram(a, b):
    def corners(q, u, v):
        q, u, v = (np.asarray(x[:3], np.float64) for x in (q, u, v))
        return sorted(map(tuple, (q, q + u, q + v, q + u + v)))

    return corners(*a) == corners(*b)


def moved(sc, seed, scale=0.01):
    """(spheres, quads, lights) of `sc` after a seeded move: every quad and sphere jittered, but a
    primitive that a book-3 light samples is translated, and its light entry with it by the same
    vector, so the light list keeps restating the geometry."""
    rng = np.random.default_rng(seed + 1000)
    spheres = jitter_spheres(sc.spheres, seed, scale)
    quads = None if sc.quads is None else jitter_quads(sc.quads, seed, scale)
    if sc.lights is None:
        return spheres, quads, None
    lights = sc.lights.copy()
    for l, L in enumerate(sc.lights):
        if int(L["kind"]) == 0:
            at = [j for j, q in enumerate(sc.quads) if _same_parallelogram((q["q"], q["u"], q["v"]), (L["a"], L["u"], L["v"]))]
            ext = max(np.linalg.norm(L["u"][:3]), np.linalg.norm(L["v"][:3]))
        else:
            at = [i for i, s in enumerate(sc.spheres) if np.array_equal(s["center_radius"], L["a"])]
            ext = float(L["a"][3])
        assert len(at) == 1, f"light {l} names one primitive of the scene"
        d = (rng.normal(0.0, scale, 3) * ext).astype(np.float32)
        lights["a"][l, :3] = L["a"][:3] + d
        if int(L["kind"]) == 0:
            quads[at[0]] = sc.quads[at[0]]
            quads["q"][at[0], :3] = sc.quads["q"][at[0], :3] + d
        else:
            spheres[at[0]] = sc.spheres[at[0]]
            spheres["center_radius"][at[0], :3] = sc.spheres["center_radius"][at[0], :3] + d
    return spheres, quads, lights


def big_scene(n_quads=300, n_spheres=40, seed=7):
    """300 quads and 40 spheres over five materials, scattered in a 40-unit cube."""
    rng = np.random.default_rng(seed)
    mats = np.concatenate([S._material(0, (0.6, 0.3, 0.2)), S._material(1, (0.8, 0.8, 0.9), fuzz=0.1),
                           S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5), S._material(4, (3.0, 3.0, 2.5)),
                           S._material(0, (0.2, 0.5, 0.7))])
    sph = np.concatenate([S._sphere(tuple(rng.uniform(-20, 20, 3)), rng.uniform(0.5, 2.0), k % len(mats))
                          for k in range(n_spheres)])
    quads = np.concatenate([quad(rng.uniform(-20, 20, 3), rng.normal(0, 1, 3) * rng.uniform(1, 3),
                                 rng.normal(0, 1, 3) * rng.uniform(1, 3), k % len(mats)) for k in range(n_quads)])
    cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=50.0,
                        lookfrom=(0.0, 5.0, 45.0), lookat=(0.0, 0.0, 0.0), n_spheres=len(sph))
    return S.SceneData(cam, sph, mats, flags=scene("NW5").flags, name="big_quads", quads=quads)
