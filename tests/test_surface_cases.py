"""Conditions on tests/surface_cases.py, on the CPU: the new scans (scenes with constant media, scanned
over their surfaces alone; the noise composite; the earth) decide nearly every ray, hit and miss, and
reach every material kind their surfaces carry; the fma helper is exact; the record layout is the header's.
"""
import fractions
import os
import re

import numpy as np
import pytest

from rustraytrace_amd import _lib

import ray_query_cases as Q
import surface_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{n}-{s}" for n, s, _ in SC.NEW_CASES]


@pytest.mark.parametrize("name,ray_set,time", SC.NEW_CASES, ids=IDS)
def test_new_scans_decide_hit_and_miss(name, ray_set, time):
    sc = SC.case_scan(name, ray_set, time)
    frac = {k: float(v.mean()) for k, v in sc.reasons.items()}
    print(f"{name} {ray_set} t={time}: n={len(sc.hit)} hits={sc.hit.mean():.3f} undecided={sc.undecided.mean():.4f} {frac}")
    assert len(sc.hit) == Q.N_RAYS
    assert sc.undecided.mean() <= Q.UNDECIDED_CAP
    assert sc.hit.mean() >= 0.10 and (~sc.hit).mean() >= 0.10


@pytest.mark.parametrize("name,ray_set,time", SC.NEW_CASES, ids=IDS)
def test_new_scans_reach_every_material_kind(name, ray_set, time):
    """In each case the scan's closest hits include every material kind the scene's surfaces carry, at
    least 8 rays each. The two composites meet it through the rays aimed at their field spheres
    (surface_cases.N_AIMED of each set's 4,096); the recipes alone reached some kinds 1 to 7 times."""
    scene = SC.scene(name)
    sc = SC.case_scan(name, ray_set, time)
    kinds = scene.materials["kind"][SC.material_index(scene)[sc.best_prim[sc.hit].astype(np.int64)]]
    count = {k: int((kinds == k).sum()) for k in SC.surface_kinds(scene)}
    print(f"{name} {ray_set}: closest hits by material kind {count}")
    assert 7 not in count, "a surface with the media's phase function"
    assert all(c >= 8 for c in count.values()), count


def test_aimed_rays_are_a_tail_of_the_recipes_sets():
    """The composites' sets are the recipe's rays but for their last N_AIMED directions; the other scenes'
    sets are the recipe's alone."""
    for name, ray_set, time in SC.NEW_CASES:
        r = SC.rays(name, ray_set, time)
        assert len(r) == Q.N_RAYS
        if name in SC.AIMED:
            stock = Q.rays("comp1", ray_set, time) if name == "comp1n" else None
            if stock is not None:  # comp1n shares comp1's two stock recipes
                k = Q.N_RAYS - SC.N_AIMED
                assert r[:k].tobytes() == stock[:k].tobytes() and r["o"][k:].tobytes() == stock["o"][k:].tobytes()
                assert (r["d"][k:] != stock["d"][k:]).any(axis=1).all()


def test_media_scenes_have_media_and_the_scan_leaves_them_out():
    for name in ("smoke", "comp3n", "final10"):
        scene = SC.scene(name)
        assert scene.media is not None and len(scene.media) > 0
        g = Q.geometry(scene)
        assert g.n_prims == len(scene.spheres) + (0 if scene.quads is None else len(scene.quads))


@pytest.mark.parametrize("builder", ["sweep", "binned"])
def test_root_leaf_in_global_memory_has_a_never_hit_point(monkeypatch, builder):
    """The root-leaf tree read from global memory (one_sphere under RRT_SCENE_IN_LDS=0, which the surface
    tests query): child 1 is the point (65504, 65504, 65504) that rrt_internal.h states, from the sweep
    builder and from the device builder's host twin. It was the box [65504, +inf)^3 with the root's link:
    a ray into the positive octant that missed the sphere entered it and visited the root for ever."""
    from rustraytrace_amd.render import build_bvh, build_bvh_binned, decode_bvh2

    monkeypatch.setenv("RRT_SCENE_IN_LDS", "0")
    sc = Q.scene("one_sphere")
    nodes, order, info = build_bvh(sc) if builder == "sweep" else build_bvh_binned(sc, 1, 1.0, 32)
    assert info["node_stride"] == 32 and info["n_nodes"] == 1
    lo, hi, first, count = decode_bvh2(nodes, 32)
    assert count[0, 0] == 1 and count[0, 1] == 0
    assert np.all(lo[0, 1] == 65504.0) and np.all(hi[0, 1] == 65504.0)


def _exact(a, b, c):
    """fma(a, b, c) rounded once to f32, by rational arithmetic: the nearest f32, ties to even."""
    x = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
    if x == 0:
        return np.float32(0.0)
    f = np.float32(float(x))  # a first guess within an ulp or so; then walk to the nearest
    best = f
    for cand in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        dc, db = abs(fractions.Fraction(float(cand)) - x), abs(fractions.Fraction(float(best)) - x)
        if dc < db or (dc == db and (int(np.float32(cand).view(np.uint32)) & 1) == 0):
            best = cand
    return np.float32(best)


def test_fma_helper_is_exact_on_random_triples():
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(2000) * 10.0 ** rng.integers(-3, 4, 2000)).astype(np.float32)
    b = (rng.standard_normal(2000) * 10.0 ** rng.integers(-3, 4, 2000)).astype(np.float32)
    c = (rng.standard_normal(2000) * 10.0 ** rng.integers(-3, 4, 2000)).astype(np.float32)
    c[:500] = (-a[:500].astype(np.float64) * b[:500].astype(np.float64)).astype(np.float32)  # cancellation
    got = SC.fma_f32(a, b, c)
    want = np.array([_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert got.tobytes() == want.tobytes()


def test_fma_helper_is_exact_where_the_double_sum_lands_on_an_f32_midpoint():
    """a * b = an f32 midpoint m exactly (24 x 24 bits: exact in double); c so small that m + c rounds to
    m in double. Rounding that double to f32 again breaks the tie to even, whatever the sign of c: the
    exact sum is off the midpoint and rounds towards c."""
    rng = np.random.default_rng(11)
    a_l, b_l, c_l = [], [], []
    while len(a_l) < 400:
        k = int(rng.integers(1, 1 << 11)) * 2 + 1  # odd, 12 bits
        q = int(rng.integers(1 << 11, 1 << 12)) * 2 + 1  # odd, 13 bits: k * q odd, 24 or 25 bits
        if (k * q).bit_length() != 25:
            continue  # 25 bits with the last one set: exactly between two f32
        e = int(rng.integers(-20, 20))
        a_l.append(np.float32(k)), b_l.append(np.float32(np.ldexp(float(q), e)))
        c_l.append(np.float32(np.ldexp(1.0 if len(a_l) % 2 else -1.0, e - 60)))
    a, b, c = (np.array(x, np.float32) for x in (a_l, b_l, c_l))
    double_sum = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert (double_sum == a.astype(np.float64) * b.astype(np.float64)).all()  # c is lost in double
    want = np.array([_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    got = SC.fma_f32(a, b, c)
    assert got.tobytes() == want.tobytes()
    assert (double_sum.astype(np.float32) != want).sum() >= 100  # the naive double rounding is wrong on these


def test_surface_record_layout_matches_the_header():
    d = _lib.SURFACE_DTYPE
    assert d.itemsize == 64
    assert d.names == ("p", "t", "normal", "prim", "albedo", "kind", "uv", "front_face", "_pad")
    assert [d.fields[k][1] for k in d.names] == [0, 12, 16, 28, 32, 44, 48, 56, 60]
    src = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    rec = re.search(r"typedef struct RrtSurface \{(.*?)\} RrtSurface;", src, re.S).group(1)
    rec = re.sub(r"/\*.*?\*/", "", rec, flags=re.S)
    assert re.findall(r"(?:float|uint32_t) (\w+)", rec) == list(d.names)
    assert _lib.SURFACE_MISS == int(re.search(r"#define RRT_SURFACE_MISS (0x[0-9a-f]+)u", src).group(1), 16)
    for fn in ("rrt_scene_surface_async", "rrt_scene_surface", "rrt_scene_primary_surface_async"):
        assert fn in _lib.EXPORTED_SYMBOLS and re.search(r"int32_t %s\(" % fn, src)
    assert "#define RRT_ABI_VERSION 11u" in src  # additive
