"""Expected surface records and the media scan cases for the surface-record tests (DeviceScene.surface,
include/rrt_hip.h rrt_scene_surface_async), shared by tests/test_surface_cases.py (CPU) and
tests/test_gpu_surface.py (the kernel). Builds on tests/ray_query_cases.py. Helper module: no tests.

The expected record is a function of the ray, the REPORTED (prim, t) and the scene, so every ray's
record is checked, the undecided ones of the scan too (which primitive the walk answers is the scan's
question, tests/ray_query_cases.py; what the record says about that primitive is this module's):

  p           fma_f32(d, t, o): the exact product and sum rounded once to f32
  normal,     oracle.sphere_hit(..., f32=True) at ray_query_cases.centres_at's centre, oracle.quad_hit(...,
  front_face  f32=True): the oracle's f32 twins of HitRecord. Their t must be the reported t bit for bit:
              a difference is a finding about the kernel, and expected() raises on it
  uv          oracle.acos_f32 / oracle.atan2_f32 of the outward normal, then the IEEE f32 divisions by 2 pi
              and pi (tests/test_gpu_recip.py proves the kernel's div_by_const equal to them); a quad's (0, 0)
  albedo      by kind: the material table; (1, 1, 1) for a dielectric; kind 3 the scene's texture bytes at
              texel()'s clamp and truncation in numpy f32; kinds 5 and 6 oracle.book2_textures(f32=True) at p
  a miss      the camera's background, or oracle.vec_f32's unit_vector and the sky gradient in numpy f32

The new scan cases are scenes with constant media (and the two texture classes the query cases lack);
ray_query_cases.geometry() keeps a scene's spheres and quads only, so their linear scan is the scan of
the surfaces. Generators are cached; callers leave results unchanged.
"""
import functools

import numpy as np

import rustraytrace_amd as rrt
from rustraytrace_amd import _lib
from oracle import oracle

import book2_class_scenes as B
import ray_query_cases as Q

NO = _lib.NO_PRIM
MISS = _lib.SURFACE_MISS
TIME = 0.37


# ---- fma ---------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """fma(a, b, c) of f32 arrays rounded once to f32. The product of two f32 is exact in double; the
    double sum is rounded to odd (the error term of the two-sum decides the sticky bit), which a final
    rounding to f32's 24 bits cannot tell from the exact value. (math.fma on doubles would round to 53
    bits to nearest first: a double rounding, wrong at the f32 midpoints test_surface_cases.py builds.)"""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # two-sum: p + c = s + e exactly
        bits = np.ascontiguousarray(s).view(np.uint64)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((bits & np.uint64(1)) == 0)
        towards = np.where(e > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, towards), s)
        return s.astype(np.float32)


# ---- the new scan cases ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "smoke":  # the_next_week 8: two quad-bounded media
        return rrt.next_week_scene(8, dict(image_width=32, **Q._SMALL))
    if name == "comp3n":
        return B.composite(3, True)
    if name == "final10":  # the_next_week 10: a sphere-bounded medium and an unbounded one
        return rrt.next_week_scene(10, dict(image_width=32, **Q._SMALL))
    if name == "comp1n":  # kinds 0, 1, 2, 5, 6
        return B.composite(1, True)
    if name == "earth":  # the_next_week 3: kind 3, a book-1 class with an image texture
        return rrt.next_week_scene(3, dict(image_width=32, **Q._SMALL))
    return Q.scene(name)


_SMOKE = dict(inside=Q._CORNELL["inside"], off=((200.0, 330.0, -800.0), (-300.0, -300.0, 100.0), (855.0, 855.0, 450.0)))
RECIPES = {
    "smoke": _SMOKE, "comp3n": _SMOKE,
    "final10": dict(inside_hi=(None, (-100.0, 150.0, -100.0), (600.0, 600.0, 500.0))),
    "comp1n": Q.RECIPES["comp1"],
    "earth": dict(camera=Q._RTOW["camera"]),
}
# (scene, ray set, time) of the new scans
MEDIA_CASES = [(n, s, TIME) for n in ("smoke", "comp3n") for s in ("inside", "off")] + [("final10", "inside_hi", TIME)]
NEW_CASES = MEDIA_CASES + [("comp1n", s, TIME) for s in ("camera", "inside")] + [("earth", "camera", TIME)]


# The composites' sixty field spheres (fifteen of each kind 0, 1, 2, 6; radius 4 to 9 in a 555 box, 0.12
# to 0.3 around the checkered spheres) are small targets: the recipes alone reach some of their kinds 1
# to 7 times in 4,096 rays (comp3n inside {1: 2, 2: 2, 6: 4}, off {1: 7, 6: 6}; comp1n camera {0: 1, 2: 7}).
# So the last N_AIMED rays of every set of these two scenes keep the recipe's origin and are aimed at the
# field spheres in turn instead, at a point within 0.3 r of the centre at the ray's time: the set stays
# 4,096 rays, and tests/test_surface_cases.py holds it to the same undecided, hit and miss conditions.
N_AIMED = 512
N_FIELD = 60
AIMED = ("comp3n", "comp1n")


@functools.lru_cache(maxsize=None)
def rays(name, ray_set, time=0.0):
    """ray_query_cases.rays, by this module's recipes for the new scenes."""
    if name not in RECIPES:
        return Q.rays(name, ray_set, time)
    eye, lo, hi = RECIPES[name][ray_set]
    rng = np.random.default_rng(Q.SEED)
    p = rng.uniform(lo, hi, (Q.N_RAYS, 3))
    if eye is not None:
        o = np.broadcast_to(np.asarray(eye, dtype=np.float32), (Q.N_RAYS, 3)).copy()
        d = p.astype(np.float32) - o
    else:
        o, d = p.astype(np.float32), rng.standard_normal((Q.N_RAYS, 3)).astype(np.float32)
    if name in AIMED:
        sc = scene(name)
        k = len(sc.spheres) - N_FIELD + np.arange(N_AIMED) % N_FIELD  # the field spheres follow the base scene's
        cr = sc.spheres["center_radius"][k].astype(np.float64)
        c = cr[:, :3] + time * sc.motion[k, :3].astype(np.float64)
        target = c + np.random.default_rng(Q.SEED + 1).uniform(-0.3, 0.3, (N_AIMED, 3)) * cr[:, 3:4]
        d[-N_AIMED:] = (target - o[-N_AIMED:]).astype(np.float32)
    r = Q.make_rays(o, d, np.inf, time)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def case_scan(name, ray_set, time=0.0):
    if name not in RECIPES:
        return Q.case_scan(name, ray_set, time)
    return Q.scan(Q.geometry(scene(name)), rays(name, ray_set, time))


def material_index(sc, spheres=None):
    """The material of every primitive in source order (spheres, then quads)."""
    sp = sc.spheres if spheres is None else spheres
    mi = np.asarray(sp["material_index"], dtype=np.int64)
    if sc.quads is not None:
        mi = np.concatenate([mi, np.asarray(sc.quads["material_index"], dtype=np.int64)])
    return mi


def surface_kinds(sc):
    """The material kinds the scene's surfaces carry."""
    return sorted(set(int(k) for k in sc.materials["kind"][material_index(sc)]))


# ---- the expected record -----------------------------------------------------------------------------------
PI = np.float32(3.14159265358979323846)
TWO_PI = np.float32(2.0) * PI


def _texel(tex, u, v):
    """texel() of rrt_kernel.hip in numpy f32: Interval::clamp, v flipped, truncation, the index clamp,
    the channel as (1 / 255) * byte."""
    h, w = tex.shape[:2]
    one, zero = np.float32(1.0), np.float32(0.0)
    u = np.minimum(np.maximum(u, zero), one).astype(np.float32)
    v = (one - np.minimum(np.maximum(v, zero), one)).astype(np.float32)
    i = np.clip((u * np.float32(w)).astype(np.float32).astype(np.int64), 0, w - 1)
    j = np.clip((v * np.float32(h)).astype(np.float32).astype(np.int64), 0, h - 1)
    cs = np.float32(1.0) / np.float32(255.0)
    return (cs * tex[j, i].astype(np.float32)).astype(np.float32)


def _background(sc, d):
    cam = sc.camera[0]
    if int(cam["params_u"][3]) == 1:
        return np.broadcast_to(np.asarray(cam["background"][:3], dtype=np.float32), (len(d), 3))
    rows = np.zeros((len(d), 9), np.float32)
    rows[:, :3] = d
    with np.errstate(all="ignore"):
        uy = oracle.vec_f32(rows)[:, 1]
        a = (np.float32(0.5) * (uy + np.float32(1.0))).astype(np.float32)
        om = (np.float32(1.0) - a).astype(np.float32)
        return np.stack([(om * np.float32(1.0) + a * np.float32(k)).astype(np.float32) for k in (0.5, 0.7, 1.0)], axis=1)


def expected(sc, r, prim, t, spheres=None, motion=None):
    """The SURFACE_DTYPE records of rays r whose closest-hit query reported (prim, t) on scene sc
    (spheres / motion: an update's new rows)."""
    g = Q.geometry(sc, spheres, motion)
    n, ns = len(r), len(g.centres)
    prim = np.asarray(prim, dtype=np.uint32)
    t = np.asarray(t, dtype=np.float32)
    out = np.zeros(n, dtype=_lib.SURFACE_DTYPE)
    hit = prim != NO
    out["prim"], out["kind"] = NO, MISS
    if (~hit).any():
        out["albedo"][~hit] = _background(sc, r["d"][~hit])
    if not hit.any():
        return out
    idx = np.nonzero(hit)[0]
    assert (prim[idx] < g.n_prims).all(), "a reported primitive is no surface of the scene"
    p = fma_f32(r["d"], t[:, None], r["o"])
    outward = np.zeros((n, 3), np.float32)
    is_sphere = hit & (prim < ns)
    tm = r["time"].astype(np.float32)
    for i in idx:
        k = int(prim[i])
        o, d, tmax = r["o"][i], r["d"][i], float(r["tmax"][i])
        if k < ns:
            c = (g.centres[k] + (tm[i] * g.motion[k]).astype(np.float32)).astype(np.float32)  # Prims::at
            res = oracle.sphere_hit(c, float(g.radii[k]), o, d, float(Q.T_MIN), tmax, f32=True)
        else:
            q = g.quads[k - ns]
            res = oracle.quad_hit(q["q"][:3], q["u"][:3], q["v"][:3], o, d, float(Q.T_MIN), tmax, f32=True)
        assert res is not None, f"ray {i}: the oracle's test of the reported primitive {k} rejects the ray"
        to, nrm, front = res
        assert np.float32(to).view(np.uint32) == t[i].view(np.uint32), \
            f"ray {i}, primitive {k}: the oracle's t {np.float32(to)!r} is not the reported {t[i]!r}"
        nrm = nrm.astype(np.float32)
        out["normal"][i] = nrm
        out["front_face"][i] = 1 if front else 0
        outward[i] = nrm if front else -nrm
    out["p"][idx], out["t"][idx], out["prim"][idx] = p[idx], t[idx], prim[idx]
    # get_sphere_uv on the outward normal, for every sphere
    si = np.nonzero(is_sphere)[0]
    if len(si):
        ow = outward[si]
        theta = oracle.acos_f32(-ow[:, 1])
        phi = (oracle.atan2_f32(np.stack([-ow[:, 2], ow[:, 0]], axis=1)) + PI).astype(np.float32)
        out["uv"][si, 0] = (phi / TWO_PI).astype(np.float32)
        out["uv"][si, 1] = (theta / PI).astype(np.float32)
    # the material
    mi = material_index(sc, spheres)[prim[idx].astype(np.int64)]
    mats = sc.materials
    out["kind"][idx] = mats["kind"][mi]
    alb = mats["albedo_fuzz"][mi, :3].astype(np.float32)
    for m in np.unique(mi):
        sel = mi == m
        rows = idx[sel]
        mat = mats[m]
        kind = int(mat["kind"])
        if kind == 2:
            alb[sel] = 1.0
        elif kind == 3:
            alb[sel] = _texel(sc.textures[int(mat["_pad"][0])], out["uv"][rows, 0], out["uv"][rows, 1])
        elif kind == 5:
            table = sc.perlin[0] if sc.perlin is not None and len(sc.perlin) else np.zeros(1, _lib.PERLIN_DTYPE)[0]
            even = oracle.book2_textures(table, p[rows], inv_scale=float(mat["albedo_fuzz"][3]), f32=True)[2]
            odd = np.array([mat["ref_idx"], mat["_pad"][:1].view(np.float32)[0], mat["_pad"][1:2].view(np.float32)[0]], np.float32)
            alb[sel] = np.where(even[:, None], alb[sel], odd[None, :])
        elif kind == 6:
            value = oracle.book2_textures(sc.perlin[int(mat["_pad"][0])], p[rows], scale=float(mat["albedo_fuzz"][3]), f32=True)[1]
            alb[sel] = value.astype(np.float32)[:, None]
        else:
            assert kind in (0, 1, 4), f"material kind {kind} on a surface"
    out["albedo"][idx] = alb
    return out


FIELDS = ("p", "t", "normal", "prim", "albedo", "kind", "uv", "front_face", "_pad")


def assert_records_equal(got, want, what=""):
    """Bit for bit in every field, naming the first differing field and ray."""
    assert got.dtype == _lib.SURFACE_DTYPE and got.shape == want.shape
    for f in FIELDS:
        a = np.ascontiguousarray(got[f]).view(np.uint32).reshape(len(got), -1)
        b = np.ascontiguousarray(want[f]).view(np.uint32).reshape(len(want), -1)
        bad = (a != b).any(axis=1)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{what}: {int(bad.sum())} records differ in `{f}`, first ray {i}: got {got[f][i]!r}, "
                                 f"want {want[f][i]!r} (prim {got['prim'][i]}, kind {got['kind'][i]})")
    assert got.tobytes() == want.tobytes(), what
