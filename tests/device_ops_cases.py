"""Inputs of the elementwise device checks (tests/test_gpu_device_ops.py) and of their CPU
companion (tests/test_device_ops_cases.py), chosen at the edges where the f32 kernel's building
blocks can go wrong: octant seams, mantissa splits, saturating conversions, exact lattice points,
closed and open interval ends, the per-ray reciprocal's range ends.

Every generator is deterministic (seeded) and returns a dict of class name -> float32 array, so the
CPU test can assert that each named class is present; rows(d) concatenates the classes into the
row layout of the device op (include/rrt_hip.h rrt_testing_device_ops). The big sets are cached:
compute once, never modify.
"""
import functools

import numpy as np

F = np.float32
INF = F(np.inf)
NAN = F(np.nan)
TWO_PI = F(2.0) * F(np.pi)  # the kernel's 2.0f * kPi
PI = F(np.pi)
DENORM_MIN = np.array([1], np.uint32).view(F)[0]   # 2^-149
DENORM_MAX = np.array([0x007fffff], np.uint32).view(F)[0]


def f32(x):
    return np.ascontiguousarray(x, dtype=F)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(F)


def step(x, k):
    """x moved k floats up (k < 0: down) in value order, elementwise."""
    x = np.array(x, dtype=F)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, INF if k > 0 else -INF, dtype=F)
    return x[()] if x.ndim == 0 else x


def around(x, r=2):
    """x and its neighbours up to r floats either side (value order), flattened."""
    return np.concatenate([step(x, k).ravel() for k in range(-r, r + 1)])


def rows(classes):
    """The classes of one generator concatenated (class order) into the op's row array."""
    parts = [np.atleast_1d(v) for v in classes.values()]
    return np.ascontiguousarray(np.concatenate(parts, axis=0), dtype=F)


def _mantissas(rng, exponents, per, signs=(0, 1)):
    """For each sign and biased exponent, `per` random 23-bit mantissas."""
    e = np.asarray(exponents, np.uint32)
    m = rng.integers(0, 1 << 23, size=(len(signs), len(e), per), dtype=np.uint32)
    s = (np.asarray(signs, np.uint32) << 31)[:, None, None]
    return from_bits((s | (e << 23)[None, :, None] | m).ravel())


SPECIALS = f32([0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX, INF, -INF, NAN])


# ---- sin / cos ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sin_cos_cases():
    rng = np.random.default_rng(0x51C05)
    k = np.arange(1 << 24, dtype=np.float64)
    seams = f32(np.arange((1 << 15) + 1, dtype=np.float64) * (np.pi / 4))
    seams = around(seams)
    return {
        # (2 pi)_f32 * (k 2^-24)_f32: the whole domain of the cosine-direction and light-sampling calls
        "phi_grid": TWO_PI * f32(k * 2.0 ** -24),
        "mantissas": _mantissas(rng, range(256), 2048),
        "octant_seams": np.concatenate([seams, -seams]),
        "big": np.concatenate([around(f32([8192.0, 16777215.0])), -around(f32([8192.0, 16777215.0]))]),
        "special": SPECIALS,
    }


# ---- log ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def log_cases():
    split = f32(np.sqrt(0.5) * 2.0 ** np.arange(-125, 128, dtype=np.float64))  # 2^-0.5 2^e, every normal binade
    return {
        "u_grid": f32(np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24),  # medium_hit's draw; u = 0 -> -inf
        "mantissa_split": around(split),
        "special": f32([DENORM_MIN, DENORM_MAX, 1.0, step(F(1), 1), step(F(1), -1), 2.0, 3.4e38, INF, NAN]),
    }


# ---- acos -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def acos_cases():
    rng = np.random.default_rng(0xAC05)
    return {
        "mantissas": _mantissas(rng, range(0, 127), 4096),  # |x| < 1: every exponent below 2^0
        "edges": np.concatenate([around(f32([0.5, 1.0])), -around(f32([0.5, 1.0]))]),
        # a normal's component can overshoot by an ulp: NaN on both sides
        "overshoot": f32([step(F(1), 1), -step(F(1), 1)]),
        "special": f32([0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX]),
    }


# ---- atan2 ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def atan2_cases():
    rng = np.random.default_rng(0xA7A2)
    t1, t3 = F(np.tan(np.pi / 8)), F(np.tan(3 * np.pi / 8))  # rrt_atanf's range splits
    pos = np.concatenate([f32([0.0, DENORM_MIN, 1e-20, 1.0, 1e20, INF]), around(f32([t1, t3]), 1)])
    axis = np.concatenate([pos, -pos, f32([NAN])])
    yy, xx = np.meshgrid(axis, axis, indexing="ij")
    ang = rng.uniform(-np.pi, np.pi, 1 << 16)
    return {
        "cross": np.stack([yy.ravel(), xx.ravel()], axis=1),
        "unit_circle": f32(np.stack([np.sin(ang), np.cos(ang)], axis=1)),
    }


# ---- the root division ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def div_a_values():
    """The divisors of rrt_testing_div_check (at most 48): the ends of refine_ra's range
    [2^-64, 2^64] with two neighbours each side, 1, 1 +- ulp, 2 - ulp, 0, a denormal, and seeded
    random mantissas across the exponent range (28 inside the range, 4 outside it)."""
    rng = np.random.default_rng(0xD1FA)
    ends = around(f32([2.0 ** -64, 2.0 ** 64]))
    fixed = f32([1.0, step(F(1), 1), step(F(1), -1), step(F(2), -1), 0.0, DENORM_MAX])
    e_in = np.round(np.linspace(-64, 63, 28)).astype(np.int64) + 127
    e_out = np.array([-100, -70, 80, 120], np.int64) + 127
    e = np.concatenate([e_in, e_out]).astype(np.uint32)
    rand = from_bits((e << 23) | rng.integers(0, 1 << 23, size=len(e), dtype=np.uint32))
    out = np.concatenate([ends, fixed, rand])
    assert len(out) == 48
    return out


@functools.lru_cache(maxsize=None)
def div_a_cases():
    """(n, a) rows for the DIV_A op: every divisor of div_a_values against random numerator bit
    patterns, numerators around the 2^-103 bound, around quotients at the acceptance bound 0.001 and
    at the overflow bound, and the specials. Below 2^22 rows."""
    rng = np.random.default_rng(0xD1F0)
    a = div_a_values()
    n_rand = from_bits(rng.integers(0, 1 << 32, size=60000, dtype=np.uint32))
    out = {"random": np.stack([np.tile(n_rand, len(a)), np.repeat(a, len(n_rand))], axis=1)}
    fin = a[np.isfinite(a) & (a > 0)]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        near_accept = np.concatenate([around(F(0.001) * x, 4) for x in fin])
        near_overflow = np.concatenate([around(F(3.4028235e38) * x, 4) for x in fin])
    out["accept_bound"] = np.stack([near_accept, np.repeat(fin, 9)], axis=1)
    out["overflow"] = np.stack([near_overflow, np.repeat(fin, 9)], axis=1)
    tiny = np.concatenate([around(f32([2.0 ** -103])), SPECIALS])
    out["tiny_special"] = np.stack([np.tile(tiny, len(a)), np.repeat(a, len(tiny))], axis=1)
    return out


@functools.lru_cache(maxsize=None)
def div_const_cases():
    rng = np.random.default_rng(0xD1C0)
    return {
        "phi_theta": f32(rng.uniform(0.0, 2 * np.pi, 1 << 16)),
        "mantissas": _mantissas(rng, range(27, 131), 512, signs=(0,)),  # 2^-100 .. 16
        "edges": np.concatenate([around(f32([2.0 ** -100, 8.0, np.pi, 2 * np.pi])), f32([0.0])]),
    }


# ---- floor-as-i32 ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def floor_i32_cases():
    small = around(f32(np.arange(0, 9)), 1)
    big = around(f32([2.0 ** 31, 2.0 ** 23, 2.0 ** 24]))
    return {
        "zero": f32([0.0, -0.0, -DENORM_MIN, DENORM_MIN]),
        "small": np.concatenate([small, -small, f32([0.5, -0.5, 255.5, -255.5])]),
        "saturate": np.concatenate([big, -big, f32([1e30, -1e30, 3e9, -3e9])]),
        "nonfinite": f32([INF, -INF, NAN]),
    }


# ---- textures: Perlin noise and the checker -------------------------------------------------------
PERLIN_SCALES = (0.2, 4.0)
CHECKER_INV_SCALE = F(1.0 / 0.32)  # rrt_build_next_week_scene's (float)(1.0 / 0.32)


@functools.lru_cache(maxsize=None)
def perlin_table():
    from rustraytrace_amd import scenes

    return scenes.next_week_scene(4).perlin[:1].copy()


def _one_coordinate(values, others):
    """Points with one coordinate from `values` (each axis in turn) and the other two from `others`."""
    pts = []
    for axis in range(3):
        for i, v in enumerate(values):
            p = np.array(others[(i + axis) % len(others)], dtype=F)
            p[axis] = v
            pts.append(p)
    return f32(pts)


@functools.lru_cache(maxsize=None)
def texture_points():
    rng = np.random.default_rng(0x9E21)
    g = np.arange(-3, 4)
    lattice = f32(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    ints = f32(np.arange(-4, 5))
    below = step(ints, -1)
    others = f32(rng.uniform(-3, 3, (7, 3)))
    wrap = f32([255.5, 256.5, -0.5])
    return {
        "near": f32(rng.uniform(-20, 20, (4096, 3))),
        "far": f32(rng.uniform(-2000, 2000, (4096, 3))),
        "lattice": lattice,
        "half_lattice": lattice + F(0.5),
        # one ulp below an integer, negative and positive: floor and the fraction u = 1 - ulp
        "below_integer": np.concatenate([np.stack([below] * 3, axis=1), _one_coordinate(below, others)]),
        "wrap": f32(np.stack(np.meshgrid(wrap, wrap, wrap, indexing="ij"), axis=-1).reshape(-1, 3)),
        # 4e7 * 64 and 1e12 pass 2^31: floor_i32 saturates within the seven octave doublings
        "saturate": _one_coordinate(f32([4e7, -4e7, 1e12, -1e12]), others),
        "nonfinite": _one_coordinate(f32([NAN, INF, -INF]), others),
    }


@functools.lru_cache(maxsize=None)
def checker_cases():
    pts = dict(texture_points())
    k = np.arange(-10, 11, dtype=np.float64)
    face = around(f32(k * 0.32), 1)  # the cell faces of scale 0.32 and the floats either side
    g = f32(np.stack(np.meshgrid(face[::3], face[1::3], face[2::3], indexing="ij"), axis=-1).reshape(-1, 3))
    pts["cell_faces"] = np.concatenate([g, _one_coordinate(face, f32([[0.1, 0.2, 0.3], [-1.0, 2.0, 0.5]]))])
    return {name: np.concatenate([np.full((len(p), 1), CHECKER_INV_SCALE, F), p], axis=1) for name, p in pts.items()}


# ---- vectors --------------------------------------------------------------------------------------
def len2_f32(a, b):
    """fma(b, b, a * a) in f32 for scalars a, b (the kernel's dot of (a, b, 0) with itself): a * a
    and b * b are exact in float64 and their sum needs fewer than 53 bits for |a|, |b| in [0.5, 1]."""
    return F(float(F(float(a) * float(a))) + float(b) * float(b))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return f32(v / np.linalg.norm(v, axis=1, keepdims=True))


@functools.lru_cache(maxsize=None)
def vec_cases():
    """Rows (v, n, e, cosine, r0)."""
    rng = np.random.default_rng(0x7EC3)

    def r0_of(ri):
        q = (F(1) - F(ri)) / (F(1) + F(ri))
        return q * q

    def pack(v, n, e=None, cosine=None, r0=None):
        v, n = f32(v).reshape(-1, 3), f32(n).reshape(-1, 3)
        m = len(v)
        e = f32(rng.choice([1 / 1.5, 1.5, 1.0], m)) if e is None else np.full(m, e, F)
        cosine = f32(rng.uniform(0, 1, m)) if cosine is None else f32(np.broadcast_to(cosine, m))
        r0 = f32([r0_of(x) for x in e]) if r0 is None else f32(np.broadcast_to(r0, m))
        return np.concatenate([v, n, e[:, None], cosine[:, None], r0[:, None]], axis=1)

    u, nn = _unit(rng, 2048), _unit(rng, 2048)
    scale = f32(10.0 ** rng.uniform(-3, 3, (2048, 1)))
    axes = f32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])
    perp_v = f32([axes[i] for i in range(6) for j in range(6) if i % 3 != j % 3])
    perp_n = f32([axes[j] for i in range(6) for j in range(6) if i % 3 != j % 3])
    # grazing refraction: e = 1 and n = z perpendicular to uv = (a, b, 0), so perp = uv and
    # k = |1 - fma(b, b, a * a)|; b scanned around 0.8 at a = 0.6 for k = 0 and k = 2^-24 exactly
    a, graze = F(0.6), {0.0: [], 2.0 ** -24: []}
    for b in around(F(0.8), 40):
        k = abs(1.0 - float(len2_f32(a, b)))
        if k in graze:
            graze[k].append([a, b, 0.0])
    x9 = around(F(0.9), 4)
    switch = np.concatenate([np.stack([s * x9, f32(np.sqrt(1.0 - x9.astype(np.float64) ** 2)), 0 * x9], axis=1)
                             for s in (F(1), F(-1))])
    zero = f32([[0, 0, 0]])
    return {
        "random_unit": pack(u, nn),
        "random_nonunit": pack(u * scale, nn * scale[::-1]),
        "parallel": pack(np.concatenate([nn[:64], -nn[:64]]), np.concatenate([nn[:64], nn[:64]])),
        "perpendicular": pack(perp_v, perp_n),
        "grazing_k0": pack(graze[0.0], [[0, 0, 1]] * len(graze[0.0]), e=1.0),
        "grazing_k2m24": pack(graze[2.0 ** -24], [[0, 0, 1]] * len(graze[2.0 ** -24]), e=1.0),
        "cosine_0_1": pack(u[:64], nn[:64], cosine=np.tile(f32([0.0, 1.0]), 32)),
        "onb_switch": pack(u[: len(switch)], switch),
        "zero": pack(np.concatenate([zero, u[:1], zero]), np.concatenate([nn[:1], zero, zero])),
    }


# ---- quads ----------------------------------------------------------------------------------------
QUADS = (  # (q, u, v): exactly representable corners
    ((-1, -1, -2), (2, 0, 0), (0, 2, 0)),        # 0: axis-aligned, normal +z
    ((3, 0, 1), (0, 0, -2), (0, 4, 0)),          # 1: axis-aligned, normal along x
    ((0, 0, 0), (1, 0, 1), (0, 1, 0)),           # 2: rotated 45 degrees about y
    ((1, 2, 3), (3, 4, 0), (0, 0, 5)),           # 3: rotated, 3-4-5 edge
    ((0.25, 0.25, 0.5), (0.0078125, 0, 0), (0, 0.0078125, 0)),  # 4: tiny
    ((555, 0, 0), (0, 555, 0), (0, 0, 555)),     # 5: a Cornell-box wall
)


def quad_records():
    from rustraytrace_amd import _lib

    q = np.zeros(len(QUADS), dtype=_lib.QUAD_DTYPE)
    for i, (a, b, c) in enumerate(QUADS):
        q["q"][i, :3], q["u"][i, :3], q["v"][i, :3] = a, b, c
    return q


@functools.lru_cache(maxsize=None)
def quad_cases():
    """Rows (o, d, tmin, closest, quad index)."""
    rng = np.random.default_rng(0x90AD)

    def row(o, d, tmin, closest, j):
        return [*o, *d, tmin, closest, j]

    out = {k: [] for k in ("corners", "edges", "outside", "random")}
    for j, (q, u, v) in enumerate(QUADS):
        q, u, v = (np.array(x, np.float64) for x in (q, u, v))
        nrm = np.cross(u, v)
        nrm /= np.linalg.norm(nrm)
        eps = 2.0 ** -10 if j == 4 else 1e-6  # the tiny quad's edge times 1e-6 is below its corner's ulp
        for name, ab in (("corners", [(0, 0), (1, 0), (0, 1), (1, 1)]),
                         ("edges", [(0.5, 0), (0.5, 1), (0, 0.5), (1, 0.5), (0.5, 0.5)]),
                         ("outside", [(-eps, 0.5), (1 + eps, 0.5), (0.5, -eps), (0.5, 1 + eps), (-eps, -eps)])):
            for al, be in ab:
                target = q + al * u + be * v
                for dist in (2.0, -3.0):  # from either side: exact for the axis-aligned quads
                    out[name].append(row(target + dist * nrm, -nrm * np.sign(dist), 0.001, np.inf, j))
        for _ in range(256):
            target = q + rng.uniform(-0.2, 1.2) * u + rng.uniform(-0.2, 1.2) * v
            o = target + rng.normal(size=3) * 3
            out["random"].append(row(o, target - o, 0.001, rng.choice([np.inf, 0.9, 1.0, 1.1]), j))
    # quad 0 (normal +z, D = -2): denom = d.z on either side of the 1e-8 cut, both signs; straight
    # down the normal so that the (huge, negative) t still lands inside over (-inf, inf)
    cut = around(F(1e-8))
    out["denom_cut"] = [row((0, 0, -1), (0, 0, s * dz), -np.inf, np.inf, 0) for dz in cut for s in (1, -1)]
    # o = origin, d = -z: t = 2 exactly; the interval is closed at both ends
    two = F(2)
    out["t_bounds"] = [row((0, 0, 0), (0, 0, -1), tmin, closest, 0)
                       for tmin, closest in ((two, INF), (step(two, 1), INF), (step(two, -1), INF), (F(0.001), two),
                                             (F(0.001), step(two, -1)), (F(0.001), step(two, 1)), (two, two))]
    # the medium's use: the boundary's hit over (-inf, inf), behind the origin included
    out["tmin_neg_inf"] = [row((0, 0, 0), (0, 0, 1), -np.inf, np.inf, 0), row((0.5, 0.5, 5), (0, 0, 1), -np.inf, np.inf, 0),
                           row((0, 0, 0), (0, 0, 1), 0.001, np.inf, 0), row((4, 1, 0), (1, 0, 0), -np.inf, np.inf, 1)]
    out["parallel"] = [row((0, 0, 0), (1, 0, 0), 0.001, np.inf, 0), row((0, 0, -2), (1, 1, 0), 0.001, np.inf, 0),
                       row((0, 0, 0), (0, 1, 0), -np.inf, np.inf, 2), row((0, 0, 0), (0, 0, 0), 0.001, np.inf, 3)]
    return {k: f32(v) for k, v in out.items()}


# ---- spheres --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere_cases():
    """Rows (o, d, c, r, closest)."""
    rng = np.random.default_rng(0x5FE2)

    def row(o, d, c, r, closest=np.inf):
        return [*o, *d, *c, r, closest]

    out = {}
    # the ray down -z passes at distance 1 from (1, 0, -1): h = 1, c = 2 - r^2, disc = 0 exactly at
    # r = 1 and -2^-23 / +2^-22 one float below / above it (small numbers, so no ulp is absorbed)
    out["tangent"] = [row((0, 0, 0), (0, 0, -1), (1, 0, -1), r) for r in around(F(1), 2)]
    out["inside"] = [row((0, 0, -4), (0, 0, -1), (0, 0, -4), 1), row((0.1, 0.2, -3.7), (1, 2, 3), (0, 0, -4), 1),
                     row((0, 0, -4), (0, 1, 0), (0, 0, -4), 1000)]
    # the origin on the surface (near root about 0: the far root answers), and 0.001 in front of it:
    # the near root on either side of the acceptance bound
    out["on_surface"] = [row((0, 0, -3), (0, 0, -1), (0, 0, -4), 1), row((0, 0, -3), (0, 0, 1), (0, 0, -4), 1)]
    out["on_surface"] += [row((0, 0, 0), (0, 0, -1), (0, 0, -cz), 1) for cz in around(F(1.001), 8)]
    out["radius"] = [row((0, 0, 0), (0, 0, -1), (0, 0, -4), r) for r in (0.0, -1.0, -0.0)]
    out["radius"] += [row((0, 0, 0), (0, 0.25, -1), (0, 1, -4), r) for r in (0.0, -1.0)]
    # |d|^2 = s^2 at the ends of the per-ray reciprocal's range [2^-64, 2^64]
    out["a_range"] = [row((0, 0, 0), (s, 0, 0), (5, 0, 0), 1) for s in around(F(2.0 ** -32), 2)]
    out["a_range"] += [row((0, 0, 0), (0, -s, 0), (0, -5e8, 0), 1e8) for s in around(F(2.0 ** 32), 2)]
    out["d_zero"] = [row((0, 0, 0), (0, 0, 0), (0, 0, -4), 1), row((0, 0, -4), (0, 0, 0), (0, 0, -4), 1)]
    # A root beyond the largest float. With a = |d|^2 in the reciprocal's range [2^-64, 2^64] no sphere
    # root overflows: c = |oc|^2 - r^2 must stay finite, so |oc| < 2^64 and the root below 2^97. So the
    # rays are short, d = (2^-70, 0, 0) (a = 2^-140: the IEEE division), and every intermediate is finite
    # (h, disc, sq about 2^-12, 2^-24, 2^-12; tests/test_device_ops_cases.py works them out):
    #   |oc| = 2^60, r = 2^59               h - sq = 2^-11, / a = 2^129: inf, and the far root too
    #   |oc| = 3 2^57, r = 2^57             h - sq = 2^-12, / a = 2^128: inf
    #   |oc| = 3 2^57, r = 2^57 (1 + 2^-22) h - sq = 2^-12 (1 - 2^-23): 2^128 (1 - 2^-23), finite and accepted, the
    #                                       nearest to the largest float these roundings reach (r one float
    #                                       lower gives inf: c moves by 2^-24 relative, the root by 2^-23)
    #   |oc| = 3 2^57, r = 2^58             h - sq = 2^-13: 2^127, finite
    # and one long root on the per-ray reciprocal: d = (2^-31, 0, 0), a = 2^-62, root about 2^90.
    short, far = F(2.0 ** -70), F(3 * 2.0 ** 57)
    out["overflow"] = [row((0, 0, 0), (short, 0, 0), (2.0 ** 60, 0, 0), 2.0 ** 59),
                       row((0, 0, 0), (short, 0, 0), (far, 0, 0), 2.0 ** 57),
                       row((0, 0, 0), (short, 0, 0), (far, 0, 0), step(F(2.0 ** 57), 2)),
                       row((0, 0, 0), (short, 0, 0), (far, 0, 0), 2.0 ** 58),
                       row((0, 0, 0), (F(2.0 ** -31), 0, 0), (2.0 ** 60, 0, 0), 2.0 ** 59)]
    # root = 3 exactly: `closest` equal to it rejects (strict <), one float above accepts
    three = F(3)
    out["closest_equal"] = [row((0, 0, 0), (0, 0, -1), (0, 0, -4), 1, c)
                            for c in (three, step(three, 1), step(three, -1), F(5), step(F(5), 1))]
    c = rng.uniform(-10, 10, (4096, 3))
    r = rng.uniform(0.05, 3, (4096, 1))
    o = rng.uniform(-10, 10, (4096, 3))
    d = (c + rng.normal(size=(4096, 3)) * r - o) * 10.0 ** rng.uniform(-2, 2, (4096, 1))
    closest = rng.choice([np.inf, 0.5, 1.0, 2.0], (4096, 1))
    out["random"] = np.concatenate([o, d, c, r, closest], axis=1)
    return {k: f32(v) for k, v in out.items()}


# ---- book 3's light list: lights_pdf, lights_random -------------------------------------------------
LIGHT_QUADS = (  # (q, u, v): exactly representable
    ((343, 554, 332), (-130, 0, 0), (0, 0, -105)),  # 0: the stock scene's ceiling light, normal -y
    ((60, 250, 420), (90, 0, 0), (0, 70, 0)),       # 1: upright, normal +z
    ((1, 2, 3), (3, 4, 0), (0, 0, 5)),              # 2: rotated, 3-4-5 edge
)
# (centre, radius). 3: r^2 = 1.5 - 2^-23 in f32 and |oc|^2 = 1.5 from (-r, -2^-11.5, 0), so r^2 / d^2 is
# the largest float below 1 (light_origins' just_outside); 4: the tangent rays of sphere_cases
LIGHT_SPHERES = (((190, 90, 190), 90), ((0, 0, -4), 1), ((278, 500, 278), 0.05), ((0, 0, 0), float(F(np.sqrt(1.5)))),
                 ((1, 0, -1), 1))
LIGHT_LISTS = {  # n_lights -> entries ("q", index) / ("s", index); 1 / 3, 1 / 5 and 1 / 7 are inexact
    1: (("s", 0),),
    2: (("q", 0), ("s", 0)),
    3: (("q", 1), ("s", 3), ("q", 0)),
    5: (("q", 0), ("q", 1), ("s", 0), ("s", 1), ("s", 2)),
    7: (("q", 0), ("s", 0), ("q", 1), ("s", 1), ("q", 2), ("s", 2), ("s", 4)),
}
# Path keys (seed, pixel, sample) whose first draw is 0xffffff * 2^-24, the largest value rnd returns:
# found by evaluating the stream's first word over pixels 0 .. 2^22 of seeds 1, 2, ... (the CPU test
# checks them against oracle.path_stream). random_int's index is then n - 1, never n.
MAX_DRAW_KEYS = ((1, 1151665, 2), (2, 2552861, 1), (5, 3719686, 0), (5, 2071782, 1), (6, 1157237, 0), (6, 2444515, 3))


def light_records(n):
    from rustraytrace_amd import _lib

    out = np.zeros(n, dtype=_lib.LIGHT_DTYPE)
    for k, (kind, j) in enumerate(LIGHT_LISTS[n]):
        if kind == "q":
            out[k]["kind"] = 0
            out[k]["a"][:3], out[k]["u"][:3], out[k]["v"][:3] = LIGHT_QUADS[j]
        else:
            out[k]["kind"] = 1
            out[k]["a"] = [*LIGHT_SPHERES[j][0], LIGHT_SPHERES[j][1]]
    return out


@functools.lru_cache(maxsize=None)
def light_origins(n):
    """Origin classes for the list of n lights: dict class -> (k, 3) float32."""
    rng = np.random.default_rng(0x11E7 + n)
    out = {"general": rng.uniform(20.0, 535.0, (6, 3))}
    plane, surface, inside, outside, far, centre = [], [], [], [], [], []
    for kind, j in LIGHT_LISTS[n]:
        if kind == "q":
            q, u, v = (np.array(x, np.float64) for x in LIGHT_QUADS[j])
            nrm = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
            for al, be in ((0.5, 0.5), (1.5, 0.25)):  # inside the quad's outline and beside it
                p = q + al * u + be * v
                plane += [p, p + 0.001 * nrm, p - 0.001 * nrm, p + 0.0005 * nrm, p - 0.002 * nrm]
        else:
            c, r = np.array(LIGHT_SPHERES[j][0], np.float64), float(LIGHT_SPHERES[j][1])
            surface += [c + (r, 0, 0), c - (0, r, 0), c + (0, 0, r)]
            inside += [c + (0.5 * r, 0, 0), c + (0.25 * r, -0.5 * r, 0.125 * r), c + (0, 0, -0.999 * r)]
            outside += [c + (float(step(F(r), 1)), 0, 0), c - (r, 2.0 ** -11.5, 0), c + (0, 1.001 * r, 0)]
            far += [c + (4096.5 * r, 0, 0), c + (3000 * r, -5000 * r, 100 * r), c - (0, 0, 1e6 * r)]
            centre += [c]
    for name, pts in (("quad_plane", plane), ("sphere_surface", surface), ("sphere_inside", inside),
                      ("sphere_just_outside", outside), ("sphere_far", far), ("sphere_centre", centre)):
        if pts:
            out[name] = np.array(pts)
    return {k: f32(v) for k, v in out.items()}


def _light_dirs(n, o):
    """Direction classes from the origin o (float64 (3,)) for the list of n lights."""
    out = {k: [] for k in ("quad_interior", "quad_edges", "quad_corners", "quad_parallel", "sphere_centre",
                           "sphere_tangent", "away", "special")}
    for kind, j in LIGHT_LISTS[n]:
        if kind == "q":
            q, u, v = (np.array(x, np.float64) for x in LIGHT_QUADS[j])
            nrm = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
            out["quad_interior"] += [q + 0.5 * u + 0.5 * v - o, q + 0.125 * u + 0.75 * v - o]
            out["quad_edges"] += [q + 0.5 * u - o, q + u + 0.5 * v - o, q + 0.5 * v - o, q + 0.5 * u + v - o]
            out["quad_corners"] += [q - o, q + u - o, q + v - o, q + u + v - o]
            # |dot(normal, d)| at and around quad_hit's 1e-8 cut, both signs, and exactly parallel
            uh = u / np.linalg.norm(u)
            out["quad_parallel"] += [uh, v] + [uh + s * float(e) * nrm for e in around(F(1e-8), 1) for s in (1, -1)]
            out["away"] += [o - (q + 0.5 * u + 0.5 * v)]
        else:
            c, r = np.array(LIGHT_SPHERES[j][0], np.float64), float(LIGHT_SPHERES[j][1])
            oc = c - o
            out["sphere_centre"] += [oc, 0.001 * oc]
            d = np.linalg.norm(oc)
            if d > r:  # the tangent cone's edge, just inside and just outside it
                w = oc / d
                a = np.cross(w, (0.0, 1.0, 0.0) if abs(w[0]) > 0.9 else (1.0, 0.0, 0.0))
                a /= np.linalg.norm(a)
                sin_t = r / d
                for k in (1.0 - 1e-6, 1.0, 1.0 + 1e-6):
                    out["sphere_tangent"] += [np.sqrt(max(1.0 - (sin_t * k) ** 2, 0.0)) * w + sin_t * k * a]
            out["away"] += [-oc]
    out["special"] = [(0, 0, 0), (0, -0.0, 0), (np.inf, 0, 0), (0, -np.inf, 1), (np.nan, 1, 0), (1, 1, np.nan),
                      (DENORM_MIN, 0, 0), (1e-30, 1e-30, -1e-30), (1e30, -1e30, 1e30)]
    return out


@functools.lru_cache(maxsize=None)
def lights_pdf_cases(n):
    """Rows (o, d) for the list of n lights: dict "<origin class>/<direction class>" -> rows."""
    out = {}
    for oname, os_ in light_origins(n).items():
        for o in os_.astype(np.float64):
            for dname, ds in _light_dirs(n, o).items():
                out.setdefault(f"{oname}/{dname}", []).extend([*o, *d] for d in ds)
    # disc = 0 exactly and one step either side (sphere 4 from the origin, straight down -z: sphere_cases)
    if ("s", 4) in LIGHT_LISTS[n]:
        out["tangent_exact/disc"] = [[x, 0, 0, 0, 0, -1] for x in (0.0, -(2.0 ** -23), 2.0 ** -24, 2.0 ** -12)]
    return {k: f32(v) for k, v in out.items() if len(v)}


@functools.lru_cache(maxsize=None)
def light_keys(n):
    """Path keys (seed, pixel, sample) for the list of n lights: 8 per index value, from the stream's first
    draw as the kernel turns it into an index (float32 u * n, truncated), then MAX_DRAW_KEYS."""
    from oracle import oracle

    per = {k: [] for k in range(n)}
    pixel = 0
    while any(len(v) < 8 for v in per.values()):
        key = (0xB3, pixel, pixel % 4)
        u = F(oracle.path_stream(*key, 1)[0] >> 8) * F(2.0 ** -24)
        idx = int(u * F(n) + F(0))
        if len(per[idx]) < 8:
            per[idx].append(key)
        pixel += 1
    return per, MAX_DRAW_KEYS


@functools.lru_cache(maxsize=None)
def lights_random_cases(n):
    """Rows (o, seed, pixel, sample as u32 bit patterns): every origin of light_origins(n) with one key per
    index value (cycling through the 8) and every MAX_DRAW_KEYS key from the first origin of each class."""
    per, top = light_keys(n)
    out, turn = {}, 0
    for oname, os_ in light_origins(n).items():
        rows_ = []
        for i, o in enumerate(os_):
            keys = [per[k][(turn + i) % 8] for k in range(n)] + (list(top) if i == 0 else [])
            for key in keys:
                rows_.append(np.concatenate([o, np.array(key, np.uint32).view(F)]))
        turn += 1
        out[oname] = f32(rows_)
    return out
