"""Inputs of the f64 kernel's elementwise device checks (tests/test_gpu_device_ops64.py) and of their
CPU companion (tests/test_device_ops64_cases.py), chosen at the edges where the f64 books kernel's
building blocks can go wrong: fdlibm's branch thresholds on the high word, the per-ray reciprocal's
range ends and the quotients at the acceptance bound and the largest finite, texel edges and image
edges of the f32 angle enclosures, the wave-uniform square-root choice.

Every generator is deterministic (seeded) and returns a dict of class name -> float64 array, so the
CPU test can assert that each named class is present; rows(d) concatenates the classes into the row
layout of the device op (include/rrt_hip.h rrt_testing_device_ops64). The sets are cached: compute
once, never modify.
"""
import functools
import os

import numpy as np

D = np.float64
INF = D(np.inf)
NAN = D(np.nan)
PI = D(np.pi)            # the kernel's kPiD
TWO_PI = D(2.0) * PI     # 2.0 * kPiD
DENORM_MIN = D(2.0 ** -1074)
DENORM_MAX = np.array([0x000FFFFFFFFFFFFF], np.uint64).view(D)[0]
MAX = np.finfo(D).max
TMIN = D(0.001)          # the acceptance bound of a root
TEXEL_TAG = 0x7F800001   # rrt_books64.hip kTexelTag


def f64(x):
    return np.ascontiguousarray(x, dtype=D)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(D)


def bits(x):
    return f64(x).view(np.uint64)


def step(x, k):
    """x moved k doubles up (k < 0: down) in value order, elementwise; k may be an array. +-0 are
    one point; a NaN stays a NaN."""
    x = np.array(x, dtype=D)
    b = x.view(np.int64)
    o = np.where(b < 0, -(b & np.int64(0x7FFFFFFFFFFFFFFF)), b) + np.asarray(k, np.int64)
    r = np.where(o < 0, (-o) | np.int64(-0x8000000000000000), o).astype(np.int64).view(D)
    r = np.where(np.isnan(x), x, r)
    return r[()] if r.ndim == 0 else r


def around(x, r=2):
    """x and its neighbours up to r doubles either side (value order), flattened."""
    return np.concatenate([np.atleast_1d(step(x, k)).ravel() for k in range(-r, r + 1)])


def rows(classes):
    """The classes of one generator concatenated (class order) into the op's row array."""
    parts = [np.atleast_1d(v) for v in classes.values()]
    return np.ascontiguousarray(np.concatenate(parts, axis=0), dtype=D)


def _random(rng, lo_exp, hi_exp, n, signs=True):
    """n doubles with a uniform binary exponent in [lo_exp, hi_exp) and a random 52-bit mantissa."""
    e = rng.integers(lo_exp + 1023, hi_exp + 1023, n, dtype=np.uint64)
    m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    s = rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63) if signs else np.uint64(0)
    return from_bits(s | (e << np.uint64(52)) | m)


SPECIALS = f64([0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX, INF, -INF, NAN])

# the high words rrt_acos64 / rrt_atan64 / rrt_atan2_64 branch on (|x| >= 1, < 0.5, <= 2^-57; atan's
# 2^66, 0.4375, 2^-29, 1.1875, 0.6875, 2.4375)
THRESHOLDS = (0x3FE00000, 0x3C600000, 0x3FF00000, 0x3FDC0000, 0x3FE60000, 0x3FF30000, 0x40038000, 0x44100000,
              0x3E200000)


def threshold_neighbours():
    """Both neighbours of each threshold, as the tests on the high word see them: the last double
    below hw << 32, the first and second at it, the last with that high word and the first of the next."""
    out = []
    for hw in THRESHOLDS:
        b = hw << 32
        out += [b - 1, b, b + 1, b | 0xFFFFFFFF, (hw + 1) << 32]
    return from_bits(np.array(out, np.uint64))


# ---- acos -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def acos_cases():
    rng = np.random.default_rng(0xAC0564)
    t = threshold_neighbours()
    one = D(1)
    n = 200_000
    return {
        "thresholds": np.concatenate([t, -t]),
        "special": np.concatenate([SPECIALS, f64([1, -1, 1 + 2.0 ** -52, -(1 + 2.0 ** -52), 1 - 2.0 ** -52,
                                                  -(1 - 2.0 ** -52), step(one, -1), -step(one, -1), 0.5, -0.5])]),
        "subnormal": np.concatenate([from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64)),
                                     -from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64))]),
        "tiny": _random(rng, -1022, -57, n),        # |x| <= 2^-57: pi / 2
        "below_half": _random(rng, -57, -1, n),     # the rational in x * x
        "above_half": _random(rng, -1, 0, n, signs=False),
        "below_minus_half": -_random(rng, -1, 0, n, signs=False),
        "beyond_one": _random(rng, 0, 1023, 4096),  # NaN
    }


# ---- atan2 ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def atan2_cases():
    """Rows (y, x)."""
    rng = np.random.default_rng(0xA7A264)
    t = threshold_neighbours()
    t = np.concatenate([t, -t])
    # the thresholds as atan's own argument: x = 1 passes y through; a power-of-two x divides exactly
    thr = [np.stack([t * abs(x), np.full(len(t), x)], axis=1) for x in (1.0, -1.0, 2.0, -2.0, 0.5, -2.0 ** -40)]
    axis = np.concatenate([SPECIALS, f64([1.0, -1.0, 1e-300, -1e-300, 1e300, -1e300, 3.0, -3.0])])
    yy, xx = np.meshgrid(axis, axis, indexing="ij")
    # k = (high word of |y| - high word of |x|) >> 20 against 60 and -60: exponent gaps 59..62 each
    # way, with the mantissas on either side of each other (the shift floors the difference)
    gap = []
    mant = f64([1.0, 1.5, step(D(2), -1), step(D(1), 1)])
    for g in (59, 60, 61, 62):
        for my in mant:
            for mx in mant:
                for sy in (1, -1):
                    for sx in (1, -1):
                        for e0 in (0, -500, 300):
                            gap.append([sy * my * 2.0 ** (e0 + g), sx * mx * 2.0 ** e0])
                            gap.append([sy * my * 2.0 ** e0, sx * mx * 2.0 ** (e0 + g)])
    n = 200_000
    out = {
        "thresholds": np.concatenate(thr),
        "cross": np.stack([yy.ravel(), xx.ravel()], axis=1),  # signed zeros, infinities, NaN, subnormals, quadrants
        "x_one": np.stack([np.concatenate([_random(rng, -40, 70, 4096), SPECIALS]), np.ones(4096 + len(SPECIALS))], axis=1),
        "exponent_gap": f64(gap),
    }
    # random mantissas in each of atan's ranges of |y / x|, every quadrant, x over many binades
    for name, lo, hi in (("ratio_tiny", -200, -29), ("ratio_small", -29, -2), ("ratio_7_16_to_19_16", -2, 1),
                         ("ratio_19_16_to_39_16", 0, 2), ("ratio_large", 1, 66), ("ratio_huge", 66, 200)):
        x = _random(rng, -100, 100, n)
        r = _random(rng, lo, hi, n)
        out[name] = np.stack([r * np.abs(x), x], axis=1)
    ang = rng.uniform(-np.pi, np.pi, n)
    out["unit_circle"] = np.stack([np.sin(ang), np.cos(ang)], axis=1)
    return out


# ---- the root division ----------------------------------------------------------------------------
# the pair a CPU model of div_a64 (ra = RN(1 / a)) turns into NaN where n / a is the largest finite
MODEL_PAIR = (float.fromhex("0x1.d528932de7769p+1021"), float.fromhex("0x1.d528932de776ap-3"))


@functools.lru_cache(maxsize=None)
def div_a_values():
    """Divisors: the ends of recip_a64's range [2^-64, 2^64] with neighbours on both sides, powers of
    two, all-ones and one-bit mantissas, random mantissas; and divisors outside the range."""
    rng = np.random.default_rng(0xD1FA64)
    p2 = 2.0 ** np.arange(-64, 65, 8, dtype=D)
    one_bit = np.concatenate([(1 + 2.0 ** -np.arange(1, 53, dtype=D)) * s for s in (1.0, 2.0 ** -63, 2.0 ** 63, 2.0 ** -3)])
    inside = np.concatenate([around(D(2.0 ** -64), 2)[2:], around(D(2.0 ** 64), 2)[:3], p2, step(p2[:-1] * 2, -1), one_bit,
                             _random(rng, -64, 64, 256, signs=False), [MODEL_PAIR[1]]])
    outside = np.concatenate([around(D(2.0 ** -64), 2)[:2], around(D(2.0 ** 64), 2)[3:],
                              f64([2.0 ** -65, 2.0 ** 65, 2.0 ** -100, 2.0 ** 200, 2.0 ** -1000, 0.0, -0.0, DENORM_MIN,
                                   DENORM_MAX, INF, NAN, -1.0, -2.0 ** -64])])
    return f64(inside), f64(outside)


def _pairs(n, a):
    n, a = np.broadcast_arrays(f64(n), f64(a))
    return np.stack([n.ravel(), a.ravel()], axis=1)


@functools.lru_cache(maxsize=None)
def div_a_cases():
    """Rows (n, a), classed by where the quotient falls."""
    rng = np.random.default_rng(0xD1FB64)
    inside, outside = div_a_values()
    a_all = np.concatenate([inside, outside])
    k5 = np.arange(-4, 5)
    with np.errstate(all="ignore"):
        # quotient within a few ulps of 0.001: n = fl(q a) and its neighbours, q around 0.001
        q = step(TMIN, k5)
        near_tmin = np.concatenate([_pairs(step(q[:, None] * a_all[None, :], k), a_all[None, :]) for k in (-2, -1, 0, 1, 2)])
        # within a few ulps of the largest finite (a <= 1: n = fl(q a) is finite), and overflowing
        a_le1 = np.concatenate([inside[inside <= 1], _random(rng, -64, 0, 4096, signs=False)])
        q = step(MAX, -np.arange(0, 5))
        near_max = np.concatenate([_pairs(step(q[:, None] * a_le1[None, :], k), a_le1[None, :]) for k in (-2, -1, 0, 1, 2)])
        a_lt1 = a_le1[a_le1 < 1]
        overflow = np.concatenate([_pairs(step(MAX * a_lt1, k), a_lt1) for k in (3, 8, 1 << 20)] +
                                  [_pairs(MAX, a_lt1), _pairs(-MAX, a_lt1)])
        # random divisors, quotients at the largest finite: where n * ra may overflow
        a_r = _random(rng, -64, 0, 400_000, signs=False)
        near_max_random = _pairs(step(MAX, -rng.integers(0, 3, a_r.size)) * a_r, a_r)
        # subnormal quotients (no decision reads them), and subnormal numerators
        qs = np.concatenate([from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64)), f64([DENORM_MIN, DENORM_MAX, 2.0 ** -1023])])
        a_ge1 = inside[inside >= 1]
        sub_q = np.concatenate([_pairs(qs[:, None] * a_ge1[None, :], a_ge1[None, :]),
                                _pairs(_random(rng, -1022, -1000, 20_000), _random(rng, 20, 64, 20_000, signs=False))])
        sub_n = _pairs(np.concatenate([qs, -qs])[:, None], a_all[None, :])
        special = _pairs(f64([0.0, -0.0, INF, -INF, NAN])[:, None], a_all[None, :])
        a_r2 = np.concatenate([_random(rng, -64, 64, 450_000, signs=False), _random(rng, -200, 200, 50_000, signs=False)])
        random = _pairs(_random(rng, -300, 300, a_r2.size), a_r2)
        # what a sphere test divides: h -+ sqrt(disc) of order 1..1e3 over a of order 1e-2..1e2
        scene = _pairs(rng.normal(size=200_000) * 10.0 ** rng.uniform(-4, 3, 200_000), 10.0 ** rng.uniform(-3, 3, 200_000))
    return {"model_pair": f64([MODEL_PAIR]), "near_tmin": near_tmin, "near_max": near_max, "overflow": overflow,
            "near_max_random": near_max_random, "subnormal_quotient": sub_q, "subnormal_numerator": sub_n,
            "special": special, "random": random, "scene": scene}


# ---- image sizes of the texel cases ------------------------------------------------------------------
def earth_size():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h, w, _ = np.load(os.path.join(root, "rustraytrace_amd", "assets", "earthmap_rgb8.npz"))["rgb8"].shape
    return int(w), int(h)


def texel_sizes():
    return ((1, 1), (2, 1), (3, 2), (7, 5), earth_size(), (4096, 2048), (1 << 20, 1 << 20), ((1 << 20) + 1, 3))


def _edge_ks(n):
    """Edge indices near 0, n / 2 and n."""
    return sorted({k for k in (0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1, n) if 0 <= k <= n})


# ---- x / (2 pi), x / pi ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def div_const_cases():
    rng = np.random.default_rng(0xD1C064)
    edges = []
    for w, h in texel_sizes():
        kw = np.unique(np.concatenate([_edge_ks(w), rng.integers(0, w + 1, 512)])).astype(D)
        kh = np.unique(np.concatenate([_edge_ks(h), rng.integers(0, h + 1, 512)])).astype(D)
        edges += [TWO_PI * kw / w, PI * kh / h]
    edges = np.concatenate(edges)
    edges = edges[(edges >= 2.0 ** -60) & (edges < 8)]
    k = np.arange(0, 257, dtype=D)
    return {
        "zero": f64([0.0]),
        "texel_edges": np.concatenate([step(edges, j) for j in range(-8, 9)]),
        # fl(atan2 + pi): multiples of ulp(pi) / 2 above 0, and the doubles below fl(2 pi)
        "phi_ends": np.concatenate([k[1:] * 2.0 ** -52, step(TWO_PI, -k.astype(np.int64)), PI - k * 2.0 ** -52]),
        "domain_ends": f64([2.0 ** -60, step(D(2.0 ** -60), 1), step(D(8), -1)]),
        "random": np.concatenate([_random(rng, -60, 3, 400_000, signs=False), rng.uniform(0, 8, 400_000)]),
        # outside the stated domain: only the in-kernel IEEE quotient is compared
        "outside": np.concatenate([SPECIALS[1:], f64([8.0, 1e300, -1.0, step(D(2.0 ** -60), -1), 2.0 ** -1000])]),
    }


def div_const_domain(x):
    """The stated domain: +0 (an angle is never -0, whose Markstein quotient would be +0) and [2^-60, 8)."""
    return ((x == 0) & ~np.signbit(x)) | ((x >= 2.0 ** -60) & (x < 8))


# ---- sqrt64 -----------------------------------------------------------------------------------------
SMALL = D(2.0 ** -767)


def sqrt_small(x):
    """rrt_books64.hip sqrt64_small: the lanes that send their whole wave to the library root (nonzero
    x below 2^-767, negatives among them; a NaN is not one)."""
    with np.errstate(invalid="ignore"):
        return (x < SMALL) & (x != 0)


def _nearly_square(rng, n):
    q = rng.integers(1 << 25, 1 << 26, n).astype(D)
    sq = step(q * q, rng.integers(-3, 4, n))
    return sq * 4.0 ** rng.integers(-380, 480, n).astype(D)  # even exponent shifts: within [2^-710, 2^1012)


@functools.lru_cache(maxsize=None)
def sqrt_cases():
    """Whole waves of 64 rows (every class is a multiple of 64 rows, so row i is lane i % 64)."""
    rng = np.random.default_rng(0x5A2764)
    W = 1024

    def big(n):
        x = np.concatenate([_random(rng, -767, 1024, n // 2, signs=False), _nearly_square(rng, n - n // 2)])
        return rng.permutation(x)

    def small(n):
        return np.concatenate([_random(rng, -1022, -767, n - n // 4, signs=False),
                               from_bits(rng.integers(1, 1 << 52, n // 4, dtype=np.uint64))])

    special_big = f64([0.0, -0.0, INF, NAN, SMALL, step(SMALL, 1), MAX])
    special_small = f64([step(SMALL, -1), DENORM_MIN, DENORM_MAX, -1.0, -INF, -DENORM_MIN, -2.0 ** -800, -MAX])
    out = {"no_small_lane": big(W * 64).reshape(W, 64)}
    sp = big(64 * 64).reshape(64, 64)
    sp[:, : len(special_big)] = special_big
    out["no_small_lane_special"] = sp
    for name, lane in (("one_small_first", 0), ("one_small_middle", 31), ("one_small_last", 63)):
        w = big(W * 64).reshape(W, 64)
        w[:, lane] = small(W)
        w[: len(special_small), lane] = special_small
        w[: len(special_big), (lane + 1) % 64] = special_big
        out[name] = w
    a = rng.permutation(small(W * 64)).reshape(W, 64)
    a[0, : len(special_small)] = special_small
    out["all_small"] = a
    return {k: v.reshape(-1) for k, v in out.items()}


# ---- as_i32 -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def as_i32_cases():
    rng = np.random.default_rng(0xA5132)
    ends = np.concatenate([around(D(v), 3) for v in (2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0, 1.0, -1.0,
                                                     0.5, 4294967296.0, 1048576.0)])
    return {"special": np.concatenate([SPECIALS, f64([1e300, -1e300])]), "ends": ends,
            "random": np.concatenate([rng.uniform(-2.0 ** 33, 2.0 ** 33, 4096), rng.uniform(-4, 4, 4096),
                                      rng.uniform(0, 1, 4096) * 2.0 ** rng.integers(0, 21, 4096)])}


# ---- attenuation records ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def att_cases():
    """Rows (word, bytes): a u32 attenuation word and a packed texel r | g << 8 | b << 16 (or 0x1000000)."""
    rng = np.random.default_rng(0xA7764)
    tags = np.arange(TEXEL_TAG - 1, TEXEL_TAG + 257, dtype=np.uint64)
    f32_bits = lambda v: np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = np.arange(256, dtype=np.uint64)
    every_byte = np.concatenate([b | ((b * 7 + 3) % 256) << 8 | (255 - b) << 16, (255 - b) | b << 8 | ((b * 11 + 5) % 256) << 16,
                                 ((b * 13 + 1) % 256) | (255 - b) << 8 | b << 16])

    def pack(words, by=None):
        words = np.asarray(words, np.uint64)
        by = every_byte[np.arange(len(words)) % len(every_byte)] if by is None else np.asarray(by, np.uint64)
        return np.stack([words.astype(D), by.astype(D)], axis=1)

    return {
        "tags": pack(tags),
        "signed_tags": pack(tags | 0x80000000),               # a negative NaN is no tag
        "quiet_nan": pack([0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0x7F800000, 0xFF800000]),
        "negative_albedo": pack(f32_bits([-0.0, -0.5, -1.0, -3.4e38, -1e-45, 0.0, 0.5, 1.0, 0.05, 0.95])),
        "random_words": pack(rng.integers(0, 1 << 32, 8192, dtype=np.uint64)),
        "every_byte": pack(f32_bits(rng.uniform(0, 1, len(every_byte))), every_byte),
        "no_data": pack([0x3F000000, TEXEL_TAG], [0x1000000, 0x1000000]),
        "byte_ends": pack([0, 0x3F800000, TEXEL_TAG + 255], [0, 0xFFFFFF, 0xFF00FF]),
    }


# ---- vectors ------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def vec_cases():
    """Rows (v, n, e, cosine, r0); v is also the attenuation of the Russian-roulette probability."""
    rng = np.random.default_rng(0x7EC364)

    def r0_of(ri):
        q = (1 - ri) / (1 + ri)
        return q * q

    def pack(v, n, e=None, cosine=None, r0=None):
        v, n = f64(v).reshape(-1, 3), f64(n).reshape(-1, 3)
        m = len(v)
        e = rng.choice(f64([1 / 1.5, 1.5, 1.0]), m) if e is None else np.broadcast_to(f64(e), m)
        cosine = rng.uniform(0, 1, m) if cosine is None else np.broadcast_to(f64(cosine), m)
        r0 = r0_of(e) if r0 is None else np.broadcast_to(f64(r0), m)
        return np.concatenate([v, n, e[:, None], cosine[:, None], r0[:, None]], axis=1)

    N = 4096
    u, nn = _unit(rng, N), _unit(rng, N)
    scale = 10.0 ** rng.uniform(-3, 3, (N, 1))
    axes = f64([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])
    perp_v = f64([axes[i] for i in range(6) for j in range(6) if i % 3 != j % 3])
    perp_n = f64([axes[j] for i in range(6) for j in range(6) if i % 3 != j % 3])
    # total internal reflection: e = 1.5, uv at angle t to n = z; sin t at and beside 1 / 1.5, where
    # 1 - |perp|^2 changes sign (refract is still evaluated: the material decides before calling it)
    st = np.concatenate([around(D(1 / 1.5), 40), f64([0.9, 0.99, 1.0]), around(D(0.6), 8)])
    tir_v = np.stack([st, 0 * st, -np.sqrt(np.abs(1 - st * st))], axis=1)
    # grazing: e = 1, n = z perpendicular to uv = (a, b, 0): perp = uv and k = |1 - (a a + b b)|
    b = around(D(0.8), 40)
    graze = np.stack([np.full_like(b, 0.6), b, 0 * b], axis=1)
    alb = f64([[NAN, 0.5, 0.2], [0.5, NAN, 0.2], [0.2, 0.5, NAN], [NAN, NAN, NAN], [-1, -2, -3], [-0.0, -0.0, -0.0],
               [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [0.05, 0.01, 0.0], [0.95, 0.1, 0.1], [1, 1, 1], [0.04, 0.05, 0.03],
               [step(D(0.05), -1), 0, 0], [step(D(0.05), 1), 0, 0], [0, step(D(0.95), 1), 0], [0, 0, step(D(0.95), -1)],
               [INF, 0, 0], [-INF, -INF, -INF], [NAN, 2.0, 0.3], [0.3, NAN, 2.0], [-0.0, NAN, -1.0], [1e-320, 0, 0]])
    zero = f64([[0, 0, 0]])
    return {
        "random_unit": pack(u, nn),
        "random_nonunit": pack(u * scale, nn * scale[::-1]),
        "parallel": pack(np.concatenate([nn[:64], -nn[:64]]), np.concatenate([nn[:64], nn[:64]])),
        "perpendicular": pack(perp_v, perp_n),
        "total_internal_reflection": pack(tir_v, [[0, 0, 1]] * len(tir_v), e=1.5),
        "grazing": pack(graze, [[0, 0, 1]] * len(graze), e=1.0),
        "cosine_0_1": pack(u[:64], nn[:64], cosine=np.tile(f64([0.0, 1.0]), 32)),
        "cosine_ends": pack(u[:8], nn[:8], cosine=f64([1.0, step(D(1), -1), step(D(1), 1), 0.0, -0.0, -1.0, 2.0, NAN])),
        "albedo": pack(alb, nn[: len(alb)]),
        "lengths": pack(np.concatenate([zero, f64([[1e-200, 0, 0], [1e200, 1e200, 0], [1e-160, 1e-160, 1e-160],
                                                   [DENORM_MIN, 0, 0], [INF, 0, 0], [NAN, 1, 1], [2.0 ** 600, 0, 0]])]),
                        nn[:8]),
    }


# ---- spheres ------------------------------------------------------------------------------------------
def f32r(x):
    """x rounded to f32, as f64 (sphere centers and radii are f32 records)."""
    return f64(np.ascontiguousarray(x, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def sphere_cases():
    """Rows (o, d, c, r, closest); c and r are f32-representable."""
    rng = np.random.default_rng(0x5FE264)

    def row(o, d, c, r, closest=np.inf):
        return [*o, *d, *c, r, closest]

    out = {}
    # the ray down -z from (x, 0, 0) passes at distance 1 - x from (1, 0, -1): with r = 1, h = 1,
    # c = 1 + (1 - x)^2 - 1, disc = 1 - (1 - x)^2: x scanned around 0 in f64 steps either side of disc = 0
    xs = np.concatenate([np.arange(-64, 65) * 2.0 ** -52, around(D(0), 8), f64([2.0 ** -30, -2.0 ** -30, 2.0 ** -27, -2.0 ** -27])])
    out["tangent"] = [row((x, 0, 0), (0, 0, -1), (1, 0, -1), 1) for x in xs]
    out["inside"] = [row((0, 0, -4), (0, 0, -1), (0, 0, -4), 1), row((0.1, 0.2, -3.7), (1, 2, 3), (0, 0, -4), 1),
                     row((0, 0, -4), (0, 1, 0), (0, 0, -4), 1000), row((0.5, 0.25, -4.125), (-3, 0.5, 0.25), (0, 0, -4), 1)]
    # the near root within ulps of 0.001: the sphere's front at z = -(cz - 1), the origin moved in f64
    # steps about cz - 1 - 0.001; and the origin on the surface (near root about 0: the far root answers)
    oz = around(D(-3 + 0.001), 24)
    out["near_tmin"] = [row((0, 0, z), (0, 0, -1), (0, 0, -4), 1) for z in oz]
    out["near_tmin"] += [row((0, 0, z), (0, 0, -2), (0, 0, -4), 1) for z in around(D(-3 + 0.002), 24)]
    out["near_tmin"] += [row((0, 0, z), (0, 0, -1), (0, 0, -4), 1) for z in around(D(-3), 4)]
    out["near_tmin"] += [row((0, 0, -3), (0, 0, 1), (0, 0, -4), 1)]
    # d = (0, 0, -s): h = 2 s, sqrt(disc) = s, a = s s, so the near root is fl(s / fl(s s)), within an ulp
    # or two of 1 / s: s stepped about 1000 puts it on either side of 0.001, an ulp at a time
    out["near_tmin"] += [row((0, 0, 0), (0, 0, -s), (0, 0, -2), 1) for s in around(D(1000), 24)]
    # root = 3 exactly: `closest` equal to it rejects (strictly less must win), one double above accepts
    three = D(3)
    out["closest_equal"] = [row((0, 0, 0), (0, 0, -1), (0, 0, -4), 1, c)
                            for c in (three, step(three, 1), step(three, -1), D(5), step(D(5), 1), step(D(5), -1), TMIN, 0.0, NAN)]
    # disc below 2^-767: short rays (a, h tiny) so that h h - a c is tiny but positive; one lane of the
    # wave then takes the library root, and the whole wave with it
    out["tiny_disc"] = [row((0, 0, 0), (0, 0, -s), (0, 0, -4), 1) for s in 2.0 ** -np.arange(380.0, 400.0)]
    out["tiny_disc"] += [row((0, 0, 0), (0, 0, -s), (0, 0, -4), 1) for s in 2.0 ** -np.arange(500.0, 520.0, 4)]
    # |d|^2 = s^2 at the ends of the per-ray reciprocal's range [2^-64, 2^64], and far outside it
    out["a_range"] = [row((0, 0, 0), (s, 0, 0), (5, 0, 0), 1) for s in around(D(2.0 ** -32), 3)]
    out["a_range"] += [row((0, 0, 0), (0, -s, 0), (0, -5e8, 0), 1e8) for s in around(D(2.0 ** 32), 3)]
    out["a_range"] += [row((0, 0, 0), (0, 0, -s), (0, 0, -4), 1) for s in (2.0 ** -40, 2.0 ** 40, 2.0 ** -300, 2.0 ** 300, 2.0 ** -520)]
    out["d_zero"] = [row((0, 0, 0), (0, 0, 0), (0, 0, -4), 1), row((0, 0, -4), (0, 0, 0), (0, 0, -4), 1),
                     row((0, 0, 0), (NAN, 0, -1), (0, 0, -4), 1), row((0, 0, 0), (0, 0, -INF), (0, 0, -4), 1)]
    # radii across the f32 range, subnormals included (sqrt(r r) must be r again), from the centre and
    # from outside; r <= 0 is stored as 0
    radii = np.concatenate([2.0 ** np.arange(-149.0, 128.0, 3), f32r(rng.uniform(1, 2, 64) * 2.0 ** rng.integers(-149, 127, 64)),
                            f64([np.float32(3.4028235e38), 2.0 ** -126, 2.0 ** -127 + 2.0 ** -149, 0.0, -0.0, -1.0])])
    out["radius"] = [row((0, 0, 0), (0, 0, -1), (0, 0, 0), r) for r in radii]
    out["radius"] += [row((0, 0, 0), (0, 0, -1), (0, 0, -float(np.float32(4 * r)) if 0 < r < 1e30 else -4.0), r) for r in radii]
    N = 8192
    c = f32r(rng.uniform(-10, 10, (N, 3)))
    r = f32r(rng.uniform(0.05, 3, (N, 1)))
    o = rng.uniform(-10, 10, (N, 3))
    d = (c + rng.normal(size=(N, 3)) * r - o) * 10.0 ** rng.uniform(-2, 2, (N, 1))
    closest = rng.choice([np.inf, 0.5, 1.0, 2.0], (N, 1))
    out["random"] = np.concatenate([o, d, c, r, closest], axis=1)
    # scattered rays: the origin on a sphere's surface (a hit point), the direction outward or inward
    n = _unit(rng, N)
    c2 = f32r(rng.uniform(-5, 5, (N, 3)))
    r2 = f32r(rng.uniform(0.2, 2, (N, 1)))
    out["from_surface"] = np.concatenate([c2 + n * r2, _unit(rng, N), c2, r2, np.full((N, 1), np.inf)], axis=1)
    return {k: f64(v) for k, v in out.items()}


# ---- texels -------------------------------------------------------------------------------------------
ULP_MOVES = (0, 1, -1, 2, -2, 1 << 10, -(1 << 10), 1 << 20, -(1 << 20), 1 << 30, -(1 << 30), 1 << 40, -(1 << 40))
K_ATAN32_ERR, K_ACOS32_ERR, K_LIBM64_ERR = 2.0 ** -21, 2.0 ** -20, 2.0 ** -40  # rrt_books64.hip


def _direction(theta, phi):
    """The outward normal whose get_sphere_uv angles are (theta, phi): theta = acos(-y), phi = atan2(-z, x) + pi."""
    theta, phi = np.broadcast_arrays(f64(theta), f64(phi))
    s = np.sin(theta)
    return np.stack([s * np.cos(phi - np.pi), -np.cos(theta), -s * np.sin(phi - np.pi)], axis=-1)


@functools.lru_cache(maxsize=None)
def texel_cases():
    """Rows (outward, w, h)."""
    rng = np.random.default_rng(0x7E8E164)
    moves = np.array(ULP_MOVES, np.int64)
    scales = f64([1.0, 0.5, 0.75, 2.0 ** -30, 2.0 ** 30])
    out = {k: [] for k in ("column_edges", "row_edges", "poles", "component_ends", "random")}
    one = D(1)
    pole_y = f64([1, step(one, -1), 1 - 2.0 ** -24, 1 - 2.0 ** -25, 1 + 2.0 ** -52, 1 - 2.0 ** -23, 1 - 2.0 ** -22])
    pole_y = np.concatenate([pole_y, -pole_y])
    pole_xz = f64([[0.0, 0.0], [0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0], [1e-9, 0.0], [0.0, 1e-9], [-1e-9, -0.0], [2.0 ** -13, 2.0 ** -13],
                   [-2.0 ** -13, 2.0 ** -12], [1e-200, -1e-200], [2.0 ** -12, -0.0]])
    ends = f64([0.0, -0.0, 2.0 ** -61, -2.0 ** -61, step(D(2.0 ** -60), -1), 2.0 ** -60, 2.0 ** 60, step(D(2.0 ** 60), 1), 2.0 ** 61, -2.0 ** 61,
                DENORM_MIN, 1e300, NAN, INF, -INF])
    for w, h in texel_sizes():
        size = np.array([w, h], D)

        def add(name, v):
            v = f64(v).reshape(-1, 3)
            out[name].append(np.concatenate([v, np.broadcast_to(size, (len(v), 2))], axis=1))

        # column edges phi = 2 pi k / w at a few latitudes, scaled, one of x / z moved
        phi = TWO_PI * f64(_edge_ks(w)) / w
        theta = f64([0.3, 1.0, np.pi / 2, 2.5])
        base = _direction(theta[:, None], phi[None, :]).reshape(-1, 3)
        base = (base[:, None, :] * scales[None, :, None]).reshape(-1, 3)
        for comp in (0, 2):
            v = np.repeat(base[:, None, :], len(moves), axis=1)
            v[:, :, comp] = step(v[:, :, comp], moves[None, :])
            add("column_edges", v)
        # row edges theta = pi (1 - k / h) at a few longitudes (scaling y would leave the edge), y moved
        theta = PI * (1 - f64(_edge_ks(h)) / h)
        phi = f64([0.1, 1.0, 2.0, 3.0, 4.5, 6.0])
        base = _direction(theta[:, None], phi[None, :]).reshape(-1, 3)
        v = np.repeat(base[:, None, :], len(moves), axis=1)
        v[:, :, 1] = step(v[:, :, 1], moves[None, :])
        add("row_edges", v)
        add("row_edges", v * f64([2.0 ** -30, 1, 2.0 ** 30]))  # x and z scaled alone: the same row
        # the poles, every sign pair of zero x and z, and a few tiny ones
        add("poles", [[x, y, z] for y in pole_y for x, z in pole_xz])
        # x and z each at the enclosure's domain ends (zero, below 2^-60, above 2^60, NaN, infinite)
        add("component_ends", [[e, 0.3, o] for e in ends for o in (0.5, -0.5, 2.0 ** -70, 0.0)])
        add("component_ends", [[o, -0.6, e] for e in ends for o in (0.5, -0.5, 2.0 ** 70, -0.0)])
        add("component_ends", [[0.5, e, 0.5] for e in ends])
        m = 6000
        u = _unit(rng, m)
        add("random", u)
        add("random", _unit(rng, m // 4) * rng.uniform(0.5, 1.0, (m // 4, 1)))
    return {k: np.concatenate(v) for k, v in out.items()}


def texel_marks(rows_):
    """For TEXEL64 rows, from the geometry in f64 (the texel coordinate s of the true angle):
    (col_must_fall_back, row_must_fall_back, col_must_be_decided, row_must_be_decided).

    must fall back: s lies within 2^-21 n 0.16 (columns; 0.32 for rows) of an integer (the image's
    edges 0 and n among them) — closer than any enclosure's half-width, so an enclosure that decided
    the texel would exclude the true angle. must be decided: the distance is above four times the
    enclosure's half-width (the kernel's e n 0.16 + 2^-30, e from its error bounds), the image is at
    most 2^20 wide, and the enclosure's domain holds: |x|, |z| in [2^-60, 2^60]; |y| < 1 - 2^-23."""
    r = f64(rows_).reshape(-1, 5)
    x, y, z, w, h = r.T
    with np.errstate(all="ignore"):
        s = (np.arctan2(-z, x) + np.pi) / (2 * np.pi) * w
        dc = np.abs(s - np.rint(s))
        col_fb = dc < 2.0 ** -21 * w * 0.16
        e = K_ATAN32_ERR + 2.0 ** -22 + K_LIBM64_ERR + 2.0 ** -48
        ax, az = np.abs(x), np.abs(z)
        dom = (np.minimum(ax, az) >= 2.0 ** -60) & (np.maximum(ax, az) <= 2.0 ** 60)
        col_dec = dom & (w <= 2.0 ** 20) & (dc > 4 * (e * w * 0.16 + 2.0 ** -30))
        t = (1 - np.arccos(-y) / np.pi) * h
        dr = np.abs(t - np.rint(t))
        row_fb = dr < 2.0 ** -21 * h * 0.32
        y32 = (-y).astype(np.float32)
        yd, yu = np.nextafter(y32, np.float32(-2)).astype(D), np.nextafter(y32, np.float32(2)).astype(D)
        dom = np.abs(y) < 1 - 2.0 ** -23
        e = 0.5 * (np.arccos(np.clip(yd, -1, 1)) - np.arccos(np.clip(yu, -1, 1))) + (K_ACOS32_ERR + K_LIBM64_ERR + 2.0 ** -49)
        row_dec = dom & (h <= 2.0 ** 20) & (dr > 4 * (e * h * 0.32 + 2.0 ** -30))
    return col_fb, row_fb, col_dec, row_dec
