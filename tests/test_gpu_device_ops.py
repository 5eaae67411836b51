"""The f32 kernel's numeric building blocks, run on the device on chosen arguments.

Whole-scene parity only sees the arguments the committed scenes produce. Here the kernel's own
__device__ functions (rrt_kernel.hip, through the test-only entries rrt_testing_device_ops and
rrt_testing_div_check) are applied elementwise to the inputs of tests/device_ops_cases.py — octant
seams, mantissa splits, lattice points, interval ends, the per-ray reciprocal's range ends — and
every result is compared bit for bit with the oracle's f32 twin (NaNs equal as a class, -0 != +0).
tests/test_device_ops_cases.py checks on the CPU that the inputs hold every named class and that
the twin is accurate against float64.
"""
import numpy as np
import pytest

import device_ops_cases as C
from oracle import oracle
from rustraytrace_amd import _lib

pytestmark = pytest.mark.gpu


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same(a, b):
    """Bit equality of two word arrays holding f32, NaNs equal as a class."""
    a, b = u32(a), u32(b)
    return (a == b) | (np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32)))


def assert_same(what, got, want, inputs):
    """got / want: (n,) or (n, k) 32-bit words; prints the first offending rows as hex bit patterns."""
    got, want = u32(got).reshape(len(inputs), -1), u32(want).reshape(len(inputs), -1)
    bad = np.flatnonzero(~same(got, want).all(axis=1))
    print(f"{what}: {len(inputs)} inputs compared, {len(bad)} differ")
    if len(bad):
        hx = lambda row: " ".join(f"{int(w):08x}" for w in np.atleast_1d(row))
        rows_in = u32(np.ascontiguousarray(inputs, dtype=np.float32)).reshape(len(inputs), -1)
        lines = [f"  in {hx(rows_in[i])} | device {hx(got[i])} | twin {hx(want[i])}" for i in bad[:8]]
        pytest.fail(f"{what}: {len(bad)} of {len(inputs)} results differ from the f32 twin\n" + "\n".join(lines))


def accepted(t_words):
    t = u32(t_words).view(np.float32)
    with np.errstate(invalid="ignore"):
        return (np.float32(0.001) < t) & (t < np.float32(np.inf))


@pytest.mark.parametrize("op,twin", [("SIN", oracle.sin_f32), ("COS", oracle.cos_f32)])
def test_sin_cos(op, twin):
    x = C.rows(C.sin_cos_cases())
    assert_same(op, _lib.device_ops(op, x), twin(x), x)


def test_log():
    x = C.rows(C.log_cases())
    assert_same("LOG", _lib.device_ops("LOG", x), oracle.log_f32(x), x)


def test_acos():
    x = C.rows(C.acos_cases())
    assert_same("ACOS", _lib.device_ops("ACOS", x), oracle.acos_f32(x), x)


def test_atan2():
    yx = C.rows(C.atan2_cases())
    assert_same("ATAN2", _lib.device_ops("ATAN2", yx), oracle.atan2_f32(yx), yx)


def test_div_a():
    """(r, r_fast, q, ra): q is numpy's float32 division (the in-kernel IEEE reference is IEEE); r
    and r_fast take the same accept / reject decision as q, and equal it when accepted or when
    the comment's domain holds (finite |n| >= 2^-103, normal finite q)."""
    na = C.rows(C.div_a_cases())
    out = _lib.device_ops("DIV_A", na)
    n, a = na[:, 0], na[:, 1]
    with np.errstate(all="ignore"):
        q = n / a
    assert_same("DIV_A q", out[:, 2], q, na)
    ra = out[:, 3].view(np.float32)
    in_range = (a >= np.float32(2.0 ** -64)) & (a <= np.float32(2.0 ** 64))
    assert np.array_equal(ra != 0, in_range), "refine_ra is nonzero exactly on [2^-64, 2^64]"
    with np.errstate(all="ignore"):
        claimed = in_range & np.isfinite(n) & (np.abs(n) >= np.float32(2.0 ** -103)) & np.isfinite(q) & \
                  (np.abs(q) >= np.float32(2.0 ** -126))
    for col, name in ((0, "div_by_a<false>"), (1, "div_by_a<true>")):
        r = out[:, col]
        assert np.array_equal(accepted(r), accepted(q)), f"{name}: accept / reject differs from the IEEE quotient's"
        must = claimed | accepted(q) | ~in_range
        assert_same(f"DIV_A {name}", r[must], u32(q)[must], na[must])


def test_div_const():
    x = C.rows(C.div_const_cases())
    out = _lib.device_ops("DIV_CONST", x)
    for col, c in ((0, C.TWO_PI), (2, C.PI)):
        want = x / np.float32(c)
        assert_same(f"DIV_CONST ieee x / {c}", out[:, col + 1], want, x)
        domain = (x == 0) | ((x >= np.float32(2.0 ** -100)) & (x <= 8))
        assert_same(f"DIV_CONST div_by_const(x, {c})", out[domain, col], want[domain], x[domain])


def test_floor_i32():
    x = C.rows(C.floor_i32_cases())
    assert_same("FLOOR_I32", _lib.device_ops("FLOOR_I32", x), oracle.floor_i32(x), x)


def test_checker():
    rows = C.rows(C.checker_cases())
    _, _, even = oracle.book2_textures(C.perlin_table(), rows[:, 1:], inv_scale=float(C.CHECKER_INV_SCALE))
    assert_same("CHECKER", _lib.device_ops("CHECKER", rows), even.astype(np.uint32), rows)


@pytest.mark.parametrize("scale", C.PERLIN_SCALES)
def test_perlin(scale):
    p = C.rows(C.texture_points())
    out = _lib.device_ops("PERLIN", p, perlin=C.perlin_table(), scale=scale)
    noise, value, _ = oracle.book2_textures(C.perlin_table(), p, scale=float(np.float32(scale)))
    want = np.stack([noise.astype(np.float32), value.astype(np.float32)], axis=1)
    for k, variant in enumerate(("generic, unrolled", "generic, rolled", "LDS, unrolled", "LDS, rolled")):
        assert_same(f"PERLIN scale {scale} ({variant})", out[:, 2 * k:2 * k + 2], want, p)
        assert_same(f"PERLIN scale {scale} ({variant} against the first variant)", out[:, 2 * k:2 * k + 2], out[:, :2], p)


def test_vec():
    rows = C.rows(C.vec_cases())
    assert_same("VEC", _lib.device_ops("VEC", rows), oracle.vec_f32(rows), rows)


def test_quad():
    rows, quads = C.rows(C.quad_cases()), C.quad_records()
    out = _lib.device_ops("QUAD", rows, quads=quads)
    hit, t = oracle.quad_hit_f32(quads, rows)
    assert 0 < hit.sum() < len(hit)
    assert_same("QUAD", out, np.stack([hit, u32(t)], axis=1), rows)


def test_sphere():
    """Device words per record (book 1: r * r stored, then book 2: r): exact_root<false>,
    exact_root<true>, test_range's (hit, t) with the IEEE division and with the per-ray reciprocal;
    last sphere_root. An exact root is the twin's t when the twin hits over (0.001, inf), and is
    not accepted when it misses."""
    rows = C.rows(C.sphere_cases())
    out = _lib.device_ops("SPHERE", rows)
    hit, t = oracle.sphere_hit_f32(rows)
    assert 0 < hit[:, 0].sum() < len(rows) and 0 < hit[:, 2].sum() < hit[:, 0].sum()
    closest = u32(np.ascontiguousarray(rows[:, 10]))
    for b, book in enumerate(("book 1", "book 2")):
        w = out[:, 6 * b:6 * b + 6]
        h_inf, t_inf = hit[:, b] != 0, u32(np.ascontiguousarray(t[:, b]))
        h_c, t_c = hit[:, 2 + b], u32(np.ascontiguousarray(t[:, 2 + b]))
        for col, name in ((0, "exact_root<false>"), (1, "exact_root<true>")):
            assert np.array_equal(accepted(w[:, col]), h_inf), f"{book} {name}: acceptance differs from the twin's hit"
            assert_same(f"SPHERE {book} {name}", w[h_inf, col], t_inf[h_inf], rows[h_inf])
        want_t = np.where(h_c != 0, t_c, closest)  # a miss leaves `closest` as it was
        for col, name in ((2, "test_range, IEEE division"), (4, "test_range, per-ray reciprocal")):
            assert_same(f"SPHERE {book} {name}", w[:, col:col + 2], np.stack([h_c, want_t], axis=1), rows)
    assert_same("SPHERE sphere_root", out[:, 12], hit[:, 4], rows)


def test_div_check():
    """rrt_testing_div_check: every f32 numerator against each divisor of device_ops_cases.div_a_values."""
    a = C.div_a_values()
    out = _lib.div_check(a)
    print("rrt_testing_div_check:", " ".join(f"out[{i}]={v}" for i, v in enumerate(out)))
    assert out[6] == len(a) << 32
    assert out[7] == (0x41000000 - 0x0D800000 + 1) + 1
    assert out[0] == 0, "div_by_a differs from the IEEE quotient on a normal quotient"
    assert out[1] == 0, "div_by_a changes an accept / reject decision or an accepted root"
    assert out[2] == 0, "div_by_a<false> differs from n / a outside the reciprocal's range"
    # div_by_a's comment claims the IEEE quotient for every n, subnormal quotients included (its guard
    # sends them to the IEEE division), so this counter is pinned too
    assert out[3] == 0, "div_by_a differs from n / a on a subnormal or zero quotient"
    assert out[4] == 0 and out[5] == 0, "div_by_const differs from x / c on its proved domain"


@pytest.mark.parametrize("n", sorted(C.LIGHT_LISTS))
def test_lights_pdf(n):
    """lights_pdf over a list of n lights (1 / n inexact for 3, 5, 7): origins on, inside, just outside and
    far from the light spheres and on the quads' planes; directions through the quads' interiors, edges and
    corners, parallel to them, tangent to the spheres, away, and with zero, infinite and NaN components."""
    rows, lights = C.rows(C.lights_pdf_cases(n)), C.light_records(n)
    assert_same(f"LIGHTS_PDF n={n}", _lib.device_ops("LIGHTS_PDF", rows, lights=lights), oracle.lights_pdf_f32(lights, rows), rows)


@pytest.mark.parametrize("n", sorted(C.LIGHT_LISTS))
def test_lights_random(n):
    """lights_random from the start of a path's stream: keys that draw every index of the list, and keys
    whose first draw is the largest rnd returns. Direction and the number of draws taken."""
    rows, lights = C.rows(C.lights_random_cases(n)), C.light_records(n)
    d, draws = oracle.lights_random_f32(lights, rows)
    out = _lib.device_ops("LIGHTS_RANDOM", rows, lights=lights)
    assert_same(f"LIGHTS_RANDOM n={n}", out, np.concatenate([u32(d), draws[:, None]], axis=1), rows)
