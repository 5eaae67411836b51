"""GPU: the root code's cold arms in mixed waves, pointwise through rrt_testing_device_ops.

div_by_a and sqrt_rn each take one ballot over the wave and branch on it: the straight-line code when
no lane is outside the fast path's domain, else a generic arm in which the lanes outside it get the
IEEE quotient (the library square root) and the others must keep what the straight-line code gives.
No committed scene puts such a lane into a wave, and tests/test_gpu_device_ops.py's rows hold their
special classes in runs, so whole waves of them. Here row i is lane i % 64 of a wave (the op's kernel
maps row to thread), and every wave of 64 rows holds a handful of special rows at scattered lanes among
ordinary ones. The SPHERE op runs test_range over a one-record range held in private memory: it
reaches div_by_a, sqrt_rn and the select accept, not the loop's stepping over a staged range
(tests/test_gpu_leaf_ranges.py renders those).

  DIV_A   first quotients in [2^-30, inf) next to n = +-0, denormal n, |n| below 2^-102, n at the
          quotient's overflow bound, and divisors outside [2^-64, 2^64] (ra = 0); also inf and NaN
  SPHERE  ordinary discriminants next to disc = 0 and nonzero disc below 2^-96 (and just above it),
          and next to the special rays of device_ops_cases.sphere_cases (origin on the surface: a zero
          first quotient; |d|^2 outside the reciprocal's range; roots beyond the largest float)

Expected values are computed on the host in f32: numpy's IEEE quotient, the oracle's f32 sphere test,
and for the constructed tangent rays the root worked out below. The CPU tests check the rows.
"""
from fractions import Fraction

import numpy as np
import pytest

import device_ops_cases as C
from oracle import oracle
from rustraytrace_amd import _lib

from test_gpu_device_ops import accepted, assert_same, u32

F = np.float32
SPECIAL_LANES = (0, 5, 17, 31, 32, 40, 62, 63)  # lanes of a wave that hold special rows


def mixed(ordinary, special):
    """Rows in waves of 64: the special rows, cycled, at SPECIAL_LANES of every wave, ordinary rows in
    the other lanes. Returns (rows, is_special)."""
    per = 64 - len(SPECIAL_LANES)
    n_waves = max(len(ordinary) // per, -(-len(special) // len(SPECIAL_LANES)))
    assert len(ordinary) >= per
    rows = np.empty((n_waves * 64, ordinary.shape[1]), np.float32)
    is_special = np.zeros(n_waves * 64, bool)
    lanes = np.arange(n_waves * 64) % 64
    is_special[np.isin(lanes, SPECIAL_LANES)] = True
    rows[is_special] = special[np.arange(is_special.sum()) % len(special)]
    rows[~is_special] = ordinary[np.arange((~is_special).sum()) % len(ordinary)]
    return rows, is_special


# ---- the root division ------------------------------------------------------------------------------
def div_rows():
    """(rows (n, a), is_special, class of each special row)."""
    rng = np.random.default_rng(0x1EAF)
    a_ord = C.from_bits((rng.integers(127 - 20, 127 + 20, 3000, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, 3000, dtype=np.uint32))
    q = C.from_bits((rng.integers(127 - 9, 127 + 20, 3000, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, 3000, dtype=np.uint32))
    ordinary = np.stack([q * a_ord * np.where(rng.random(3000) < 0.5, F(-1), F(1)), a_ord], axis=1).astype(np.float32)
    a_in = C.f32([1.0, 3.0, 2.0 ** -64, 2.0 ** 64, 0.7, 1e-6, 5e8])
    big = F(3.4028235e38)
    special, cls = [], []
    for a in a_in:
        for name, ns in (("zero", C.f32([0.0, -0.0])), ("denormal", C.f32([C.DENORM_MIN, -C.DENORM_MAX])),
                         ("tiny", C.f32([2.0 ** -104, -(2.0 ** -110), 1.5 * 2.0 ** -103])),
                         ("inf_nan", C.f32([np.inf, -np.inf, np.nan]))):
            special += [(n, a) for n in ns]
            cls += [name] * len(ns)
        with np.errstate(over="ignore"):
            top = C.around(big * a, 3)
        top = top[np.isfinite(top)]
        special += [(n, a) for n in top]
        cls += ["overflow"] * len(top)
    for a in C.f32([2.0 ** -70, 2.0 ** 80, 0.0, C.DENORM_MAX, np.inf, C.step(F(2.0 ** -64), -1), C.step(F(2.0 ** 64), 1)]):
        ns = C.f32([1.0, -3.5, 2.0 ** -60, 1e30, 0.0])
        special += [(n, a) for n in ns]
        cls += ["ra_zero"] * len(ns)
    rows, is_special = mixed(ordinary, C.f32(special))
    k = is_special.sum()
    return rows, is_special, np.array(cls)[np.arange(k) % len(cls)]


def test_div_rows_hold_the_classes():
    rows, is_special, cls = div_rows()
    assert len(rows) % 64 == 0 and 2000 <= len(rows) <= 8000
    n, a = rows[:, 0], rows[:, 1]
    with np.errstate(all="ignore"):
        in_range = (a >= F(2.0 ** -64)) & (a <= F(2.0 ** 64))
        q = n / a
        fast = in_range & (np.abs(q) >= F(2.0 ** -29)) & (np.abs(q) < F(2.0 ** 126))  # first quotient well inside [2^-30, inf)
    assert fast[~is_special].all(), "ordinary rows take the straight-line quotient"
    assert not fast[is_special][cls != "overflow"].any()
    sp = rows[is_special]
    assert set(cls) == {"zero", "denormal", "tiny", "inf_nan", "overflow", "ra_zero"}
    assert (sp[cls == "zero", 0] == 0).all() and (np.abs(sp[cls == "tiny", 0]) < F(2.0 ** -102)).all()
    assert (np.abs(sp[cls == "denormal", 0]) < F(2.0 ** -126)).all()
    with np.errstate(all="ignore"):
        qo = sp[cls == "overflow", 0] / sp[cls == "overflow", 1]
    assert np.isinf(qo).any() and (qo == F(3.4028235e38)).any(), "quotients at and past the largest float"
    assert not ((sp[cls == "ra_zero", 1] >= F(2.0 ** -64)) & (sp[cls == "ra_zero", 1] <= F(2.0 ** 64))).any()
    for w in range(len(rows) // 64):  # every wave is mixed
        s = is_special[64 * w:64 * w + 64]
        assert s.sum() == len(SPECIAL_LANES) and fast[64 * w:64 * w + 64][~s].all()


@pytest.mark.gpu
def test_div_by_a_in_mixed_waves():
    """Every row's div_by_a is numpy's f32 quotient, bit for bit: the special lanes through the IEEE
    division of the generic arm, the ordinary lanes beside them through the four fmas."""
    rows, is_special, _ = div_rows()
    out = _lib.device_ops("DIV_A", rows)
    with np.errstate(all="ignore"):
        q = rows[:, 0] / rows[:, 1]
    assert_same("DIV_A in-kernel IEEE quotient", out[:, 2], q, rows)
    assert_same("DIV_A div_by_a, special lanes", out[is_special, 0], u32(q)[is_special], rows[is_special])
    assert_same("DIV_A div_by_a, ordinary lanes", out[~is_special, 0], u32(q)[~is_special], rows[~is_special])


# ---- the discriminant's square root -------------------------------------------------------------------
# A ray down -z from the origin with d = (0, 0, -2^-32) (a = 2^-64, the reciprocal's lower end) against a
# sphere of radius 0 at (0, 0, -4 (1 + k 2^-20)): h = 2^-30 (1 + k 2^-20), h^2 = 2^-60 (1 + k 2^-19 + k^2 2^-40)
# exactly (the fma keeps it), |oc|^2 rounds to 16 (1 + k 2^-19) for k < 256, so disc = k^2 2^-100 exactly:
# 0 at k = 0, below 2^-96 for 0 < k < 4... the square root is k 2^-50, h - sq = 2^-30, and the root
# 2^-30 / 2^-64 = 2^34 for every k.
TANGENT_K = (0, 1, 2, 3, 4, 5, 9, 15, 16, 17, 40, 200)
TANGENT_ROOT = F(2.0 ** 34)


def tangent_rows():
    return C.f32([[0, 0, 0, 0, 0, -(2.0 ** -32), 0, 0, -4.0 * (1.0 + k * 2.0 ** -20), 0.0, np.inf] for k in TANGENT_K])


def _exact_disc(row):
    """h^2 - RN(a c) in exact arithmetic from the f32 steps before it (dot's fma order, -ffp-contract=off).
    One value for both record forms: book 1's stored w and book 2's r * r are the same f32 product."""
    o, d, c, r = row[0:3], row[3:6], row[6:9], row[9]
    oc = (c - o).astype(np.float32)
    fma = lambda x, y, z: F(float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))))
    dot = lambda u, v: fma(u[2], v[2], fma(u[1], v[1], F(u[0] * v[0])))
    h, a = dot(d, oc), dot(d, d)
    w = F(r * r)
    cc = F(dot(oc, oc) - w)
    return Fraction(float(h)) ** 2 - Fraction(float(F(a * cc)))


def sphere_rows():
    sc = C.sphere_cases()
    special = np.concatenate([tangent_rows()] + [sc[k] for k in ("tangent", "inside", "on_surface", "a_range", "d_zero", "overflow")])
    rows, is_special = mixed(sc["random"][:2800], special)
    return rows, is_special, len(special)


def test_sphere_rows_hold_the_classes():
    t = tangent_rows()
    for k, row in zip(TANGENT_K, t):
        assert _exact_disc(row) == Fraction(k * k, 2 ** 100)
    discs = [Fraction(k * k, 2 ** 100) for k in TANGENT_K]
    assert discs[0] == 0 and sum(0 < x < Fraction(1, 2 ** 96) for x in discs) >= 3 and sum(x >= Fraction(1, 2 ** 96) for x in discs) >= 3
    hit, root = oracle.sphere_hit_f32(t)
    assert (hit[:, 0] != 0).all() and (root[:, 0] == TANGENT_ROOT).all(), "the f32 twin finds the worked-out root"
    rows, is_special, n_special = sphere_rows()
    assert len(rows) % 64 == 0 and 2000 <= len(rows) <= 8000
    assert is_special.sum() >= n_special, "every special row is placed"
    with np.errstate(all="ignore"):
        ordinary_disc = [_exact_disc(r) for r in rows[~is_special][:200]]
    assert all(x < 0 or x > Fraction(1, 2 ** 60) for x in ordinary_disc), "ordinary rows: sqrt_rn_big's domain"
    assert any(x > 0 for x in ordinary_disc)
    assert all(is_special[64 * w:64 * w + 64].sum() == len(SPECIAL_LANES) for w in range(len(rows) // 64))


@pytest.mark.gpu
def test_sphere_roots_in_mixed_waves():
    """tests/test_gpu_device_ops.py::test_sphere's comparisons on the mixed rows, and the tangent rays'
    root 2^34 from every discriminant class."""
    rows, is_special, _ = sphere_rows()
    out = _lib.device_ops("SPHERE", rows)
    hit, t = oracle.sphere_hit_f32(rows)
    closest = u32(np.ascontiguousarray(rows[:, 10]))
    for b, book in enumerate(("book 1", "book 2")):
        w = out[:, 6 * b:6 * b + 6]
        h_inf, t_inf = hit[:, b] != 0, u32(np.ascontiguousarray(t[:, b]))
        h_c, t_c = hit[:, 2 + b], u32(np.ascontiguousarray(t[:, 2 + b]))
        assert 0 < h_inf[is_special].sum() < is_special.sum() and 0 < h_inf[~is_special].sum() < (~is_special).sum()
        assert np.array_equal(accepted(w[:, 0]), h_inf), f"{book} exact_root: acceptance differs from the twin's hit"
        assert_same(f"SPHERE {book} exact_root", w[h_inf, 0], t_inf[h_inf], rows[h_inf])
        want_t = np.where(h_c != 0, t_c, closest)  # a miss leaves `closest` as it was
        assert_same(f"SPHERE {book} test_range", w[:, 2:4], np.stack([h_c, want_t], axis=1), rows)
        tang = np.flatnonzero(is_special)[:len(TANGENT_K)]  # the first special rows placed
        assert np.array_equal(rows[tang], tangent_rows())
        assert_same(f"SPHERE {book} tangent roots", w[tang, 0], np.full(len(tang), TANGENT_ROOT), rows[tang])
        assert (w[tang, 2] == 1).all()
