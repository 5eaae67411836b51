"""The f64 books kernel's numeric building blocks, run on the device on chosen arguments.

Whole-scene parity (tests/test_gpu_books64.py) only sees the arguments C1 / C2 / C4 / C5 produce, and
one texture size. Here the kernel's own __device__ functions (rrt_books64.hip, through the test-only
entry rrt_testing_device_ops64) are applied elementwise to the inputs of tests/device_ops64_cases.py —
fdlibm's high-word thresholds, the per-ray reciprocal's range ends and the quotients at the acceptance
bound and at the largest finite, texel and image edges of the f32 angle enclosures, waves with and
without a lane below 2^-767 — and every result is compared bit for bit (NaNs equal as a class,
-0 != +0) with the oracle's books path, or with numpy's float64 where the operation is an IEEE one.
tests/test_device_ops64_cases.py checks on the CPU that the inputs hold every named class.
"""
import numpy as np
import pytest

import device_ops64_cases as C
from oracle import oracle
from rustraytrace_amd import _lib

pytestmark = pytest.mark.gpu


def u64(x):
    x = np.ascontiguousarray(x)
    if x.dtype.itemsize != 8:  # i32 / u32 words as the device stores them: zero-extended from 32 bits
        x = x.astype(np.int64) & np.int64(0xFFFFFFFF)
    return x.view(np.uint64)


def same(a, b):
    """Bit equality of two word arrays holding f64, NaNs equal as a class."""
    a, b = u64(a), u64(b)
    return (a == b) | (np.isnan(a.view(np.float64)) & np.isnan(b.view(np.float64)))


def assert_same(what, got, want, inputs):
    """got / want: (n,) or (n, k) 64-bit words; prints the first offending rows as hex bit patterns."""
    got, want = u64(got).reshape(len(inputs), -1), u64(want).reshape(len(inputs), -1)
    bad = np.flatnonzero(~same(got, want).all(axis=1))
    print(f"{what}: {len(inputs)} inputs compared, {len(bad)} differ")
    if len(bad):
        hx = lambda row: " ".join(f"{int(w):016x}" for w in np.atleast_1d(row))
        rows_in = u64(np.ascontiguousarray(inputs, dtype=np.float64)).reshape(len(inputs), -1)
        lines = [f"  in {hx(rows_in[i])} | device {hx(got[i])} | want {hx(want[i])}" for i in bad[:8]]
        pytest.fail(f"{what}: {len(bad)} of {len(inputs)} results differ\n" + "\n".join(lines))


def accepted(t_words):
    t = u64(t_words).view(np.float64)
    with np.errstate(invalid="ignore"):
        return (C.TMIN < t) & (t < np.inf)


def test_acos():
    x = C.rows(C.acos_cases())
    want, _ = oracle.acos_atan2_f64(x, 0.0)
    assert_same("ACOS64", _lib.device_ops64("ACOS64", x), want, x)


def test_atan2():
    yx = C.rows(C.atan2_cases())
    _, want = oracle.acos_atan2_f64(yx[:, 1], yx[:, 0])
    assert_same("ATAN2_64", _lib.device_ops64("ATAN2_64", yx), want, yx)


def test_div_a():
    """(r, q, ra): q is numpy's float64 division (the in-kernel quotient is the IEEE one); ra is nonzero
    exactly on [2^-64, 2^64]; r takes q's accept / reject decision over (0.001, inf) on every row,
    equals q where q is accepted, and is n / a outside the range."""
    na = C.rows(C.div_a_cases())
    out = _lib.device_ops64("DIV_A64", na)
    n, a = na[:, 0], na[:, 1]
    with np.errstate(all="ignore"):
        q = n / a
    assert_same("DIV_A64 in-kernel n / a", out[:, 1], q, na)
    ra = out[:, 2].view(np.float64)
    with np.errstate(invalid="ignore"):
        in_range = (a >= 2.0 ** -64) & (a <= 2.0 ** 64)
    assert np.array_equal(ra != 0, in_range), "recip_a64 is nonzero exactly on [2^-64, 2^64]"
    r = out[:, 0]
    differ = ~same(r, q)
    with np.errstate(invalid="ignore"):
        aq = np.abs(q)
        unread = in_range & (aq < 2.0 ** -1022)           # subnormal or zero quotients: no decision reads them
        rejected = in_range & ~accepted(q) & ~unread      # normal quotients outside (0.001, inf), NaN and inf
    flipped = accepted(r) != accepted(q)
    print(f"DIV_A64: {len(na)} pairs compared; accept / reject differs on {int(flipped.sum())}; "
          f"accepted quotients that differ {int((differ & accepted(q)).sum())}; out of range that differ "
          f"{int((differ & ~in_range).sum())}; rejected normal quotients that differ {int((differ & rejected).sum())}; "
          f"unread (subnormal or zero) quotients that differ {int((differ & unread).sum())} of {int(unread.sum())}")
    if flipped.any():
        i = np.flatnonzero(flipped)[:8]
        lines = [f"  n {n[j].hex()} a {a[j].hex()} | div_a64 {r.view(np.float64)[j].hex()} | n / a {q[j].hex()}" for j in i]
        pytest.fail(f"DIV_A64: accept / reject over (0.001, inf) differs from the IEEE quotient's on {int(flipped.sum())} pairs\n" +
                    "\n".join(lines))
    must = accepted(q) | ~in_range
    assert_same("DIV_A64 accepted or out of range", r[must], u64(q)[must], na[must])
    # since div_a64 sends a first quotient outside [2^-896, inf) to the IEEE division, every quotient is
    # the IEEE one, the unread ones included
    assert_same("DIV_A64 every quotient", r, q, na)


def test_div_const():
    x = C.rows(C.div_const_cases())
    out = _lib.device_ops64("DIV_CONST64", x)
    domain = C.div_const_domain(x)
    for col, c in ((0, C.TWO_PI), (2, C.PI)):
        with np.errstate(all="ignore"):
            want = x / c
        assert_same(f"DIV_CONST64 ieee x / {c}", out[:, col + 1], want, x)
        assert_same(f"DIV_CONST64 div_by_const64(x, {c})", out[domain, col], want[domain], x[domain])


def test_sqrt():
    d = C.sqrt_cases()
    x = C.rows(d)
    small = C.sqrt_small(x.reshape(-1, 64)).sum(axis=1)
    assert (small == 0).any() and (small == 1).any() and (small == 64).any()
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    assert_same("SQRT64", _lib.device_ops64("SQRT64", x), want, x)


def test_as_i32():
    x = C.rows(C.as_i32_cases())
    assert_same("AS_I32", _lib.device_ops64("AS_I32", x), oracle.as_i32_f64(x), x)


def test_att():
    """att_decode: a texel tag kTexelTag + b is byte b's channel, every other word the f32 it holds
    (negative, -0 and quiet NaNs included); texel_value64: the three channels, or (0, 1, 1) without data."""
    rows = C.rows(C.att_cases())
    out = _lib.device_ops64("ATT64", rows)
    ch = oracle.texel_channels_f64()
    words, by = rows[:, 0].astype(np.uint64), rows[:, 1].astype(np.uint64)
    tag = (words >= C.TEXEL_TAG) & (words < C.TEXEL_TAG + 256)
    assert tag.sum() >= 256 and (~tag).sum() >= 256
    with np.errstate(invalid="ignore"):  # widening a signalling NaN
        as_f32 = words.astype(np.uint32).view(np.float32).astype(np.float64)
    att = np.where(tag, ch[np.where(tag, words - C.TEXEL_TAG, 0).astype(np.int64)], as_f32)
    assert_same("ATT64 att_decode", out[:, 0], att, rows)
    px = np.stack([ch[(by >> np.uint64(s) & np.uint64(255)).astype(np.int64)] for s in (0, 8, 16)], axis=1)
    px[by == 0x1000000] = (0.0, 1.0, 1.0)
    assert_same("ATT64 texel_value64", out[:, 1:], px, rows)


def test_vec():
    rows = C.rows(C.vec_cases())
    assert_same("VEC64", _lib.device_ops64("VEC64", rows), oracle.vec_f64(rows), rows)


def test_sphere():
    """Device words per record (the f32 record, then the widened Sphere64): exact_root64, leaves64's
    (hit, t) against `closest`. An exact root is the oracle's t when it hits over (0.001, inf) and is not
    accepted when it misses; a miss leaves `closest` as it was."""
    rows = C.rows(C.sphere_cases())
    out = _lib.device_ops64("SPHERE64", rows)
    hit, t = oracle.sphere_hit_f64(rows)
    assert 0 < hit[:, 0].sum() < len(rows) and 0 < hit[:, 1].sum() < hit[:, 0].sum()
    closest = u64(np.ascontiguousarray(rows[:, 10]))
    h_inf, t_inf = hit[:, 0] != 0, u64(np.ascontiguousarray(t[:, 0]))
    h_c, t_c = hit[:, 1], u64(np.ascontiguousarray(t[:, 1]))
    want_t = np.where(h_c != 0, t_c, closest)
    for b, rec in enumerate(("float4", "Sphere64")):
        w = out[:, 3 * b:3 * b + 3]
        assert np.array_equal(accepted(w[:, 0]), h_inf), f"{rec} exact_root64: acceptance differs from the oracle's hit"
        assert_same(f"SPHERE64 {rec} exact_root64", w[h_inf, 0], t_inf[h_inf], rows[h_inf])
        assert_same(f"SPHERE64 {rec} leaves64", w[:, 1:3], np.stack([u64(h_c), want_t], axis=1), rows)
    assert_same("SPHERE64 Sphere64 against float4", out[:, 3:6], out[:, 0:3], rows)


def test_texel():
    """The chosen texel equals the oracle's and the kernel's own fdlibm-only texel on every row; a row
    whose true coordinate lies closer to an integer than any enclosure's half-width must have fallen
    back (a decided one is a broken enclosure), a row far from every edge within the enclosures' domain
    must be decided, and no image above 2^20 is decided."""
    rows = C.rows(C.texel_cases())
    out = _lib.device_ops64("TEXEL64", rows)
    want = oracle.texel_index_f64(rows)
    assert_same("TEXEL64 (i, j) against the oracle", out[:, 0:2], want, rows)
    assert_same("TEXEL64 (i, j) against the kernel's fdlibm path", out[:, 0:2], out[:, 4:6], rows)
    col_fast, row_fast = out[:, 2] != 0, out[:, 3] != 0
    col_fb, row_fb, col_dec, row_dec = C.texel_marks(rows)
    print(f"TEXEL64: {len(rows)} rows; columns decided {int(col_fast.sum())}, fell back {int((~col_fast).sum())}; "
          f"rows decided {int(row_fast.sum())}, fell back {int((~row_fast).sum())}; must fall back "
          f"{int(col_fb.sum())} / {int(row_fb.sum())}, of them decided {int((col_fb & col_fast).sum())} / "
          f"{int((row_fb & row_fast).sum())}; must be decided {int(col_dec.sum())} / {int(row_dec.sum())}, of them "
          f"fell back {int((col_dec & ~col_fast).sum())} / {int((row_dec & ~row_fast).sum())}")
    assert col_fast.any() and (~col_fast).any() and row_fast.any() and (~row_fast).any()
    assert not col_fast[rows[:, 3] > 2 ** 20].any() and not row_fast[rows[:, 4] > 2 ** 20].any()
    for name, fb, fast in (("column", col_fb, col_fast), ("row", row_fb, row_fast)):
        bad = np.flatnonzero(fb & fast)
        assert len(bad) == 0, f"{name} decided within reach of an edge: " + "; ".join(
            " ".join(float(v).hex() for v in rows[i]) for i in bad[:4])
    for name, dec, fast in (("column", col_dec, col_fast), ("row", row_dec, row_fast)):
        bad = np.flatnonzero(dec & ~fast)
        assert len(bad) == 0, f"{name} fell back far from every edge: " + "; ".join(
            " ".join(float(v).hex() for v in rows[i]) for i in bad[:4])
