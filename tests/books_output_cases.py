"""Shared inputs of the books-path output tests (tests/test_books_output.py on the host,
tests/test_gpu_books_output.py on the device): channel sums for color.rs:6-32 write_color, chosen
where a byte can move, and a numpy f64 restatement of it.

For each samples-per-pixel value in SPPS the channel values are
  * every quantisation step spp * (k / 256)^2, k = 0 ... 256 (k = 0: zero and its subnormal
    neighbours), each with its +-1 ... +-4 ulp neighbours (np.nextafter) — where a square root that is
    not correctly rounded, or a product taken in another precision, moves a byte;
  * spp * 0.999^2 (the clamp), spp (1.0) and 0.25 * spp, with the same neighbours;
  * 0, -0, +-inf, NaN, -1, +-5e-324, DBL_MIN, 1e-300, 1e300 and DBL_MAX;
  * 4,000 uniform values in [-0.3, 1.4] * spp.
6,352 values per spp. Channel 0 holds them in order, channel 1 reversed, channel 2 rolled by 1,237;
w holds spp, the sample count a render leaves there (the quantiser does not read it).
"""
import functools

import numpy as np

SPPS = (1, 13, 512, 1000, 5000)
N_ROWS = 6352
DBL_MAX = np.finfo(np.float64).max


def _neighbours(v):
    """v and its +-1 ... +-4 ulp neighbours, in ascending order."""
    out = [v]
    lo = hi = np.float64(v)
    for _ in range(4):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out = [lo] + out + [hi]
    return out


@functools.lru_cache(maxsize=None)
def _values(spp):
    s = np.float64(spp)
    v = []
    for k in range(257):
        v += _neighbours(s * (np.float64(k) / 256.0) ** 2)
    for x in (s * np.float64(0.999) ** 2, s, 0.25 * s):
        v += _neighbours(x)
    v += [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, 1e300, DBL_MAX]
    rng = np.random.default_rng(spp)
    v = np.concatenate([np.asarray(v, dtype=np.float64), rng.uniform(-0.3, 1.4, size=4000) * s])
    assert v.shape == (N_ROWS,)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def accum64(spp):
    """(N_ROWS, 4) float64 sums for `spp`, read-only (computed once, shared by the tests)."""
    v = _values(spp)
    a = np.empty((N_ROWS, 4), dtype=np.float64)
    a[:, 0] = v
    a[:, 1] = v[::-1]
    a[:, 2] = np.roll(v, 1237)
    a[:, 3] = spp
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def accum32(spp):
    """The same sums rounded to f32 (DBL_MAX and 1e300 become inf), for the float-accum entries."""
    with np.errstate(over="ignore"):
        a = accum64(spp).astype(np.float32)
    a.setflags(write=False)
    return a


def write_color_numpy(accum, spp):
    """color.rs:6-32 over (n, 4) sums in numpy's f64 (np.sqrt is the IEEE root): (n, 3) uint8.
    x = (1 / spp) * sum; sqrt if x > 0 else 0; Interval(0, 0.999).clamp as its two comparisons (a
    NaN passes); (256 * x) as i32, NaN -> 0."""
    scale = np.float64(1.0) / np.float64(spp)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        x = scale * np.asarray(accum, dtype=np.float64)[:, :3]
        x = np.where(x > 0.0, np.sqrt(np.where(x > 0.0, x, 0.0)), 0.0)
        x = np.where(x < 0.0, 0.0, x)
        x = np.where(x > 0.999, 0.999, x)
        v = 256.0 * x
        return np.where(np.isnan(v), 0, np.where(np.isnan(v), 0.0, v).astype(np.int32)).astype(np.uint8)


def fill(accum, n_px):
    """n_px rows out of `accum`, cycled from row 0 (n_px may exceed the set)."""
    return np.ascontiguousarray(np.resize(accum, (n_px, 4)))
