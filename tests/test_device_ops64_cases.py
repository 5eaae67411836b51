"""CPU companion of tests/test_gpu_device_ops64.py: the inputs of tests/device_ops64_cases.py hold
every named class (so a refactor of the generators cannot silently drop an edge), and the oracle's
f64 acos / atan2 stay within 1 ulp of the platform libm on those very inputs."""
import numpy as np

import device_ops64_cases as C
from oracle import oracle

MAX_ROWS = 2_100_000  # each op's GPU test stays a matter of seconds


def ordered(x):
    b = C.f64(x).view(np.int64)
    return np.where(b < 0, -(b & np.int64(0x7FFFFFFFFFFFFFFF)), b)


def ulps(u, v):
    """Distance in doubles; NaN against NaN is 0, NaN against a number is huge."""
    u, v = C.f64(u), C.f64(v)
    d = np.abs(ordered(u) - ordered(v))
    both, one = np.isnan(u) & np.isnan(v), np.isnan(u) ^ np.isnan(v)
    return np.where(both, 0, np.where(one, np.int64(1) << 62, d))


def has(values, wanted):
    """Every element of `wanted` occurs in `values`, bit for bit."""
    return np.isin(C.bits(wanted), C.bits(values)).all()


def test_every_op_stays_small():
    for gen in (C.acos_cases, C.atan2_cases, C.div_a_cases, C.div_const_cases, C.sqrt_cases, C.as_i32_cases, C.att_cases,
                C.vec_cases, C.sphere_cases, C.texel_cases):
        n = len(C.rows(gen()))
        print(f"{gen.__name__}: {n} rows")
        assert 0 < n <= MAX_ROWS, gen.__name__


def test_step_moves_in_value_order():
    assert C.step(1.0, 1) == 1 + 2.0 ** -52 and C.step(1.0, -1) == 1 - 2.0 ** -53
    assert C.step(0.0, -1) == -C.DENORM_MIN and C.step(-1.0, 1) == -(1 - 2.0 ** -53)
    assert np.isnan(C.step(np.nan, 3)) and C.step(C.MAX, 1) == np.inf


def test_acos_classes_and_oracle_accuracy():
    d = C.acos_cases()
    x = C.rows(d)
    for hw in C.THRESHOLDS:
        at = C.from_bits(np.array([hw << 32], np.uint64))[0]
        assert has(x, [at, -at, C.step(at, -1), -C.step(at, -1), C.step(at, 1)]), hex(hw)
    one = np.float64(1)
    assert has(x, [0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -52, -(1 + 2.0 ** -52), 1 - 2.0 ** -52, C.step(one, -1), np.inf, -np.inf])
    assert np.isnan(x).any() and ((x != 0) & (np.abs(x) < 2.0 ** -1022)).sum() >= 100
    ax = np.abs(x)
    for lo, hi, sign in ((0, 2.0 ** -57, 0), (2.0 ** -57, 0.5, 0), (0.5, 1, 1), (0.5, 1, -1)):
        sel = (ax >= lo) & (ax < hi) & ((sign == 0) | (np.sign(x) == sign))
        assert sel.sum() >= 200_000, (lo, hi, sign)
    got, _ = oracle.acos_atan2_f64(x, 0.0)
    with np.errstate(invalid="ignore"):
        want = np.arccos(x)
    assert ulps(got, want).max() <= 1
    assert np.array_equal(np.isnan(got), ax > 1) or np.array_equal(np.isnan(got), ~(ax <= 1))


def test_atan2_classes_and_oracle_accuracy():
    d = C.atan2_cases()
    yx = C.rows(d)
    y, x = yx[:, 0], yx[:, 1]
    for hw in C.THRESHOLDS:  # as atan's own argument (x = 1) and as |y / x| (x = -1)
        at = C.from_bits(np.array([hw << 32], np.uint64))[0]
        for xv in (1.0, -1.0):
            sel = x == xv
            assert has(y[sel], [at, -at, C.step(at, -1), -C.step(at, -1), C.step(at, 1)]), hex(hw)
    fin = np.isfinite(y) & np.isfinite(x) & (x != 0) & (y != 0)
    for sy in (1, -1):
        for sx in (1, -1):
            assert (fin & (np.sign(y) == sy) & (np.sign(x) == sx)).sum() >= 100_000
            assert (np.isinf(y) & np.isinf(x) & (np.sign(y) == sy) & (np.sign(x) == sx)).any()
            assert ((y == 0) & (x == 0) & (np.signbit(y) == (sy < 0)) & (np.signbit(x) == (sx < 0))).any()
    assert (np.isnan(y) & ~np.isnan(x)).any() and (np.isnan(x) & ~np.isnan(y)).any()
    assert ((x == 1) & fin).sum() >= 4096
    hi = lambda v: (np.abs(v).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    k = (hi(y) - hi(x)) >> 20
    for g in (59, 60, 61, 62):
        assert (fin & (k == g)).any() and (fin & (k == -g) & (x < 0)).any() and (fin & (k == -g) & (x > 0)).any(), g
    with np.errstate(all="ignore"):
        ratio = np.abs(y / x)
    for lo, hi_ in ((0, 2.0 ** -29), (2.0 ** -29, 0.4375), (0.4375, 0.6875), (0.6875, 1.1875), (1.1875, 2.4375), (2.4375, 2.0 ** 66),
                    (2.0 ** 66, np.inf)):
        assert (fin & (ratio >= lo) & (ratio < hi_)).sum() >= 50_000, (lo, hi_)
    _, got = oracle.acos_atan2_f64(x, y)
    assert ulps(got, np.arctan2(y, x)).max() <= 1


def test_div_a_classes():
    d = C.div_a_cases()
    inside, outside = C.div_a_values()
    lo, hi = np.float64(2.0 ** -64), np.float64(2.0 ** 64)
    assert ((inside >= lo) & (inside <= hi)).all() and not ((outside >= lo) & (outside <= hi)).any()
    assert has(inside, [lo, C.step(lo, 1), C.step(lo, 2), hi, C.step(hi, -1), C.step(hi, -2)])
    assert has(outside, [C.step(lo, -1), C.step(lo, -2), C.step(hi, 1), C.step(hi, 2), 0.0, np.inf, -1.0]) and np.isnan(outside).any()
    mant = C.bits(inside) & np.uint64((1 << 52) - 1)
    assert (mant == 0).sum() >= 16 and (mant == (1 << 52) - 1).sum() >= 8
    assert len({int(m) for m in mant if m and (int(m) & (int(m) - 1)) == 0}) == 52  # one-bit mantissas
    in_range = lambda a: (a >= lo) & (a <= hi)
    with np.errstate(all="ignore"):
        q = {k: v[:, 0] / v[:, 1] for k, v in d.items()}
    assert q["model_pair"][0] == C.MAX and tuple(d["model_pair"][0]) == C.MODEL_PAIR
    near = ulps(q["near_tmin"], np.full(len(q["near_tmin"]), C.TMIN)) <= 8
    a = d["near_tmin"][:, 1]
    assert (near & in_range(a)).sum() >= 10_000 and (near & in_range(a) & (q["near_tmin"] > C.TMIN)).any() and \
           (near & in_range(a) & (q["near_tmin"] <= C.TMIN)).any()
    for name in ("near_max", "near_max_random"):
        a = d[name][:, 1]
        assert in_range(a).all()
        assert (q[name] == C.MAX).sum() >= 1000 and (np.isfinite(q[name]) & (q[name] >= C.step(C.MAX, -8))).sum() >= 10_000, name
    assert np.isinf(q["overflow"]).sum() >= 10_000 and np.isfinite(d["overflow"]).all()
    sub = lambda v: (v != 0) & (np.abs(v) < 2.0 ** -1022)
    assert (sub(q["subnormal_quotient"]) & in_range(d["subnormal_quotient"][:, 1])).sum() >= 10_000
    assert (sub(d["subnormal_numerator"][:, 0]) & in_range(d["subnormal_numerator"][:, 1])).sum() >= 10_000
    n = d["special"][:, 0]
    assert has(n, [0.0, -0.0, np.inf, -np.inf]) and np.isnan(n).any()
    assert len(d["random"]) >= 400_000 and in_range(d["scene"][:, 1]).all()


def test_div_const_classes():
    d = C.div_const_cases()
    x = C.rows(d)
    dom = C.div_const_domain(x)
    assert dom.sum() >= 800_000 and (~dom).sum() >= 10 and has(x, [0.0, 2.0 ** -60, C.step(np.float64(8), -1)])
    for w, h in C.texel_sizes():  # both neighbours of every edge near 0, n / 2, n
        for k in C._edge_ks(w):
            e = C.TWO_PI * k / w
            if 2.0 ** -60 <= e < 7.9:
                assert has(x, [C.step(e, -1), e, C.step(e, 1)]), (w, k)
        for k in C._edge_ks(h):
            e = C.PI * k / h
            if 2.0 ** -60 <= e:
                assert has(x, [C.step(e, -1), e, C.step(e, 1)]), (h, k)
    assert has(x, [2.0 ** -52, 2.0 ** -51, C.TWO_PI, C.step(C.TWO_PI, -1), C.PI])
    assert len(d["outside"]) >= 10 and not C.div_const_domain(d["outside"]).any()


def test_sqrt_waves():
    d = C.sqrt_cases()
    want = {"no_small_lane": None, "no_small_lane_special": None, "one_small_first": 0, "one_small_middle": 31, "one_small_last": 63}
    for name, lane in want.items():
        small = C.sqrt_small(d[name].reshape(-1, 64))
        if lane is None:
            assert not small.any(), name
        else:
            assert (small.sum(axis=1) == 1).all() and small[:, lane].all(), name
    assert C.sqrt_small(d["all_small"]).all() and len(d["all_small"]) % 64 == 0
    x = C.rows(d)
    assert len(x) % 64 == 0
    assert has(x, [0.0, -0.0, np.inf, -np.inf, -1.0, C.SMALL, C.step(C.SMALL, -1), C.step(C.SMALL, 1), C.DENORM_MIN]) and np.isnan(x).any()
    # nearly-square mantissas: the root of a neighbour of k^2 rounds next to k
    big = d["no_small_lane"]
    r = np.sqrt(big)
    m = np.frexp(r)[0] * 2.0 ** 26
    assert (np.abs(m - np.rint(m)) < 2.0 ** -20).sum() >= 10_000


def test_as_i32_and_att_classes():
    x = C.rows(C.as_i32_cases())
    assert has(x, [2147483647.0, 2147483648.0, -2147483648.0, C.step(np.float64(2147483647.0), -1), C.step(np.float64(-2147483648.0), 1),
                   0.0, -0.0, np.inf, -np.inf]) and np.isnan(x).any()
    want = np.array([2147483647, 2147483647, -2147483648, 2147483646, -2147483647, 0, 0], np.int32)
    assert np.array_equal(oracle.as_i32_f64([2147483647.0, 3e9, -3e9, 2147483646.5, -2147483647.5, np.nan, -0.9]), want)
    a = C.rows(C.att_cases())
    words, by = a[:, 0].astype(np.uint64), a[:, 1].astype(np.uint64)
    assert np.array_equal(words.astype(np.float64), a[:, 0]) and words.max() < 1 << 32 and by.max() <= 0x1000000
    assert np.isin(np.arange(C.TEXEL_TAG - 1, C.TEXEL_TAG + 257, dtype=np.uint64), words).all()
    assert np.isin(np.array([0x7FC00000, 0x80000000, 0xBF000000, 0xBF800000], np.uint64), words).all()
    px = by[by != 0x1000000]
    for shift in (0, 8, 16):
        assert len(np.unique((px >> np.uint64(shift)) & np.uint64(255))) == 256
    assert (by == 0x1000000).any()
    ch = oracle.texel_channels_f64()
    assert ch[0] == 0 and ch[255] == 1.0 and np.array_equal(ch, (1.0 / 255.0) * np.arange(256.0))


def test_vec_classes():
    d = C.vec_cases()
    for name in ("random_unit", "random_nonunit", "parallel", "perpendicular", "total_internal_reflection", "grazing", "cosine_0_1",
                 "cosine_ends", "albedo", "lengths"):
        assert len(d[name]) > 0 and d[name].shape[1] == 9, name
    t = d["total_internal_reflection"]
    perp2 = (t[:, 6] * t[:, 0]) ** 2  # |e (uv + cos n)|^2 for uv = (s, 0, -c), n = z
    assert (perp2 > 1).sum() >= 20 and (perp2 < 1).sum() >= 20 and (np.abs(1 - perp2) < 2.0 ** -48).any()
    g = d["grazing"]
    k = 1 - (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    assert (k > 0).any() and (k < 0).any() and (np.abs(k) < 2.0 ** -50).any()
    assert (d["cosine_ends"][:, 7] == 1).any() and (d["cosine_0_1"][:, 7] == 1).any()
    alb = d["albedo"][:, :3]
    assert np.isnan(alb).any(axis=1).sum() >= 4 and (alb < 0).all(axis=1).any() and (np.signbit(alb) & (alb == 0)).all(axis=1).any()
    want = oracle.vec_f64(d["albedo"])[:, 10]
    # a NaN first component stays (no comparison replaces it); a NaN elsewhere is passed over
    assert np.nanmin(want) == 0.05 and np.nanmax(want) == 0.95 and np.array_equal(np.isnan(want), np.isnan(alb[:, 0]))
    assert np.isnan(alb[:, 0]).sum() >= 2 and np.isnan(alb[~np.isnan(alb[:, 0]), 1:]).any()


def test_sphere_classes():
    d = C.sphere_cases()
    r = C.rows(d)
    assert np.array_equal(C.f32r(r[:, 6:10]), r[:, 6:10]), "centers and radii are f32 records"

    def disc(v):
        o, dd, c, rad = v[:, 0:3], v[:, 3:6], v[:, 6:9], np.maximum(v[:, 9], 0)
        oc = c - o
        a = (dd * dd).sum(axis=1)
        h = (dd * oc).sum(axis=1)
        return h * h - a * ((oc * oc).sum(axis=1) - rad * rad), a

    with np.errstate(all="ignore"):
        ds, _ = disc(d["tangent"])
        assert (ds < 0).sum() >= 20 and (ds == 0).any() and ((ds > 0) & (ds < 2.0 ** -40)).sum() >= 20
        ds, _ = disc(d["tiny_disc"])
        assert ((ds > 0) & (ds < C.SMALL)).sum() >= 20
        _, a = disc(d["a_range"])
        assert (a < 2.0 ** -64).any() and (a > 2.0 ** 64).any() and ((a >= 2.0 ** -64) & (a <= 2.0 ** 64)).any()
        hit, t = oracle.sphere_hit_f64(r)
    lo, hi = 0, 0
    for name, v in d.items():
        hi = lo + len(v)
        if name == "near_tmin":
            tt = t[lo:hi, 0]
            assert (ulps(tt, np.full(hi - lo, C.TMIN)) <= 64).sum() >= 8 and (np.abs(tt - 2) < 1e-2).sum() >= 8
        if name == "closest_equal":
            assert hit[lo, 0] == 1 and t[lo, 0] == 3 and hit[lo, 1] == 0 and hit[lo + 1, 1] == 1
        if name == "inside":
            assert hit[lo:hi, 0].all()
        lo = hi
    rad = d["radius"][:, 9]
    assert ((rad > 0) & (rad < 2.0 ** -126)).sum() >= 10 and (rad > 2.0 ** 120).any() and (rad < 0).any()
    assert 0.2 < hit[:, 0].mean() < 0.95 and 0 < hit[:, 1].sum() < hit[:, 0].sum()


def test_texel_classes():
    d = C.texel_cases()
    r = C.rows(d)
    sizes = {(int(w), int(h)) for w, h in np.unique(r[:, 3:5], axis=0)}
    assert sizes == set(C.texel_sizes()) and {(1, 1), (2, 1), (3, 2), (7, 5), (4096, 2048), (1 << 20, 1 << 20),
                                              ((1 << 20) + 1, 3)} <= sizes
    assert C.earth_size() == (1024, 512)
    marks = C.texel_marks(r)
    for name, m in zip(("column must fall back", "row must fall back", "column must be decided", "row must be decided"), marks):
        print(f"TEXEL64 {name}: {m.mean():.3f} of {len(r)} rows")
        assert m.mean() >= 0.10, name
    assert not (marks[0] & marks[2]).any() and not (marks[1] & marks[3]).any()
    assert not marks[2][r[:, 3] > 2.0 ** 20].any()
    # edges: the f64 direction lands within a few ulps of the edge, and the moves reach 2^40 ulps
    ce = d["column_edges"]
    with np.errstate(all="ignore"):
        s = (np.arctan2(-ce[:, 2], ce[:, 0]) + np.pi) / (2 * np.pi) * ce[:, 3]
        assert (np.abs(s - np.rint(s)) < 2.0 ** -45 * ce[:, 3]).sum() >= 5 * len(ce) // 13
        re = d["row_edges"]
        t = (1 - np.arccos(-re[:, 1]) / np.pi) * re[:, 4]
        assert (np.abs(t - np.rint(t)) < 2.0 ** -40 * re[:, 4]).sum() >= 3 * len(re) // 13
    assert set(C.ULP_MOVES) == {0, 1, -1, 2, -2, 1 << 10, -(1 << 10), 1 << 20, -(1 << 20), 1 << 30, -(1 << 30), 1 << 40, -(1 << 40)}
    p = d["poles"]
    one = np.float64(1)
    assert has(np.abs(p[:, 1]), [1.0, C.step(one, -1), 1 - 2.0 ** -24, 1 - 2.0 ** -25, 1 + 2.0 ** -52])
    assert (p[:, 1] > 0).any() and (p[:, 1] < 0).any()
    zz = p[(p[:, 0] == 0) & (p[:, 2] == 0)]
    assert {(bool(a), bool(b)) for a, b in zip(np.signbit(zz[:, 0]), np.signbit(zz[:, 2]))} == {(False, False), (False, True), (True, False), (True, True)}
    e = d["component_ends"]
    for col in (0, 2):
        v = np.abs(e[:, col])
        assert (v == 0).any() and ((v > 0) & (v < 2.0 ** -60)).any() and (v > 2.0 ** 60).any() and np.isnan(v).any()
    assert len(d["random"]) >= 8 * 6000
