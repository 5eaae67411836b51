"""CPU companion of tests/test_gpu_device_ops.py: the input sets (tests/device_ops_cases.py) hold
every class they name, so the device tests cannot pass vacuously, and on the full sets the oracle's
f32 twins — what the device results are compared with bit for bit — stay within the project's
accuracy bounds against numpy float64."""
import numpy as np

import device_ops_cases as C
from oracle import oracle

F = np.float32
GENERATORS = (C.sin_cos_cases, C.log_cases, C.acos_cases, C.atan2_cases, C.div_a_cases, C.div_const_cases,
              C.floor_i32_cases, C.texture_points, C.checker_cases, C.vec_cases, C.quad_cases, C.sphere_cases)
COLUMNS = {"sin_cos_cases": 1, "log_cases": 1, "acos_cases": 1, "atan2_cases": 2, "div_a_cases": 2,
           "div_const_cases": 1, "floor_i32_cases": 1, "texture_points": 3, "checker_cases": 4, "vec_cases": 9,
           "quad_cases": 9, "sphere_cases": 11}


def has(x, v):
    """v occurs in x as a bit pattern (so -0 and +0 are told apart)."""
    return bool((np.ascontiguousarray(x, F).view(np.uint32) == np.array([v], F).view(np.uint32)[0]).any())


def test_generators_return_float32_classes_and_are_deterministic():
    for gen in GENERATORS:
        classes = gen()
        for name, arr in classes.items():
            assert isinstance(arr, np.ndarray) and arr.dtype == np.float32, (gen.__name__, name)
            assert len(arr) >= 1, f"{gen.__name__}: class {name} is empty"
        r = C.rows(classes)
        assert r.dtype == np.float32 and r.reshape(len(r), -1).shape[1] == COLUMNS[gen.__name__]
        if r.size < 1 << 20:
            gen.cache_clear()
            assert np.array_equal(C.rows(gen()).view(np.uint32), r.view(np.uint32)), gen.__name__


def test_sin_cos_classes():
    c = C.sin_cos_cases()
    assert len(c["phi_grid"]) == 1 << 24 and c["phi_grid"][0] == 0 and c["phi_grid"].max() < 6.2832
    assert len(np.unique(c["phi_grid"])) > (1 << 24) * 0.6  # the product's roundings merge some neighbours
    assert len(c["mantissas"]) == 2 * 256 * 2048
    e = (c["mantissas"].view(np.uint32) >> 23) & 255
    assert np.array_equal(np.bincount(e, minlength=256), np.full(256, 4096))
    assert np.signbit(c["mantissas"]).sum() == 256 * 2048
    assert len(c["octant_seams"]) == 2 * 5 * ((1 << 15) + 1)
    for k in (1, 2, 3, 4, 1000, 1 << 15):
        assert has(c["octant_seams"], F(k * np.pi / 4)) and has(c["octant_seams"], -F(k * np.pi / 4))
    for v in (8192.0, C.step(F(8192), 1), C.step(F(8192), -1), 16777215.0, 16777216.0, 16777214.0, -8192.0):
        assert has(c["big"], v)
    for v in (0.0, -0.0, C.DENORM_MIN, -C.DENORM_MAX, np.inf, -np.inf):
        assert has(c["special"], v)
    assert np.isnan(c["special"]).any()


def test_log_acos_atan2_classes():
    lg = C.log_cases()
    assert len(lg["u_grid"]) == 1 << 24 and lg["u_grid"][0] == 0 and lg["u_grid"][-1] == F(1 - 2.0 ** -24)
    assert np.array_equal(lg["u_grid"][:4], F(2.0 ** -24) * np.arange(4, dtype=F))
    s = F(np.sqrt(0.5))
    for e in (-125, -1, 0, 1, 127):
        for k in (-2, 0, 2):
            assert has(lg["mantissa_split"], C.step(F(float(s) * 2.0 ** e), k))
    ac = C.acos_cases()
    assert len(ac["mantissas"]) == 2 * 127 * 4096 and np.abs(ac["mantissas"]).max() < 1
    for v in (0.5, -0.5, 1.0, -1.0, C.step(F(0.5), 2), C.step(F(1), -2), C.step(F(-0.5), -2)):
        assert has(ac["edges"], v)
    assert has(ac["overshoot"], C.step(F(1), 1)) and has(ac["overshoot"], C.step(F(-1), -1))
    assert has(ac["special"], 0.0) and has(ac["special"], -0.0) and has(ac["special"], C.DENORM_MIN)
    at = C.atan2_cases()
    axis = np.unique(at["cross"][:, 0].view(np.uint32))
    assert len(at["cross"]) == len(axis) ** 2 and len(axis) == 2 * (6 + 6) + 1
    for v in (0.0, -0.0, C.DENORM_MIN, 1e-20, -1e-20, 1.0, -1.0, 1e20, np.inf, -np.inf,
              F(np.tan(np.pi / 8)), C.step(F(np.tan(np.pi / 8)), 1), C.step(F(np.tan(3 * np.pi / 8)), -1)):
        assert has(at["cross"][:, 0], v) and has(at["cross"][:, 1], v)
    assert np.isnan(at["cross"]).any(axis=1).sum() == 2 * len(axis) - 1
    assert len(at["unit_circle"]) == 1 << 16
    assert np.abs(np.hypot(*at["unit_circle"].T.astype(np.float64)) - 1).max() < 1e-6


def test_division_classes():
    a = C.div_a_values()
    assert a.dtype == np.float32 and len(a) == 48 and len(np.unique(a.view(np.uint32))) == 48
    lo, hi = F(2.0 ** -64), F(2.0 ** 64)
    for v in (lo, hi, 1.0, 0.0, C.DENORM_MAX, C.step(F(1), 1), C.step(F(1), -1), C.step(F(2), -1)):
        assert has(a, v)
    for end in (lo, hi):
        for k in (-2, -1, 1, 2):
            assert has(a, C.step(end, k))
    inside = (a >= lo) & (a <= hi)
    assert inside.sum() >= 36 and (~inside).sum() >= 10
    assert len(np.unique((a[inside].view(np.uint32) >> 23))) >= 28  # across the exponent range
    d = C.div_a_cases()
    na = C.rows(d)
    assert na.shape[1] == 2 and len(na) <= 1 << 22
    assert set(np.unique(na[:, 1].view(np.uint32))) == set(a.view(np.uint32))
    with np.errstate(all="ignore"):
        q = d["accept_bound"][:, 0] / d["accept_bound"][:, 1]
        assert (q > F(0.001)).any() and (q <= F(0.001)).any()
        q = d["overflow"][:, 0] / d["overflow"][:, 1]
        assert np.isinf(q).any() and np.isfinite(q).any()
    assert np.isnan(d["tiny_special"][:, 0]).any() and np.isinf(d["tiny_special"][:, 0]).any()
    x = C.rows(C.div_const_cases())
    assert has(x, 0.0) and has(x, 2.0 ** -100) and has(x, 8.0) and ((x > 0) & (x < 1e-20)).any()


def test_floor_and_texture_classes():
    fl = C.rows(C.floor_i32_cases())
    for v in (0.0, -0.0, -C.DENORM_MIN, 1.0, C.step(F(1), -1), C.step(F(-1), -1), C.step(F(-3), 1), 2.0 ** 31, -2.0 ** 31,
              C.step(F(2.0 ** 31), -1), C.step(F(-2.0 ** 31), -1), 1e30, -1e30, np.inf, -np.inf):
        assert has(fl, v)
    assert np.isnan(fl).any()
    p = C.texture_points()
    assert p["near"].shape == (4096, 3) and np.abs(p["near"]).max() <= 20
    assert p["far"].shape == (4096, 3) and 20 < np.abs(p["far"]).max() <= 2000
    assert (p["lattice"] == np.floor(p["lattice"])).all() and has(p["lattice"], -3.0) and has(p["lattice"], 0.0)
    assert ((p["half_lattice"] - np.floor(p["half_lattice"])) == 0.5).all()
    b = p["below_integer"]
    assert has(b, C.step(F(-2), -1)) and has(b, C.step(F(3), -1)) and has(b, C.step(F(0), -1))
    for v in (255.5, 256.5, -0.5):
        assert has(p["wrap"], v)
    for v in (4e7, -4e7, 1e12, -1e12):
        assert has(p["saturate"], v)
    assert float(F(4e7)) * 64 > 2.0 ** 31 > float(F(4e7)) * 32
    nf = p["nonfinite"]
    assert np.isnan(nf).any() and has(nf, np.inf) and has(nf, -np.inf) and (~np.isfinite(nf)).sum(axis=1).max() == 1
    table = C.perlin_table()
    assert table.shape == (1,) and table.dtype.itemsize == 6144
    assert C.PERLIN_SCALES == (0.2, 4.0)
    ck = C.checker_cases()
    assert set(p) < set(ck) and (C.rows(ck)[:, 0] == F(1.0 / 0.32)).all()
    assert has(ck["cell_faces"][:, 1:], F(0.32)) and has(ck["cell_faces"][:, 1:], F(-0.64)) and has(ck["cell_faces"][:, 1:], 0.0)
    _, _, even = oracle.book2_textures(table, C.rows(ck)[:, 1:], inv_scale=float(C.CHECKER_INV_SCALE))
    assert 0.3 < even.mean() < 0.7


def test_vector_and_intersection_classes():
    v = C.vec_cases()
    unit = v["random_unit"]
    assert np.abs(np.linalg.norm(unit[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.abs(np.linalg.norm(v["random_nonunit"][:, :3].astype(np.float64), axis=1) - 1).max() > 10
    par = v["parallel"]
    assert (par[:, :3] == par[:, 3:6]).all(axis=1).any() and (par[:, :3] == -par[:, 3:6]).all(axis=1).any()
    assert ((v["perpendicular"][:, :3] * v["perpendicular"][:, 3:6]).sum(axis=1) == 0).all()
    for name, k in (("grazing_k0", 0.0), ("grazing_k2m24", 2.0 ** -24)):
        g = v[name]
        assert len(g) >= 1 and (g[:, 6] == 1).all() and (g[:, 2] == 0).all() and (g[:, 3:6] == (0, 0, 1)).all()
        assert all(abs(1.0 - float(C.len2_f32(r[0], r[1]))) == k for r in g)
    assert set(v["cosine_0_1"][:, 7]) == {F(0), F(1)}
    x = v["onb_switch"][:, 3]
    assert has(x, 0.9) and has(x, -0.9) and (np.abs(x) > F(0.9)).any() and (np.abs(x) < F(0.9)).any()
    assert (v["zero"][:, :3] == 0).all(axis=1).any() and (v["zero"][:, 3:6] == 0).all(axis=1).any()

    q = C.quad_cases()
    rows, quads = C.rows(q), C.quad_records()
    assert len(quads) == len(C.QUADS) and set(rows[:, 8]) == set(F(j) for j in range(len(quads)))
    hit = lambda name: oracle.quad_hit_f32(quads, q[name])[0]
    axis_aligned = np.isin(q["corners"][:, 8], (0, 1, 5))
    assert hit("corners")[axis_aligned].all() and hit("edges")[np.isin(q["edges"][:, 8], (0, 1, 5))].all()
    assert not hit("outside").any()
    cut = hit("denom_cut")
    assert np.array_equal(cut != 0, np.abs(q["denom_cut"][:, 5]) >= F(1e-8)) and 0 < cut.sum() < len(cut)
    assert list(hit("t_bounds")) == [1, 0, 1, 1, 0, 1, 1]  # closed at both ends
    assert np.isneginf(q["tmin_neg_inf"][:, 6]).sum() == 3 and list(hit("tmin_neg_inf")) == [1, 1, 0, 1]
    assert not hit("parallel").any()
    assert 0 < hit("random").sum() < len(q["random"])

    s = C.sphere_cases()
    sh = lambda name: oracle.sphere_hit_f32(s[name])
    tangent = sh("tangent")[0][:, 0]
    assert list(tangent) == [0, 0, 1, 1, 1]  # disc < 0 below r = 1, 0 at it, > 0 above
    assert sh("inside")[0][:, 0].all()
    h, t = sh("on_surface")
    assert h[0, 0] and t[0, 0] == 2 and not h[1, 0]
    near = t[2:, 0]
    assert (near < F(0.002)).any() and (near > F(1.9)).any()  # the near root on either side of 0.001
    assert has(s["radius"][:, 9], 0.0) and (s["radius"][:, 9] < 0).any()
    a = (s["a_range"][:, 3:6].astype(np.float64) ** 2).sum(axis=1)
    assert (a < 2.0 ** -64).any() and (a > 2.0 ** 64).any() and ((a >= 2.0 ** -64) & (a <= 2.0 ** 64)).sum() >= 6
    assert sh("a_range")[0][:, 0].all()
    assert (s["d_zero"][:, 3:6] == 0).all() and not sh("d_zero")[0].any()
    # the overflow rows reach the division: along the x axis from the origin every product below is
    # exact in f32 (powers of two times small integers), h, disc and sq are finite, and the IEEE
    # quotient (h - sq) / a is inf, the float below the largest, or finite
    ov = s["overflow"]
    assert (ov[:, :3] == 0).all() and (ov[:, 4:6] == 0).all() and (ov[:, 7:9] == 0).all()
    dx, cx, rr = ov[:, 3], ov[:, 6], ov[:, 9]
    with np.errstate(over="ignore"):
        a, h, cc = dx * dx, dx * cx, cx * cx - rr * rr
        disc = (h.astype(np.float64) ** 2 - (a * cc).astype(np.float64)).astype(F)  # fma(h, h, -(a * c)): exact here
        sq = np.sqrt(disc)
        near, far = (h - sq) / a, (h + sq) / a
    assert np.isfinite(np.stack([a, h, cc, disc, sq])).all() and (disc > 0).all() and (a > 0).all()
    assert (a[:4] < F(2.0 ** -64)).all() and F(2.0 ** -64) <= a[4] <= F(2.0 ** 64)
    big = np.finfo(F).max
    assert list(near) == [np.inf, np.inf, np.nextafter(big, F(0)), F(2.0 ** 127), F(2.0 ** 90)]
    assert np.isinf(far[:2]).all()
    oh, ot = sh("overflow")
    assert list(oh[:, 0]) == [0, 0, 1, 1, 1] and np.array_equal(ot[2:, 0], near[2:])
    assert list(sh("closest_equal")[0][:, 2]) == [0, 1, 0, 1, 1]  # strict <: the far root 5 answers from closest > 5
    hr = sh("random")[0]
    assert 0 < hr[:, 2].sum() < hr[:, 0].sum() < len(hr)


def test_twins_are_accurate_on_the_full_sets():
    x = C.rows(C.sin_cos_cases())
    ok = np.isfinite(x) & (np.abs(x) <= 8192)
    x64 = x[ok].astype(np.float64)
    assert ok.sum() > (1 << 24) + 400000
    sin_err = np.abs(oracle.sin_f32(x)[ok] - np.sin(x64)).max()
    cos_err = np.abs(oracle.cos_f32(x)[ok] - np.cos(x64)).max()
    print(f"sin {sin_err:.3g} cos {cos_err:.3g} on {ok.sum()} arguments within 8192")
    assert sin_err < 2e-7 and cos_err < 2e-7

    u = C.log_cases()["u_grid"]
    lg = oracle.log_f32(u)
    assert lg[0] == -np.inf
    want = np.log(u[1:].astype(np.float64))
    err = np.abs(lg[1:] - want)
    rel = err / np.abs(want)  # every u in (0, 1): log u < 0
    print(f"log abs {err.max():.3g} rel {rel.max():.3g} on {len(want)} arguments")
    assert err.max() < 1e-6 and rel.max() < 2e-7

    ac = C.rows(C.acos_cases())
    ac = ac[np.abs(ac) <= 1]
    assert np.abs(oracle.acos_f32(ac) - np.arccos(ac.astype(np.float64))).max() < 4e-7
    assert np.isnan(oracle.acos_f32(C.acos_cases()["overshoot"])).all()
    yx = C.atan2_cases()["unit_circle"]
    yx64 = yx.astype(np.float64)
    assert np.abs(oracle.atan2_f32(yx) - np.arctan2(yx64[:, 0], yx64[:, 1])).max() < 4e-7


# ---- book 3's light list ----------------------------------------------------------------------------
def _ratio(n, sphere, o):
    """r * r / dot(oc, oc) in float32, as lights_pdf and lights_random form it."""
    c, r = C.LIGHT_SPHERES[sphere]
    oc = C.f32(c) - C.f32(o)
    d2 = F(F(oc[0] * oc[0]) + F(oc[1] * oc[1])) + F(oc[2] * oc[2])
    with np.errstate(divide="ignore"):
        return F(F(r) * F(r)) / F(d2)


def test_light_lists_and_origin_classes():
    assert sorted(C.LIGHT_LISTS) == [1, 2, 3, 5, 7]
    for n in C.LIGHT_LISTS:
        lt = C.light_records(n)
        assert len(lt) == n and set(lt["kind"]) <= {0, 1}
        if n > 2:
            assert float(F(1) / F(n)) != 1.0 / n  # the weight is inexact
        org = C.light_origins(n)
        assert {"general", "sphere_surface", "sphere_inside", "sphere_just_outside", "sphere_far", "sphere_centre"} <= set(org)
        assert ("quad_plane" in org) == (n > 1)
        spheres = [j for kind, j in C.LIGHT_LISTS[n] if kind == "s"]
        for k, j in enumerate(spheres):
            on = [_ratio(n, j, o) for o in org["sphere_surface"][3 * k:3 * k + 3]]
            # dist == r exactly, cos_max = 0 (the tiny sphere's origins round: on either side of its surface)
            assert all(r == 1 for r in on) if j != 2 else all(abs(float(r) - 1) < 1e-3 for r in on)
            assert all(_ratio(n, j, o) > 1 for o in org["sphere_inside"][3 * k:3 * k + 3])  # sqrt of a negative
            out3 = [_ratio(n, j, o) for o in org["sphere_just_outside"][3 * k:3 * k + 3]]
            # the origin's own rounding moves the tiny sphere's ratios either way; one at least is just below 1
            assert all(0.99 < r < 1.01 for r in out3) and any(r < 1 for r in out3)
            far3 = [_ratio(n, j, o) for o in org["sphere_far"][3 * k:3 * k + 3]]
            assert far3[0] < F(2.0 ** -23) and far3[1] < F(2.0 ** -25) and far3[2] < F(2.0 ** -25)  # 1 - x == 1
            assert _ratio(n, j, org["sphere_centre"][k]) == np.inf
        for a, b in zip(org.get("quad_plane", [])[0::5], org.get("quad_plane", [])[1::5]):
            assert 0.0005 < np.abs(a - b).max() <= 0.00101  # on the plane and within 0.001 of it
    # the largest ratio below 1: sphere 3 from (-r, -2^-11.5, 0)
    o = [x for x in C.light_origins(3)["sphere_just_outside"] if x[1] != 0 and x[0] < 0][0]
    assert _ratio(3, 3, o) == F(1) - F(2.0 ** -24)


def test_light_pdf_direction_classes_on_the_twin():
    total = 0
    for n in C.LIGHT_LISTS:
        lt, cases = C.light_records(n), C.lights_pdf_cases(n)
        names = {k.split("/")[1] for k in cases}
        assert {"sphere_centre", "sphere_tangent", "away", "special"} <= names
        assert ({"quad_interior", "quad_edges", "quad_corners", "quad_parallel"} <= names) == (n > 1)
        rows = C.rows(cases)
        total += len(rows)
        pdf = oracle.lights_pdf_f32(lt, rows)
        # every outcome occurs: a miss, a finite density, 1 / 0 from a far sphere, NaN from inside one
        assert (pdf == 0).any() and (np.isfinite(pdf) & (pdf > 0)).any() and np.isposinf(pdf).any() and np.isnan(pdf).any()
        assert np.isnan(rows[:, 3:]).any() and np.isinf(rows[:, 3:]).any() and (rows[:, 3:] == 0).all(axis=1).any()
        with np.errstate(invalid="ignore"):
            assert not (pdf < 0).any()
        inside = oracle.lights_pdf_f32(lt, cases["sphere_inside/sphere_centre"])
        assert np.isnan(inside).mean() > 0.5  # all but where the exit lies within tmin of a long direction
        far = oracle.lights_pdf_f32(lt, cases["sphere_far/sphere_centre"])
        assert np.isposinf(far).any()
        if n > 1:  # around the parallel cut some rows hit and some miss; the interiors hit from general origins
            par = oracle.lights_pdf_f32(lt, cases["general/quad_parallel"])
            assert (par == 0).any()
            assert not (oracle.lights_pdf_f32(lt, cases["general/quad_interior"]) == 0).any()
    # disc = 0 hits and one step outside misses sphere 4; the ray down -z hits sphere 1 as well in every row
    t = oracle.lights_pdf_f32(C.light_records(7), C.lights_pdf_cases(7)["tangent_exact/disc"])
    assert 0 < t[1] < min(t[0], t[2])
    print(f"LIGHTS_PDF: {total} rows")
    assert 2000 < total < 20000


def test_light_keys_reach_every_index_and_the_largest_draw():
    total = 0
    for n in C.LIGHT_LISTS:
        per, top = C.light_keys(n)
        lt = C.light_records(n)
        for idx, keys in per.items():
            assert len(keys) == 8
            for key in keys:
                u = F(oracle.path_stream(*key, 1)[0] >> 8) * F(2.0 ** -24)
                assert int(u * F(n)) == idx
        for key in top:
            assert oracle.path_stream(*key, 1)[0] >> 8 == 0xFFFFFF
            assert int(F(0xFFFFFF) * F(2.0 ** -24) * F(n)) == n - 1  # never n: the product rounds below n
        rows = C.rows(C.lights_random_cases(n))
        total += len(rows)
        d, draws = oracle.lights_random_f32(lt, rows)
        assert (draws == 3).all()  # the index, then two more, for a quad and for a sphere alike
        # the direction identifies the light drawn: from a general origin, the sampled direction hits list
        # entry idx alone among single-entry lists more often than not; here only that every entry's kind is met
        assert np.isnan(d).any() and np.isfinite(d).all(axis=1).any()
        # a far sphere: z = 1, the direction is the axis to the centre, of unit length
        far = C.lights_random_cases(n)["sphere_far"]
        fd, _ = oracle.lights_random_f32(lt, far)
        unit = np.abs(np.linalg.norm(fd.astype(np.float64), axis=1) - 1) < 1e-6
        assert unit.any()
    print(f"LIGHTS_RANDOM: {total} rows")
    assert 500 < total < 5000


def test_light_twins_against_float64():
    """lights_pdf's twin against the closed forms in float64 at well-conditioned rows: a lone sphere seen
    from outside, 1 / (2 pi (1 - cos_max)); a quad, dist^2 / (cosine area); weights 1 / n."""
    lt = C.light_records(1)
    (c, r), rng = C.LIGHT_SPHERES[0], np.random.default_rng(7)
    o = np.array(c) + rng.normal(size=(64, 3)) * 400
    o = o[np.linalg.norm(o - c, axis=1) > 2 * r]
    rows = np.concatenate([o, np.array(c) - o], axis=1)
    want = 1 / (2 * np.pi * (1 - np.sqrt(1 - r * r / ((o - c) ** 2).sum(axis=1))))
    got = oracle.lights_pdf_f32(lt, rows).astype(np.float64)
    assert np.abs(got / want - 1).max() < 1e-4
    lt2 = C.light_records(2)
    q, u, v = (np.array(x, np.float64) for x in C.LIGHT_QUADS[0])
    o = np.array([[278.0, 100.0, 278.0], [100.0, 300.0, 400.0]])
    tgt = q + 0.5 * u + 0.5 * v
    d = tgt - o
    dist2 = (d * d).sum(axis=1)
    cosine = np.abs(d[:, 1]) / np.sqrt(dist2)
    want = 0.5 * dist2 / (cosine * 130 * 105)
    got = oracle.lights_pdf_f32(lt2, np.concatenate([o, d], axis=1)).astype(np.float64)
    assert np.abs(got / want - 1).max() < 1e-5  # the sphere of list 2 is not on these rays
