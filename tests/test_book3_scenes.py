"""Conditions on the scenes of tests/book3_scenes.py, on the oracle and the launch plan alone (no
device): what tests/test_gpu_book3_scenes.py assumes of them when it renders the book-3 integrator
beyond the stock scene.

Every scene is free of ties: the oracle's own tree (TWIN), its walk of the sweep builder's tree in both
node formats and its walk of the binned builder's tree in both shapes give one frame and one ray count
("one frame" where the light pdf is NaN: the same NaN pixels and the same bits elsewhere). inside_light
has 20 or more NaN pixels and at most a tenth of the frame, and none without its inner spheres; every
other frame is finite. In multi_light the media, the free-standing light's orientation and the emissive
sphere's place on the light list each change the frame; far_light's floor sees cos_max == 1 exactly.
Every scene plans as kernel class 4 in both placements. A red GPU test is then the kernel's fault.
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from rustraytrace_amd import _lib
from rustraytrace_amd.render import build_bvh_binned

import book3_scenes as B
from test_book2_class_scenes import PLACEMENT_IDS, PLACEMENTS, place, plan_of
from test_launch_plan import check_f32_plan

# (generator, args): the five scenes, and the variants the GPU file renders at other sample counts
FRAMES = [(name, ()) for name in B.SCENES] + [("multi_light", (B.FIELD_SEED["multi_light"], 16)),
                                             ("multi_light", (B.FIELD_SEED["multi_light"], 1)),
                                             ("multi_light", (B.FIELD_SEED["multi_light"], 10)),
                                             ("inside_light", (B.FIELD_SEED["inside_light"], 81, 24))]
FRAME_IDS = [name + "".join(f"-{a}" for a in args[1:]) for name, args in FRAMES]


def frames_equal(a, b):
    """The same NaN pixels' channels and the same values everywhere else."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0.0, a), np.where(nb, 0.0, b))


@functools.lru_cache(maxsize=None)
def twin(name, *args, **kw):
    """(frame, rays) of the oracle's own books-structured tree; read-only."""
    frame, rays, _ = oracle.render(B.scene(name, *args, **kw), oracle.TWIN, threads=16)
    frame.setflags(write=False)
    return frame, rays


@functools.lru_cache(maxsize=None)
def kbvh(in_lds, name, *args):
    """(frame, rays) of the oracle's walk of the host tree of B.built(in_lds, name, *args); read-only."""
    scene, nodes, order, info = B.built(in_lds, name, *args)
    frame, rays, _ = oracle.render_kbvh(scene, nodes, order, info, threads=16)
    frame.setflags(write=False)
    return frame, rays


def check_class4(scene, info, order, in_lds, perlin_in_lds=None):
    q, plan = plan_of(scene, info, order)
    if perlin_in_lds is None:
        check_f32_plan(q, plan)
    assert plan["ok"] == 1 and plan["kernel_class"] == 4
    assert plan["scene_in_lds"] == (1 if in_lds is None else 0)
    assert info["node_stride"] == (80 if in_lds is None else 32)
    assert q["n_perlin"] == (1 if scene.perlin is not None else 0)
    assert plan["perlin_in_lds"] == (1 if scene.perlin is not None and perlin_in_lds is None else 0)
    return plan


# ---- tie-freedom and launch plans -------------------------------------------------------------------
@pytest.mark.parametrize("in_lds", PLACEMENTS, ids=PLACEMENT_IDS)
@pytest.mark.parametrize("name,args", FRAMES, ids=FRAME_IDS)
def test_trees_agree_and_plan_class_4(monkeypatch, name, args, in_lds):
    place(monkeypatch, in_lds)
    scene, nodes, order, info = B.built(in_lds, name, *args)
    assert scene.width <= 48 and scene.height <= 48 and scene.spp <= 81
    assert scene.spp == int(round(scene.spp ** 0.5)) ** 2
    assert scene.spp <= 16 or name == "inside_light"  # the chunked-sum frame alone has more
    check_class4(scene, info, order, in_lds)
    if scene.perlin is not None:
        place(monkeypatch, in_lds, "0")
        check_class4(scene, info, order, in_lds, "0")
        place(monkeypatch, in_lds)
    t, trays = twin(name, *args)
    k, krays = kbvh(in_lds, name, *args)
    assert frames_equal(k, t) and krays == trays
    assert np.isfinite(t).all() == (name != "inside_light")
    bn, border, binfo = build_bvh_binned(scene, *((3, 2.0, 80) if in_lds is None else (1, 2.0, 32)))
    check_class4(scene, binfo, border, in_lds)
    b, brays, _ = oracle.render_kbvh(scene, bn, border, binfo, threads=16)
    assert frames_equal(b, t) and brays == trays


def test_multi_light_scene_structure():
    sc = B.multi_light()
    assert (sc.width, sc.height, sc.spp, sc.max_depth) == (36, 36, 4, 10)
    assert sc.flags == _lib.FLAG_RAY_TIME | _lib.FLAG_BOOK3
    assert sc.lights["kind"].tolist() == [0, 0, 1, 1, 1] and len(sc.lights) % 2 == 1
    assert len(sc.media) == 2 and sorted(sc.media["boundary_kind"].tolist()) == [0, 1]
    kinds = sc.materials["kind"][sc.spheres["material_index"]]
    field = kinds[3:3 + B.N_FIELD]
    assert B.N_FIELD >= 40 and [int(k) for k in field[:4]] == [0, 1, 2, 5]
    assert np.count_nonzero(sc.motion[:, 1]) == B.N_FIELD // 4
    assert (kinds == 4).sum() == 1  # the emissive sphere, in the world
    emissive = sc.spheres["center_radius"][kinds == 4][0]
    assert any(np.array_equal(emissive, a) for a in sc.lights["a"][sc.lights["kind"] == 1])  # and on the list
    # the field keeps clear of every light sphere, at both ends of a motion
    cr = sc.spheres["center_radius"][3:3 + B.N_FIELD].astype(np.float64)
    for (c, r) in B.LIGHT_SPHERES:
        for dy in (0.0, 15.0):
            d = np.linalg.norm(cr[:, :3] + (0.0, dy, 0.0) - np.array(c), axis=1)
            assert (d >= r + cr[:, 3] + 20.0 - 1e-3)[(sc.motion[3:3 + B.N_FIELD, 1] != 0) | (dy == 0.0)].all()
    noisy = B.multi_light_noise()
    assert len(noisy.perlin) == 1 and (noisy.materials["kind"] == 6).sum() == 1
    assert (B.far_light().lights["kind"].tolist(), B.one_light_sphere().lights["kind"].tolist()) == ([0, 1], [1])


# ---- NaN paths --------------------------------------------------------------------------------------
def test_inside_light_nan_pixels():
    frame, _ = twin("inside_light")
    n = int(B.nan_mask(frame).sum())
    print(f"inside_light: {n} NaN pixels of {frame.shape[0] * frame.shape[1]}")
    assert 20 <= n <= frame.shape[0] * frame.shape[1] // 10
    bare, _ = twin("inside_light", inner=False)
    assert np.isfinite(bare).all()
    assert frames_equal(bare, twin("multi_light")[0])  # the same scene
    many, _ = twin("inside_light", B.FIELD_SEED["inside_light"], 81, 24)
    assert B.nan_mask(many).sum() >= 20 and not B.nan_mask(many).all()


# ---- each feature of multi_light changes the frame ------------------------------------------------
@pytest.mark.parametrize("variant", ["media", "free_flipped", "emissive_listed"])
def test_multi_light_features_are_seen(variant):
    full, _ = twin("multi_light")
    kw = {variant: variant == "free_flipped"}  # media=False, free_flipped=True, emissive_listed=False
    other, _ = twin("multi_light", **kw)
    assert np.isfinite(other).all()
    n = int((full != other).any(-1).sum())
    print(f"multi_light against {kw}: {n} pixels differ")
    assert n >= 20  # more than a stray pixel


def test_noise_material_is_seen():
    assert int((twin("multi_light_noise")[0] != twin("multi_light")[0]).any(-1).sum()) >= 4


# ---- far_light: cos_max == 1 --------------------------------------------------------------------------
def cos_max_is_one(sphere_light, points):
    """Whether the f32 light pdf of the lone sphere, seen from each point, is 1 / 0: where the pdf's root
    exists the pdf is 1 / (2 pi (1 - cos_max)), +inf exactly when cos_max == 1, whatever the direction. At
    r^2 / d^2 below an ulp the root's discriminant h^2 - a c cancels to either sign, so each point looks
    along the axis to the centre in eight lengths (eight roundings): some find the root."""
    pts = np.asarray(points, np.float32)
    axis = sphere_light["a"][0, :3][None, :] - pts
    pdf = np.stack([oracle.lights_pdf_f32(sphere_light, np.concatenate([pts, axis * np.float32(s)], axis=1))
                    for s in (1.0, 0.75, 0.6, 1.3, 0.37, 1.9, 0.11, 2.7)])
    assert ((pdf == 0) | np.isposinf(pdf) | (pdf > 0)).all()
    return np.isposinf(pdf).any(axis=0) & ~(np.isfinite(pdf) & (pdf > 0)).any(axis=0)


def test_far_light_floor_sees_cos_max_one():
    sc = B.far_light()
    sphere = sc.lights[sc.lights["kind"] == 1]
    assert len(sphere) == 1 and len(sc.lights) == 2 and sphere["a"][0, 3] == np.float32(B.FAR[1])
    x, z = np.meshgrid(np.linspace(1.0, 554.0, 48), np.linspace(1.0, 554.0, 48))
    floor = np.stack([x.ravel(), np.zeros(x.size), z.ravel()], axis=1)
    one = cos_max_is_one(sphere, floor)
    print(f"far_light: cos_max == 1 from {int(one.sum())} of {len(floor)} floor points")
    assert one.mean() > 0.9  # "more than half": all of them, but for a point no length finds the root from
    near = np.array(B.FAR[0]) + [[0.0, -1.0, 0.0], [0.0, -50.0, 0.0]]  # and not from close by
    assert not cos_max_is_one(sphere, near).any()
    # with both lights the floor's pdf towards the sphere is still 1 / 0
    rows = np.concatenate([floor, np.array(B.FAR[0]) - floor], axis=1)
    both = oracle.lights_pdf_f32(sc.lights, rows)
    assert np.isposinf(both).mean() > 0.3 and not np.isnan(both).any()  # about half: the root's cancellation


# ---- BOOKS against TWIN --------------------------------------------------------------------------------
def test_multi_light_books_vs_twin_statistical():
    """The bound and the size of tests/test_book3.py's test on the stock scene (40 x 40 x 64, 1 %)."""
    sc = B.multi_light(B.FIELD_SEED["multi_light"], 64, 40)
    t, rt, _ = oracle.render(sc, oracle.TWIN, threads=16)
    b, rb, _ = oracle.render(sc, oracle.BOOKS, threads=16)
    assert np.isfinite(t).all() and np.isfinite(b).all()
    dm, dr = abs(t[..., :3].mean() - b[..., :3].mean()) / b[..., :3].mean(), abs(rt - rb) / rb
    print(f"multi_light BOOKS vs TWIN: mean radiance differs by {dm:.2e}, rays by {dr:.2e}")
    assert dm < 0.01 and dr < 0.01
