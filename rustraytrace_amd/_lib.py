"""ctypes binding of librrt_hip.so (include/rrt_hip.h).

This is the Python twin of the cgo/Rust `extern "C"` shim a reference maintainer would add
(see INTEGRATION.md): plain pointers and sizes, numpy arrays for the #[repr(C)] structs of
src/gpu/mod.rs:13-42. There is no fallback: if the shared object is missing or fails to
load, every entry raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRT_LIB_PATH") or os.path.join(PKG_DIR, "librrt_hip.so")  # override: experiments only

# ---- #[repr(C)] layouts (gpu/mod.rs:13-42) as numpy dtypes ------------------------------------
CAMERA_DTYPE = np.dtype(
    [
        ("origin", "<f4", 4),
        ("pixel00", "<f4", 4),
        ("pixel_delta_u", "<f4", 4),
        ("pixel_delta_v", "<f4", 4),
        ("u", "<f4", 4),
        ("v", "<f4", 4),
        ("background", "<f4", 4),
        ("params_f", "<f4", 4),
        ("params_u", "<u4", 4),
    ]
)
SPHERE_DTYPE = np.dtype([("center_radius", "<f4", 4), ("material_index", "<u4"), ("_pad", "<u4", 3)])
MATERIAL_DTYPE = np.dtype([("albedo_fuzz", "<f4", 4), ("kind", "<u4"), ("ref_idx", "<f4"), ("_pad", "<u4", 2)])
assert CAMERA_DTYPE.itemsize == 144 and SPHERE_DTYPE.itemsize == 32 and MATERIAL_DTYPE.itemsize == 32

MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_TEXTURED_LAMBERTIAN, MAT_DIFFUSE_LIGHT = range(5)
FLAG_RAY_TIME = 0x1
FLAG_QUIET = 0x2
FLAG_BOOK3 = 0x4
FLAG_F64 = 0x8  # the books path's f64 arithmetic (include/rrt_hip.h RRT_FLAG_F64)
FLAG_DEVICE_BVH = 0x10  # scene creation builds the BVH on the device (RRT_FLAG_DEVICE_BVH)
FLAG_FAST_BVH = 0x40  # the device builds the BVH by the LBVH builder (RRT_FLAG_FAST_BVH; implies FLAG_DEVICE_BVH)
FLAG_F64_BOOK2 = 0x20  # the f64 books path for moving spheres, quads, checker textures (RRT_FLAG_F64_BOOK2)

# Every symbol include/rrt_hip.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "rrt_hip_render",
    "rrt_hip_last_error",
    "rrt_hip_abi_version",
    "rrt_accum_chunk",
    "rrt_scene_create",
    "rrt_scene_destroy",
    "rrt_tile_rows",
    "rrt_tile_row_index",
    "rrt_render_tile_async",
    "rrt_scene_read_counters",
    "rrt_scene_reset_counters",
    "rrt_scene_count_work",
    "rrt_scene_bvh_info",
    "rrt_build_bvh",
    "rrt_build_in_one_weekend_scene",
    "rrt_make_camera",
    "rrt_apply_overrides",
    "rrt_write_ppm_from_accum",
    "rrt_format_ppm_from_accum",
    "rrt_quantize_accum",
    "rrt_hip_render_rgb8",
    "rrt_hip_render_rgb8_ex",
    "rrt_quantize_accum_books",
    "rrt_quantize_accum_async",
    "rrt_format_pnm_from_rgb8",
    "rrt_write_pnm_from_rgb8",
    "rrt_hip_render_ex",
    "rrt_scene_create_ex",
    "rrt_build_bvh_ex",
    "rrt_build_bvh_binned",
    "rrt_scene_read_bvh",
    "rrt_build_next_week_scene",
    "rrt_build_rest_of_your_life_scene",
    "rrt_flatten_scene",
    "rrt_device_count",
    "rrt_hip_render_f64",
    "rrt_render_tile_f64_async",
    "rrt_quantize_accum_books_f64",
    "rrt_quantize_accum_books_async",
    "rrt_quantize_accum_books_f64_async",
    "rrt_hip_render_f64_rgb8",
    "rrt_hip_render_f64_ex",
    "rrt_hip_render_f64_rgb8_ex",
    "rrt_testing_device_wrap",
    "rrt_testing_f64_layout",
    "rrt_testing_lds_node_link",
    "rrt_testing_launch_plan",
    "rrt_testing_recip_check",
    "rrt_testing_trig32_check",
    "rrt_testing_sqrt64_check",
    "rrt_testing_device_ops",
    "rrt_testing_div_check",
    "rrt_testing_device_ops64",
    "rrt_scene_set_camera",
    "rrt_scene_update_spheres",
    "rrt_testing_sphere_boxes",
    "rrt_testing_scene_read_table",
    "rrt_testing_scene_update_stats",
    "rrt_scene_refit_spheres",
    "rrt_scene_tree_cost",
    "rrt_refit_bvh_binned",
    "rrt_testing_scene_refit_stats",
    "rrt_testing_refit_form",
    "rrt_scene_update_geometry",
    "rrt_scene_refit_geometry",
    "rrt_refit_bvh_binned_ex",
    "rrt_testing_quad_records",
    "rrt_scene_update_world",
    "rrt_scene_refit_world",
    "rrt_refit_bvh_binned_world",
    "rrt_testing_medium_records",
    "rrt_build_bvh_lbvh",
    "rrt_refit_bvh_lbvh_world",
    "rrt_scene_set_builder",
    "rrt_testing_scene_build_stats",
    "rrt_testing_lbvh_form",
    "rrt_scene_query_async",
    "rrt_scene_query",
    "rrt_scene_primary_hits_async",
    "rrt_scene_surface_async",
    "rrt_scene_surface",
    "rrt_scene_primary_surface_async",
    "rrt_testing_scene_fail_update",
)

# == RrtRay / RrtHit (include/rrt_hip.h): a query ray and its answer
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("tmax", "<f4"), ("d", "<f4", 3), ("time", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<u4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 8
NO_PRIM = 0xFFFFFFFF  # RRT_NO_PRIM
QUERY_MODES = {"closest": 0, "any": 1}  # RRT_QUERY_CLOSEST, RRT_QUERY_ANY
# == RrtSurface (include/rrt_hip.h): the HitRecord of a closest hit
SURFACE_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4"), ("normal", "<f4", 3), ("prim", "<u4"), ("albedo", "<f4", 3),
                          ("kind", "<u4"), ("uv", "<f4", 2), ("front_face", "<u4"), ("_pad", "<u4")])
assert SURFACE_DTYPE.itemsize == 64
SURFACE_MISS = 0xFFFFFFFF  # RRT_SURFACE_MISS

# == RrtSceneTable (include/rrt_hip.h, test support): table -> (code, row dtype)
SCENE_TABLES = {
    "boxes": (0, np.dtype("<f8")), "prim_cr": (1, np.dtype("<f4")), "prim_mtl": (2, np.dtype("<u4")),
    "prim_motion": (3, np.dtype("<f4")), "prim_inv_r64": (4, np.dtype("<f8")), "prim_diel64": (5, np.dtype("<f8")),
}


# The tables rrt_scene_update_geometry re-forms beyond SCENE_TABLES (RrtSceneTable 6-9), in source
# order: table -> (code, row dtype). GQUAD_DTYPE / GQUAD64_DTYPE / GLIGHT_DTYPE give their records.
SCENE_GEOMETRY_TABLES = {
    "gquads": (6, np.dtype("<f4")), "gquads64": (7, np.dtype("<f8")), "quad_rows": (8, np.dtype("<f4")),
    "glights": (9, np.dtype("<u4")),
}
GQUAD_DTYPE = np.dtype([("q", "<f4", 4), ("u", "<f4", 4), ("v", "<f4", 4), ("n", "<f4", 4), ("w", "<f4", 4)])  # q[3] = D
GQUAD64_DTYPE = np.dtype([("q", "<f8", 3), ("u", "<f8", 3), ("v", "<f8", 3), ("n", "<f8", 3), ("w", "<f8", 3), ("D", "<f8")])
GLIGHT_DTYPE = np.dtype([("sphere", "<f4", 4), ("kind", "<u4"), ("quad", "<u4"), ("area", "<f4"), ("_pad", "<u4")])
assert GQUAD_DTYPE.itemsize == 80 and GQUAD64_DTYPE.itemsize == 128 and GLIGHT_DTYPE.itemsize == 32


# The table rrt_scene_update_world re-forms beyond those (RrtSceneTable 10), in source order.
# GMEDIUM_DTYPE gives its records.
SCENE_MEDIA_TABLES = {"gmedia": (10, np.dtype("<u4"))}
GMEDIUM_DTYPE = np.dtype([("sphere", "<f4", 4), ("kind", "<u4"), ("first", "<u4"), ("count", "<u4"),
                          ("neg_inv_density", "<f4")])
assert GMEDIUM_DTYPE.itemsize == 32


class RrtSceneMedia(ctypes.Structure):  # include/rrt_hip.h
    _fields_ = [("media", c_void_p), ("n_media", c_uint32), ("n_boundary_quads", c_uint32), ("boundary_quads", c_void_p)]


class RrtSceneGeometry(ctypes.Structure):  # include/rrt_hip.h
    _fields_ = [("spheres", c_void_p), ("n_spheres", c_uint32), ("sphere_motion", c_void_p), ("quads", c_void_p),
                ("n_quads", c_uint32), ("lights", c_void_p), ("n_lights", c_uint32)]


class RrtSceneUpdateStats(ctypes.Structure):  # include/rrt_hip.h, test support
    _fields_ = [("updates", c_uint64), ("last_allocations", c_uint64), ("last_levels", c_uint64)]


class RrtSceneRefitStats(ctypes.Structure):  # include/rrt_hip.h, test support
    _fields_ = [("refits", c_uint64), ("last_allocations", c_uint64), ("last_launches", c_uint64), ("last_form", c_uint64)]


class RrtSceneBuildStats(ctypes.Structure):  # include/rrt_hip.h, test support
    _fields_ = [("builder", c_uint64), ("launches", c_uint64), ("blocking_reads", c_uint64), ("form", c_uint64),
                ("shape_attempts", c_uint64)]


BUILDERS = {"binned": 0, "lbvh": 1}  # RRT_BUILDER_*


class RrtTreeCost(ctypes.Structure):  # include/rrt_hip.h
    _fields_ = [("sah", c_double), ("sah_at_build", c_double), ("refits_since_build", c_uint64)]


def refit_form(form: int) -> None:
    """rrt_testing_refit_form (test support): force the refit's per-level launches (0) or its single
    workgroup (1); -1 restores the automatic choice."""
    check(load().rrt_testing_refit_form(int(form)))

def lbvh_form(form: int) -> None:
    """rrt_testing_lbvh_form (test support): force the fast builder's launch-per-phase form (0) or its
    single workgroup (1); -1 restores the automatic choice."""
    check(load().rrt_testing_lbvh_form(int(form)))

# == RrtDeviceOp (include/rrt_hip.h, test support): op -> (code, f32 columns in, 32-bit words out)
DEVICE_OPS = {
    "SIN": (0, 1, 1), "COS": (1, 1, 1), "LOG": (2, 1, 1), "ACOS": (3, 1, 1), "ATAN2": (4, 2, 1),
    "DIV_A": (5, 2, 4), "DIV_CONST": (6, 1, 4), "FLOOR_I32": (7, 1, 1), "CHECKER": (8, 4, 1),
    "PERLIN": (9, 3, 8), "VEC": (10, 9, 13), "QUAD": (11, 9, 2), "SPHERE": (12, 11, 13),
    "LIGHTS_PDF": (13, 6, 1), "LIGHTS_RANDOM": (14, 6, 4), "SLOPES": (15, 6, 13),
}

# == RrtDeviceOp64 (include/rrt_hip.h, test support): op -> (code, f64 columns in, 64-bit words out)
DEVICE_OPS64 = {
    "ACOS64": (0, 1, 1), "ATAN2_64": (1, 2, 1), "DIV_A64": (2, 2, 3), "DIV_CONST64": (3, 1, 4), "SQRT64": (4, 1, 1),
    "AS_I32": (5, 1, 1), "ATT64": (6, 2, 4), "VEC64": (7, 9, 11), "TEXEL64": (8, 5, 6), "SPHERE64": (9, 11, 6),
    "QUAD64": (10, 9, 2), "CHECKER64": (11, 4, 1),
}


class RrtTexture(ctypes.Structure):
    _fields_ = [("rgb8", POINTER(c_uint8)), ("width", c_int32), ("height", c_int32)]


# == RrtPerlin (include/rrt_hip.h): 256 x float4 random vectors + 3 x 256 u16 permutations (+pad)
PERLIN_DTYPE = np.dtype([("randvec", "<f4", (256, 4)), ("perm_x", "<u2", 256), ("perm_y", "<u2", 256),
                         ("perm_z", "<u2", 256), ("_pad", "<u2", 256)])


# == RrtQuad (include/rrt_hip.h): corner q, edges u, v (xyz + pad), material index; 64 B
QUAD_DTYPE = np.dtype([("q", "<f4", 4), ("u", "<f4", 4), ("v", "<f4", 4), ("material_index", "<u4"),
                       ("_pad", "<u4", 3)])


# == RrtLight (include/rrt_hip.h): book-3 MIS light, kind 0 quad (a = q, u, v) / 1 sphere (a = c, r); 64 B
LIGHT_DTYPE = np.dtype([("kind", "<u4"), ("_pad", "<u4", 3), ("a", "<f4", 4), ("u", "<f4", 4), ("v", "<f4", 4)])

# == RrtMedium (include/rrt_hip.h): boundary sphere or quad range, phase material, density; 48 B
MEDIUM_DTYPE = np.dtype([("sphere", "<f4", 4), ("boundary_kind", "<u4"), ("first", "<u4"), ("count", "<u4"),
                         ("material_index", "<u4"), ("density", "<f4"), ("_pad", "<u4", 3)])


class RrtSceneExt(ctypes.Structure):
    _fields_ = [("sphere_motion", c_void_p), ("perlin", c_void_p), ("n_perlin", c_uint32), ("n_quads", c_uint32),
                ("quads", c_void_p), ("media", c_void_p), ("n_media", c_uint32), ("n_boundary_quads", c_uint32),
                ("boundary_quads", c_void_p), ("lights", c_void_p), ("n_lights", c_uint32), ("_pad", c_uint32)]


class RrtBookScene(ctypes.Structure):
    _fields_ = [("camera", ctypes.c_uint8 * 144), ("spheres", c_void_p), ("sphere_motion", c_void_p),
                ("materials", c_void_p), ("quads", c_void_p), ("perlin", c_void_p), ("media", c_void_p),
                ("boundary_quads", c_void_p), ("lights", c_void_p)] + [
        (f, c_uint32) for f in ("sphere_cap", "n_spheres", "material_cap", "n_materials", "quad_cap", "n_quads",
                                "perlin_cap", "n_perlin", "media_cap", "n_media", "boundary_quad_cap",
                                "n_boundary_quads", "light_cap", "n_lights", "uses_texture0", "flags")]


# == RrtSceneNode (include/rrt_hip.h): one node of the books' object graph, f64 payload; 112 B
NODE_DTYPE = np.dtype([("kind", "<u4"), ("material", "<u4"), ("first", "<u4"), ("count", "<u4"),
                       ("a", "<f8", 4), ("b", "<f8", 4), ("c", "<f8", 4)])
NODE_SPHERE, NODE_QUAD, NODE_LIST, NODE_BVH, NODE_TRANSLATE, NODE_ROTATE_Y, NODE_CONSTANT_MEDIUM = range(7)


class RrtOverrides(ctypes.Structure):
    _fields_ = [
        ("has_aspect_ratio", c_int32), ("aspect_ratio", c_double),
        ("has_image_width", c_int32), ("image_width", c_int32),
        ("has_samples_per_pixel", c_int32), ("samples_per_pixel", c_int32),
        ("has_max_depth", c_int32), ("max_depth", c_int32),
        ("has_vfov", c_int32), ("vfov", c_double),
        ("has_lookfrom", c_int32), ("lookfrom", c_double * 3),
        ("has_lookat", c_int32), ("lookat", c_double * 3),
        ("has_vup", c_int32), ("vup", c_double * 3),
        ("has_defocus_angle", c_int32), ("defocus_angle", c_double),
        ("has_focus_dist", c_int32), ("focus_dist", c_double),
        ("has_background", c_int32), ("background", c_double * 3),
    ]


class RrtTile(ctypes.Structure):
    _fields_ = [
        ("band_rows", c_uint32),
        ("rank", c_uint32),
        ("n_ranks", c_uint32),
        ("sample_begin", c_uint32),
        ("sample_end", c_uint32),
    ]


class RrtCounters(ctypes.Structure):
    _fields_ = [
        ("rays", c_uint64),
        ("paths", c_uint64),
        ("node_visits", c_uint64),
        ("box_tests", c_uint64),
        ("sphere_tests", c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RrtBvhInfo(ctypes.Structure):
    _fields_ = [
        ("n_nodes", c_uint32),
        ("n_leaves", c_uint32),
        ("max_depth", c_uint32),
        ("max_leaf_size", c_uint32),
        ("node_bytes", c_uint64),
        ("prim_bytes", c_uint64),
        ("width", c_uint32),
        ("max_leaf_param", c_uint32),
        ("node_stride", c_uint32),
        ("n_unbounded", c_uint32),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if not k.startswith("_")}


class RrtLaunchPlanQuery(ctypes.Structure):  # include/rrt_hip.h, test support
    _fields_ = [(f, c_uint32) for f in ("n_nodes", "n_prims", "stack_depth", "node_stride", "book", "specular",
                                        "image_tex", "n_perlin", "n_media", "n_quads", "f64", "bvh4_in_lds",
                                        "min_waves", "global_waves", "f64_book2", "_pad")]


class RrtLaunchPlan(ctypes.Structure):  # include/rrt_hip.h, test support
    _fields_ = [("ok", c_uint32), ("f64", c_uint32), ("kernel_class", c_int32), ("shape", c_int32)] + [
        (f, c_uint32) for f in ("stack_bytes", "threads", "waves", "waves_noise_free", "scene_in_lds", "perlin_in_lds",
                                "inv_r_in_lds", "rec32_in_lds", "raise_limit", "_pad")] + [("lds_bytes", c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if not k.startswith("_")}


def launch_plan(**query) -> dict:
    """rrt_testing_launch_plan (test support): the launch shape for a scene given by its counts
    (RrtLaunchPlanQuery fields as keywords); {"ok": 0} when scene creation would refuse it."""
    q, out = RrtLaunchPlanQuery(), RrtLaunchPlan()
    for k, v in query.items():
        if not hasattr(q, k) or k.startswith("_"):
            raise KeyError(f"unknown launch-plan query field {k!r}")
        setattr(q, k, int(v))
    check(load().rrt_testing_launch_plan(ctypes.byref(q), ctypes.byref(out)))
    return out.as_dict()


def device_ops(op: str, rows, quads=None, perlin=None, scale=0.0, lights=None) -> np.ndarray:
    """rrt_testing_device_ops (test support): the f32 kernel's building block `op` (a DEVICE_OPS
    name) on each row of `rows` (float32, n x columns in); returns the n x words-out results as
    uint32 (view as float32 where the op returns floats). quads: QUAD_DTYPE records for QUAD;
    perlin: one PERLIN_DTYPE table and `scale` for PERLIN; lights: LIGHT_DTYPE records for LIGHTS_PDF
    and LIGHTS_RANDOM."""
    code, cin, cout = DEVICE_OPS[op]
    x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, cin)
    out = np.zeros((len(x), cout), dtype=np.uint32)
    aux = None
    if op == "QUAD":
        q = np.ascontiguousarray(quads, dtype=QUAD_DTYPE)
        aux = np.zeros(16 + q.nbytes, dtype=np.uint8)
        aux[:4] = np.frombuffer(np.uint32(len(q)).tobytes(), dtype=np.uint8)
        aux[16:] = np.frombuffer(q.tobytes(), dtype=np.uint8)
    elif op in ("LIGHTS_PDF", "LIGHTS_RANDOM"):
        lt = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        aux = np.zeros(16 + lt.nbytes, dtype=np.uint8)
        aux[:4] = np.frombuffer(np.uint32(len(lt)).tobytes(), dtype=np.uint8)
        aux[16:] = np.frombuffer(lt.tobytes(), dtype=np.uint8)
    elif op == "PERLIN":
        t = np.ascontiguousarray(perlin, dtype=PERLIN_DTYPE).reshape(-1)[:1]
        aux = np.frombuffer(t.tobytes() + np.float32(scale).tobytes(), dtype=np.uint8).copy()
    check(load().rrt_testing_device_ops(code, len(x), ptr(x), ptr(out), ptr(aux)))
    return out


def device_ops64(op: str, rows, quads=None) -> np.ndarray:
    """rrt_testing_device_ops64 (test support): the f64 books kernel's building block `op` (a
    DEVICE_OPS64 name) on each row of `rows` (float64, n x columns in); returns the n x words-out
    results as uint64 (view as float64 where the op returns doubles). Row i runs on lane i % 64 of
    wave i / 64. quads: QUAD_DTYPE records for QUAD64."""
    code, cin, cout = DEVICE_OPS64[op]
    x = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, cin)
    out = np.zeros((len(x), cout), dtype=np.uint64)
    aux = None
    if op == "QUAD64":  # the aux layout of device_ops' QUAD
        q = np.ascontiguousarray(quads, dtype=QUAD_DTYPE)
        aux = np.zeros(16 + q.nbytes, dtype=np.uint8)
        aux[:4] = np.frombuffer(np.uint32(len(q)).tobytes(), dtype=np.uint8)
        aux[16:] = np.frombuffer(q.tobytes(), dtype=np.uint8)
    check(load().rrt_testing_device_ops64(code, len(x), ptr(x), ptr(out), ptr(aux)))
    return out


def sphere_boxes(spheres, motion=None) -> np.ndarray:
    """rrt_testing_sphere_boxes (test support): each sphere's padded f64 box, (n, 6) float64 (min xyz,
    max xyz), by the host compilation of the function rrt_scene_update_spheres runs on the device."""
    sp = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    m = None if motion is None else np.ascontiguousarray(motion, dtype=np.float32).reshape(len(sp), 4)
    out = np.zeros((len(sp), 6), dtype=np.float64)
    check(load().rrt_testing_sphere_boxes(ptr(sp), len(sp), ptr(m), ptr(out)))
    return out


def quad_records(quads):
    """rrt_testing_quad_records (test support): what each quad contributes to a scene, by the host
    compilation of the functions rrt_scene_update_geometry runs on the device: (boxes (n, 6) float64 as
    min xyz, max xyz; GQUAD_DTYPE records; GQUAD64_DTYPE records)."""
    q = np.ascontiguousarray(quads, dtype=QUAD_DTYPE)
    boxes = np.zeros((len(q), 6), dtype=np.float64)
    g32, g64 = np.zeros(len(q), dtype=GQUAD_DTYPE), np.zeros(len(q), dtype=GQUAD64_DTYPE)
    check(load().rrt_testing_quad_records(ptr(q), len(q), ptr(boxes), ptr(g32), ptr(g64)))
    return boxes, g32, g64


def medium_records(media, boundary_quads=None, n_quads=0):
    """rrt_testing_medium_records (test support): what each constant medium contributes to a scene, by the
    host compilation of the functions rrt_scene_update_world runs on the device: (boxes (n, 6) float64 as
    min xyz, max xyz; GMEDIUM_DTYPE records with first = n_quads + the medium's first)."""
    md = np.ascontiguousarray(media, dtype=MEDIUM_DTYPE)
    bq = None if boundary_quads is None else np.ascontiguousarray(boundary_quads, dtype=QUAD_DTYPE)
    boxes = np.zeros((len(md), 6), dtype=np.float64)
    g = np.zeros(len(md), dtype=GMEDIUM_DTYPE)
    check(load().rrt_testing_medium_records(ptr(md), len(md), ptr(bq), 0 if bq is None else len(bq), int(n_quads),
                                            ptr(boxes), ptr(g)))
    return boxes, g


def div_check(a_values) -> list:
    """rrt_testing_div_check (test support): the eight counters for the divisors a_values."""
    a = np.ascontiguousarray(a_values, dtype=np.float32).ravel()
    out = (ctypes.c_uint64 * 8)(*([7] * 8))
    check(load().rrt_testing_div_check(ptr(a), len(a), out))
    return [int(v) for v in out]


class RrtError(RuntimeError):
    """A non-zero return of the C-ABI (the Rust shim's Err(rrt_hip_last_error()))."""

    def __init__(self, code: int, message: str):
        super().__init__(f"rrt error {code}: {message}")
        self.code = code


_LIB = None


def load() -> ctypes.CDLL:
    """Load librrt_hip.so from the package directory; raise if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the HIP backend)"
        )
    # One HIP runtime per process: torch bundles its own libamdhip64 (soname libamdhip64.so.7)
    # which satisfies our DT_NEEDED when it is loaded first. Loaded the other way round,
    # torch would map a second runtime and lose the device ("One runtime").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    P = c_void_p
    sig = {
        "rrt_hip_render": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32, c_uint32, P]),
        "rrt_hip_last_error": (c_char_p, []),
        "rrt_hip_abi_version": (c_uint32, []),
        "rrt_accum_chunk": (c_uint32, []),
        "rrt_scene_create": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_int32, P]),
        "rrt_scene_destroy": (c_int32, [P]),
        "rrt_tile_rows": (c_int32, [c_uint32, P, P]),
        "rrt_tile_row_index": (c_int32, [c_uint32, P, c_uint32, P]),
        "rrt_render_tile_async": (c_int32, [P, P, P, P]),
        "rrt_scene_read_counters": (c_int32, [P, P]),
        "rrt_scene_reset_counters": (c_int32, [P]),
        "rrt_scene_count_work": (c_int32, [P, P, P]),
        "rrt_scene_bvh_info": (c_int32, [P, P]),
        "rrt_build_bvh": (c_int32, [P, c_uint32, c_uint32, c_uint32, P, c_size_t, P, P]),
        "rrt_build_in_one_weekend_scene": (c_int32, [P, c_uint64, c_int32, P, P, P, c_uint32, P]),
        "rrt_make_camera": (
            c_int32,
            [c_double, c_int32, c_int32, c_int32, c_double, P, P, P, c_double, c_double, P, c_uint32, c_uint32, P],
        ),
        "rrt_apply_overrides": (c_int32, [P, c_int32] + [P] * 12),
        "rrt_write_ppm_from_accum": (c_int32, [c_uint32, c_uint32, P, c_uint32, c_char_p]),
        "rrt_format_ppm_from_accum": (c_int32, [c_uint32, c_uint32, P, c_uint32, P, c_size_t, P]),
        "rrt_quantize_accum": (c_int32, [c_uint32, c_uint32, P, c_uint32, P]),
        "rrt_quantize_accum_books": (c_int32, [c_uint32, c_uint32, P, c_uint32, P]),
        "rrt_hip_render_rgb8": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32, c_uint32, P]),
        "rrt_hip_render_rgb8_ex": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32,
                                             P]),
        "rrt_quantize_accum_async": (c_int32, [c_uint32, P, c_uint32, P, P]),
        "rrt_format_pnm_from_rgb8": (c_int32, [c_uint32, c_uint32, P, c_int32, P, c_size_t, P]),
        "rrt_write_pnm_from_rgb8": (c_int32, [c_uint32, c_uint32, P, c_int32, c_char_p]),
        "rrt_hip_render_ex": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32, P]),
        "rrt_scene_create_ex": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, P, c_uint32, c_int32, P]),
        "rrt_build_bvh_ex": (c_int32, [P, c_uint32, P, c_uint32, c_uint32, P, c_size_t, P, P]),
        "rrt_build_bvh_binned": (c_int32, [P, c_uint32, P, c_uint32, c_double, c_uint32, P, c_size_t, P, P]),
        "rrt_scene_read_bvh": (c_int32, [P, P, c_size_t, P]),
        "rrt_build_next_week_scene": (c_int32, [c_int32, P, c_uint64, P]),
        "rrt_build_rest_of_your_life_scene": (c_int32, [P, c_uint64, P]),
        "rrt_flatten_scene": (c_int32, [P, c_uint32, P, c_uint32, c_uint32, P]),
        "rrt_device_count": (c_int32, [P]),
        "rrt_hip_render_f64": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32, c_uint32, P]),
        "rrt_render_tile_f64_async": (c_int32, [P, P, P, P]),
        "rrt_quantize_accum_books_f64": (c_int32, [c_uint32, c_uint32, P, c_uint32, P]),
        "rrt_quantize_accum_books_async": (c_int32, [c_uint32, P, c_uint32, P, P]),
        "rrt_quantize_accum_books_f64_async": (c_int32, [c_uint32, P, c_uint32, P, P]),
        "rrt_hip_render_f64_ex": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32, P]),
        "rrt_hip_render_f64_rgb8_ex": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32,
                                                 P]),
        "rrt_hip_render_f64_rgb8": (c_int32, [P, P, c_uint32, P, c_uint32, P, c_uint32, c_uint32, c_uint32, c_uint32,
                                              P]),
        "rrt_testing_device_wrap": (None, [c_int32]),
        "rrt_testing_f64_layout": (None, [c_int32]),
        "rrt_testing_lds_node_link": (c_uint32, [c_uint32]),
        "rrt_testing_launch_plan": (c_int32, [P, P]),
        "rrt_testing_recip_check": (c_int32, [P]),
        "rrt_testing_trig32_check": (c_int32, [P]),
        "rrt_testing_sqrt64_check": (c_int32, [P]),
        "rrt_testing_device_ops": (c_int32, [c_uint32, c_uint32, P, P, P]),
        "rrt_testing_device_ops64": (c_int32, [c_uint32, c_uint32, P, P, P]),
        "rrt_testing_div_check": (c_int32, [P, c_uint32, P]),
        "rrt_scene_set_camera": (c_int32, [P, P]),
        "rrt_scene_update_spheres": (c_int32, [P, P, c_uint32, P, P]),
        "rrt_testing_sphere_boxes": (c_int32, [P, c_uint32, P, P]),
        "rrt_testing_scene_read_table": (c_int32, [P, c_uint32, P, c_size_t, P]),
        "rrt_testing_scene_update_stats": (c_int32, [P, P]),
        "rrt_scene_refit_spheres": (c_int32, [P, P, c_uint32, P, P]),
        "rrt_scene_tree_cost": (c_int32, [P, P]),
        "rrt_refit_bvh_binned": (c_int32, [P, c_uint32, P, c_uint32, c_double, c_uint32, P, P, P, c_size_t, P, P, P]),
        "rrt_testing_scene_refit_stats": (c_int32, [P, P]),
        "rrt_testing_refit_form": (c_int32, [c_int32]),
        "rrt_scene_update_geometry": (c_int32, [P, P, P]),
        "rrt_scene_refit_geometry": (c_int32, [P, P, P]),
        "rrt_refit_bvh_binned_ex": (c_int32, [P, c_uint32, P, c_uint32, c_double, c_uint32, P, P, P, P, c_size_t, P, P, P]),
        "rrt_testing_quad_records": (c_int32, [P, c_uint32, P, P, P]),
        "rrt_scene_update_world": (c_int32, [P, P, P, P]),
        "rrt_scene_refit_world": (c_int32, [P, P, P, P]),
        "rrt_refit_bvh_binned_world": (c_int32, [P, c_uint32, P, c_uint32, c_double, c_uint32, P, P, P, c_size_t, P, P, P]),
        "rrt_build_bvh_lbvh": (c_int32, [P, c_uint32, P, c_uint32, c_uint32, P, c_size_t, P, P]),
        "rrt_refit_bvh_lbvh_world": (c_int32, [P, c_uint32, P, c_uint32, c_uint32, P, P, P, c_size_t, P, P, P]),
        "rrt_scene_set_builder": (c_int32, [P, c_uint32]),
        "rrt_testing_scene_build_stats": (c_int32, [P, P]),
        "rrt_testing_lbvh_form": (c_int32, [c_int32]),
        "rrt_testing_medium_records": (c_int32, [P, c_uint32, P, c_uint32, c_uint32, P, P]),
        "rrt_scene_query_async": (c_int32, [P, P, c_uint32, c_uint32, P, P]),
        "rrt_scene_query": (c_int32, [P, P, c_uint32, c_uint32, P]),
        "rrt_scene_primary_hits_async": (c_int32, [P, c_float, P, P]),
        "rrt_scene_surface_async": (c_int32, [P, P, c_uint32, P, P]),
        "rrt_scene_surface": (c_int32, [P, P, c_uint32, P]),
        "rrt_scene_primary_surface_async": (c_int32, [P, c_float, P, P]),
        "rrt_testing_scene_fail_update": (c_int32, [P]),
    }
    experiment = "RRT_LIB_PATH" in os.environ  # A/B of older builds: tolerate symbols they lack
    for name, (res, args) in sig.items():
        if experiment and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().rrt_hip_last_error()
        raise RrtError(rc, msg.decode() if msg else "")


def ptr(a) -> c_void_p:
    """Address of a numpy array / ctypes object (None for empty / None)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if a.size == 0:
            return None
        assert a.flags["C_CONTIGUOUS"], "arrays passed through the C-ABI must be C-contiguous"
        return c_void_p(a.ctypes.data)
    return ctypes.cast(ctypes.byref(a), c_void_p)


def make_overrides(**kw) -> RrtOverrides:
    """RenderOverrides (config.rs:1-14) with the given fields set to Some(value)."""
    ov = RrtOverrides()
    for k, v in kw.items():
        if v is None:
            continue
        if not hasattr(ov, "has_" + k):
            raise KeyError(f"unknown override {k!r}")
        setattr(ov, "has_" + k, 1)
        if k in ("lookfrom", "lookat", "vup", "background"):
            getattr(ov, k)[:] = [float(x) for x in v]
        else:
            setattr(ov, k, v)
    return ov
