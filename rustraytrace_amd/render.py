"""Render entry points over the C-ABI, mirroring the reference's Rust surface:

* `render_in_one_weekend()`  == cuda::render_in_one_weekend (cuda/mod.rs:337-340, 442-445)
* `render(scene)`            == cuda::imp::render(camera, &spheres, &materials) (cuda/mod.rs:342-439)
                                returning the RGBA accum instead of printing it
* `write_ppm_from_accum`     == render_io::write_ppm_from_accum (render_io.rs:3-31)
* `DeviceScene`              device-resident scene for benches / multi-rank hosts
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional

import numpy as np

from . import _lib
from .scenes import SceneData, build_in_one_weekend_scene, COMMITTED_OVERRIDES


def _textures(scene: SceneData):
    if not scene.textures:
        return None, 0, []
    arr = (_lib.RrtTexture * len(scene.textures))()
    keep = []
    for i, t in enumerate(scene.textures):
        t = np.ascontiguousarray(t, dtype=np.uint8)
        assert t.ndim == 3 and t.shape[2] == 3, "textures are (H, W, 3) RGB8"
        keep.append(t)
        arr[i].rgb8 = t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        arr[i].height, arr[i].width = int(t.shape[0]), int(t.shape[1])
    return arr, len(scene.textures), keep


def scene_ext(scene: SceneData):
    """(RrtSceneExt or None, keep-alive list) for the book-2 data of `scene` (motion, Perlin, quads)."""
    quads, media = getattr(scene, "quads", None), getattr(scene, "media", None)
    bquads, lights = getattr(scene, "boundary_quads", None), getattr(scene, "lights", None)
    if scene.motion is None and scene.perlin is None and quads is None and media is None and lights is None:
        return None, []
    ext = _lib.RrtSceneExt()
    keep = []
    if scene.motion is not None:
        m = np.ascontiguousarray(scene.motion, dtype=np.float32)
        assert m.shape == (len(scene.spheres), 4), "motion is (n_spheres, 4) float32"
        keep.append(m)
        ext.sphere_motion = m.ctypes.data
    if scene.perlin is not None:
        t = np.ascontiguousarray(scene.perlin, dtype=_lib.PERLIN_DTYPE)
        keep.append(t)
        ext.perlin = t.ctypes.data
        ext.n_perlin = len(t)
    if quads is not None:
        q = np.ascontiguousarray(quads, dtype=_lib.QUAD_DTYPE)
        keep.append(q)
        ext.quads = q.ctypes.data
        ext.n_quads = len(q)
    if media is not None:
        md = np.ascontiguousarray(media, dtype=_lib.MEDIUM_DTYPE)
        keep.append(md)
        ext.media = md.ctypes.data
        ext.n_media = len(md)
    if bquads is not None:
        bq = np.ascontiguousarray(bquads, dtype=_lib.QUAD_DTYPE)
        keep.append(bq)
        ext.boundary_quads = bq.ctypes.data
        ext.n_boundary_quads = len(bq)
    if lights is not None:
        lt = np.ascontiguousarray(lights, dtype=_lib.LIGHT_DTYPE)
        keep.append(lt)
        ext.lights = lt.ctypes.data
        ext.n_lights = len(lt)
    return ext, keep


def render(scene: SceneData, spp: Optional[int] = None, n_gpus: int = 1, quiet: bool = True,
           device_bvh: bool = False, fast_bvh: bool = False) -> np.ndarray:
    """Render `scene` on `n_gpus` GPUs; returns the RGBA float32 accum (H, W, 4), w = sample count."""
    lib = _lib.load()
    accum = np.zeros((scene.height, scene.width, 4), dtype=np.float32)
    tex, ntex, keep = _textures(scene)
    ext, keep_ext = scene_ext(scene)
    flags = scene.flags | (_lib.FLAG_QUIET if quiet else 0) | (_lib.FLAG_DEVICE_BVH if device_bvh else 0) | (_lib.FLAG_FAST_BVH if fast_bvh else 0)
    _lib.check(lib.rrt_hip_render_ex(_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres),
                                     _lib.ptr(scene.materials), len(scene.materials),
                                     ctypes.cast(tex, ctypes.c_void_p) if tex is not None else None, ntex,
                                     ctypes.byref(ext) if ext is not None else None,
                                     int(spp or 0), int(n_gpus), flags, _lib.ptr(accum)))
    del keep, keep_ext
    return accum


def _f64_ex_args(scene: SceneData, spp, n_gpus, quiet, device_bvh, out, fast_bvh=False):
    """The argument list of the f64 _ex one-shots (RrtSceneExt passed, both f64 flags implied) and what
    must stay alive during the call."""
    tex, ntex, keep = _textures(scene)
    ext, keep_ext = scene_ext(scene)
    flags = scene.flags | (_lib.FLAG_QUIET if quiet else 0) | (_lib.FLAG_DEVICE_BVH if device_bvh else 0) | (_lib.FLAG_FAST_BVH if fast_bvh else 0)
    args = (_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres), _lib.ptr(scene.materials),
            len(scene.materials), ctypes.cast(tex, ctypes.c_void_p) if tex is not None else None, ntex,
            ctypes.byref(ext) if ext is not None else None, int(spp or 0), int(n_gpus), flags, _lib.ptr(out))
    return args, (keep, keep_ext, ext)


def render_f64(scene: SceneData, spp: Optional[int] = None, n_gpus: int = 1, quiet: bool = True,
               device_bvh: bool = False, book2: bool = False, fast_bvh: bool = False) -> np.ndarray:
    """rrt_hip_render_f64: the books path's own f64 arithmetic (RRT_FLAG_F64, book-1 scenes);
    returns the RGBA float64 accum (H, W, 4) of f64 sums, w = sample count. book2=True:
    rrt_hip_render_f64_ex with the scene's RrtSceneExt (RRT_FLAG_F64_BOOK2: moving spheres, quads,
    checker textures)."""
    lib = _lib.load()
    if book2:
        accum = np.zeros((scene.height, scene.width, 4), dtype=np.float64)
        args, keep = _f64_ex_args(scene, spp, n_gpus, quiet, device_bvh, accum, fast_bvh)
        _lib.check(lib.rrt_hip_render_f64_ex(*args))
        del keep
        return accum
    if getattr(scene, "motion", None) is not None or getattr(scene, "quads", None) is not None:
        raise ValueError("render_f64: book-1 scenes only (RRT_FLAG_F64)")
    accum = np.zeros((scene.height, scene.width, 4), dtype=np.float64)
    tex, ntex, keep = _textures(scene)
    flags = scene.flags | _lib.FLAG_F64 | (_lib.FLAG_QUIET if quiet else 0) | (_lib.FLAG_DEVICE_BVH if device_bvh else 0) | (_lib.FLAG_FAST_BVH if fast_bvh else 0)
    _lib.check(lib.rrt_hip_render_f64(_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres),
                                      _lib.ptr(scene.materials), len(scene.materials),
                                      ctypes.cast(tex, ctypes.c_void_p) if tex is not None else None, ntex,
                                      int(spp or 0), int(n_gpus), flags, _lib.ptr(accum)))
    del keep
    return accum


def render_rgb8(scene: SceneData, spp: Optional[int] = None, n_gpus: int = 1, quiet: bool = True,
                device_bvh: bool = False, fast_bvh: bool = False) -> np.ndarray:
    """rrt_hip_render_rgb8_ex: render and quantise on the device (render_io.rs quantiser);
    returns (H, W, 3) uint8, identical to quantize_accum(render(scene)) at the same spp, for
    every book (the scene's RrtSceneExt — motion, Perlin tables, quads, media, lights — is passed)."""
    lib = _lib.load()
    out = np.zeros((scene.height, scene.width, 3), dtype=np.uint8)
    tex, ntex, keep = _textures(scene)
    ext, keep_ext = scene_ext(scene)
    flags = scene.flags | (_lib.FLAG_QUIET if quiet else 0) | (_lib.FLAG_DEVICE_BVH if device_bvh else 0) | (_lib.FLAG_FAST_BVH if fast_bvh else 0)
    _lib.check(lib.rrt_hip_render_rgb8_ex(_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres),
                                          _lib.ptr(scene.materials), len(scene.materials),
                                          ctypes.cast(tex, ctypes.c_void_p) if tex is not None else None, ntex,
                                          ctypes.byref(ext) if ext is not None else None,
                                          int(spp or 0), int(n_gpus), flags, _lib.ptr(out)))
    del keep, keep_ext
    return out


def quantize_accum_async(n_pixels: int, d_accum_ptr: int, samples_per_pixel: int, d_rgb8_ptr: int,
                         stream_ptr: int = 0) -> None:
    """rrt_quantize_accum_async on device pointers (e.g. torch tensors' data_ptr())."""
    _lib.check(_lib.load().rrt_quantize_accum_async(int(n_pixels), ctypes.c_void_p(d_accum_ptr), int(samples_per_pixel),
                                                    ctypes.c_void_p(d_rgb8_ptr), ctypes.c_void_p(stream_ptr)))


def render_f64_rgb8(scene: SceneData, spp: Optional[int] = None, n_gpus: int = 1, quiet: bool = True,
                    device_bvh: bool = False, book2: bool = False, fast_bvh: bool = False) -> np.ndarray:
    """rrt_hip_render_f64_rgb8: the f64 books kernel (RRT_FLAG_F64, book-1 scenes), then the books
    path's quantiser (color.rs) on the device; returns (H, W, 3) uint8, identical to
    quantize_accum_books_f64(render_f64(scene)) at the same spp. book2=True: rrt_hip_render_f64_rgb8_ex
    with the scene's RrtSceneExt (RRT_FLAG_F64_BOOK2)."""
    lib = _lib.load()
    if book2:
        out = np.zeros((scene.height, scene.width, 3), dtype=np.uint8)
        args, keep = _f64_ex_args(scene, spp, n_gpus, quiet, device_bvh, out, fast_bvh)
        _lib.check(lib.rrt_hip_render_f64_rgb8_ex(*args))
        del keep
        return out
    if getattr(scene, "motion", None) is not None or getattr(scene, "quads", None) is not None:
        raise ValueError("render_f64_rgb8: book-1 scenes only (RRT_FLAG_F64)")
    out = np.zeros((scene.height, scene.width, 3), dtype=np.uint8)
    tex, ntex, keep = _textures(scene)
    flags = scene.flags | _lib.FLAG_F64 | (_lib.FLAG_QUIET if quiet else 0) | (_lib.FLAG_DEVICE_BVH if device_bvh else 0) | (_lib.FLAG_FAST_BVH if fast_bvh else 0)
    _lib.check(lib.rrt_hip_render_f64_rgb8(_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres),
                                           _lib.ptr(scene.materials), len(scene.materials),
                                           ctypes.cast(tex, ctypes.c_void_p) if tex is not None else None, ntex,
                                           int(spp or 0), int(n_gpus), flags, _lib.ptr(out)))
    del keep
    return out


def quantize_accum_books_async(n_pixels: int, d_accum_ptr: int, samples_per_pixel: int, d_rgb8_ptr: int,
                               stream_ptr: int = 0, f64: bool = False) -> None:
    """rrt_quantize_accum_books_async (float4 records) or, with f64=True, rrt_quantize_accum_books_f64_async
    (4 doubles per pixel) on device pointers: the books path's quantiser (color.rs) enqueued on the stream."""
    lib = _lib.load()
    fn = lib.rrt_quantize_accum_books_f64_async if f64 else lib.rrt_quantize_accum_books_async
    _lib.check(fn(int(n_pixels), ctypes.c_void_p(d_accum_ptr), int(samples_per_pixel), ctypes.c_void_p(d_rgb8_ptr),
                  ctypes.c_void_p(stream_ptr)))


def format_pnm_from_rgb8(width: int, height: int, rgb8: np.ndarray, binary: bool = False) -> bytes:
    """P3 (byte-identical to format_ppm_from_accum of the same image) or binary P6."""
    lib = _lib.load()
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    assert rgb8.size == width * height * 3
    n = ctypes.c_size_t(0)
    _lib.check(lib.rrt_format_pnm_from_rgb8(width, height, _lib.ptr(rgb8), int(binary), None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value)
    _lib.check(lib.rrt_format_pnm_from_rgb8(width, height, _lib.ptr(rgb8), int(binary), buf, n.value,
                                            ctypes.byref(n)))
    return buf.raw[: n.value]


def write_pnm_from_rgb8(width: int, height: int, rgb8: np.ndarray, binary: bool = False, path: str = "-") -> None:
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    assert rgb8.size == width * height * 3
    _lib.check(_lib.load().rrt_write_pnm_from_rgb8(width, height, _lib.ptr(rgb8), int(binary), path.encode()))


def render_in_one_weekend(path: str = "-", n_gpus: int = 1, overrides: Optional[dict] = None) -> None:
    """cuda::render_in_one_weekend: RTOW scene under config::OVERRIDES -> P3 PPM on stdout (or `path`)."""
    scene = build_in_one_weekend_scene(COMMITTED_OVERRIDES if overrides is None else overrides)
    accum = render(scene, n_gpus=n_gpus, quiet=False)
    write_ppm_from_accum(scene.width, scene.height, accum, scene.spp, path)


def write_ppm_from_accum(width: int, height: int, accum: np.ndarray, samples_per_pixel: int, path: str = "-") -> None:
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    assert accum.size == width * height * 4
    _lib.check(_lib.load().rrt_write_ppm_from_accum(width, height, _lib.ptr(accum), samples_per_pixel,
                                                    path.encode()))


def format_ppm_from_accum(width: int, height: int, accum: np.ndarray, samples_per_pixel: int) -> bytes:
    lib = _lib.load()
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    assert accum.size == width * height * 4
    n = ctypes.c_size_t(0)
    _lib.check(lib.rrt_format_ppm_from_accum(width, height, _lib.ptr(accum), samples_per_pixel, None, 0,
                                             ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value)
    _lib.check(lib.rrt_format_ppm_from_accum(width, height, _lib.ptr(accum), samples_per_pixel, buf, n.value,
                                             ctypes.byref(n)))
    return buf.raw[: n.value]


def quantize_accum(width: int, height: int, accum: np.ndarray, samples_per_pixel: int) -> np.ndarray:
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    out = np.zeros((height, width, 3), dtype=np.uint8)
    _lib.check(_lib.load().rrt_quantize_accum(width, height, _lib.ptr(accum), samples_per_pixel, _lib.ptr(out)))
    return out


def quantize_accum_books(width: int, height: int, accum: np.ndarray, samples_per_pixel: int) -> np.ndarray:
    """color.rs:6-32 write_color (the books CPU path's f64 quantiser) over a float accum:
    (H, W, 3) uint8. Differs from quantize_accum (render_io.rs) only on non-finite sums
    (+inf -> 255 here, 0 there) and where f64 vs f32 scaling crosses a byte boundary."""
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    out = np.zeros((height, width, 3), dtype=np.uint8)
    _lib.check(_lib.load().rrt_quantize_accum_books(width, height, _lib.ptr(accum), samples_per_pixel, _lib.ptr(out)))
    return out


def quantize_accum_books_f64(width: int, height: int, accum: np.ndarray, samples_per_pixel: int) -> np.ndarray:
    """color.rs:6-32 write_color over f64 sums (render_f64): the books path's bytes, (H, W, 3) uint8."""
    accum = np.ascontiguousarray(accum, dtype=np.float64)
    out = np.zeros((height, width, 3), dtype=np.uint8)
    _lib.check(_lib.load().rrt_quantize_accum_books_f64(width, height, _lib.ptr(accum), samples_per_pixel,
                                                        _lib.ptr(out)))
    return out


def device_count() -> int:
    n = ctypes.c_int32(0)
    _lib.check(_lib.load().rrt_device_count(ctypes.byref(n)))
    return n.value


def tile_rows(height: int, tile) -> int:
    n = ctypes.c_uint32(0)
    _lib.check(_lib.load().rrt_tile_rows(height, ctypes.byref(tile), ctypes.byref(n)))
    return n.value


def tile_row_indices(height: int, tile) -> np.ndarray:
    lib = _lib.load()
    rows = tile_rows(height, tile)
    out = np.empty(rows, dtype=np.int64)
    r = ctypes.c_uint32(0)
    for i in range(rows):
        _lib.check(lib.rrt_tile_row_index(height, ctypes.byref(tile), i, ctypes.byref(r)))
        out[i] = r.value
    return out


def _two_call(call, n_prims: int, info):
    """The BVH entries' two calls: call(nodes_p, cap, order_p), which fills `info`, once for the size
    and once into buffers of that size. Returns (node bytes uint8, leaf order uint32, info dict)."""
    _lib.check(call(None, 0, None))
    nodes = np.zeros(info.node_bytes, dtype=np.uint8)
    order = np.zeros(max(n_prims, 1), dtype=np.uint32)
    _lib.check(call(_lib.ptr(nodes), nodes.size, _lib.ptr(order)))
    return nodes, order[:n_prims], info.as_dict()


def _sphere_rows(spheres, motion):
    """(spheres as SPHERE_DTYPE, motion as (n_spheres, 4) float32 or None) of a change's new rows."""
    sp = np.ascontiguousarray(spheres, dtype=_lib.SPHERE_DTYPE)
    m = None
    if motion is not None:
        m = np.ascontiguousarray(motion, dtype=np.float32)
        assert m.shape == (len(sp), 4), "motion is (n_spheres, 4) float32"
    return sp, m


def build_bvh(scene: SceneData, width: int = 0, max_leaf: int = 0):
    """The BVH rrt_scene_create builds for `scene` (host only): (node bytes uint8, leaf-order
    permutation uint32, info dict). width/max_leaf 0 = the library defaults."""
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    n = len(scene.spheres)
    ext, keep = scene_ext(scene)
    n_prims = n + (0 if ext is None else ext.n_quads + ext.n_media)
    if ext is not None or np.isin(scene.materials["kind"], (5, 6)).any():
        width = 2  # book-2 scenes render with the BVH2 kernel variant (rrt_scene_create_ex)
    def build(nodes_p, cap, order_p):
        if ext is None:
            return lib.rrt_build_bvh(_lib.ptr(scene.spheres), n, width, max_leaf, nodes_p, cap, order_p,
                                     ctypes.byref(info))
        return lib.rrt_build_bvh_ex(_lib.ptr(scene.spheres), n, ctypes.byref(ext), width, max_leaf, nodes_p, cap,
                                    order_p, ctypes.byref(info))

    return _two_call(build, n_prims, info)


def build_bvh_binned(scene: SceneData, max_leaf: int, node_cost: float, node_stride: int):
    """rrt_build_bvh_binned (host only): the tree RRT_FLAG_DEVICE_BVH builds for one shape (max_leaf,
    node_cost) and node format (node_stride 80 or 32), by the device builder's sequential host twin.
    Returns (node bytes uint8, leaf-order permutation uint32, info dict) like build_bvh."""
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    n = len(scene.spheres)
    ext, keep = scene_ext(scene)
    n_prims = n + (0 if ext is None else ext.n_quads + ext.n_media)
    extp = ctypes.byref(ext) if ext is not None else None

    def build(nodes_p, cap, order_p):
        return lib.rrt_build_bvh_binned(_lib.ptr(scene.spheres), n, extp, int(max_leaf), float(node_cost),
                                        int(node_stride), nodes_p, cap, order_p, ctypes.byref(info))

    return _two_call(build, n_prims, info)


def build_bvh_lbvh(scene: SceneData, max_leaf: int, node_stride: int):
    """rrt_build_bvh_lbvh (host only): the tree RRT_FLAG_FAST_BVH builds for one shape (max_leaf) and node
    format (node_stride 80 or 32), by the LBVH builder's sequential host twin. Returns (node bytes uint8,
    leaf-order permutation uint32, info dict) like build_bvh."""
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    n = len(scene.spheres)
    ext, keep = scene_ext(scene)
    n_prims = n + (0 if ext is None else ext.n_quads + ext.n_media)
    extp = ctypes.byref(ext) if ext is not None else None

    def build(nodes_p, cap, order_p):
        return lib.rrt_build_bvh_lbvh(_lib.ptr(scene.spheres), n, extp, int(max_leaf), int(node_stride), nodes_p, cap,
                                      order_p, ctypes.byref(info))

    return _two_call(build, n_prims, info)


def refit_bvh_lbvh_world(built_scene: SceneData, new_scene: SceneData, max_leaf: int, node_stride: int):
    """rrt_refit_bvh_lbvh_world (host only): build_bvh_lbvh's tree of `built_scene` with its boxes
    recomputed over new_scene's spheres, motion, quads, media and boundary quads: the specification of
    the refits of a scene the LBVH builder built. Returns (node bytes, leaf order, info dict, sah)."""
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    sah = ctypes.c_double(0.0)
    n = len(built_scene.spheres)
    sp = np.ascontiguousarray(new_scene.spheres, dtype=_lib.SPHERE_DTYPE)
    assert len(sp) == n, "a refit keeps the sphere count"
    ext, keep = scene_ext(built_scene)
    new_ext, keep_new = scene_ext(new_scene)
    n_prims = n + (0 if ext is None else ext.n_quads + ext.n_media)
    extp = ctypes.byref(ext) if ext is not None else None
    new_extp = ctypes.byref(new_ext) if new_ext is not None else None

    def refit(nodes_p, cap, order_p):
        return lib.rrt_refit_bvh_lbvh_world(_lib.ptr(built_scene.spheres), n, extp, int(max_leaf), int(node_stride),
                                            _lib.ptr(sp), new_extp, nodes_p, cap, order_p, ctypes.byref(info),
                                            ctypes.byref(sah))

    return (*_two_call(refit, n_prims, info), float(sah.value))


def refit_bvh_binned(built_scene: SceneData, new_spheres, new_motion, max_leaf: int, node_cost: float, node_stride: int,
                     new_quads=None):
    """rrt_refit_bvh_binned_ex (host only): build_bvh_binned's tree of `built_scene` with its boxes
    recomputed over new_spheres, new_motion (None = all zero) and new_quads (None = the built ones),
    the specification of DeviceScene.refit_spheres and refit_geometry. Returns (node bytes, leaf
    order, info dict, sah)."""
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    sah = ctypes.c_double(0.0)
    n = len(built_scene.spheres)
    sp, m = _sphere_rows(new_spheres, new_motion)
    assert len(sp) == n, "a refit keeps the sphere count"
    ext, keep = scene_ext(built_scene)
    n_prims = n + (0 if ext is None else ext.n_quads + ext.n_media)
    extp = ctypes.byref(ext) if ext is not None else None
    q = None
    if new_quads is not None:
        q = np.ascontiguousarray(new_quads, dtype=_lib.QUAD_DTYPE)
        assert len(q) == (0 if ext is None else ext.n_quads), "a refit keeps the quad count"

    def refit(nodes_p, cap, order_p):
        return lib.rrt_refit_bvh_binned_ex(_lib.ptr(built_scene.spheres), n, extp, int(max_leaf), float(node_cost),
                                           int(node_stride), _lib.ptr(sp), _lib.ptr(m), _lib.ptr(q), nodes_p, cap,
                                           order_p, ctypes.byref(info), ctypes.byref(sah))

    return (*_two_call(refit, n_prims, info), float(sah.value))


def refit_bvh_binned_world(built_scene: SceneData, new_scene: SceneData, max_leaf: int, node_cost: float, node_stride: int):
    """rrt_refit_bvh_binned_world (host only): build_bvh_binned's tree of `built_scene` with its boxes
    recomputed over new_scene's spheres, motion, quads, media and boundary quads (the same counts and
    medium structure), the classification and leaf order kept: the specification of
    DeviceScene.refit_world. Returns (node bytes, leaf order, info dict, sah)."""
    lib = _lib.load()
    info = _lib.RrtBvhInfo()
    sah = ctypes.c_double(0.0)
    n = len(built_scene.spheres)
    sp = np.ascontiguousarray(new_scene.spheres, dtype=_lib.SPHERE_DTYPE)
    assert len(sp) == n, "a refit keeps the sphere count"
    ext, keep = scene_ext(built_scene)
    new_ext, keep_new = scene_ext(new_scene)
    n_prims = n + (0 if ext is None else ext.n_quads + ext.n_media)
    extp = ctypes.byref(ext) if ext is not None else None
    new_extp = ctypes.byref(new_ext) if new_ext is not None else None

    def refit(nodes_p, cap, order_p):
        return lib.rrt_refit_bvh_binned_world(_lib.ptr(built_scene.spheres), n, extp, int(max_leaf), float(node_cost),
                                              int(node_stride), _lib.ptr(sp), new_extp, nodes_p, cap, order_p,
                                              ctypes.byref(info), ctypes.byref(sah))

    return (*_two_call(refit, n_prims, info), float(sah.value))


def decode_bvh2(nodes: np.ndarray, stride: int):
    """Decode build_bvh's width-2 node bytes (rrt_internal.h; stride = info["node_stride"]: 80 =
    GNode, sign-ordered lo/hi/lo planes, 32 = GNodeH, f16 planes): per node and child, box lo/hi (n, 2, 3),
    first primitive or child node (n, 2) and leaf count (n, 2; 0 = internal)."""
    words = stride // 4
    f = nodes.view(np.float32).reshape(-1, words)
    u = nodes.view(np.uint32).reshape(-1, words)
    if stride == 80:
        box = f[:, :18].reshape(-1, 2, 3, 3)  # [node][child][axis][lo, hi, lo]
        assert np.array_equal(box[..., 2], box[..., 0])
        lo, hi, links = box[..., 0].copy(), box[..., 1].copy(), u[:, 18:20]
    elif stride == 32:  # GNodeH: f16 planes, lo | hi << 16 per child and axis
        box = nodes.view(np.float16).reshape(-1, 16)[:, :12].astype(np.float32).reshape(-1, 2, 3, 2)  # [node][child][axis][lo, hi]
        lo, hi, links = box[..., 0].copy(), box[..., 1].copy(), u[:, 6:8]
    else:
        raise ValueError(f"decode_bvh2: stride {stride}")
    return lo, hi, (links & 0x0FFFFFFF).astype(np.int64), (links >> 28).astype(np.int64)


def make_tile(band_rows=16, rank=0, n_ranks=1, sample_begin=0, sample_end=0) -> _lib.RrtTile:
    t = _lib.RrtTile()
    t.band_rows, t.rank, t.n_ranks, t.sample_begin, t.sample_end = band_rows, rank, n_ranks, sample_begin, sample_end
    return t


class DeviceScene:
    """RrtScene*: scene + BVH resident on one device; renders tiles asynchronously on a stream."""

    def __init__(self, scene: SceneData, device: int = 0, f64: bool = False, device_bvh: bool = False,
                 f64_book2: bool = False, fast_bvh: bool = False):
        """f64=True: the books path's f64 kernel (RRT_FLAG_F64, book-1 scenes); with f64_book2=True also
        moving spheres, quads and checker textures (RRT_FLAG_F64_BOOK2, which implies f64). device_bvh=True:
        the BVH is built on the device (RRT_FLAG_DEVICE_BVH) instead of the host. fast_bvh=True: on the
        device by the LBVH builder (RRT_FLAG_FAST_BVH, implies device_bvh): cheap rebuilds, a slower tree."""
        lib = _lib.load()
        self.scene = scene
        self.device = int(device)
        flags = scene.flags | (_lib.FLAG_F64 if f64 else 0) | (_lib.FLAG_DEVICE_BVH if device_bvh else 0) | (_lib.FLAG_FAST_BVH if fast_bvh else 0)
        flags |= _lib.FLAG_F64_BOOK2 if f64_book2 else 0
        self._lib = lib
        self._h = ctypes.c_void_p()
        tex, ntex, keep = _textures(scene)
        ext, keep_ext = scene_ext(scene)
        texp = ctypes.cast(tex, ctypes.c_void_p) if tex is not None else None
        if ext is None:
            _lib.check(lib.rrt_scene_create(_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres),
                                            _lib.ptr(scene.materials), len(scene.materials), texp, ntex,
                                            flags, int(device), ctypes.byref(self._h)))
        else:
            _lib.check(lib.rrt_scene_create_ex(_lib.ptr(scene.camera), _lib.ptr(scene.spheres), len(scene.spheres),
                                               _lib.ptr(scene.materials), len(scene.materials), texp, ntex,
                                               ctypes.byref(ext), flags, int(device), ctypes.byref(self._h)))
        del keep, keep_ext

    def close(self):
        if self._h:
            self._lib.rrt_scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def tile(band_rows=16, rank=0, n_ranks=1, sample_begin=0, sample_end=None, spp=None) -> _lib.RrtTile:
        t = _lib.RrtTile()
        t.band_rows, t.rank, t.n_ranks = band_rows, rank, n_ranks
        t.sample_begin = sample_begin
        t.sample_end = sample_end if sample_end is not None else (sample_begin + (spp or 0))
        return t

    def tile_rows(self, tile) -> int:
        return tile_rows(self.scene.height, tile)

    def tile_row_indices(self, tile) -> np.ndarray:
        return tile_row_indices(self.scene.height, tile)

    def render_tile_async(self, tile, d_accum_ptr: int, stream_ptr: int = 0) -> None:
        _lib.check(self._lib.rrt_render_tile_async(self._h, ctypes.byref(tile), ctypes.c_void_p(d_accum_ptr),
                                                   ctypes.c_void_p(stream_ptr)))

    def render_tile_f64_async(self, tile, d_accum_ptr: int, stream_ptr: int = 0) -> None:
        """rrt_render_tile_f64_async: f64 sums (rows x W x 4 doubles) of a DeviceScene(f64=True)."""
        _lib.check(self._lib.rrt_render_tile_f64_async(self._h, ctypes.byref(tile), ctypes.c_void_p(d_accum_ptr),
                                                       ctypes.c_void_p(stream_ptr)))

    def counters(self) -> dict:
        c = _lib.RrtCounters()
        _lib.check(self._lib.rrt_scene_read_counters(self._h, ctypes.byref(c)))
        return c.as_dict()

    def reset_counters(self) -> None:
        _lib.check(self._lib.rrt_scene_reset_counters(self._h))

    def count_work(self, tile) -> dict:
        c = _lib.RrtCounters()
        _lib.check(self._lib.rrt_scene_count_work(self._h, ctypes.byref(tile), ctypes.byref(c)))
        return c.as_dict()

    def set_camera(self, camera) -> None:
        """rrt_scene_set_camera: replaces what scene creation derived from the camera (rays, seed,
        max_depth, background, width / height, book 3's sqrt_spp); renders enqueued afterwards use it."""
        cam = np.ascontiguousarray(camera, dtype=_lib.CAMERA_DTYPE).reshape(1)
        _lib.check(self._lib.rrt_scene_set_camera(self._h, _lib.ptr(cam)))
        self.scene = dataclasses.replace(self.scene, camera=cam.copy())

    def query(self, rays, mode: str = "closest") -> np.ndarray:
        """rrt_scene_query: the render's closest-hit query over (0.001, tmax) for each ray of `rays`
        (_lib.RAY_DTYPE: o, tmax, d, time), without shading; returns _lib.HIT_DTYPE records (t, prim),
        prim the primitive's index in source order (spheres, then quads) or _lib.NO_PRIM for a miss.
        mode "any": a hit, not necessarily the closest. Synchronous; f32 scenes without media."""
        r = np.ascontiguousarray(rays, dtype=_lib.RAY_DTYPE).ravel()
        hits = np.zeros(len(r), dtype=_lib.HIT_DTYPE)
        _lib.check(self._lib.rrt_scene_query(self._h, _lib.ptr(r), len(r), self._mode(mode), _lib.ptr(hits)))
        return hits

    @staticmethod
    def _mode(mode) -> int:
        return _lib.QUERY_MODES[mode] if isinstance(mode, str) else int(mode)

    def query_async(self, d_rays_ptr: int, n: int, d_hits_ptr: int, mode="closest", stream_ptr: int = 0) -> None:
        """rrt_scene_query_async: n RAY_DTYPE records at d_rays_ptr answered into n HIT_DTYPE records
        at d_hits_ptr (device memory), enqueued on the stream behind the updates and refits on it."""
        _lib.check(self._lib.rrt_scene_query_async(self._h, ctypes.c_void_p(d_rays_ptr), int(n), self._mode(mode),
                                                   ctypes.c_void_p(d_hits_ptr), ctypes.c_void_p(stream_ptr)))

    def primary_hits_async(self, d_hits_ptr: int, time: float = 0.0, stream_ptr: int = 0) -> None:
        """rrt_scene_primary_hits_async: height x width HIT_DTYPE records at d_hits_ptr (device memory),
        record (y, x) the closest hit of the camera's ray through pixel (x, y) with zero jitter and no
        defocus, at `time`."""
        _lib.check(self._lib.rrt_scene_primary_hits_async(self._h, ctypes.c_float(time), ctypes.c_void_p(d_hits_ptr),
                                                          ctypes.c_void_p(stream_ptr)))

    def primary_hits(self, time: float = 0.0) -> np.ndarray:
        """primary_hits_async into a torch buffer on the scene's device, synchronised: an (H, W) array
        of HIT_DTYPE (an id and depth buffer of the current camera)."""
        import torch

        h, w = self.scene.height, self.scene.width
        with torch.cuda.device(self.device):
            buf = torch.zeros(max(h * w, 1) * 2, dtype=torch.int32, device=f"cuda:{self.device}")
            self.primary_hits_async(buf.data_ptr(), time, torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().synchronize()
            out = buf.cpu().numpy()[: h * w * 2]
        return out.view(_lib.HIT_DTYPE).reshape(h, w).copy()

    def surface(self, rays) -> np.ndarray:
        """rrt_scene_surface: the closest-hit query of `rays` (_lib.RAY_DTYPE) answered with the hit's
        HitRecord, _lib.SURFACE_DTYPE records: p, t, normal (against the ray), prim, albedo, kind, uv,
        front_face; a miss has prim = _lib.NO_PRIM, kind = _lib.SURFACE_MISS and the background in albedo.
        Constant media are passed over: the closest surface. Synchronous; f32 scenes."""
        r = np.ascontiguousarray(rays, dtype=_lib.RAY_DTYPE).ravel()
        out = np.zeros(len(r), dtype=_lib.SURFACE_DTYPE)
        _lib.check(self._lib.rrt_scene_surface(self._h, _lib.ptr(r), len(r), _lib.ptr(out)))
        return out

    def surface_async(self, d_rays_ptr: int, n: int, d_out_ptr: int, stream_ptr: int = 0) -> None:
        """rrt_scene_surface_async: n RAY_DTYPE records at d_rays_ptr answered into n SURFACE_DTYPE records
        at d_out_ptr (device memory, 16-byte aligned), enqueued on the stream behind the updates and refits on it."""
        _lib.check(self._lib.rrt_scene_surface_async(self._h, ctypes.c_void_p(d_rays_ptr), int(n), ctypes.c_void_p(d_out_ptr),
                                                     ctypes.c_void_p(stream_ptr)))

    def primary_surface_async(self, d_out_ptr: int, time: float = 0.0, stream_ptr: int = 0) -> None:
        """rrt_scene_primary_surface_async: height x width SURFACE_DTYPE records at d_out_ptr (device
        memory), record (y, x) the surface record of primary_hits_async's ray through pixel (x, y)."""
        _lib.check(self._lib.rrt_scene_primary_surface_async(self._h, ctypes.c_float(time), ctypes.c_void_p(d_out_ptr),
                                                             ctypes.c_void_p(stream_ptr)))

    def primary_surface(self, time: float = 0.0) -> np.ndarray:
        """primary_surface_async into a torch buffer on the scene's device, synchronised: an (H, W) array
        of SURFACE_DTYPE (the G-buffer of the current camera: albedo, normal, position, depth, id)."""
        import torch

        h, w = self.scene.height, self.scene.width
        with torch.cuda.device(self.device):
            buf = torch.zeros(max(h * w, 1) * 16, dtype=torch.int32, device=f"cuda:{self.device}")
            self.primary_surface_async(buf.data_ptr(), time, torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().synchronize()
            out = buf.cpu().numpy()[: h * w * 16]
        return out.view(_lib.SURFACE_DTYPE).reshape(h, w).copy()

    def testing_fail_update(self) -> str:
        """rrt_testing_scene_fail_update (test support): leaves the scene invalid, as a change that failed
        midway does; returns the message. A later update that succeeds makes it valid again."""
        rc = self._lib.rrt_testing_scene_fail_update(self._h)
        assert rc == -1, rc
        return self._lib.rrt_hip_last_error().decode()

    def update_spheres(self, spheres, motion=None, stream_ptr: int = 0) -> None:
        """rrt_scene_update_spheres: replaces the spheres (and, for a book-2 world, their motion rows;
        None = all zero) of a DeviceScene(device_bvh=True), rebuilds the BVH on the device and re-forms
        the per-primitive tables; the scene then equals one freshly created from the new inputs. Waits
        for the stream, returns synchronised."""
        self._change("rrt_scene_update_spheres", stream_ptr, spheres, motion)

    def refit_spheres(self, spheres, motion=None, stream_ptr: int = 0) -> None:
        """rrt_scene_refit_spheres: replaces the spheres (and motion rows) like update_spheres but keeps
        the tree's topology and leaf order and recomputes only its boxes; everything is enqueued on
        the stream and the call does not wait for the device. tree_cost() tells when to rebuild."""
        self._change("rrt_scene_refit_spheres", stream_ptr, spheres, motion)

    def _change(self, entry: str, stream_ptr: int, spheres, motion, quads=None, lights=None, media=None,
                boundary_quads=None) -> None:
        """The body of the six update_* and refit_* methods: calls the library's `entry` with the new
        rows and, once it succeeded, makes them self.scene's."""
        fn, stream = getattr(self._lib, entry), ctypes.c_void_p(stream_ptr)
        if entry.endswith("_spheres"):
            sp, m = _sphere_rows(spheres, motion)
            _lib.check(fn(self._h, _lib.ptr(sp), len(sp), _lib.ptr(m), stream))
            self.scene = dataclasses.replace(self.scene, spheres=sp.copy(), motion=None if m is None else m.copy())
            return
        g, new = self._geometry(spheres, motion, quads, lights)
        args = [ctypes.byref(g)]
        if entry.endswith("_world"):
            wm, new = self._media(new, media, boundary_quads)
            args.append(None if wm is None else ctypes.byref(wm))
        _lib.check(fn(self._h, *args, stream))
        self.scene = new

    def _geometry(self, spheres, motion, quads, lights):
        """(RrtSceneGeometry, the replaced SceneData) of a geometry change; the struct borrows the
        new scene's arrays."""
        sc = self.scene
        sp, m = _sphere_rows(sc.spheres if spheres is None else spheres, motion)
        new = dataclasses.replace(sc, spheres=sp.copy(), motion=None if m is None else m.copy())
        g = _lib.RrtSceneGeometry()
        g.spheres, g.n_spheres = (new.spheres.ctypes.data if len(sp) else None), len(sp)
        g.sphere_motion = new.motion.ctypes.data if m is not None and len(sp) else None
        if quads is not None:
            new = dataclasses.replace(new, quads=np.ascontiguousarray(quads, dtype=_lib.QUAD_DTYPE).copy())
            g.quads, g.n_quads = new.quads.ctypes.data, len(new.quads)  # the address even of an empty array
        if lights is None and sc.flags & _lib.FLAG_BOOK3:
            lights = sc.lights
        if lights is not None:
            new = dataclasses.replace(new, lights=np.ascontiguousarray(lights, dtype=_lib.LIGHT_DTYPE).copy())
            g.lights, g.n_lights = new.lights.ctypes.data, len(new.lights)
        return g, new

    def update_geometry(self, spheres=None, motion=None, quads=None, lights=None, stream_ptr: int = 0) -> None:
        """rrt_scene_update_geometry: update_spheres extended to the quads (None = keep them) and, for a
        book-3 scene, the light list (None = the current lights): the BVH is rebuilt on the device and
        everything derived from the geometry re-formed there; the scene then equals one freshly created
        from the new inputs. spheres=None passes the current spheres; motion=None is all zero. Waits
        for the stream, returns synchronised."""
        self._change("rrt_scene_update_geometry", stream_ptr, spheres, motion, quads, lights)

    def refit_geometry(self, spheres=None, motion=None, quads=None, lights=None, stream_ptr: int = 0) -> None:
        """rrt_scene_refit_geometry: the same replacement as update_geometry, but the tree keeps its
        topology and leaf order and only its boxes are recomputed; everything is enqueued on the stream
        and the call does not wait for the device. tree_cost() tells when to rebuild."""
        self._change("rrt_scene_refit_geometry", stream_ptr, spheres, motion, quads, lights)

    def _media(self, new, media, boundary_quads):
        """(RrtSceneMedia or None, the replaced SceneData) of a world change; the struct borrows the
        new scene's arrays."""
        if media is None and boundary_quads is None:
            return None, new
        wm = _lib.RrtSceneMedia()
        if media is not None:
            new = dataclasses.replace(new, media=np.ascontiguousarray(media, dtype=_lib.MEDIUM_DTYPE).copy())
            wm.media, wm.n_media = new.media.ctypes.data, len(new.media)
        if boundary_quads is not None:
            new = dataclasses.replace(new, boundary_quads=np.ascontiguousarray(boundary_quads, dtype=_lib.QUAD_DTYPE).copy())
            wm.boundary_quads, wm.n_boundary_quads = new.boundary_quads.ctypes.data, len(new.boundary_quads)
        return wm, new

    def update_world(self, spheres=None, motion=None, quads=None, lights=None, media=None, boundary_quads=None,
                     stream_ptr: int = 0) -> None:
        """rrt_scene_update_world: update_geometry extended to the constant media and their boundary quads
        (None = keep them), on scenes with or without media: which media are tested outside the tree is
        decided again from the new inputs, the BVH rebuilt on the device over the rest and everything
        derived re-formed there; the scene then equals one freshly created from the new inputs. Waits
        for the stream, returns synchronised."""
        self._change("rrt_scene_update_world", stream_ptr, spheres, motion, quads, lights, media, boundary_quads)

    def refit_world(self, spheres=None, motion=None, quads=None, lights=None, media=None, boundary_quads=None,
                    stream_ptr: int = 0) -> None:
        """rrt_scene_refit_world: the same replacement as update_world, but the tree keeps its topology,
        its leaf order and the last build's choice of the media tested outside it, and only its boxes
        are recomputed; everything is enqueued on the stream and the call does not wait for the device.
        tree_cost() tells when to rebuild."""
        self._change("rrt_scene_refit_world", stream_ptr, spheres, motion, quads, lights, media, boundary_quads)

    def tree_cost(self) -> dict:
        """rrt_scene_tree_cost: the SAH cost of the tree held now, of the last build's tree, and the
        refits since that build. Synchronises the device."""
        c = _lib.RrtTreeCost()
        _lib.check(self._lib.rrt_scene_tree_cost(self._h, ctypes.byref(c)))
        return {"sah": float(c.sah), "sah_at_build": float(c.sah_at_build), "refits_since_build": int(c.refits_since_build)}

    def set_builder(self, builder: str) -> None:
        """rrt_scene_set_builder: the builder of the next update_*: "binned" (quality) or "lbvh" (speed)."""
        if builder not in _lib.BUILDERS:
            raise ValueError(f"set_builder: {builder!r} is not one of {sorted(_lib.BUILDERS)}")
        _lib.check(self._lib.rrt_scene_set_builder(self._h, _lib.BUILDERS[builder]))

    def build_stats(self) -> dict:
        """rrt_testing_scene_build_stats (test support): of the last device build, the builder ("binned" or
        "lbvh"), its kernel launches (a library sort counts once), blocking reads, form (1: the LBVH's
        single workgroup) and shape attempts."""
        st = _lib.RrtSceneBuildStats()
        _lib.check(self._lib.rrt_testing_scene_build_stats(self._h, ctypes.byref(st)))
        d = {k: int(getattr(st, k)) for k, _ in st._fields_}
        d["builder"] = {v: k for k, v in _lib.BUILDERS.items()}[d["builder"]]
        return d

    def refit_stats(self) -> dict:
        """rrt_testing_scene_refit_stats (test support): refits so far; the last one's device
        allocations, kernel launches and form (1: the single workgroup, 0: one launch per level)."""
        st = _lib.RrtSceneRefitStats()
        _lib.check(self._lib.rrt_testing_scene_refit_stats(self._h, ctypes.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    def read_table(self, name: str) -> np.ndarray:
        """rrt_testing_scene_read_table (test support): one of the scene's device tables (a
        _lib.SCENE_TABLES, _lib.SCENE_GEOMETRY_TABLES or _lib.SCENE_MEDIA_TABLES name) as a flat array;
        empty when the scene does not hold it."""
        code, dtype = (_lib.SCENE_TABLES.get(name) or _lib.SCENE_GEOMETRY_TABLES.get(name) or _lib.SCENE_MEDIA_TABLES[name])
        n = ctypes.c_size_t(0)
        _lib.check(self._lib.rrt_testing_scene_read_table(self._h, code, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value // dtype.itemsize, dtype=dtype)
        if n.value:
            _lib.check(self._lib.rrt_testing_scene_read_table(self._h, code, _lib.ptr(out), n.value, ctypes.byref(n)))
        return out

    def update_stats(self) -> dict:
        """rrt_testing_scene_update_stats (test support): updates so far, and the device allocations
        and builder levels of the last one."""
        st = _lib.RrtSceneUpdateStats()
        _lib.check(self._lib.rrt_testing_scene_update_stats(self._h, ctypes.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    def bvh_info(self) -> dict:
        b = _lib.RrtBvhInfo()
        _lib.check(self._lib.rrt_scene_bvh_info(self._h, ctypes.byref(b)))
        return b.as_dict()

    def read_bvh(self):
        """rrt_scene_read_bvh: the node bytes (uint8) and leaf order (uint32) this scene holds on its
        device, with either builder, and the info dict (as build_bvh returns them)."""
        info = self.bvh_info()
        ext, keep = scene_ext(self.scene)
        n_prims = len(self.scene.spheres) + (0 if ext is None else ext.n_quads + ext.n_media)
        del keep
        nodes = np.zeros(info["node_bytes"], dtype=np.uint8)
        order = np.zeros(max(n_prims, 1), dtype=np.uint32)
        _lib.check(self._lib.rrt_scene_read_bvh(self._h, _lib.ptr(nodes), nodes.size, _lib.ptr(order)))
        return nodes, order[:n_prims], info
