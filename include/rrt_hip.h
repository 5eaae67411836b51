/*
 * rrt_hip.h — C-ABI of librrt_hip.so, the MI355X (gfx950) path-tracing backend.
 *
 * This is the drop-in boundary for the reference's GPU-backend slot:
 *   src/main.rs:58-71            `--backend cuda` -> cuda::render_in_one_weekend()
 *   src/cuda/mod.rs:337-439      imp::render(camera, &spheres, &materials) -> Result<(), String>
 *   src/gpu/mod.rs:124-301       build_in_one_weekend_scene() -> (CameraUniform, Vec<SphereGpu>, Vec<MaterialGpu>)
 *   src/render_io.rs:3-31        write_ppm_from_accum(w, h, &[f32] RGBA accum, spp)
 *
 * Plain C types only (no torch / HIP types in signatures). Every entry point returns
 * 0 on success or a negative RRT_E* code; rrt_hip_last_error() then holds the message
 * (thread-local, valid until the next call on that thread) — the Rust shim maps a
 * non-zero return to Err(rrt_hip_last_error()) exactly like cuda/mod.rs maps its
 * `map_err(|e| format!(...))` strings.
 *
 * Struct layouts are byte-identical to the reference's #[repr(C)] Pod structs, so the
 * Rust side passes `bytemuck::cast_slice` views of its existing vectors unchanged.
 */
#ifndef RRT_HIP_H
#define RRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: book 1; 2: RrtSceneExt (motion, Perlin), kinds 5-6; 3: quads, constant-density media and
 * book-3 light lists in RrtSceneExt, kind 7, RRT_FLAG_BOOK3, rrt_build_next_week_scene /
 * rrt_build_rest_of_your_life_scene with struct outputs; 4: RrtBvhInfo.node_stride (80-B LDS /
 * 64-B global BVH2 nodes), xoshiro128+ path streams, tail-split accumulation chunks;
 * 5: exit_skip (f32 bounces never re-hit the primitive they leave), rrt_hip_render_rgb8_ex,
 * rrt_quantize_accum_books, chunk partials bounded by RRT_PARTIAL_MB (sample passes);
 * 6: RrtBvhInfo.n_unbounded (scene-enclosing media tested after the BVH walk; was _pad);
 * 7: RRT_FLAG_F64 (the books path's f64 arithmetic), rrt_hip_render_f64, rrt_render_tile_f64_async,
 * rrt_quantize_accum_books_f64; 8: RrtTile bands dealt in serpentine order (was b % n_ranks);
 * 9: rrt_accum_chunk() = 256 and the frame's chunk halved while S <= 2K down to a quarter (frames
 * over 512 samples sum in chunks of 256; was 128), rrt_testing_device_wrap, rrt_testing_recip_check
 * (test-only entry points, no drop-in counterpart); 10: tail chunks of K/4 samples (was K/8), the
 * f64 books path's sums in camera.rs:72-76's sample order with the throughput formed back to front
 * (bit-identical to the books path), rrt_testing_f64_layout; 11: frames of at most
 * rrt_accum_chunk() / 4 samples (no big chunk) keep tail chunks of K/8; rrt_testing_trig32_check. */
#define RRT_ABI_VERSION 11u

/* ---- scene ABI (== src/gpu/mod.rs:13-42) ------------------------------------------ */

/* == CameraUniform (gpu/mod.rs:15-25), 144 B.
 * params_f = [defocus_radius, image_width, image_height, samples_per_pixel]
 * params_u = [max_depth, sample_seed, n_spheres, background_mode(0 sky, 1 `background`)] */
typedef struct RrtCamera {
    float origin[4];
    float pixel00[4];
    float pixel_delta_u[4];
    float pixel_delta_v[4];
    float u[4];
    float v[4];
    float background[4];
    float params_f[4];
    uint32_t params_u[4];
} RrtCamera;

/* == SphereGpu (gpu/mod.rs:29-33), 32 B. */
typedef struct RrtSphere {
    float center_radius[4];
    uint32_t material_index;
    uint32_t _pad[3];
} RrtSphere;

/* == MaterialGpu (gpu/mod.rs:37-42), 32 B. kind 0..2 are the reference's; 3..6 extend the
 * ABI for book 2 (the_next_week/material.rs:27-53,116-135, texture.rs:39-77,111-126):
 *   3 = textured Lambertian, _pad[0] = texture index into the RrtTexture array
 *   4 = diffuse light, albedo_fuzz.xyz = emitted radiance
 *   5 = Lambertian with a solid-colour CheckerTexture: albedo_fuzz.xyz = even colour,
 *       albedo_fuzz[3] = inv_scale (1/scale), odd colour = (ref_idx, bits of _pad[0], bits of _pad[1])
 *   6 = Lambertian with a NoiseTexture: albedo_fuzz[3] = scale, _pad[0] = Perlin table index
 *       into RrtSceneExt.perlin
 *   7 = Isotropic (material.rs:137-158), albedo_fuzz.xyz = albedo: the phase function of a
 *       medium (RrtMedium); scatters into random_unit_vector() */
typedef struct RrtMaterial {
    float albedo_fuzz[4];
    uint32_t kind;
    float ref_idx;
    uint32_t _pad[2];
} RrtMaterial;

enum {
    RRT_MAT_LAMBERTIAN = 0,
    RRT_MAT_METAL = 1,
    RRT_MAT_DIELECTRIC = 2,
    RRT_MAT_TEXTURED_LAMBERTIAN = 3,
    RRT_MAT_DIFFUSE_LIGHT = 4,
    RRT_MAT_CHECKER_LAMBERTIAN = 5,
    RRT_MAT_NOISE_LAMBERTIAN = 6,
    RRT_MAT_ISOTROPIC = 7
};

/* == Perlin (the_next_week/perlin.rs:4-22): 256 unit random vectors and the three
 * permutations of 0..255. 4 KB. The reference draws them from the thread-local entropy RNG;
 * rrt_build_next_week_scene draws them from a seeded stream (parity unpinned). */
typedef struct RrtPerlin {
    float randvec[256][4]; /* xyz, w unused */
    uint16_t perm_x[256];
    uint16_t perm_y[256];
    uint16_t perm_z[256];
    uint16_t _pad[256];
} RrtPerlin;

/* == Quad (the_next_week/quad.rs:9-41), 64 B: corner q, edge vectors u, v (xyz; w unused) and
 * its material. Instanced quads (RotateY / Translate, hittable.rs:65-170) are passed already
 * transformed to world space (rrt_build_next_week_scene bakes make_box + RotateY + Translate). */
typedef struct RrtQuad {
    float q[4];
    float u[4];
    float v[4];
    uint32_t material_index;
    uint32_t _pad[3];
} RrtQuad;

/* == ConstantMedium (the_next_week/constant_medium.rs), 48 B: a volume of constant density inside a
 * boundary — a sphere (boundary_kind 0: center xyz, radius in `sphere`) or a set of quads
 * (boundary_kind 1: RrtSceneExt.boundary_quads[first .. first + count), e.g. a baked make_box).
 * The boundary is not a surface of the scene (add it separately if it is one). material_index
 * names the phase function (RRT_MAT_ISOTROPIC). Free-flight draw: the reference takes
 * `random_double()` from its entropy stream inside hit(), so its stream position depends on the
 * BVH walk; here the draw is u = splitmix64(path_rng ^ (bounce << 32) ^ medium) >> 40 (path_rng:
 * the first 64 bits of the path's xoshiro128+ state at the segment start; 24 bits,
 * times 2^-24) — one independent uniform per (path, segment, medium), the same whichever order a
 * BVH tests the primitives in. hit_distance = (-1/density) * ln(u) in f32 (a Cephes logf). */
typedef struct RrtMedium {
    float sphere[4];
    uint32_t boundary_kind;
    uint32_t first;
    uint32_t count;
    uint32_t material_index;
    float density;
    uint32_t _pad[3];
} RrtMedium;

enum { RRT_BOUNDARY_SPHERE = 0, RRT_BOUNDARY_QUADS = 1 };

/* == a book-3 light-list entry (the_rest_of_your_life/mod.rs `lights`, sampled by HittablePdf,
 * pdf.rs:58-78): a Quad (kind 0: corner q = a.xyz, edges u, v; quad.rs:93-107 pdf_value /
 * random) or a Sphere (kind 1: center a.xyz, radius a[3]; sphere.rs:55-66, 102-122). 64 B.
 * Sampling targets only: not surfaces of the scene (add those separately). */
typedef struct RrtLight {
    uint32_t kind;
    uint32_t _pad[3];
    float a[4];
    float u[4];
    float v[4];
} RrtLight;

enum { RRT_LIGHT_QUAD = 0, RRT_LIGHT_SPHERE = 1 };

/* Book-2 scene data beyond the flat sphere/material ABI. NULL = none.
 * sphere_motion: n_spheres x 4 floats, (center2 - center1).xyz of Sphere::new_moving
 * (the_next_week/sphere.rs:24-40; the sphere's center at ray time t is center1 + t*motion;
 * zero = static). Requires RRT_FLAG_RAY_TIME (rays carry the camera's time draw).
 * quads: n_quads quads (materials: Lambertian, checker, noise, metal, dielectric or light;
 * not image-textured). media: n_media constant-density volumes; boundary_quads: the quads their
 * quad boundaries index (material_index unused). Primitive order for rrt_build_bvh_ex:
 * spheres, then quads (n_spheres + j), then media (n_spheres + n_quads + m). */
typedef struct RrtSceneExt {
    const float *sphere_motion;
    const RrtPerlin *perlin;
    uint32_t n_perlin;
    uint32_t n_quads;
    const RrtQuad *quads;
    const RrtMedium *media;
    uint32_t n_media;
    uint32_t n_boundary_quads;
    const RrtQuad *boundary_quads;
    const RrtLight *lights; /* book 3 (RRT_FLAG_BOOK3): the MIS light list */
    uint32_t n_lights;
    uint32_t _pad;
} RrtSceneExt;

/* Image texture, RGB8 row-major (rtw_image.rs:57-67 `to_rgb8().into_raw()`). Borrowed. */
typedef struct RrtTexture {
    const uint8_t *rgb8;
    int32_t width;
    int32_t height;
} RrtTexture;

/* == config::RenderOverrides (config.rs:1-14): has_* = Some(..). */
typedef struct RrtOverrides {
    int32_t has_aspect_ratio;   double aspect_ratio;
    int32_t has_image_width;    int32_t image_width;
    int32_t has_samples_per_pixel; int32_t samples_per_pixel;
    int32_t has_max_depth;      int32_t max_depth;
    int32_t has_vfov;           double vfov;
    int32_t has_lookfrom;       double lookfrom[3];
    int32_t has_lookat;         double lookat[3];
    int32_t has_vup;            double vup[3];
    int32_t has_defocus_angle;  double defocus_angle;
    int32_t has_focus_dist;     double focus_dist;
    int32_t has_background;     double background[3];
} RrtOverrides;

/* ---- flags ------------------------------------------------------------------------ */
/* Book-2 camera: each camera ray draws a `time` sample after the jitter/disk draws
 * (the_next_week/camera.rs:160). Required for bit-parity with the book-2 oracle. */
#define RRT_FLAG_RAY_TIME 0x1u
/* Suppress the stderr progress lines (cuda/mod.rs:426-431 style). */
#define RRT_FLAG_QUIET 0x2u
/* Book-3 integrator (the_rest_of_your_life/camera.rs:96-254): stratified camera samples
 * (samples_per_pixel must be a square, sqrt_spp^2; sample s = s_j * sqrt_spp + s_i), one-sided
 * DiffuseLight, Lambertian / Isotropic scatter by the mixture pdf 0.5 * lights + 0.5 * material
 * (cosine / sphere pdf) over RrtSceneExt.lights, Russian roulette folded into the weight.
 * Requires RRT_FLAG_RAY_TIME (the book-3 camera draws a time per ray). */
#define RRT_FLAG_BOOK3 0x4u
/* The books path's own arithmetic (ABI v7): the kernel computes in f64, in the reference CPU path's
 * operation order (vec3.rs, sphere.rs:24-51, material.rs, camera.rs:152-209; no FP contraction),
 * on the same per-path random stream as the f32 kernel, and sums in f64 — so every path takes the
 * books path's decisions and the sums match it to a few f64 ulps (the north star's check "against
 * the repo's own CPU books path"). Book-1 scenes: material kinds 0-4, sky or background, no
 * RrtSceneExt data, not RRT_FLAG_BOOK3 (RRT_E_INVALID otherwise). Float entries return the f64 sums
 * rounded to f32; rrt_hip_render_f64 / rrt_render_tile_f64_async return them unrounded. */
#define RRT_FLAG_F64 0x8u
/* Scene creation builds the BVH on the device instead of the host (additive; RRT_ABI_VERSION is
 * unchanged): a binned SAH builder (16 bins per axis, all three axes; rrt_bvh_binned.h) that emits
 * the node formats the render kernels already read, so the kernels are the same. Accepted by
 * rrt_scene_create / _ex and every one-shot entry (rrt_hip_render, _ex, _f64, _rgb8, _rgb8_ex,
 * _f64_rgb8). The composition is scene creation's own: the LDS shape (leaves of up to 3, node price 2,
 * or 1.5 with RRT_FLAG_F64) kept if it fits, else the global shape (single-primitive leaves, 32-B
 * nodes), else the fallbacks of the host path; RRT_MAX_LEAF, RRT_MAX_LEAF_GLOBAL, RRT_SAH_CT and
 * RRT_F64_SAH_CT_LDS apply, RRT_BVH_SPLIT is ignored, RRT_BVH_WIDTH=4 is refused (RRT_E_INVALID).
 * The tree differs from the host builder's (other splits), never a primitive's result; its bytes
 * are those of rrt_build_bvh_binned for the kept shape. A tree of at most one primitive is the
 * root-leaf form and is written by the host builder. RrtBvhInfo.max_leaf_param then reports the kept
 * shape's leaf size. Without the flag nothing changes. */
#define RRT_FLAG_DEVICE_BVH 0x10u
/* The f64 books path for the slice of book 2 its kernel covers (additive; RRT_ABI_VERSION is
 * unchanged). Implies RRT_FLAG_F64. rrt_scene_create_ex then also accepts sphere_motion (needs
 * RRT_FLAG_RAY_TIME, as for f32: the path keeps the camera's time draw and every sphere is tested at
 * center1 + time * motion, the_next_week/sphere.rs:44), quads (quad.rs:61-87 on the unrounded f64
 * plane; Lambertian, checker, metal, dielectric or diffuse-light materials) and material kinds 0-5 on
 * spheres (checker textures, texture.rs:66-77; kind 3 image textures as for RRT_FLAG_F64). Bit-identical
 * to the reference's CPU books path on the_next_week scenes 1, 2, 5 and 7 (exact t-ties between two
 * primitives aside, which go by tree order on either side). Still RRT_E_INVALID, before any device
 * call: Perlin tables or kind 6, media, boundary quads or kind 7, lights or RRT_FLAG_BOOK3, more than
 * 65535 BVH nodes; the message names this flag and the item. A book-1 scene created with the flag
 * renders the bits RRT_FLAG_F64 alone renders. RRT_FLAG_F64 alone keeps refusing book-2 data. */
#define RRT_FLAG_F64_BOOK2 0x20u
/* The fast builder (additive; RRT_ABI_VERSION is unchanged): scene creation and every later
 * rrt_scene_update_* build the tree on the device by an LBVH (rrt_bvh_lbvh.h: 30-bit Morton codes of
 * the centroids, one sort, Karras' topology) instead of the binned SAH builder: a fixed number of
 * launches whatever the tree's depth and one blocking read per build, against the binned builder's
 * eight launches and one read per level. The tree traces slower (DESIGN.md section 5 has both numbers per
 * scene); it is the choice for geometry that moves too much for a refit. Implies RRT_FLAG_DEVICE_BVH
 * and is accepted wherever that flag is; RRT_BVH_WIDTH=4 is refused (RRT_E_INVALID), RRT_BVH_SPLIT,
 * RRT_SAH_CT and RRT_F64_SAH_CT_LDS are ignored (no SAH decision is made), RRT_MAX_LEAF and
 * RRT_MAX_LEAF_GLOBAL apply. The composition is the device flag's: the LDS shape (leaves of up to 3)
 * kept if it fits, else the global shape (single-primitive leaves, 32-B nodes), else the host path's
 * fallbacks; both shapes come out of one sorted order, so no shape is built twice. The bytes are
 * those of rrt_build_bvh_lbvh for the kept shape, whose leaf size RrtBvhInfo.max_leaf_param reports.
 * A tree of at most one primitive is written by the host builder. The refits keep the tree's
 * topology and rrt_scene_tree_cost works, as for the binned builder; rrt_scene_set_builder switches
 * between the two. Without the flag nothing changes. */
#define RRT_FLAG_FAST_BVH 0x40u

/* ---- error codes ------------------------------------------------------------------ */
#define RRT_OK 0
#define RRT_E_INVALID (-1)
#define RRT_E_HIP (-2)
#define RRT_E_NOMEM (-3)
#define RRT_E_NODEV (-4)
#define RRT_E_IO (-5)

/* ---- one-shot drop-in entry (replaces cuda::imp::render, cuda/mod.rs:342-439) ----------
 * Renders total_spp samples per pixel of the scene on n_gpus devices (row-interleaved
 * bands, one host thread per device), writes RGBA float accum into caller-owned
 * accum_out[W*H*4] (W,H = params_f[1], params_f[2]); accum_out[4i+3] = sample count.
 * total_spp == 0 means params_f[3] (cuda/mod.rs:384). BVH is built inside. */
int32_t rrt_hip_render(const RrtCamera *cam,
                       const RrtSphere *spheres, uint32_t n_spheres,
                       const RrtMaterial *materials, uint32_t n_materials,
                       const RrtTexture *textures, uint32_t n_textures,
                       uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                       float *accum_out);

/* rrt_hip_render with book-2 scene data (moving spheres, Perlin tables); ext may be NULL. */
int32_t rrt_hip_render_ex(const RrtCamera *cam,
                          const RrtSphere *spheres, uint32_t n_spheres,
                          const RrtMaterial *materials, uint32_t n_materials,
                          const RrtTexture *textures, uint32_t n_textures,
                          const RrtSceneExt *ext,
                          uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                          float *accum_out);

/* rrt_hip_render with RRT_FLAG_F64 implied, returning the f64 sums unrounded: accum_out[W*H*4]
 * doubles (RGB sums, [4i+3] = sample count). The books path's own arithmetic end to end (the
 * reference's CPU ray_color sums pixel_color in f64, camera.rs:73-76); quantise with
 * rrt_quantize_accum_books_f64 for the bytes camera.rs:87-94 prints. */
int32_t rrt_hip_render_f64(const RrtCamera *cam,
                           const RrtSphere *spheres, uint32_t n_spheres,
                           const RrtMaterial *materials, uint32_t n_materials,
                           const RrtTexture *textures, uint32_t n_textures,
                           uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                           double *accum_out);

/* rrt_hip_render_f64 with book-2 scene data: RRT_FLAG_F64 and RRT_FLAG_F64_BOOK2 are implied; ext
 * may be NULL (then it is rrt_hip_render_f64). Same multi-device path. */
int32_t rrt_hip_render_f64_ex(const RrtCamera *cam,
                              const RrtSphere *spheres, uint32_t n_spheres,
                              const RrtMaterial *materials, uint32_t n_materials,
                              const RrtTexture *textures, uint32_t n_textures,
                              const RrtSceneExt *ext,
                              uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                              double *accum_out);

/* Thread-local message for the last failing call on this thread ("" if none). */
const char *rrt_hip_last_error(void);
uint32_t rrt_hip_abi_version(void);

/* Summation order of the accum: a pixel's RGB = sum over consecutive chunks of its S samples
 * (counted from the tile's sample_begin) of each chunk's in-order sample sum, chunks added in
 * order: ((c0 + c1) + c2) + ... With K = rrt_accum_chunk() halved while S <= 2K, down to
 * rrt_accum_chunk() / 4 (ABI v9: 256 for S > 512, 128 for 256 < S <= 512, 64 below; big chunks at
 * high spp, small ones at low spp), and k = max(1, K / 4), or max(1, K / 8) for
 * S <= rrt_accum_chunk() / 4 (ABI v11; K / 8 for every S before v10): the first
 * nb = (S - 1) / K chunks hold K samples each (nb = 0 when S <= K), the remaining S - nb*K
 * samples form chunks of k (the last one possibly shorter) — small units at the end of the
 * work queue keep the persistent grid's tail short. Needed to reproduce it bit for bit.
 * The chunk partial sums live in a device buffer of at most RRT_PARTIAL_MB MiB (env, default
 * 2048); a render with more chunks than fit runs as consecutive sample passes of whole chunks,
 * each continuing the same fold, so the bits do not depend on the budget.
 * The f64 books path (RRT_FLAG_F64) sums each pixel's samples in sample order instead, as
 * camera.rs:72-76 does: ((s0 + s1) + s2) + ... from 0. */
uint32_t rrt_accum_chunk(void);

/* ---- device-resident API (bench / multi-rank hosts) --------------------------------- */
typedef struct RrtScene RrtScene;

/* A tile = the rows this rank owns (row bands of `band_rows`, dealt in serpentine order: band b
 * lies in period p = b / n_ranks at slot s = b % n_ranks and belongs to rank s when p is even,
 * n_ranks - 1 - s when p is odd) crossed with the sample range [sample_begin, sample_end). The
 * tile's rows are its bands in image order. */
typedef struct RrtTile {
    uint32_t band_rows;
    uint32_t rank;
    uint32_t n_ranks;
    uint32_t sample_begin;
    uint32_t sample_end;
} RrtTile;

/* Counters accumulated by every render launch on the scene since the last reset.
 * rays = closest-hit queries (camera + scattered: one world.hit, camera.rs:187).
 * node_visits / sphere_tests are only filled by rrt_scene_count_work (instrumented). */
typedef struct RrtCounters {
    uint64_t rays;
    uint64_t paths;
    uint64_t node_visits;
    uint64_t box_tests;
    uint64_t sphere_tests;
} RrtCounters;

/* Uploads the scene to `device`, builds the BVH (SAH, bvh.rs:21-156 criterion) on the host. */
int32_t rrt_scene_create(const RrtCamera *cam,
                         const RrtSphere *spheres, uint32_t n_spheres,
                         const RrtMaterial *materials, uint32_t n_materials,
                         const RrtTexture *textures, uint32_t n_textures,
                         uint32_t flags, int32_t device, RrtScene **out);
/* rrt_scene_create with book-2 scene data; ext may be NULL. */
int32_t rrt_scene_create_ex(const RrtCamera *cam,
                            const RrtSphere *spheres, uint32_t n_spheres,
                            const RrtMaterial *materials, uint32_t n_materials,
                            const RrtTexture *textures, uint32_t n_textures,
                            const RrtSceneExt *ext,
                            uint32_t flags, int32_t device, RrtScene **out);
int32_t rrt_scene_destroy(RrtScene *scene);

/* Number of image rows `tile` owns in an image of `height` rows (its accum is rows*W float4). */
int32_t rrt_tile_rows(uint32_t height, const RrtTile *tile, uint32_t *rows_out);
/* Global image row of the tile's local row `local_row`. */
int32_t rrt_tile_row_index(uint32_t height, const RrtTile *tile, uint32_t local_row, uint32_t *row_out);

/* Enqueue the render of `tile` on `stream` (a hipStream_t, NULL = default stream).
 * d_accum: device pointer to rows*W*4 floats, OVERWRITTEN with this tile's sums
 * (RGB sums over the tile's samples, w = sample count). Asynchronous.
 * One render in flight per RrtScene: the scene owns one work-queue head and one chunk-partial
 * buffer, so renders of the same scene must be ordered on one stream (or synchronised);
 * concurrent renders on different streams need one RrtScene each. */
int32_t rrt_render_tile_async(RrtScene *scene, const RrtTile *tile, float *d_accum, void *stream);
/* The same for a scene created with RRT_FLAG_F64: d_accum = rows*W*4 doubles (f64 sums, w = count),
 * overwritten. (rrt_render_tile_async on such a scene writes the f64 sums rounded to f32.) */
int32_t rrt_render_tile_f64_async(RrtScene *scene, const RrtTile *tile, double *d_accum, void *stream);

/* Counters (synchronises the scene's device). */
int32_t rrt_scene_read_counters(RrtScene *scene, RrtCounters *out);
int32_t rrt_scene_reset_counters(RrtScene *scene);
/* Runs the instrumented kernel variant (same seed => same paths) over `tile` into a
 * scratch accum and returns node visits / box tests / sphere tests / rays / paths. */
int32_t rrt_scene_count_work(RrtScene *scene, const RrtTile *tile, RrtCounters *out);

/* BVH summary: nodes, leaves, max depth, bytes resident. */
typedef struct RrtBvhInfo {
    uint32_t n_nodes;
    uint32_t n_leaves;
    uint32_t max_depth;
    uint32_t max_leaf_size;
    uint64_t node_bytes;
    uint64_t prim_bytes;
    uint32_t width;          /* 2: binary nodes, 4: 128-B 4-wide nodes */
    uint32_t max_leaf_param; /* leaf size the builder was asked for */
    uint32_t node_stride;    /* bytes per node: 80 (BVH2 staged in LDS: sign-ordered planes), 32 (BVH2 read
                                from global memory: GNodeH, f16 planes), 128 (BVH4); layouts in DESIGN.md */
    uint32_t n_unbounded;    /* the last n_unbounded primitives of the leaf order are not in the tree: media
                                whose boundary sphere holds the whole scene, tested after the walk (ABI v6) */
} RrtBvhInfo;
int32_t rrt_scene_bvh_info(const RrtScene *scene, RrtBvhInfo *out);

/* Host-only: the BVH rrt_scene_create would build for these spheres (width / max_leaf 0 =
 * the defaults; max_leaf <= 7 for width 2, <= 15 for width 4), as the device node array (80-B or
 * 32-B BVH2 nodes — info->node_stride, the layout scene creation picks — or 128-B BVH4 nodes,
 * layouts in DESIGN.md) and the leaf-order permutation of the spheres.
 * Call with nodes_cap 0 to size (info->node_bytes). Lets a checker walk exactly the tree the
 * kernel walks. */
int32_t rrt_build_bvh(const RrtSphere *spheres, uint32_t n_spheres, uint32_t width, uint32_t max_leaf,
                      void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out, RrtBvhInfo *info);
/* The same over the book-2 scene (ext may be NULL): a moving sphere's box spans both ends of its
 * motion (Aabb::from_boxes, the_next_week/sphere.rs:31-33); quads join the primitives as indices
 * n_spheres + j (prim_order_out then holds n_spheres + n_quads entries). */
int32_t rrt_build_bvh_ex(const RrtSphere *spheres, uint32_t n_spheres, const RrtSceneExt *ext, uint32_t width,
                         uint32_t max_leaf, void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out,
                         RrtBvhInfo *info);

/* Host-only: the tree RRT_FLAG_DEVICE_BVH builds for one shape and node format, by the sequential
 * host twin of the device builder (same header, same bytes): leaves of up to max_leaf (1..7)
 * primitives, the SAH node price node_cost, node_stride 80 (GNode) or 32 (GNodeH). Same primitive
 * order, unbounded media and sizing protocol (nodes_cap 0 sizes) as rrt_build_bvh_ex. It is the
 * specification the device builder is held to, and the tree a checker passes to a BVH-walking
 * reference. */
int32_t rrt_build_bvh_binned(const RrtSphere *spheres, uint32_t n_spheres, const RrtSceneExt *ext, uint32_t max_leaf,
                             double node_cost, uint32_t node_stride, void *nodes_out, size_t nodes_cap,
                             uint32_t *prim_order_out, RrtBvhInfo *info);

/* Host-only: the tree RRT_FLAG_FAST_BVH builds for one shape and node format, by the sequential host
 * twin of the device LBVH builder (rrt_bvh_lbvh.h on both sides, same bytes). Sizing protocol,
 * primitive order, unbounded media and refusals are rrt_build_bvh_binned's; there is no node_cost
 * because no SAH decision is made. RRT_BVH_WIDTH=4 is refused. */
int32_t rrt_build_bvh_lbvh(const RrtSphere *spheres, uint32_t n_spheres, const RrtSceneExt *ext, uint32_t max_leaf,
                           uint32_t node_stride, void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out,
                           RrtBvhInfo *info);

/* The node array and leaf order the created scene holds, whichever builder made them: nodes_out of
 * at least rrt_scene_bvh_info's node_bytes, prim_order_out of n_spheres + n_quads + n_media entries
 * (the last n_unbounded outside the tree). Copies from the scene's device. Also the only view of the
 * tree of an RRT_FLAG_F64 scene, or of a scene whose book-2 materials tip the LDS fit, which
 * rrt_build_bvh_ex cannot reproduce. */
int32_t rrt_scene_read_bvh(RrtScene *scene, void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out);

/* ---- changing a created scene (additive; RRT_ABI_VERSION is unchanged) ------------------ */

/* Replaces everything scene creation derives from the camera: rays, seed, max_depth, background,
 * width/height, and for RRT_FLAG_BOOK3 the sqrt_spp rule with its validation. Host state only: it
 * affects renders enqueued after it returns. Works on every scene; a refused camera leaves the
 * scene as it was. */
int32_t rrt_scene_set_camera(RrtScene *scene, const RrtCamera *cam);

/* Replaces the scene's spheres (centers, radii, material_index) and, for a book-2 world, their
 * motion rows (n_spheres x 4 floats as RrtSceneExt.sphere_motion; NULL = all zero). Rebuilds the BVH
 * on the device and re-forms every per-primitive table there; the scene then holds, bit for bit,
 * what rrt_scene_create_ex would make of the new inputs (tree, leaf order, tables, every frame).
 * n_spheres must equal the scene's. Quads, materials, textures and Perlin tables are kept. Waits
 * for `stream` (and for a refit still in flight), then runs and returns synchronised. From the
 * second update of a scene on, no device memory is allocated or freed.
 * Refused with RRT_E_INVALID, before any device call and with the scene untouched: null arguments
 * or another n_spheres; a material_index out of range; a scene not created with
 * RRT_FLAG_DEVICE_BVH; a scene with media; an RRT_FLAG_BOOK3 scene; a tree of fewer than 2
 * primitives; a non-zero motion row on a scene that was not created as a book-2 world (the kernel
 * class is fixed at creation; a book-2 world accepts any motion, all-zero included).
 * A failure after device work has begun (a HIP error, or a tree over the depth or node limits of
 * scene creation) leaves the scene invalid: its renders fail, naming the failed update, until a
 * later update succeeds. */
int32_t rrt_scene_update_spheres(RrtScene *scene, const RrtSphere *spheres, uint32_t n_spheres,
                                 const float *motion, void *stream);

/* Refit: the same replacement of the spheres (and motion rows) as rrt_scene_update_spheres, with the
 * same arguments and the same refusals before any device call, but the tree keeps the topology and
 * leaf order of the last build (scene creation or the last update): only its boxes are recomputed,
 * bottom-up from the moved spheres, on the device. The result is, bit for bit, the tree of
 * rrt_refit_bvh_binned and the per-primitive tables of a fresh scene in the kept leaf order; frames are
 * correct for the new spheres (every stored box contains its primitives), and an RRT_FLAG_F64
 * scene's are bit for bit a fresh scene's. RrtBvhInfo, depth and the launch plan cannot change.
 * Everything is enqueued on `stream` (NULL: the default stream): the copy of the rows, the boxes, the
 * refit, the node pack and the tables. The call returns without waiting for the device, the caller's
 * arrays may be reused as soon as it returns, and a render enqueued on `stream` afterwards sees the
 * refitted scene; work on another stream is the caller's to order. The first change of a scene
 * allocates (and waits for `stream` if it has to replace the node array); later refits allocate and
 * free nothing. Refits compose; a later rrt_scene_update_spheres rebuilds, after which the scene is
 * again the freshly created one. A refitted tree renders more slowly the further the spheres have
 * moved: rrt_scene_tree_cost tells when to rebuild. A HIP error after device work began leaves the
 * scene invalid exactly as a failed update does. */
int32_t rrt_scene_refit_spheres(RrtScene *scene, const RrtSphere *spheres, uint32_t n_spheres,
                                const float *motion, void *stream);

/* The SAH cost of the tree the scene holds now (sah), of the tree its last build made (sah_at_build)
 * and the refits since. Over the builder's unrounded f64 boxes: node k's term is w0 A(box0) + w1
 * A(box1), A the surface area, w a leaf child's primitive count or the kept shape's node price for a
 * node child; the terms are summed for k = 0 .. n-1 in that order and divided by the root box's
 * area, so the value is defined bit for bit (rrt_refit_bvh_binned's sah_out). Synchronises the
 * scene's device; on demand, not for every frame. Needs a scene the device builder built. */
typedef struct RrtTreeCost {
    double sah;
    double sah_at_build;
    uint64_t refits_since_build;
} RrtTreeCost;
int32_t rrt_scene_tree_cost(RrtScene *scene, RrtTreeCost *out);

/* Host-only: the specification the device refit is held to. Builds the tree of rrt_build_bvh_binned
 * over the built_* inputs, recomputes its boxes over the new spheres and motion rows (NULL = all
 * zero; quads and media keep their boxes), and writes the nodes with the new root box's slack. Same
 * sizing protocol and refusals as rrt_build_bvh_binned; the leaf order and info are the built
 * tree's. sah_out (may be NULL): the refitted tree's cost as rrt_scene_tree_cost defines it. */
int32_t rrt_refit_bvh_binned(const RrtSphere *built_spheres, uint32_t n_spheres, const RrtSceneExt *built_ext,
                             uint32_t max_leaf, double node_cost, uint32_t node_stride,
                             const RrtSphere *new_spheres, const float *new_motion,
                             void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out,
                             RrtBvhInfo *info, double *sah_out);

/* ---- changing quads and book-3 lights too (additive; RRT_ABI_VERSION is unchanged) -------- */

/* The geometry of a created scene, replaced as a whole. spheres / n_spheres / sphere_motion: as the
 * arguments of rrt_scene_update_spheres (n_spheres must equal the scene's; motion NULL = all zero).
 * quads: NULL keeps the scene's quads; else n_quads must equal the scene's, and each quad's q, u, v,
 * and material_index replace the old. lights: for an RRT_FLAG_BOOK3 scene required, n_lights equal
 * to the scene's and each entry's kind unchanged (the light list restates geometry: move a light
 * with the quad or sphere it samples); for any other scene NULL / 0. Materials, textures and Perlin
 * tables are kept. */
typedef struct RrtSceneGeometry {
    const RrtSphere *spheres;
    uint32_t n_spheres;
    const float *sphere_motion;
    const RrtQuad *quads;
    uint32_t n_quads;
    const RrtLight *lights;
    uint32_t n_lights;
} RrtSceneGeometry;

/* rrt_scene_update_spheres' contract extended to quads and lights: rebuilds the BVH on the device
 * over the new sphere and quad boxes and re-forms there everything scene creation derives from the
 * geometry, after which the scene holds, bit for bit, what rrt_scene_create_ex makes of the new
 * inputs: the tree, the leaf order and RrtBvhInfo, every per-primitive table, the quad records (scene
 * quads and light quads; the unrounded ones of an RRT_FLAG_F64_BOOK2 scene), the quads' table rows
 * and material indices, the light records, every frame and its ray count. Waits for `stream` (and for
 * a refit still in flight), then runs and returns synchronised. From the second geometry change of a
 * scene on, no device memory is allocated or freed.
 * Refused with RRT_E_INVALID, before any device call and with the scene untouched: everything
 * rrt_scene_update_spheres refuses except RRT_FLAG_BOOK3 (a scene without RRT_FLAG_DEVICE_BVH, with
 * media, of fewer than 2 primitives, ...); a scene with boundary quads; another n_quads or n_lights;
 * a light whose kind differs from the scene's entry; lights missing on an RRT_FLAG_BOOK3 scene or
 * given on any other; a quad material_index out of range or naming an image-textured material
 * (scene creation's rule); a quad (or a quad light) whose q, u or v is not finite or whose u x v has
 * a zero or non-finite squared length. The last is refused because a NaN formed on the host and one
 * formed on the device need not agree in sign and payload, so the bit-for-bit contract cannot cover
 * such quads (scene creation still accepts them).
 * A failure after device work has begun leaves the scene invalid exactly as a failed
 * rrt_scene_update_spheres does. */
int32_t rrt_scene_update_geometry(RrtScene *scene, const RrtSceneGeometry *geometry, void *stream);

/* rrt_scene_refit_spheres' contract extended to quads and lights, with rrt_scene_update_geometry's
 * arguments and refusals: the tree keeps the topology and leaf order of the last build, its boxes
 * are recomputed bottom-up from the new sphere and quad boxes (bit for bit rrt_refit_bvh_binned_ex),
 * and every derived record and table is re-formed, in the kept leaf order. Everything is enqueued on
 * `stream` with no host synchronisation; the pinned staging buffer holds the quad and light rows
 * behind the spheres', sized once at the first geometry refit. Later geometry refits allocate and
 * free nothing. Refits of both kinds compose with each other and with either update, and
 * rrt_scene_tree_cost keeps working across them. */
int32_t rrt_scene_refit_geometry(RrtScene *scene, const RrtSceneGeometry *geometry, void *stream);

/* Host-only: rrt_refit_bvh_binned with new quads as well (new_quads: built_ext's n_quads records, or
 * NULL = the built ones; media keep their boxes). The specification of rrt_scene_refit_geometry's
 * tree, sah_out included. */
int32_t rrt_refit_bvh_binned_ex(const RrtSphere *built_spheres, uint32_t n_spheres, const RrtSceneExt *built_ext,
                                uint32_t max_leaf, double node_cost, uint32_t node_stride,
                                const RrtSphere *new_spheres, const float *new_motion, const RrtQuad *new_quads,
                                void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out,
                                RrtBvhInfo *info, double *sah_out);

/* ---- changing constant media and their boundaries too (additive; RRT_ABI_VERSION is unchanged) ---- */

/* The media of a created scene, replaced as a whole. media: NULL keeps the scene's media; else
 * n_media must equal the scene's and each entry's boundary_kind, first and count must equal the
 * scene's entry (the structure is fixed at creation, as a light's kind is): its sphere row, density
 * and material_index replace the old. boundary_quads: NULL keeps the scene's boundary quads; else
 * n_boundary_quads must equal the scene's and each quad's q, u, v replace the old. */
typedef struct RrtSceneMedia {
    const RrtMedium *media;          /* NULL keeps the scene's media */
    uint32_t n_media;
    uint32_t n_boundary_quads;
    const RrtQuad *boundary_quads;   /* NULL keeps the scene's boundary quads */
} RrtSceneMedia;

/* rrt_scene_update_geometry's contract extended to constant media: accepts every scene that entry
 * accepts, and also scenes with media and / or boundary quads (f32 scenes: the f64 kernels refuse
 * media at creation). media == NULL keeps the scene's media and boundary quads. Which media are
 * tested outside the tree (RrtBvhInfo.n_unbounded) is decided again on the host from the new inputs,
 * by scene creation's rule, and may change between updates, the tree's primitive count with it.
 * Afterwards the scene holds, bit for bit, what rrt_scene_create_ex with RRT_FLAG_DEVICE_BVH makes of
 * the new inputs: the classification and the tail of the leaf order, the tree over the remaining
 * primitives, every per-primitive table, the quad records (scene quads, boundary quads, light
 * quads), the medium records, the light records, every frame and its ray count. From the second
 * change of a scene on, no device memory is allocated or freed, whichever way the classification
 * flips.
 * Refused with RRT_E_INVALID, before any device call and with the scene untouched: everything
 * rrt_scene_update_geometry refuses except media and boundary quads; another n_media or
 * n_boundary_quads; a medium whose boundary_kind, first or count differs from the scene's entry; a
 * medium material_index out of range or naming no RRT_MAT_ISOTROPIC material, or a density that is
 * not positive and finite (scene creation's rules); a sphere-bounded medium whose sphere row is not
 * finite; a boundary quad whose q, u or v is not finite or whose u x v has a zero or non-finite
 * squared length (rrt_scene_update_geometry's reason); a new classification that leaves fewer than 2
 * primitives in the tree. */
int32_t rrt_scene_update_world(RrtScene *scene, const RrtSceneGeometry *geometry,
                               const RrtSceneMedia *media, void *stream);

/* rrt_scene_refit_geometry's contract extended to constant media, with rrt_scene_update_world's
 * arguments and refusals (but the last): topology, leaf order and the classification of the last
 * build are kept — a medium tested after the walk stays correct wherever the geometry moves, a
 * medium in the tree as long as its box is recomputed, which this does from its new boundary (bit
 * for bit rrt_refit_bvh_binned_world). Everything is enqueued on `stream` with no host wait; the
 * pinned staging buffer holds spheres | motion | quads | lights | media | boundary quads, sized
 * once. Refits compose with each other, with the sphere and geometry refits where those apply, and
 * with every update; rrt_scene_tree_cost keeps working across them. */
int32_t rrt_scene_refit_world(RrtScene *scene, const RrtSceneGeometry *geometry,
                              const RrtSceneMedia *media, void *stream);

/* Host-only: rrt_refit_bvh_binned_ex with the new geometry taken from a second RrtSceneExt (its
 * sphere_motion, NULL = all zero; its quads, media and boundary_quads, NULL = the built ones;
 * new_ext == NULL = no motion, everything else as built). The counts, and
 * each medium's boundary_kind, first and count, must equal built_ext's. The classification and the
 * leaf order are the built tree's. The specification of rrt_scene_refit_world's tree, sah_out
 * included. */
int32_t rrt_refit_bvh_binned_world(const RrtSphere *built_spheres, uint32_t n_spheres,
                                   const RrtSceneExt *built_ext, uint32_t max_leaf, double node_cost,
                                   uint32_t node_stride, const RrtSphere *new_spheres,
                                   const RrtSceneExt *new_ext,
                                   void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out,
                                   RrtBvhInfo *info, double *sah_out);

/* Host-only: rrt_refit_bvh_binned_world over the tree of rrt_build_bvh_lbvh: the specification of the
 * three refits of a scene whose current tree the fast builder made. sah_out weighs a node child by 2
 * (what rrt_scene_tree_cost uses for such an f32 scene; an f64 scene's LDS shape weighs it by 1.5). */
int32_t rrt_refit_bvh_lbvh_world(const RrtSphere *built_spheres, uint32_t n_spheres,
                                 const RrtSceneExt *built_ext, uint32_t max_leaf, uint32_t node_stride,
                                 const RrtSphere *new_spheres, const RrtSceneExt *new_ext,
                                 void *nodes_out, size_t nodes_cap, uint32_t *prim_order_out,
                                 RrtBvhInfo *info, double *sah_out);

/* Chooses the builder of the scene's next rrt_scene_update_*: RRT_BUILDER_BINNED (quality) or
 * RRT_BUILDER_LBVH (speed). Host state only. Works on every scene the device builder built (either
 * flag, at least 2 primitives in the tree; RRT_E_INVALID otherwise, and for another value). Meant for
 * fast rebuilds while things move and one quality rebuild when they stop. The first update after a
 * switch may allocate the other builder's workspace; later ones allocate nothing. Refits and
 * rrt_scene_tree_cost follow whichever build is current. */
enum { RRT_BUILDER_BINNED = 0, RRT_BUILDER_LBVH = 1 };
int32_t rrt_scene_set_builder(RrtScene *scene, uint32_t builder);

/* ---- ray queries on a created scene ---------------------------------------------------- */

/* The render's closest-hit query (world.hit(ray, Interval(0.001, t_max)): hittable_list.rs,
 * bvh.rs:159-172, camera.rs:187) on the caller's rays, without shading: the kernel runs the node step
 * and the leaf tests the render runs, on the tree and the primitive tables the render reads.
 *
 * One ray: origin o, direction d (any length), the interval's end tmax, and the time at which moving
 * spheres are met (center + time * motion, rounded as the render rounds it; ignored by a scene
 * without motion rows). A sphere's root is accepted in the open interval (0.001, tmax), a quad's in
 * the closed interval [0.001, tmax], each against the running closest hit exactly as the render's leaf
 * tests accept it: tmax is the closest hit the walk starts from (the render starts from +inf, which
 * gives the render's own query). A tmax that is NaN or <= 0.001 finds nothing. No primitive is skipped.
 *
 * One answer: prim is the hit primitive's index in source order, spheres first, then quads as
 * n_spheres + j (rrt_build_bvh_ex's order), and t its root; a miss gives prim = RRT_NO_PRIM, t = 0.
 * RRT_QUERY_CLOSEST: the closest hit; of two primitives at exactly the same t the tree's order decides,
 * as in the render. RRT_QUERY_ANY: the ray leaves the tree after the first batch of leaf tests that
 * accepted something, and (t, prim) is that hit: prim != RRT_NO_PRIM exactly when the closest query
 * finds a hit, but it need not be the closest one. A ray's answer does not depend on the other rays of
 * the call. */
typedef struct RrtRay { float o[3]; float tmax; float d[3]; float time; } RrtRay;   /* 32 B */
typedef struct RrtHit { float t; uint32_t prim; } RrtHit;                           /* 8 B  */
#define RRT_NO_PRIM 0xffffffffu
enum { RRT_QUERY_CLOSEST = 0, RRT_QUERY_ANY = 1 };

/* n rays at d_rays (device memory, 16-byte aligned) answered into d_hits (device memory, 8-byte
 * aligned), enqueued on `stream`: the query sees every update or refit enqueued on that stream before
 * it, and like a render it is the scene's one piece of work in flight. RrtCounters are left alone.
 * n = 0 enqueues nothing. The first query of a scene allocates a device copy of the leaf order (blocking);
 * an rrt_scene_update_* replaces its contents, a refit keeps it, and later queries allocate nothing.
 * Refused with RRT_E_INVALID before any device call, the message naming the item: a null scene, null
 * or misaligned pointers with n > 0, an unknown mode, a scene with constant media (volumes with a
 * stochastic free flight, not surfaces), an RRT_FLAG_F64 scene (it holds the f64 kernel's tables), a
 * width-4 tree (RRT_BVH_WIDTH=4), a scene left invalid by a failed update. Book-3 scenes without media
 * are accepted. */
int32_t rrt_scene_query_async(RrtScene *scene, const RrtRay *d_rays, uint32_t n, uint32_t mode,
                              RrtHit *d_hits, void *stream);
/* The same for host arrays, synchronous, through device buffers the scene keeps and grows. */
int32_t rrt_scene_query(RrtScene *scene, const RrtRay *rays, uint32_t n, uint32_t mode, RrtHit *hits);
/* width * height records in row-major order (the camera's as rrt_scene_set_camera last left it):
 * record (x, y) is the closest hit of the path tracer's camera ray with zero jitter and no defocus,
 * origin = camera.origin, direction = ((pixel00 + du * (float)x) + dv * (float)y) - origin per
 * component with every operation rounded to f32, tmax = +inf, the given time. The same kernel as
 * the ray-array entries, the ray formed in the kernel; 64 consecutive lanes take an 8 x 8 pixel tile.
 * Refusals as above. */
int32_t rrt_scene_primary_hits_async(RrtScene *scene, float time, RrtHit *d_hits, void *stream);

/* ---- surface records of a created scene ------------------------------------------------- */

/* The closest-hit query above, answered with the reference's HitRecord (hittable.rs:20-32) instead of
 * (t, prim): the kernel that walked the tree writes the record from the values it holds when the walk
 * ends, each field in the f32 operations the render's shading step forms it by, so a picker, a
 * denoiser's albedo and normal buffers or a light baker read what a path would have seen. Closest hit
 * only. The rays, tmax and time mean what they mean for rrt_scene_query_async, and (prim, t) are bit for
 * bit what RRT_QUERY_CLOSEST answers for the ray on a scene that entry accepts.
 *
 * A hit:
 *   p          origin + t * direction, one fused multiply-add per component (Ray::at)
 *   t, prim    the root and the primitive's index in source order, as in RrtHit
 *   normal     the outward normal, negated when the ray meets the surface from inside (front_face = 0).
 *              Outward: a sphere's (p - center(time)) * (1 / r) with the 1 / r the render reads; a
 *              quad's stored unit normal
 *   front_face 1 when dot(direction, outward normal) < 0
 *   uv         a sphere's get_sphere_uv (sphere.rs:46-52) of the outward normal n:
 *              ((atan2(-n.z, n.x) + pi) / 2 pi, acos(-n.y) / pi), computed for every sphere whatever its
 *              material. A quad's is (0, 0): the kernels never read a quad's (u, v), because quads take
 *              no image texture
 *   kind       the material's kind (RrtMaterial): 0 Lambertian, 1 metal, 2 dielectric, 3 image texture,
 *              4 diffuse light, 5 checker, 6 noise
 *   albedo     by kind: 0, 1 the material's albedo; 2 (1, 1, 1); 3 the texel the render samples at uv;
 *              4 the emitted radiance, unconditionally (book 3's lights emit from their front face only:
 *              apply that with front_face); 5 the checker's colour at p; 6 the noise value at p in all
 *              three channels
 * A miss (also: a tmax that finds nothing, an empty tree): prim = RRT_NO_PRIM, kind = RRT_SURFACE_MISS,
 * albedo = the background term the render adds for that ray (the camera's background colour in
 * background mode 1, else the sky gradient on the unit direction), every other field 0. _pad is 0.
 *
 * Constant media are accepted here, and never answered: a medium, in the tree or tested after the walk,
 * is passed over without a test, so the record is the closest SURFACE, as if the scene's media and
 * their boundary quads were absent (kind 7, the isotropic phase function, is never reported). */
typedef struct RrtSurface {      /* 64 B, 16-byte aligned on the device */
    float p[3];      float t;
    float normal[3]; uint32_t prim;
    float albedo[3]; uint32_t kind;
    float uv[2];     uint32_t front_face; uint32_t _pad;
} RrtSurface;
#define RRT_SURFACE_MISS 0xffffffffu

/* n rays at d_rays answered into n records at d_out (device memory, both 16-byte aligned), enqueued on
 * `stream` like rrt_scene_query_async: behind the updates and refits on that stream, the scene's one
 * piece of work in flight, counters left alone, n = 0 enqueues nothing, the leaf-order copy shared with
 * the queries above. Refusals as there, the message naming the item, except that constant media are
 * accepted: a null scene, null or misaligned pointers with n > 0, an RRT_FLAG_F64 scene, a width-4
 * tree, a scene left invalid by a failed update. */
int32_t rrt_scene_surface_async(RrtScene *scene, const RrtRay *d_rays, uint32_t n, RrtSurface *d_out, void *stream);
/* The same for host arrays, synchronous, through the device buffers rrt_scene_query grows. */
int32_t rrt_scene_surface(RrtScene *scene, const RrtRay *rays, uint32_t n, RrtSurface *out);
/* width * height records in row-major order: the G-buffer of the current camera. Record (x, y) is the
 * surface record of rrt_scene_primary_hits_async's ray through pixel (x, y), formed in the kernel by
 * that entry's expression, in the same 8 x 8 tiles. */
int32_t rrt_scene_primary_surface_async(RrtScene *scene, float time, RrtSurface *d_out, void *stream);

/* ---- host-side callers of the boundary ------------------------------------------------ */

/* == gpu::build_in_one_weekend_scene (gpu/mod.rs:124-301): RTOW final scene from
 * SmallRng::seed_from_u64(seed) (reference: 0x5EED_1234) with the grid a,b in
 * [-grid_half, grid_half) (reference: 11; 50 = the 10k-sphere stress config).
 * Writes up to sphere_cap spheres/materials; *n_spheres = needed count (call with
 * cap 0 to size). ov may be NULL (= RenderOverrides::none()). */
int32_t rrt_build_in_one_weekend_scene(const RrtOverrides *ov, uint64_t seed, int32_t grid_half,
                                       RrtCamera *cam, RrtSphere *spheres, RrtMaterial *materials,
                                       uint32_t sphere_cap, uint32_t *n_spheres);

/* Book-2 scenes (the_next_week/mod.rs:68-587) flattened into the ABI: 1 bouncing_spheres,
 * 2 checkered_spheres, 3 earth, 4 perlin_spheres, 5 quads, 6 simple_light, 7 cornell_box,
 * 8 cornell_smoke, 9 final_scene(800, 10000, 40), 10 final_scene(400, 250, 4) (main.rs's
 * default arm). Random draws come from SmallRng(seed) in the books' order (the reference uses
 * the entropy RNG: parity unpinned). Instanced geometry (make_box, RotateY, Translate, the
 * rotated sphere cluster of final_scene) is baked to world space. The caller sets the *_cap
 * fields and buffers (a buffer may be NULL with cap 0 to size); every n_* is set to the count
 * needed. uses_texture0 = 1 when a material samples texture 0, the earth image the caller
 * supplies. The camera carries book 2's background (bg_mode 1); render with RRT_FLAG_RAY_TIME
 * and an RrtSceneExt over these arrays. */
typedef struct RrtBookScene {
    RrtCamera camera;
    RrtSphere *spheres;
    float *sphere_motion; /* sphere_cap x 4 floats, may be NULL */
    RrtMaterial *materials;
    RrtQuad *quads;
    RrtPerlin *perlin;
    RrtMedium *media;
    RrtQuad *boundary_quads;
    RrtLight *lights;
    uint32_t sphere_cap, n_spheres;
    uint32_t material_cap, n_materials;
    uint32_t quad_cap, n_quads;
    uint32_t perlin_cap, n_perlin;
    uint32_t media_cap, n_media;
    uint32_t boundary_quad_cap, n_boundary_quads;
    uint32_t light_cap, n_lights;
    uint32_t uses_texture0;
    uint32_t flags; /* the RRT_FLAG_* the scene renders with (RAY_TIME; BOOK3 for book 3) */
} RrtBookScene;

int32_t rrt_build_next_week_scene(int32_t scene, const RrtOverrides *ov, uint64_t seed, RrtBookScene *out);

/* The book-3 scene (the_rest_of_your_life/mod.rs:69-161): the Cornell box with one rotated box
 * and a glass sphere, the light list {the light quad, the glass sphere} for MIS. The camera's
 * samples_per_pixel is rounded down to sqrt_spp^2 (Camera::initialize, camera.rs:115-117).
 * Render with out->flags (RRT_FLAG_RAY_TIME | RRT_FLAG_BOOK3) and an RrtSceneExt over the arrays
 * (lights included). */
int32_t rrt_build_rest_of_your_life_scene(const RrtOverrides *ov, uint64_t seed, RrtBookScene *out);

/* == A node of the books' object graph (the_next_week/hittable.rs:172-180 HittableObject), for
 * rrt_flatten_scene. 112 B; the payload is f64 like the books' Vec3, rounded to f32 once, after
 * the transforms. Children of a LIST / BVH node are children[first .. first + count);
 * TRANSLATE, ROTATE_Y and CONSTANT_MEDIUM take exactly one child (count 1).
 *   SPHERE          a = center1.xyz, radius; b.xyz = center2 - center1 (Sphere::new_moving; 0 = static)
 *   QUAD            a.xyz = q, b.xyz = u, c.xyz = v
 *   LIST, BVH       (no payload; a BVH node is flattened like a list: the backend builds its own tree)
 *   TRANSLATE       a.xyz = offset (hittable.rs:65-97)
 *   ROTATE_Y        a[0] = angle in degrees (hittable.rs:99-170)
 *   CONSTANT_MEDIUM a[0] = density; material = its Isotropic phase material; the child subtree is
 *                   the boundary: one sphere, or quads only (constant_medium.rs)
 * material: the RrtMaterial index of a SPHERE / QUAD / CONSTANT_MEDIUM. */
typedef struct RrtSceneNode {
    uint32_t kind;
    uint32_t material;
    uint32_t first;
    uint32_t count;
    double a[4];
    double b[4];
    double c[4];
} RrtSceneNode;

enum {
    RRT_NODE_SPHERE = 0,
    RRT_NODE_QUAD = 1,
    RRT_NODE_LIST = 2,
    RRT_NODE_BVH = 3,
    RRT_NODE_TRANSLATE = 4,
    RRT_NODE_ROTATE_Y = 5,
    RRT_NODE_CONSTANT_MEDIUM = 6
};

/* Flatten the object graph under `root` into the ABI's flat arrays: spheres with
 * motion rows, quads, media and their boundary quads, with every Translate / RotateY composed
 * and applied to the geometry in f64 (points rotate and translate, edge and motion vectors
 * rotate) — geometrically the reference's per-ray instance transforms, once per build instead of
 * twice per ray and instance. Graph sharing (one Arc under several parents) is flattened once
 * per path, as the reference would hit it once per path. Writes into out's sphere / motion /
 * quad / media / boundary-quad arrays under their caps (caps 0 = size only); camera, materials,
 * Perlin tables and lights are the caller's and left untouched. Errors: a cycle or depth > 64,
 * a child index out of range, a medium boundary mixing spheres and quads or holding a medium. */
int32_t rrt_flatten_scene(const RrtSceneNode *nodes, uint32_t n_nodes, const uint32_t *children,
                          uint32_t n_children, uint32_t root, RrtBookScene *out);

/* Camera::initialize (in_one_weekend/camera.rs:102-150) in f64, cast to the f32 ABI as
 * gpu/mod.rs:278-298 does. lookfrom/lookat/vup are 3-vectors. */
int32_t rrt_make_camera(double aspect_ratio, int32_t image_width, int32_t samples_per_pixel,
                        int32_t max_depth, double vfov, const double *lookfrom, const double *lookat,
                        const double *vup, double defocus_angle, double focus_dist,
                        const double *background /* NULL = sky */, uint32_t sample_seed,
                        uint32_t n_spheres, RrtCamera *cam);

/* Apply RenderOverrides to a Camera's parameters (in_one_weekend/mod.rs:23-55; book 2
 * the_next_week/mod.rs:31-65 also applies `background`). in/out by pointer. */
int32_t rrt_apply_overrides(const RrtOverrides *ov, int32_t book,
                            double *aspect_ratio, int32_t *image_width, int32_t *samples_per_pixel,
                            int32_t *max_depth, double *vfov, double *lookfrom, double *lookat,
                            double *vup, double *defocus_angle, double *focus_dist,
                            double *background, int32_t *has_background);

/* == render_io::write_ppm_from_accum (render_io.rs:3-31), byte-identical P3 text.
 * Writes to `path` ("-" = stdout). */
int32_t rrt_write_ppm_from_accum(uint32_t width, uint32_t height, const float *accum,
                                 uint32_t samples_per_pixel, const char *path);
/* Same bytes into a caller buffer; *written = bytes needed (call with cap 0 to size). */
int32_t rrt_format_ppm_from_accum(uint32_t width, uint32_t height, const float *accum,
                                  uint32_t samples_per_pixel, char *buf, size_t cap, size_t *written);
/* Quantiser only (render_io.rs:8-26): rgb8[3*W*H]. */
int32_t rrt_quantize_accum(uint32_t width, uint32_t height, const float *accum,
                           uint32_t samples_per_pixel, uint8_t *rgb8);

/* == books::in_one_weekend::color::write_color (color.rs:6-32), the books CPU path's quantiser,
 * over a float accum: per channel x = (1.0 / spp) * sum in f64 (camera.rs:107, 80), sqrt if
 * x > 0 else 0, Interval(0, 0.999).clamp, (256 * x) as i32 — so +inf gives 255 and NaN 0, where
 * render_io maps every non-finite value to 0. rgb8[3*W*H]; format P3 (the same "r g b" lines
 * camera.rs:87-94 prints) with rrt_format_pnm_from_rgb8. spp >= 1. */
int32_t rrt_quantize_accum_books(uint32_t width, uint32_t height, const float *accum,
                                 uint32_t samples_per_pixel, uint8_t *rgb8);
/* The same quantiser over f64 sums (rrt_hip_render_f64): the books path's bytes for its own f64
 * pixel_color, with no f32 rounding in between. */
int32_t rrt_quantize_accum_books_f64(uint32_t width, uint32_t height, const double *accum,
                                     uint32_t samples_per_pixel, uint8_t *rgb8);

/* ---- output step after the boundary: device quantiser, P6 ---------------
 * render_io.rs writes P3 ASCII (~25 MB at 1080p) from a float accum copied to the host
 * (16 B/pixel). These entries quantise on the device (3 B/pixel over PCIe) and format P3 or
 * binary P6 from the quantised bytes. */

/* rrt_hip_render, then the render_io quantiser on each device: rgb8_out[3*W*H] holds the
 * bytes render_io::write_ppm_from_accum would print for the float accum (identical to
 * rrt_quantize_accum of rrt_hip_render's accum_out with samples_per_pixel = total_spp). */
int32_t rrt_hip_render_rgb8(const RrtCamera *cam,
                            const RrtSphere *spheres, uint32_t n_spheres,
                            const RrtMaterial *materials, uint32_t n_materials,
                            const RrtTexture *textures, uint32_t n_textures,
                            uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                            uint8_t *rgb8_out);

/* rrt_hip_render_rgb8 with book-2/3 scene data (moving spheres, Perlin tables, quads, media,
 * light lists); ext may be NULL. Same bytes as rrt_quantize_accum of rrt_hip_render_ex's accum. */
int32_t rrt_hip_render_rgb8_ex(const RrtCamera *cam,
                               const RrtSphere *spheres, uint32_t n_spheres,
                               const RrtMaterial *materials, uint32_t n_materials,
                               const RrtTexture *textures, uint32_t n_textures,
                               const RrtSceneExt *ext,
                               uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                               uint8_t *rgb8_out);

/* Enqueue the render_io quantiser on `stream` (hipStream_t, NULL = default): d_accum =
 * n_pixels float4 (RGB sums; w ignored), d_rgb8 = n_pixels*3 bytes, scale 1/samples_per_pixel
 * in f32 as render_io.rs:10 computes it. Asynchronous; byte-identical to rrt_quantize_accum. */
int32_t rrt_quantize_accum_async(uint32_t n_pixels, const float *d_accum, uint32_t samples_per_pixel,
                                 uint8_t *d_rgb8, void *stream);

/* ---- the same output step for the books path (color.rs:6-32 on the device) ----------------
 * The RRT_FLAG_F64 kernel's f64 sums are 32 B/pixel; these entries quantise them where they are
 * and move 3 B/pixel. */

/* Enqueue the books path's quantiser (rrt_quantize_accum_books) on `stream` (hipStream_t, NULL =
 * default): d_accum = n_pixels float4 on the device (RGB sums; w is not read), d_rgb8 = n_pixels*3
 * bytes on the device (4-byte aligned, as hipMalloc returns it), scale 1.0 / samples_per_pixel in
 * f64. Asynchronous; byte-identical to rrt_quantize_accum_books. samples_per_pixel = 0 or a null
 * pointer with n_pixels > 0: RRT_E_INVALID; n_pixels = 0 enqueues nothing. */
int32_t rrt_quantize_accum_books_async(uint32_t n_pixels, const float *d_accum, uint32_t samples_per_pixel,
                                       uint8_t *d_rgb8, void *stream);
/* The same over f64 sums: d_accum = n_pixels x 4 doubles (rrt_render_tile_f64_async's rows).
 * Byte-identical to rrt_quantize_accum_books_f64. */
int32_t rrt_quantize_accum_books_f64_async(uint32_t n_pixels, const double *d_accum, uint32_t samples_per_pixel,
                                           uint8_t *d_rgb8, void *stream);

/* rrt_hip_render_f64 (RRT_FLAG_F64 is implied; book-1 scenes), then the books path's quantiser on
 * each device: rgb8_out[3*W*H] holds the bytes camera.rs:87-94 prints through color.rs — identical
 * to rrt_quantize_accum_books_f64 of rrt_hip_render_f64's accum_out with samples_per_pixel =
 * total_spp. Format them with rrt_format_pnm_from_rgb8. The _ex form below takes an
 * RrtSceneExt. */
int32_t rrt_hip_render_f64_rgb8(const RrtCamera *cam,
                                const RrtSphere *spheres, uint32_t n_spheres,
                                const RrtMaterial *materials, uint32_t n_materials,
                                const RrtTexture *textures, uint32_t n_textures,
                                uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                                uint8_t *rgb8_out);
/* The same with book-2 scene data (RRT_FLAG_F64 and RRT_FLAG_F64_BOOK2 implied; ext may be NULL):
 * rrt_hip_render_f64_ex, then the books quantiser on each device. */
int32_t rrt_hip_render_f64_rgb8_ex(const RrtCamera *cam,
                                   const RrtSphere *spheres, uint32_t n_spheres,
                                   const RrtMaterial *materials, uint32_t n_materials,
                                   const RrtTexture *textures, uint32_t n_textures,
                                   const RrtSceneExt *ext,
                                   uint32_t total_spp, uint32_t n_gpus, uint32_t flags,
                                   uint8_t *rgb8_out);

/* PNM from quantised pixels: binary = 0 -> P3 text byte-identical to
 * rrt_format_ppm_from_accum of the same image; binary = 1 -> P6 ("P6\nW H\n255\n" + rgb8).
 * *written = bytes needed (call with cap 0 to size). */
int32_t rrt_format_pnm_from_rgb8(uint32_t width, uint32_t height, const uint8_t *rgb8, int32_t binary,
                                 char *buf, size_t cap, size_t *written);
int32_t rrt_write_pnm_from_rgb8(uint32_t width, uint32_t height, const uint8_t *rgb8, int32_t binary,
                                const char *path);

/* Number of visible HIP devices (0 when no GPU). */
int32_t rrt_device_count(int32_t *count);

/* Test support, not part of the drop-in (no reference counterpart): on != 0 lets a one-shot render
 * (rrt_hip_render*, n_gpus > 1) run worker g on device g % device_count, so the multi-device path
 * runs on a one-GPU box (tests/test_gpu_multidevice.py). Off by default and at every load of the
 * library: without it n_gpus must not exceed the visible devices. Process-wide. */
void rrt_testing_device_wrap(int32_t on);

/* Test support, not part of the drop-in: forces the LDS layout in which the f64 books kernel
 * (RRT_FLAG_F64) stages a scene that fits its block — bit 0: f64-widened sphere records, bit 1: the
 * 1/r table, bit 2: the f32 pre-test records beside widened ones (with bit 0) — instead of its
 * automatic choice; -1 (the default at every load) restores it. A forced layout over the block's
 * 64 KB fails scene creation and the render. Every layout renders the same bits (tests/test_gpu_books64.py).
 * Process-wide. */
void rrt_testing_f64_layout(int32_t layout);

/* Test support, not part of the drop-in (RRT_ABI_VERSION is unchanged and the Rust shim does not bind
 * it): a BVH2 node link as the f32 kernel stages it in LDS — the child's byte offset in the staged
 * node array (index x 80) for an inner link, the word itself for a leaf link (first primitive |
 * count << 28, count > 0). The function the kernel's staging loop applies; no device is needed
 * (tests/test_lds_links.py). */
uint32_t rrt_testing_lds_node_link(uint32_t link);

/* Test support, not part of the drop-in (RRT_ABI_VERSION is unchanged and the Rust shim does not bind
 * them). rrt_testing_sphere_boxes: the padded f64 box of each sphere (out: n_spheres x 6 doubles,
 * min xyz then max xyz; motion as in rrt_scene_update_spheres) by the host compilation of the
 * function the update runs on the device. rrt_testing_scene_read_table: one of the scene's device
 * tables (RrtSceneTable; rows in leaf order except the boxes, which are in primitive order and held
 * only by a scene the device builder built); cap 0 sizes (*bytes_out, 0 for a table the scene does
 * not hold). rrt_testing_scene_update_stats: the scene's successful updates, and the device
 * allocations and builder levels of the last one. */
typedef enum RrtSceneTable {
    RRT_TABLE_BOXES = 0,        /* 6 doubles per primitive */
    RRT_TABLE_PRIM_CR = 1,      /* float4 */
    RRT_TABLE_PRIM_MTL = 2,     /* 32-B material record */
    RRT_TABLE_PRIM_MOTION = 3,  /* float4, book-2 worlds */
    RRT_TABLE_PRIM_INV_R64 = 4, /* double, RRT_FLAG_F64 */
    RRT_TABLE_PRIM_DIEL64 = 5,  /* 4 doubles, RRT_FLAG_F64 */
    /* the geometry tables (rrt_scene_update_geometry), in source order */
    RRT_TABLE_GQUADS = 6,       /* 80-B quad records: the scene's quads, boundary quads, light quads */
    RRT_TABLE_GQUADS64 = 7,     /* 128-B unrounded quad records, RRT_FLAG_F64_BOOK2 (instead of 6) */
    RRT_TABLE_QUAD_ROWS = 8,    /* 2 float4 per quad: its prim_cr row, its prim_motion row (held by
                                   a scene the device builder built) */
    RRT_TABLE_GLIGHTS = 9,      /* 32-B light records, RRT_FLAG_BOOK3 */
    RRT_TABLE_GMEDIA = 10       /* 32-B medium records (rrt_scene_update_world), in source order */
} RrtSceneTable;
typedef struct RrtSceneUpdateStats {
    uint64_t updates;
    uint64_t last_allocations;
    uint64_t last_levels;
} RrtSceneUpdateStats;
int32_t rrt_testing_sphere_boxes(const RrtSphere *spheres, uint32_t n_spheres, const float *motion, double *out);
int32_t rrt_testing_scene_read_table(RrtScene *scene, uint32_t what, void *out, size_t cap, size_t *bytes_out);
int32_t rrt_testing_scene_update_stats(const RrtScene *scene, RrtSceneUpdateStats *out);
/* Test support, not part of the drop-in: what a quad contributes to a scene, by the host compilation
 * of the functions rrt_scene_update_geometry runs on the device (and scene creation on the host).
 * Any output may be NULL. boxes6: n_quads x 6 doubles (min xyz, max xyz), the padded box; gquad:
 * n_quads 80-B records (RRT_TABLE_GQUADS' layout); gquad64: n_quads 128-B records
 * (RRT_TABLE_GQUADS64's: q, u, v, n, w as 3 doubles each, then D). */
int32_t rrt_testing_quad_records(const RrtQuad *quads, uint32_t n_quads, double *boxes6, void *gquad, void *gquad64);
/* Test support, not part of the drop-in: what a constant medium contributes to a scene, by the host
 * compilation of the functions rrt_scene_update_world runs on the device (and scene creation on the
 * host). Either output may be NULL. boxes6: n_media x 6 doubles (min xyz, max xyz), the medium's
 * box; gmedium: n_media 32-B records (RRT_TABLE_GMEDIA's layout: the sphere, kind, first = n_quads +
 * the medium's first, count, -1 / density). A quad boundary's range must lie within
 * n_boundary_quads. */
int32_t rrt_testing_medium_records(const RrtMedium *media, uint32_t n_media, const RrtQuad *boundary_quads,
                                   uint32_t n_boundary_quads, uint32_t n_quads, double *boxes6, void *gmedium);

/* Test support, not part of the drop-in. rrt_testing_scene_refit_stats: the scene's refits so far,
 * and of the last one the device allocations, the kernel launches and the form of the bottom-up
 * pass (1: one workgroup looping over the levels, 0: one launch per level).
 * rrt_testing_refit_form: forces the per-level launches (0) or the single workgroup (1) whatever the
 * tree's size; -1 (the default at every load) restores the automatic choice. With the single
 * workgroup forced, a refit of a tree over its node bound is refused. Both forms write the same
 * bytes (tests/test_gpu_scene_refit.py). Process-wide. */
typedef struct RrtSceneRefitStats {
    uint64_t refits;
    uint64_t last_allocations;
    uint64_t last_launches;
    uint64_t last_form;
} RrtSceneRefitStats;
int32_t rrt_testing_scene_refit_stats(const RrtScene *scene, RrtSceneRefitStats *out);
int32_t rrt_testing_refit_form(int32_t form);

/* Test support, not part of the drop-in. rrt_testing_scene_build_stats: of the scene's last device
 * build (creation or update): the builder (RRT_BUILDER_*), the kernel launches the builder made (a
 * library sort counts as one), its blocking reads of device memory, the form (1: the single-workgroup
 * LBVH launch, 0 otherwise) and the shapes it built (binned: builds run; LBVH: finishing passes).
 * rrt_testing_lbvh_form: forces the LBVH's launch-per-phase form (0) or its single workgroup (1); -1
 * restores the automatic choice. With the single workgroup forced a build over its primitive bound
 * fails. Both forms write the same bytes. Process-wide. */
typedef struct RrtSceneBuildStats {
    uint64_t builder;
    uint64_t launches;
    uint64_t blocking_reads;
    uint64_t form;
    uint64_t shape_attempts;
} RrtSceneBuildStats;
int32_t rrt_testing_scene_build_stats(const RrtScene *scene, RrtSceneBuildStats *out);
int32_t rrt_testing_lbvh_form(int32_t form);

/* Test support, not part of the drop-in (RRT_ABI_VERSION is unchanged and the Rust shim does not bind
 * it). rrt_testing_scene_fail_update: leaves the scene in the state a change that failed midway leaves
 * it in (an update fails midway only on a device error, which no test provokes): the scene is invalid,
 * every render, refit and query of it is refused with RRT_E_INVALID naming this call, and a later
 * rrt_scene_update_* that succeeds makes it valid again. Touches no device memory. Returns
 * RRT_E_INVALID itself, with the message the failed change would have set. */
int32_t rrt_testing_scene_fail_update(RrtScene *scene);

/* Test support, not part of the drop-in (no reference counterpart; RRT_ABI_VERSION is unchanged and
 * the Rust shim does not bind it): the launch shape the library picks for a scene, computed on the
 * host from the scene's counts alone by the code the render launches and rrt_scene_create use. No
 * device is needed (tests/test_launch_plan.py).
 * Query: n_nodes, n_prims and stack_depth (BVH depth + 1) as rrt_build_bvh reports them; node_stride
 * 80 (BVH2 staged in LDS), 32 (BVH2 read from global memory) or 128 (the width-4 tree, staged when
 * bvh4_in_lds); book 0 (book 1), 2 (the scene has book-2 data: motion, quads, media, checker / noise
 * materials) or 3 (RRT_FLAG_BOOK3); specular / image_tex: some material is metal or dielectric /
 * image-textured; n_perlin, n_media, n_quads as in RrtSceneExt; f64: RRT_FLAG_F64; f64_book2:
 * RRT_FLAG_F64_BOOK2 (with f64 = 1 and book = 2: the f64 kernel's book-2 class, ok = 0 with n_perlin or
 * n_media; 0 leaves every other answer as it was); min_waves /
 * global_waves: 0 for the defaults (the RRT_MIN_WAVES / RRT_GLOBAL_WAVES overrides otherwise). The
 * RRT_PERLIN_IN_LDS=0 override of the environment is honoured as scene creation honours it.
 * Result: ok = 0 when rrt_scene_create refuses such a scene (no launch shape), else the kernel class
 * (f32: -2 diffuse, -1 untextured, 0 full book 1, 1-3 book 2 spheres / quads / media, 4 book 3; f64:
 * 0 full, 1 untextured, 2 diffuse, 3 book 2), its block (threads, launch-bounds waves per SIMD, 1 = none),
 * bytes per stack entry, what is staged in LDS, the block's dynamic LDS bytes, and raise_limit = 1
 * when those exceed 64 KiB and the launch raises the kernel's dynamic-LDS limit (at most 160 KiB). */
typedef struct RrtLaunchPlanQuery {
    uint32_t n_nodes, n_prims, stack_depth, node_stride;
    uint32_t book, specular, image_tex, n_perlin;
    uint32_t n_media, n_quads, f64, bvh4_in_lds;
    uint32_t min_waves, global_waves, f64_book2, _pad;
} RrtLaunchPlanQuery;
typedef struct RrtLaunchPlan {
    uint32_t ok, f64;
    int32_t kernel_class, shape;
    uint32_t stack_bytes, threads, waves, waves_noise_free;
    uint32_t scene_in_lds, perlin_in_lds, inv_r_in_lds, rec32_in_lds;
    uint32_t raise_limit, _pad;
    uint64_t lds_bytes;
} RrtLaunchPlan;
int32_t rrt_testing_launch_plan(const RrtLaunchPlanQuery *query, RrtLaunchPlan *plan);

/* Test support, not part of the drop-in: runs the f32 kernel's short reciprocal (v_rcp_f32 + one
 * fma Newton step) and short square root over every f32 bit pattern against the IEEE results;
 * mismatches (3 x u64): [0] patterns with |s| in [2^-126, 2^126), +-0, +-inf or NaN whose
 * reciprocal differs, [1] patterns with |s| < 2^126 or NaN whose clamped ray slope differs, [2]
 * patterns +-0 or |s| >= 2^-96 of either sign (negatives, infinities and NaN included) whose square
 * root differs from the IEEE one (tests/test_gpu_recip.py: all 0). */
int32_t rrt_testing_recip_check(uint64_t *mismatches);

/* Test support, not part of the drop-in (ABI v11): the largest absolute errors of the device's f32
 * acosf over every f32 in [-1, 1] (out[0]) and atanf over every f32 in [0, 1] (out[1]) against its
 * f64 acos / atan, and the bounds the f64 kernel's texel enclosures assume for them (out[2],
 * out[3]; tests/test_gpu_trig32.py: each error at most half its bound). */
int32_t rrt_testing_trig32_check(double *out);

/* Test support, not part of the drop-in (ABI v11): the f64 kernel's IEEE square root without the
 * library expansion's identity scalings (rrt_books64.hip sqrt64_big) against the library root, bit
 * for bit, on 2^28 arguments from 2^-767 to the largest finite (random and nearly-square mantissas)
 * plus +-0 and +inf: out[0] = differing results, out[1] = arguments checked
 * (tests/test_gpu_trig32.py: 0 differ). */
int32_t rrt_testing_sqrt64_check(uint64_t *out);

/* Test support, not part of the drop-in (no reference counterpart; RRT_ABI_VERSION is unchanged and
 * the Rust shim does not bind it): the f32 kernel's own numeric building blocks (rrt_kernel.hip)
 * applied elementwise on the device, so tests can choose their arguments (tests/test_gpu_device_ops.py
 * compares every result bit for bit with the oracle's f32 twin). `in` holds n rows of f32 columns,
 * `out` receives n rows of 32-bit words (f32 bits unless noted); host pointers, copied inside.
 *   op          in columns                        out columns
 *   SIN COS LOG ACOS   x                          f(x)                    (rrt_sinf, rrt_cosf, rrt_logf, rrt_acosf)
 *   ATAN2       y, x                              rrt_atan2f(y, x)
 *   DIV_A       n, a                              div_by_a<false>(n) on ra = refine_ra(a), div_by_a<true>(n)
 *                                                 (the former when ra = 0), the IEEE n / a, ra
 *   DIV_CONST   x                                 div_by_const(x, 2 pi), IEEE x / (2 pi), div_by_const(x, pi), IEEE x / pi
 *   FLOOR_I32   x                                 floor_i32(x) (i32)
 *   CHECKER     inv_scale, p.xyz                  checker_even (u32 0 / 1)
 *   PERLIN      p.xyz                             (perlin_noise, noise_value) x 4: generic pointer with the corner
 *                                                 loop unrolled, rolled; the LDS pointer unrolled, rolled.
 *                                                 aux: one RrtPerlin table, then the f32 scale (packed into the
 *                                                 device table by scene creation's code, staged into LDS as the
 *                                                 render stages it)
 *   VEC         v.xyz, n.xyz, e, cosine, r0       unit(v) 3, reflect(v, n) 3, refract(v, n, e) 3,
 *                                                 reflectance_r0(cosine, r0), onb_transform(n, v) 3
 *   QUAD        o.xyz, d.xyz, tmin, closest, j    quad_hit of quad j over [tmin, closest]: hit (u32), t (0 on a miss).
 *                                                 aux: u32 count, 12 bytes of padding, then count RrtQuad records
 *                                                 (derived planes formed by scene creation's code); j < count
 *   SPHERE      o.xyz, d.xyz, c.xyz, r, closest   for the book-1 record (r * r stored), then the book-2 record (r):
 *                                                 exact_root<false>, exact_root<true> (the former when the ray's ra = 0),
 *                                                 test_range's decision against `closest` with the IEEE division
 *                                                 (hit u32, t), the same with the per-ray reciprocal (hit, t); last
 *                                                 sphere_root over (0.001, inf) (u32). 13 words. r < 0 is taken as 0.
 *   LIGHTS_PDF  o.xyz, d.xyz                      lights_pdf(P, o, d): book 3's HittableList::pdf_value over the light list
 *   LIGHTS_RANDOM  o.xyz, seed, pixel, sample     lights_random(P, o, rng) 3, then the number of draws it took from the
 *               (the last three as u32 bit        stream (u32). The lane seeds its stream as the render seeds the path
 *               patterns)                         (seed, pixel, sample): the first draw is the path's first.
 *                                                 aux of both: u32 count, 12 bytes of padding, then count RrtLight records
 *                                                 (device records and the quads' derived planes formed by scene
 *                                                 creation's code); 1 <= count <= 65536
 *   SLOPES      o.xyz, d.xyz                      ray_consts(o, d) as the traversal reads it: inv 3, oi 3, the plane-pair
 *                                                 offsets ox, oy, oz (u32) of a staged node; then clamped_slope of each
 *                                                 component of d on its own 3 (what inv must equal); last ox of the
 *                                                 f16-node form (the three rotations packed, u32). 13 words.
 * div_by_a<true> / <false> (and with them exact_root<true> / <false> and test_range's two divisions)
 * are the same function since div_by_a guards its own range; both instantiations are still run.
 * Every input, NaN and infinities included, is ordinary arithmetic. */
enum RrtDeviceOp {
    RRT_OP_SIN = 0,
    RRT_OP_COS = 1,
    RRT_OP_LOG = 2,
    RRT_OP_ACOS = 3,
    RRT_OP_ATAN2 = 4,
    RRT_OP_DIV_A = 5,
    RRT_OP_DIV_CONST = 6,
    RRT_OP_FLOOR_I32 = 7,
    RRT_OP_CHECKER = 8,
    RRT_OP_PERLIN = 9,
    RRT_OP_VEC = 10,
    RRT_OP_QUAD = 11,
    RRT_OP_SPHERE = 12,
    RRT_OP_LIGHTS_PDF = 13,
    RRT_OP_LIGHTS_RANDOM = 14,
    RRT_OP_SLOPES = 15
};
int32_t rrt_testing_device_ops(uint32_t op, uint32_t n, const void *in, void *out, const void *aux);

/* Test support, not part of the drop-in: the sphere tests' root division (rrt_kernel.hip div_by_a on
 * the per-ray reciprocal refine_ra(a)) against the IEEE quotient q = n / a, for each of the n_a <= 48
 * divisors a over every f32 bit pattern n, both div_by_a<false> and <true>; and div_by_const on the
 * device. "Same" is bit equality or both NaN; a root t is accepted when 0.001 < t < inf. out (8 x u64):
 *   [0] a in [2^-64, 2^64], finite |n| >= 2^-103, q finite and |q| >= 2^-126: results that differ from q
 *   [1] a in that range, every n: accepted(result) != accepted(q), or both accepted and not the same
 *   [2] a outside it (ra = 0): div_by_a<false> differs from q
 *   [3] a in the range, q subnormal or zero: results whose bits differ from q's (no decision reads them)
 *   [4], [5] x = 0 and every f32 x in [2^-100, 8] whose div_by_const(x, 2 pi) / (x, pi) differs from x / c
 *   [6] (n, a) pairs checked (n_a << 32), [7] x values checked
 * (tests/test_gpu_device_ops.py: [0], [1], [2], [4], [5] are 0). */
int32_t rrt_testing_div_check(const float *a_values, uint32_t n_a, uint64_t *out);

/* Test support, not part of the drop-in (no reference counterpart; RRT_ABI_VERSION is unchanged and
 * the Rust shim does not bind it): the f64 books kernel's own building blocks (rrt_books64.hip)
 * applied elementwise on the device (tests/test_gpu_device_ops64.py compares every result bit for
 * bit with the oracle's f64 path or with the IEEE operation). `in` holds n rows of f64 columns, `out`
 * receives n rows of 64-bit words (f64 bits unless noted; i32 and flags zero-extended from 32 bits);
 * host pointers, copied inside. Row i runs on lane i % 64 of wave i / 64. aux: QUAD64's records, else NULL.
 *   op           in columns                        out columns
 *   ACOS64       x                                 rrt_acos64(x)
 *   ATAN2_64     y, x                              rrt_atan2_64(y, x)
 *   DIV_A64      n, a                              div_a64(n, a, ra) on ra = recip_a64(a), the IEEE n / a, ra
 *   DIV_CONST64  x                                 div_by_const64(x, 2 pi), IEEE x / (2 pi), div_by_const64(x, pi), IEEE x / pi
 *   SQRT64       x                                 sqrt64(x): the wave-uniform choice between sqrt64_big and the
 *                                                  library root is taken over the 64 rows of the lane's wave
 *   AS_I32       x                                 as_i32_rs(x) (i32)
 *   ATT64        word, bytes                       att_decode(word) for the u32 `word` (an f32 bit pattern or a texel
 *                                                  tag), texel_value64(bytes) 3 for bytes = r | g << 8 | b << 16 or
 *                                                  0x1000000 (no image data); both columns hold whole numbers
 *   VEC64        v.xyz, n.xyz, e, cosine, r0       unit_vector(v) 3, reflect(v, n) 3, refract(v, n, e) 3,
 *                                                  reflectance_r0(cosine, r0), rr_probability64(v)
 *   TEXEL64      outward.xyz, w, h                 the texel column i and row j of get_sphere_uv(outward) in a w x h
 *                                                  image as the render chooses them (texel_index64), whether the
 *                                                  column and the row were decided by the f32 enclosure (u32 0 / 1
 *                                                  each), then i and j from the fdlibm angles alone. 1 <= w, h <= 2^30
 *   SPHERE64     o.xyz, d.xyz, c.xyz, r, closest   (c and r f32-representable; r < 0 is taken as 0) for the f32 record
 *                                                  (float4) and then the record widened as the LDS staging widens it
 *                                                  (Sphere64): exact_root64, leaves64's decision over a one-sphere
 *                                                  leaf against `closest` (hit u32, t: `closest` on a miss). 6 words.
 *   QUAD64       o.xyz, d.xyz, tmin, closest, j    quad_hit64 of quad j over the closed [tmin, closest]: hit (u32), t (0 on
 *                                                  a miss). aux: u32 count, 12 bytes of padding, then count RrtQuad
 *                                                  records (f64 planes formed by scene creation's code); j < count
 *   CHECKER64    inv_scale, p.xyz                  checker_even64 (u32 0 / 1)
 * Every input, NaN and infinities included, is ordinary arithmetic. */
enum RrtDeviceOp64 {
    RRT_OP_ACOS64 = 0,
    RRT_OP_ATAN2_64 = 1,
    RRT_OP_DIV_A64 = 2,
    RRT_OP_DIV_CONST64 = 3,
    RRT_OP_SQRT64 = 4,
    RRT_OP_AS_I32 = 5,
    RRT_OP_ATT64 = 6,
    RRT_OP_VEC64 = 7,
    RRT_OP_TEXEL64 = 8,
    RRT_OP_SPHERE64 = 9,
    RRT_OP_QUAD64 = 10,
    RRT_OP_CHECKER64 = 11
};
int32_t rrt_testing_device_ops64(uint32_t op, uint32_t n, const void *in, void *out, const void *aux);

#ifdef __cplusplus
}
#endif
#endif /* RRT_HIP_H */
