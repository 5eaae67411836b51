// rrt_internal.h — layouts shared by the host runtime (rrt_host.cpp) and the gfx950
// megakernel (rrt_kernel.hip). Not part of the public C-ABI (include/rrt_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rrt {

// BVH2 node, 80 B, both children's boxes stored in the parent so one node visit reads one
// record. Boxes are f32 rounded outward (and grown by the slab test's rounding bound, rrt_host.cpp
// BoxSlack) from the f64 SAH build. Each axis is stored lo, hi, lo: a ray whose 1/d_a is negative
// reads its (entry, exit) plane pair at offset 1 (hi, lo), otherwise at 0 (lo, hi), so the slab
// test takes no min/max per axis. Links: a child node index (count 0), or for a leaf its first
// primitive | count << 28 — which is also the postponed-leaf record the kernel keeps.
struct alignas(16) GNode {
    float box[2][9];    // child c, axis a: lo, hi, lo at [c][3a .. 3a+2] (f32, rounded outward)
    uint32_t link[2];   // child c: node index (internal), or first primitive | count << 28 (leaf)
};
static_assert(sizeof(GNode) == 80, "GNode must be 80 B");
// The same node in 32 B, for scenes read from global memory (beyond the LDS budget): each plane
// as an f16 rounded outward (lo down, hi up; subnormals pushed out to 0 or the smallest normal),
// lo | hi << 16 per axis, and the min/max slab test. Two 16-B loads per visit: a scene read from
// L2 spends its time in the vector memory pipeline (TA/TD busy ~90 %), and the slab test reads
// each f16 plane with v_fma_mix_f32 (exact f16 -> f32 inside the FMA), so the decode costs no
// instruction. Looser boxes only add visits (C5 +0.06 %); hits are decided by the primitive
// tests. Same-box against the 64-B f32 node (round 2's layout): C5 +7.5 %, bouncing spheres
// +4.6 %, final_scene +-0.3 %. A never-hit child is the point (65504, 65504, 65504).
//   c0[a] / c1[a] = child c's axis-a planes; link as GNode::link
struct alignas(16) GNodeH {
    uint32_t c0[3];
    uint32_t c1[3];
    uint32_t link[2];
};
static_assert(sizeof(GNodeH) == 32, "GNodeH must be 32 B");
constexpr uint32_t kLinkCountShift = 28;
constexpr uint32_t kLinkFirstMask = (1u << kLinkCountShift) - 1u;
constexpr uint32_t kMaxLeafPrims = 7;  // two leaf children's counts share one 4-bit field
// A GNode link as the f32 kernel stages it in LDS: the node array sits at LDS offset 0, so an inner
// link (count 0) becomes the child's byte offset there — the address the node step reads, with no
// index * 80 per visit — and a leaf link (first primitive | count << 28) stays what it is. A staged
// scene is at most kLdsSceneBudget (40 KB), so every offset fits a 16-bit stack entry; the root is
// still 0. Nodes read from global memory (GNodeH) keep indices.
__host__ __device__ constexpr uint32_t lds_node_link(uint32_t link) {
    return link > kLinkFirstMask ? link : link * (uint32_t)sizeof(GNode);
}
constexpr uint32_t kMaxUnbounded = 4;  // media tested outside the BVH (rrt_host.cpp unbounded_media)

// BVH4 node, 128 B: the boxes of 4 children as SoA float4s (child c in component c), the
// child refs and primitive counts (0 = internal node). Collapsed from the binary SAH tree.
struct alignas(16) GNode4 {
    float4 lox, hix, loy, hiy, loz, hiz;
    int4 child;
    int4 count;
};
static_assert(sizeof(GNode4) == 128, "GNode4 must be 128 B");

// Material, SoA split into two 16-B records (kind-dependent payload).
//   a = albedo.rgb (or emitted rgb for lights), fuzz (pre-clamped to <= 1, material.rs:49)
//   b = kind, ref_idx bits, texture index, 0
struct alignas(16) GMaterial {
    float4 a;
    int4 b;
};

// Perlin tables on the device (the_next_week/perlin.rs:4-22): the 256 random unit vectors
// and the three permutations packed per index: perm_x | perm_y << 8 | perm_z << 16.
struct alignas(16) GPerlin {
    float4 randvec[256];
    uint32_t perm[256];
};

// Quad (the_next_week/quad.rs:9-41) with its derived plane: q.xyz corner, q.w = D = dot(n, q);
// u, v edges; n = unit(cross(u, v)); w = cross(u, v) / |cross(u, v)|^2 (computed in f64 on the
// host, quad.rs's `(1/x) * v` divisions, then rounded to f32). 80 B.
struct alignas(16) GQuad {
    float4 q;
    float4 u;
    float4 v;
    float4 n;
    float4 w;
};
// The same quad unrounded, for the f64 books kernel's book-2 class (rrt_books64.hip kF64Book2): the f32
// corner and edges widened, and the derived plane as quad.rs:21-37 forms it in f64 (the values GQuad
// rounds). 128 B.
struct alignas(16) GQuad64 {
    double q[3], u[3], v[3], n[3], w[3];
    double D;
};
static_assert(sizeof(GQuad64) == 128, "GQuad64 must be 128 B");

// ConstantMedium (the_next_week/constant_medium.rs): boundary sphere (xyz, r) or quads
// [first, first + count) of KParams.quads (after the scene's own quads); neg_inv_density =
// -1/density (f64 on the host, rounded to f32). 32 B.
struct alignas(16) GMedium {
    float4 sphere;
    uint32_t kind;  // 0 sphere, 1 quads
    uint32_t first;
    uint32_t count;
    float neg_inv_density;
};

// Book-3 MIS light: sphere (center xyz, radius w) or quad (index into KParams.quads, its area
// |u x v| in f64 rounded to f32). 32 B.
struct alignas(16) GLight {
    float4 sphere;
    uint32_t kind;  // 0 quad, 1 sphere
    uint32_t quad;
    float area;
    uint32_t _pad;
};

struct GTexture {
    int32_t offset;  // byte offset into the texture pool
    int32_t width;
    int32_t height;
    int32_t pad;
};

// Everything the megakernel needs, passed by value (kernarg segment).
// n / d for 0 <= n < 2^31 and a fixed d >= 1: q = (umulhi(n, m) + n) >> s with s = ceil(log2 d),
// m = floor(2^32 (2^s - d) / d) + 1 (Granlund-Montgomery; exact, tests/test_oracle.py checks it).
// d = 0 gives {0, 0} (callers never divide by it).
struct FastDiv {
    uint32_t m, s;
};
__host__ __device__ inline FastDiv make_fastdiv(uint32_t d) {
    if (d == 0) return FastDiv{0u, 0u};
    uint32_t s = 0;
    while (s < 32 && (1ull << s) < d) ++s;
    return FastDiv{(uint32_t)((((1ull << s) - d) << 32) / d + 1ull), s};
}
__host__ __device__ inline uint32_t fast_div(uint32_t n, FastDiv f) {
    return (uint32_t)((((uint64_t)n * f.m) >> 32) + n) >> f.s;
}

// f64 sums of the books path: RGB + sample count (32 B; two 16-B stores)
struct alignas(16) D4 {
    double x, y, z, w;
};
static_assert(sizeof(D4) == 32, "D4 must be 32 B");

// A chunk partial: the RGB sums of one (chunk, pixel) — the sample count is the chunk schedule's,
// so 12 B instead of a float4's 16.
struct F3 {
    float x, y, z;
};

struct KParams {
    const void *nodes;           // GNode[] (bvh_width 2) or GNode4[] (bvh_width 4)
    const float4 *prim_cr;       // sphere center.xyz, radius — in BVH leaf order
    const GMaterial *prim_mtl;   // each primitive's material record, same order (one fetch per hit)
    const float4 *prim_motion;   // (center2 - center1).xyz per primitive, same order; null = static scene
    const GPerlin *perlin;       // Perlin tables (noise textures)
    const GQuad *quads;          // quads, then media boundary quads; a quad's leaf-order primitive record is
                                 // (q.xyz, -(1 + index)) with (normal.xyz, D) in its motion slot; a
                                 // medium's (0, 0, 0, -(1 + n_quads + index)). A scene of the f64 kernel's
                                 // book-2 class (flags & kFlagF64Book2) points this at its GQuad64 records
                                 // instead (same leaf-order convention; no f32 kernel runs on such a scene)
    const GMedium *media;
    const GLight *lights;        // book 3: the MIS light list
    const uint8_t *tex_pool;
    const GTexture *texs;
    float4 *accum;               // tile-local rows * width
    unsigned long long *counters;  // RrtCounters layout (5 x u64)

    // camera (f32, from the RrtCamera ABI; disk_u/v = u/v * defocus_radius in f32)
    float p00[3];
    float du[3];
    float dv[3];
    float center[3];
    float disk_u[3];
    float disk_v[3];
    float background[3];
    float defocus_radius;

    uint32_t max_depth;
    uint32_t seed;
    uint32_t bg_mode;
    uint32_t flags;

    uint32_t width;
    uint32_t height;
    uint32_t tile_rows;     // rows owned by this tile
    uint32_t band_rows;
    uint32_t rank;
    uint32_t n_ranks;
    uint32_t sample_begin;
    uint32_t sample_end;
    uint32_t n_work_tiles;  // 8x8 pixel tiles in this tile
    uint32_t tiles_x;

    uint32_t n_nodes;
    uint32_t n_prims;
    uint32_t n_unbounded;   // the last n_unbounded leaf-order primitives: media tested after the walk
    uint32_t n_perlin;
    uint32_t perlin_in_lds; // book-2 kernels stage the Perlin tables in LDS after the scene
    uint32_t n_quads;       // the scene's quads (boundary quads follow them)
    uint32_t n_media;
    uint32_t n_lights;
    uint32_t image_tex;     // some material samples an image texture (book-1 kernels: texture path compiled in)
    uint32_t specular;      // some material is metal or dielectric (book-1 kernels: those branches compiled in)
    uint32_t sqrt_spp;      // book 3: stratified camera samples (sqrt_spp^2 per pixel)
    float recip_sqrt_spp;   // 1/sqrt_spp in f64, rounded
    uint32_t stack_depth;   // entries needed (BVH depth + 1)
    uint32_t scene_in_lds;  // stage nodes + spheres + their materials in LDS per block
    uint32_t trav_frac;     // leave the traversal loop when <= live*trav_frac/256 lanes still traverse
    uint32_t leaf_frac;     // run the postponed-leaf loop when > live*leaf_frac/256 lanes wait on leaf tests
    uint32_t bvh_width;     // 2 or 4
    uint32_t min_waves;     // launch-bounds occupancy request (waves per SIMD)
    uint32_t global_waves;  // the same for scenes read from L2 (not staged in LDS); < 6 = no bound

    // persistent work queue: units = (pixel, sample chunk), the n_big chunks of `chunk` samples
    // of every tile first (tile-major), then the tail chunks of `chunk_small` (rrt_accum_chunk)
    uint32_t chunk;           // samples per big chunk
    uint32_t chunk_small;     // samples per tail chunk: max(1, chunk / 8)
    uint32_t n_big;           // big chunks per pixel: (S - 1) / chunk (0 when S <= chunk)
    uint32_t n_chunks;        // n_big + ceil((S - n_big * chunk) / chunk_small)
    // Sample passes: the chunks are rendered pass_chunks at a time (one launch + combine per
    // pass) so the partial buffer stays within its budget; each launch's queue holds the pass's
    // chunks [chunk_begin, chunk_begin + pass_n): its pass_big big chunks first, then its tail
    // chunks. The combine continues the same left fold over chunks, so passes never change bits.
    uint32_t pass_chunks;     // chunks per pass (host: partial budget / pixels), >= 1
    uint32_t chunk_begin;     // this launch's first chunk (set per pass by launch_render)
    uint32_t pass_n;          // this launch's chunks
    uint32_t pass_big;        // this launch's big chunks (they precede its tail chunks)
    uint32_t n_big_units;     // n_work_tiles * pass_big * 64
    uint32_t n_units;         // n_work_tiles * pass_n * 64
    uint32_t n_cus;           // compute units of the device (grid sizing)
    // Division by the queue's uniform divisors as multiply-high + add + shift (FastDiv): the
    // generic 32-bit division sequence is ~35 instructions, paid at every unit start and end.
    FastDiv fd_pass_big, fd_pass_tail, fd_tiles_x, fd_band_rows, fd_n_ranks, fd_chunk, fd_chunk_small, fd_sqrt_spp;
    uint32_t *unit_counter;   // device queue heads: kQueues counters 128 B apart (zeroed per launch)
    F3 *partial;              // [pass chunk][tile pixel] RGB partial sums when n_chunks > 1 (12 B: the
                              // combine derives the count): a chunk's pixels are contiguous, so an
                              // 8x8 tile's rows fill whole 128-B lines

    // The f64 books path (flags & kFlagF64, rrt_books64.hip); appended so the f32 kernels' field
    // offsets stay unchanged. Sums and chunk partials as D4 (RGB sums, w = count) in the same
    // layouts as accum / partial; the camera's raw u, v (defocus_disk_u = u * defocus_radius is
    // formed in f64, camera.rs:136-138).
    D4 *accum64;
    D4 *partial64;
    float cam_u[3];
    float cam_v[3];
    // 1 / r per leaf-order sphere in f64 (sphere.rs:48's (p - center) / radius is (1/r) * v,
    // vec3.rs:142-148: the same IEEE quotient, formed once on the host). One entry per leaf-order
    // primitive: a quad's (book-2 class) holds 1 / its tag and is never read
    const double *prim_inv_r64;
    uint32_t inv_r_in_lds;  // f64 kernel, scene in LDS: the 1/r table staged too (fits the block's 64 KB)
    // the camera block widened to f64 on the host, as camera.rs:136-180 forms it from the f32 ABI
    // values: pixel00, delta_u, delta_v, center, defocus_disk_u = u * radius, defocus_disk_v
    double cam64[6][3];
    // per leaf-order primitive, a dielectric's (1 / eta, r0(1 / eta), r0(eta), 0) in f64, formed on
    // the host in the reference's operations (material.rs:75-102); zeros for other materials. Spheres
    // and quads alike (a quad can be dielectric)
    const double4 *prim_diel64;
    // the f32 sphere pre-test (rrt_sphere32.h) is enabled: every sphere center and radius within
    // 2^20 (its proven domain); rec32_in_lds: the widened-record layout also stages the f32 records
    uint32_t sphere32;
    uint32_t rec32_in_lds;
    // The f64 books path's summation in camera.rs:72-76's order (seq = 1): each pixel's first
    // S - T samples are one chunk summed from 0 in the lane (written to accum64 with w = S - T), the
    // last T samples tail chunks whose per-sample radiances go to seq64 ([tail sample of the pass]
    // [tile pixel] x 3 doubles; seq_first = the pass's first tail sample, relative to sample_begin),
    // folded into accum64 in sample order after the pass (launch_render_f64_seq).
    uint32_t seq;
    uint32_t seq_first;
    double *seq64;       // [tail chunk of the pass][j < chunk_small][tile pixel] x 3: nonzero radiances packed
    uint32_t *seqmask;   // [tail chunk of the pass][tile pixel]: which of the chunk's samples they are
    // the f64 path's attenuation history ([bounce][lane slot] x 3 floats, rrt_books64.hip
    // fold_back64): max_depth x hist_lanes records; the launch keeps blocks x threads <= hist_lanes
    float *hist;
    uint32_t hist_lanes;
};

// RRT_FLAG_F64 (include/rrt_hip.h): the f64 books-arithmetic kernel (rrt_books64.hip)
constexpr uint32_t kFlagF64 = 0x8u;
// RRT_FLAG_F64_BOOK2: kept in KParams.flags only for a scene that has book-2 data (the f64 kernel's
// class kF64Book2); a book-1 scene created with it renders as RRT_FLAG_F64 alone
constexpr uint32_t kFlagF64Book2 = 0x20u;

// Traversal stack entries held in LDS per lane: up to 64 (BVH depth <= 63).
constexpr int kMaxStackDepth = 64;
constexpr uint32_t kQueues = 8;  // work-queue counters (blocks dealt round-robin, one per XCD)
#ifndef RRT_BLOCK
#define RRT_BLOCK 512
#endif
#ifndef RRT_WAVES
#define RRT_WAVES 6
#endif
#ifndef RRT_TILE_W
#define RRT_TILE_W 8
#endif
// work-unit tile: 64 consecutive unit ids = kTileW x kTileH pixels of one chunk
constexpr uint32_t kTileW = RRT_TILE_W, kTileH = 64u / RRT_TILE_W;
constexpr int kBlock = RRT_BLOCK;          // threads per block (4 or 8 waves)
constexpr int kWavesPerSimd = RRT_WAVES;   // launch-bounds occupancy target of the main variant
constexpr int kGlobalBlock = 256;         // book-1 kernels whose scene is read from L2: block size
#ifndef RRT_B1_GLOBAL_WAVES
#define RRT_B1_GLOBAL_WAVES 7
#endif
constexpr int kGlobalWaves = RRT_B1_GLOBAL_WAVES;  // and waves per SIMD (7: 72 VGPRs)
#ifndef RRT_B2_WAVES
#define RRT_B2_WAVES 5
#endif
#ifndef RRT_B2_BLOCK
#define RRT_B2_BLOCK 256
#endif
// Book 3 at 256 x 5 (its noise-free kernel needs ~112 VGPRs): B3 +4.8 % same-box over the
// unbounded 512-thread blocks (4 waves), +3.9 % over 256 x 4.
#ifndef RRT_B3_WAVES
#define RRT_B3_WAVES 5
#endif
constexpr int kBook2Waves = RRT_B2_WAVES;  // book-2 kernels (classes 1-3): launch bound (1 = none)
constexpr int kBook2Block = RRT_B2_BLOCK;  // and block size; book 3 and unbounded launches use kBlock
constexpr int kBook3Waves = RRT_B3_WAVES;  // book 3 (class 4): launch bound (1 = none, 512-thread blocks;
                                           // else kBook2Block-thread blocks)
// Per-block LDS budget for staging the scene (BVH nodes + spheres + per-sphere materials)
// next to the stack. RTOW: 13.5 KB nodes + 486 x 48 B = 36.9 KB; + ~11 KB of stack per
// 512-thread block keeps 3 blocks (6 waves/SIMD) within the CU's 160 KB.
constexpr size_t kLdsSceneBudget = 40 * 1024;
constexpr size_t kPrimBytes = sizeof(float4) + sizeof(GMaterial);  // per primitive: sphere + material
constexpr size_t kMotionBytes = sizeof(float4);                     // + motion, scenes with moving spheres

// Dynamic LDS one block may declare: 64 KiB by default, up to the CU's 160 KiB (gfx950,
// MI355X_MICROARCH.md occupancy section) once the kernel's hipFuncAttributeMaxDynamicSharedMemorySize
// is raised to the size.
constexpr size_t kLdsDefaultMax = 64u * 1024u;
constexpr size_t kLdsBlockMax = 160u * 1024u;

// The shape of a scene's render launch, decided on the host without a HIP call (plan_launch); the
// launches (rrt_kernel.hip launch_variant, rrt_books64.hip launch64) run what it says and declare
// its lds_bytes, and scene creation asks it where the Perlin tables go and whether a launch exists.
//   f32 (rrt_kernel.hip): the block's LDS is the traversal stack (stack_depth x threads x
//     stack_bytes, rounded up to 16 B) + the staged scene (nodes, 48 B per primitive, + 16 B of
//     motion in the book-2/3 classes) + the Perlin tables when perlin_in_lds. Each kernel class has an
//     ordered list of launch shapes, all of them instantiated: the first is the tuned one (C2's
//     class: 1024 x 8, then 512 x 6). The plan takes the first whose LDS fits 64 KiB — the tuned shape
//     whenever it fits, so no measured config moves — else the smallest of them with the limit raised
//     (raise_limit), which every scene rrt_scene_create accepts fits into 160 KiB: 512 threads need at
//     most 64 KB of 16-bit stack + the 40 KB scene budget, the 32-bit stack at most 128 KB.
//   f64 (rrt_books64.hip): the class's block and, for a staged scene, the richest layout within its
//     budget (lds_budget64), as before.
// ok = 0: no shape within kLdsBlockMax (or a stack deeper than kMaxStackDepth): scene creation fails.
struct LaunchPlan {
    uint32_t ok;
    uint32_t f64;
    int32_t kclass;         // f32: -2 diffuse, -1 untextured, 0 full book 1, 1-3 book 2 (spheres, quads, media),
                            // 4 book 3; f64: 0 full, 1 untextured, 2 diffuse, 3 book 2 (kFlagF64Book2)
    int32_t arm;            // f32: the launch shape's place in rrt_kernel.hip's LaunchArm; f64: the scene mode
                            // (0 global, 1 staged with f32 sphere records, 2 staged with widened records)
    uint32_t stack_bytes;   // per stack entry: 2, or 4 for more than 65535 nodes
    uint32_t threads;       // per block
    uint32_t waves;         // launch-bounds waves per SIMD (1: no bound)
    uint32_t waves_nf;      // the same for the noise-free kernel of book-2/3 scenes without Perlin tables
    uint32_t scene_in_lds;  // the scene is staged in LDS
    uint32_t perlin_in_lds; // f32: the Perlin tables too
    uint32_t inv_r_in_lds;  // f64: the 1/r table too
    uint32_t rec32_in_lds;  // f64: the f32 pre-test records beside widened ones
    uint32_t raise_limit;   // lds_bytes > 64 KiB: the launch raises the kernel's dynamic-LDS limit first
    uint64_t lds_bytes;     // dynamic LDS of the block
};
// From the scene's counts and flags in p (n_nodes, n_prims, stack_depth, bvh_width, scene_in_lds,
// prim_motion / n_quads / n_media / flags for the class, specular, image_tex, n_perlin,
// perlin_in_lds, min_waves, global_waves; f64: sphere32 too). Pure: no device, no HIP call.
LaunchPlan plan_launch(const KParams &p);
LaunchPlan plan_launch_f64(const KParams &p);  // rrt_books64.hip; plan_launch forwards flags & kFlagF64 here
// Whether a book-2/3 scene's Perlin tables are staged in LDS: when the launch planned with them
// still fits the default 64 KiB.
bool perlin_fits_lds(KParams p);

// The ray-query kernel's parameters (rrt_scene_query_async, rrt_scene_primary_hits_async): the
// scene's tree and geometry tables as the render reads them, the leaf order, and the rays.
struct QParams {
    const void *nodes;          // GNode[] (staged in LDS) or GNodeH[]
    const float4 *prim_cr;      // leaf order
    const float4 *prim_motion;  // leaf order; null = a book-1 scene (r * r records)
    const GQuad *quads;
    const uint32_t *order;      // leaf position -> primitive in source order (spheres, then quads)
    const float4 *rays;         // RrtRay as (o.xyz, tmax), (d.xyz, time); null = the camera's primary rays
    uint2 *hits;                // RrtHit as (t bits, prim)
    uint32_t n;                 // rays, or width * height
    uint32_t n_groups;          // 64-ray groups: ceil(n / 64), or the camera's 8 x 8 pixel tiles
    uint32_t mode;              // RRT_QUERY_CLOSEST / RRT_QUERY_ANY
    uint32_t n_nodes, n_prims, n_quads;
    uint32_t stack_depth, leaf_frac;
    uint32_t width, height, tiles_x;  // primary rays
    float time;                       // primary rays
    float p00[3], du[3], dv[3], center[3];
    // surface records (rrt_scene_surface_async, rrt_scene_primary_surface_async), appended so the plain
    // queries' field offsets stay: surf != null selects the kernels with the record epilogue, which
    // write there instead of hits; the rest is the launcher's, the tables as the render reads them
    uint4 *surf;                 // RrtSurface as four 16-byte words
    const GMaterial *prim_mtl;   // leaf order
    const GPerlin *perlin;
    const uint8_t *tex_pool;
    const GTexture *texs;
    uint32_t bg_mode;
    float background[3];
};
// The query on `stream`, in the instantiation the scene's render plan names (tree placement, stack
// type) for the scene's geometry form; p.n_groups, tiles_x are the launcher's. n_cus: grid sizing.
hipError_t launch_query(const KParams &scene, QParams q, hipStream_t stream);

// Launch wrappers implemented in rrt_kernel.hip.
hipError_t launch_render(const KParams &p, hipStream_t stream);
hipError_t launch_render_counting(const KParams &p, hipStream_t stream);
// render_io quantiser on the device (d_accum: n_pixels x float4; d_rgb8: n_pixels x 3 B).
hipError_t launch_quantize(const float *d_accum, uint8_t *d_rgb8, uint32_t n_pixels, float scale, hipStream_t stream);
// The books path's quantiser (color.rs write_color) on the device, implemented in rrt_books64.hip:
// d_accum = n_pixels x float4, or n_pixels x D4 of f64 sums; scale = 1 / spp in f64; d_rgb8 as above.
hipError_t launch_quantize_books(const float *d_accum, uint8_t *d_rgb8, uint32_t n_pixels, double scale,
                                 hipStream_t stream);
hipError_t launch_quantize_books_f64(const double *d_accum, uint8_t *d_rgb8, uint32_t n_pixels, double scale,
                                     hipStream_t stream);
// Test support (rrt_testing_recip_check): the kernel's recip_rn / clamped_slope against the IEEE
// quotient (and sqrt_rn_big against the IEEE sqrt) over every f32 bit pattern; d_out: 3 zeroed u64
// mismatch counters
hipError_t launch_recip_check(unsigned long long *d_out, hipStream_t stream);
// Test support (rrt_testing_device_ops): the f32 kernel's own building blocks applied elementwise.
// device_op_columns: the 32-bit words per row of `in` and `out` for an RrtDeviceOp (0, 0: no such
// op). d_aux: one GPerlin table (PERLIN, with `scale`) or n_aux GQuad records (QUAD).
void device_op_columns(uint32_t op, uint32_t &cols_in, uint32_t &cols_out);
hipError_t launch_device_ops(uint32_t op, uint32_t n, const float *d_in, uint32_t *d_out, const void *d_aux,
                             uint32_t n_aux, float scale, hipStream_t stream);
// Test support (rrt_testing_div_check): div_by_a on refine_ra(a) against the IEEE quotient over every
// f32 numerator for each of the n_a divisors, and div_by_const over x = 0 and [2^-100, 8]; d_out: 8
// zeroed u64 counters
hipError_t launch_div_check(const float *d_a, uint32_t n_a, unsigned long long *d_out, hipStream_t stream);
// Test support (rrt_testing_trig32_check, rrt_books64.hip): the largest errors of the device's acosf
// over [-1, 1] and atanf over [0, 1] against its f64 acos / atan (d_out: 2 zeroed u64 holding f64
// bits), and the error bounds the f64 kernel's texel enclosures assume (bounds[2])
hipError_t launch_trig32_check(unsigned long long *d_out, double *bounds, hipStream_t stream);
hipError_t launch_sqrt64_check(unsigned long long *d_out, hipStream_t stream);
// Test support (rrt_testing_device_ops64, rrt_books64.hip): the f64 kernel's own building blocks applied
// elementwise. device_op64_columns: the f64 columns per row of `in` and the 64-bit words per row of
// `out` for an RrtDeviceOp64 (0, 0: no such op).
void device_op64_columns(uint32_t op, uint32_t &cols_in, uint32_t &cols_out);
// d_aux: n_aux GQuad64 records (QUAD64), else null.
hipError_t launch_device_ops64(uint32_t op, uint32_t n, const double *d_in, uint64_t *d_out, const void *d_aux,
                               uint32_t n_aux, hipStream_t stream);
// Implemented in rrt_books64.hip: one sample pass of the f64 books kernel (+ its chunk combine)
// into p.accum64, and the f64 sums rounded to the f32 RGBA accum of the ABI.
hipError_t launch_render_pass_f64(const KParams &p, bool count, hipStream_t stream);
// The f64 render in sequential-sum mode (p.seq): the prefix + tail-chunk passes and the in-order
// folds of the tail samples (rrt_books64.hip).
hipError_t launch_render_f64_seq(const KParams &p, bool count, hipStream_t stream);
// LDS of the f64 kernel's block with the scene staged in its smallest form (Node112 nodes, f32
// sphere records, no 1/r table): the host stages an f64 scene only when this is <= 64 KB
size_t f64_lds_min_bytes(uint32_t n_nodes, uint32_t n_prims, uint32_t stack_depth);
hipError_t launch_accum64_to_f32(const D4 *d_accum64, float4 *d_accum, uint32_t n_pixels, hipStream_t stream);
// Test support (rrt_testing_f64_layout): force the f64 kernel's LDS layout of a staged scene (-1: auto)
void set_f64_layout(int layout);

// RRT_FLAG_DEVICE_BVH (include/rrt_hip.h): scene creation builds the tree on the device
constexpr uint32_t kFlagDeviceBvh = 0x10u;
// The binned SAH builder of rrt_bvh_binned.h on the current device (rrt_bvh_build.hip). upload:
// one padded box per primitive and the n_tree >= 2 primitives of the tree in their original order
// (host pointers). build: the tree of one shape, kept on the device in raw f64 form; may be called
// again for another shape. emit: the last build's nodes in the 80-B or 32-B format as a fresh
// hipMalloc'd array the caller owns, and the leaf order (n_tree entries) to the host. Synchronous,
// on the default stream. Every array is sized for n_boxes primitives, the scene's count, so that
// set_objects() can put any of them into the tree later.
namespace bvhb {
struct Box6;
struct Summary;
}  // namespace bvhb
// Of one shape choice (stats_begin() .. ): rrt_testing_scene_build_stats.
struct BuildStats {
    uint64_t builder, launches, blocking_reads, form, shape_attempts;
};
class DeviceBvhBuilder {
public:
    DeviceBvhBuilder();
    ~DeviceBvhBuilder();
    DeviceBvhBuilder(const DeviceBvhBuilder &) = delete;
    DeviceBvhBuilder &operator=(const DeviceBvhBuilder &) = delete;
    hipError_t upload(const bvhb::Box6 *boxes, uint32_t n_boxes, const uint32_t *objs, uint32_t n_tree);
    // Replaces the tree's primitives before a build (rrt_scene_update_world: a medium enters or
    // leaves the tree): 2 <= n_tree <= n_boxes indices into the boxes, in their original order. One
    // blocking copy, no allocation. The tree held stays the last build's until build() runs again.
    hipError_t set_objects(const uint32_t *objs, uint32_t n_tree);
    uint32_t n_tree() const;
    hipError_t build(uint32_t max_leaf, double node_cost, bvhb::Summary *out);
    hipError_t emit(uint32_t stride, uint8_t **d_nodes_out, uint32_t *order_out);
    uint32_t levels() const;  // of the last build: one blocking read each
    // A builder kept by its scene (rrt_scene_update_spheres) is built again over new boxes without
    // another upload: the caller rewrites device_boxes() in place (n_boxes rows, same primitives),
    // build() starts from the uploaded order again, and emit_into() packs the nodes into a buffer the
    // caller owns (cap_bytes >= n_nodes x stride, else hipErrorInvalidValue). reserve() sizes the
    // per-level arrays for the widest level any tree over the n_boxes primitives can have (n_boxes / 2
    // tasks), after which build() allocates nothing, whatever set_objects() brings. device_order(): the last build's leaf order on
    // the device. allocations(): hipMalloc calls made by this builder so far.
    bvhb::Box6 *device_boxes();
    const uint32_t *device_order() const;
    hipError_t reserve();
    hipError_t emit_into(uint32_t stride, uint8_t *d_nodes, size_t cap_bytes, uint32_t *order_out);
    uint64_t allocations() const;
    // Refit (rrt_scene_refit_spheres): the boxes of the last build's tree recomputed bottom-up from
    // device_boxes() (rrt_bvh_binned.h refit_raw), links and leaf order kept, then the root's slack,
    // all enqueued on `stream` with no host synchronisation and no allocation: one launch per level,
    // deepest first, or for a small tree one single-workgroup launch that loops over the levels.
    // emit_refit() packs the refitted nodes on the same stream with the slack read on the device.
    // refit_launches() / refit_form() (1: the single workgroup): the last refit's.
    hipError_t refit(hipStream_t stream);
    bool refit_form_ok() const;  // false: the single workgroup is forced (set_refit_form) on a tree over its bound
    static uint32_t refit_small_max_nodes();
    hipError_t emit_refit(uint32_t stride, uint8_t *d_nodes, size_t cap_bytes, hipStream_t stream);
    uint32_t refit_launches() const;
    uint32_t refit_form() const;
    // The SAH cost (rrt_bvh_binned.h sah_term / sah_of_terms) of the tree held now and of the last
    // build's tree, on the default stream, synchronous (the caller has synchronised the device). The
    // first refit after a build sets the build's terms aside on its stream, so refit() needs
    // reserve_refit() once beforehand (it allocates; reserve_cost() is tree_cost()'s own part).
    hipError_t reserve_cost();
    hipError_t reserve_refit();
    hipError_t tree_cost(double *sah, double *sah_at_build);
    uint64_t refits_since_build() const;
    // The fast builder (rrt_bvh_lbvh.h) over the same boxes, objects and tree storage, so that emit,
    // emit_into, refit, emit_refit and tree_cost serve its tree as they serve build()'s. lbvh_build:
    // the sorted order and topology, and by the build's one blocking read the summaries of two shapes
    // (leaves of up to leaf_a, leaf_b); the small form also finishes one in its launch: shape 0 when
    // its node count is at most fit_nodes, else shape 1 (the caller's prediction of its own choice).
    // lbvh_finish: shape 0 or 1 becomes the held tree (numbers, links, boxes; no read), node_cost the
    // price tree_cost() weighs its node children by. The workspace is allocated by the first
    // lbvh_build (reserve_lbvh), sized for n_boxes; later ones allocate nothing.
    hipError_t reserve_lbvh();
    hipError_t lbvh_build(uint32_t leaf_a, uint32_t leaf_b, uint32_t fit_nodes, bvhb::Summary out[2]);
    hipError_t lbvh_finish(int shape, double node_cost, bvhb::Summary *out);
    static uint32_t lbvh_small_max();
    void stats_begin();
    BuildStats stats() const;

private:
    struct Impl;
    Impl *impl_;
};

// The scene-update kernels (rrt_scene_update.hip), on `stream` (the default stream when null):
//   launch_sphere_boxes  one lane per sphere: its padded f64 box (rrt_sphere_box.h) into boxes[i];
//                        spheres = RrtSphere records, motion = n x 4 floats or null
//   launch_leaf_tables   one lane per leaf position: the per-primitive tables scene creation forms
struct LeafTables {
    uint32_t n_prims, n_spheres, book2, f64;
    // leaf position -> primitive (spheres, then quads as n_spheres + j, then media as n_spheres +
    // n_quads + m): the builder's n_tree entries, then the unbounded media, held here by value
    const uint32_t *order;
    uint32_t n_tree, n_quads;
    uint32_t unbounded[kMaxUnbounded];
    const void *media;         // RrtMedium[n_media], source order (their material indices)
    const void *spheres;       // RrtSphere[n_spheres], source order
    const float *motion;       // n_spheres x 4, or null (all zero)
    const GMaterial *mats;     // the material table, source order
    const double4 *mat_diel;   // f64: per material, a dielectric's constants (zeros otherwise)
    const float4 *quad_rows;   // per quad: its prim_cr row, its prim_motion row
    const uint32_t *quad_mat;  // per quad: its material index
    float4 *prim_cr;
    GMaterial *prim_mtl;
    float4 *prim_motion;       // book2
    double *prim_inv_r64;      // f64
    double4 *prim_diel64;      // f64
};
hipError_t launch_sphere_boxes(uint32_t n, const void *d_spheres, const float *d_motion, void *d_boxes,
                               hipStream_t stream = nullptr);
hipError_t launch_leaf_tables(const LeafTables &t, hipStream_t stream = nullptr);
// rrt_scene_update_geometry / rrt_scene_refit_geometry (rrt_quad_form.h on the device), one lane per row:
//   launch_quad_boxes    quad j's padded f64 box into boxes[j] (the caller passes the builder's
//                        boxes + n_spheres); quads = RrtQuad records
//   launch_quad_records  quad j's GQuad into gquads[j] or GQuad64 into gquads64[j] (either may be
//                        null), its two leaf-table rows into quad_rows[2j, 2j + 1] and its
//                        material index into quad_mat[j]
//   launch_lights        light l's GLight into glights[l] and, for a quad light, its GQuad into
//                        gquads[light_quad[l]]; lights = RrtLight records
hipError_t launch_quad_boxes(uint32_t n, const void *d_quads, void *d_boxes, hipStream_t stream = nullptr);
hipError_t launch_quad_records(uint32_t n, const void *d_quads, GQuad *gquads, GQuad64 *gquads64, float4 *quad_rows,
                               uint32_t *quad_mat, hipStream_t stream = nullptr);
hipError_t launch_lights(uint32_t n, const void *d_lights, const uint32_t *light_quad, GLight *glights, GQuad *gquads,
                         hipStream_t stream = nullptr);
// rrt_scene_update_world / rrt_scene_refit_world (rrt_medium_form.h on the device), one lane per row:
//   launch_medium_boxes    medium m's box into boxes[m] (the caller passes the builder's boxes +
//                          n_spheres + n_quads); media = RrtMedium records whose quad ranges lie
//                          within the n_bquads RrtQuad records of bquads (a lane whose range does not
//                          writes nothing)
//   launch_medium_records  medium m's GMedium into gmedia[m]
//   launch_bquad_records   boundary quad k's GQuad into gquads[k] (the caller passes the scene's
//                          GQuad array + n_quads)
hipError_t launch_medium_boxes(uint32_t n, const void *d_media, const void *d_bquads, uint32_t n_bquads, void *d_boxes,
                               hipStream_t stream = nullptr);
hipError_t launch_medium_records(uint32_t n, const void *d_media, uint32_t n_quads, GMedium *gmedia,
                                 hipStream_t stream = nullptr);
hipError_t launch_bquad_records(uint32_t n, const void *d_bquads, GQuad *gquads, hipStream_t stream = nullptr);
// Test support (rrt_testing_refit_form): force the refit's per-level launches (0) or its single
// workgroup (1); -1: the automatic choice. False for another value.
bool set_refit_form(int form);
// rrt_testing_lbvh_form: the fast builder's launch-per-phase form (0) or its single workgroup (1).
bool set_lbvh_form(int form);
constexpr uint32_t kFlagFastBvh = 0x40u;

}  // namespace rrt
