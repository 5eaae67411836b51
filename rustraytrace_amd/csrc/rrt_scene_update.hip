// rrt_scene_update.hip — the device side of rrt_scene_update_spheres and rrt_scene_refit_spheres: the spheres' padded boxes for
// the builder (rrt_bvh_build.hip) and, after the build, the per-primitive tables in leaf order. Both
// kernels restate what scene creation computes on the host (rrt_host.cpp prim_boxes and
// prim_table_row) so that an updated scene holds the bytes of a freshly created one. One lane per
// row, plain vector stores; nothing here is worth tuning (a 10^5-sphere scene moves ~10 MB).
// rrt_scene_update_geometry and rrt_scene_refit_geometry add the quads and the book-3 lights: their
// boxes, GQuad / GQuad64 records, leaf-table rows and GLight records, all from rrt_quad_form.h, the
// definition scene creation itself calls. rrt_scene_update_world and rrt_scene_refit_world add the
// constant media: their boxes and GMedium records from rrt_medium_form.h, their boundary quads' GQuad
// records and their leaf-table rows.
#include "rrt_internal.h"
#include "rrt_sphere_box.h"
#include "rrt_quad_form.h"
#include "rrt_medium_form.h"
#include "../../include/rrt_hip.h"

namespace rrt {

namespace {

constexpr int kBlk = 256;
static_assert(sizeof(RrtSphere) == 32, "RrtSphere is 32 B");

__global__ __launch_bounds__(kBlk) void k_sphere_boxes(uint32_t n, const RrtSphere *spheres, const float *motion,
                                                       bvhb::Box6 *boxes) {
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    const float4 cr4 = *reinterpret_cast<const float4 *>(spheres[i].center_radius);
    const float cr[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
    if (motion) {
        const float4 m4 = reinterpret_cast<const float4 *>(motion)[i];
        const float m[3] = {m4.x, m4.y, m4.z};
        boxes[i] = sphere_box(cr, m);
    } else {
        boxes[i] = sphere_box(cr, nullptr);
    }
}

// 1 / r as scene creation's `1.0f / r` (the correctly rounded f32 quotient, +inf at r = 0): the f64
// quotient rounded to f32. A 24-bit divisor's reciprocal is a power of two or at least 2^-48 (relative)
// away from every f32 rounding boundary, which the f64 quotient's 2^-53 cannot bridge, so the two
// roundings give the one; f64 division here is IEEE (no fast-math) and keeps f32's subnormal quotients.
__device__ __forceinline__ float recip_f32(float r) { return (float)(1.0 / (double)r); }

__global__ __launch_bounds__(kBlk) void k_leaf_tables(LeafTables t) {
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i >= t.n_prims) return;
    // the builder's order holds the tree's primitives; the unbounded media follow them
    // (selected by compares: a lane-indexed read of the by-value array would go through scratch)
    uint32_t o;
    if (i < t.n_tree) {
        o = t.order[i];
    } else {
        const uint32_t k = i - t.n_tree;
        o = k == 0u ? t.unbounded[0] : k == 1u ? t.unbounded[1] : k == 2u ? t.unbounded[2] : t.unbounded[3];
    }
    float4 cr, mo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    GMaterial mtl;
    uint32_t mat;
    if (o >= t.n_spheres + t.n_quads) {  // a medium: its tag, no geometry, its phase material
        const uint32_t m = o - t.n_spheres - t.n_quads;
        cr = medium_row_cr(t.n_quads, m);
        mat = reinterpret_cast<const RrtMedium *>(t.media)[m].material_index;
        mtl = t.mats[mat];
    } else if (o >= t.n_spheres) {  // a quad: its stored plane, (q, tag) and (normal, D)
        const uint32_t j = o - t.n_spheres;
        cr = t.quad_rows[2u * j];
        mo = t.quad_rows[2u * j + 1u];
        mat = t.quad_mat[j];
        mtl = t.mats[mat];
    } else {
        const RrtSphere *sp = reinterpret_cast<const RrtSphere *>(t.spheres) + o;
        const float4 c = *reinterpret_cast<const float4 *>(sp->center_radius);
        const float r = c.w < 0.0f ? 0.0f : c.w;  // max(radius, 0)
        mat = sp->material_index;
        mtl = t.mats[mat];
        if (t.book2 || t.f64) {
            cr = make_float4(c.x, c.y, c.z, r);
        } else {  // book-1 layout: r * r rounded once in f32, 1 / r in b.w
            cr = make_float4(c.x, c.y, c.z, __fmul_rn(r, r));
            mtl.b.w = __float_as_int(recip_f32(r));
        }
        if (t.motion) {
            const float4 m = reinterpret_cast<const float4 *>(t.motion)[o];
            mo = make_float4(m.x, m.y, m.z, 0.0f);
        }
        if (t.book2) mo.w = recip_f32(r);
    }
    t.prim_cr[i] = cr;
    t.prim_mtl[i] = mtl;
    if (t.book2) t.prim_motion[i] = mo;
    if (t.f64) {
        t.prim_inv_r64[i] = 1.0 / (double)cr.w;
        t.prim_diel64[i] = mtl.b.x == (int)RRT_MAT_DIELECTRIC ? t.mat_diel[mat] : make_double4(0.0, 0.0, 0.0, 0.0);
    }
}

// ---- quads and book-3 lights (rrt_scene_update_geometry, rrt_scene_refit_geometry) ---------------
static_assert(sizeof(RrtQuad) == 64 && sizeof(RrtLight) == 64, "RrtQuad and RrtLight are 64 B");

// a row's q, u, v (or a light's a, u, v) by three 16-B loads from 16-B aligned records
struct Quv {
    float q[3], u[3], v[3];
};
__device__ __forceinline__ Quv load_quv(const float *q4) {
    const float4 q = reinterpret_cast<const float4 *>(q4)[0], u = reinterpret_cast<const float4 *>(q4)[1],
                 v = reinterpret_cast<const float4 *>(q4)[2];
    return Quv{{q.x, q.y, q.z}, {u.x, u.y, u.z}, {v.x, v.y, v.z}};
}

__global__ __launch_bounds__(kBlk) void k_quad_boxes(uint32_t n, const RrtQuad *quads, bvhb::Box6 *boxes) {
    const uint32_t j = blockIdx.x * kBlk + threadIdx.x;
    if (j >= n) return;
    const Quv r = load_quv(quads[j].q);
    boxes[j] = quad_box(r.q, r.u, r.v);
}

__global__ __launch_bounds__(kBlk) void k_quad_records(uint32_t n, const RrtQuad *quads, GQuad *gquads, GQuad64 *gquads64,
                                                       float4 *quad_rows, uint32_t *quad_mat) {
    const uint32_t j = blockIdx.x * kBlk + threadIdx.x;
    if (j >= n) return;
    const Quv r = load_quv(quads[j].q);
    const GQuad g = quad_record32(r.q, r.u, r.v);
    if (gquads) gquads[j] = g;
    if (gquads64) gquads64[j] = quad_record64(r.q, r.u, r.v);
    quad_rows[2u * j] = quad_row_cr(g, j);
    quad_rows[2u * j + 1u] = quad_row_plane(g);
    quad_mat[j] = quads[j].material_index;
}

__global__ __launch_bounds__(kBlk) void k_lights(uint32_t n, const RrtLight *lights, const uint32_t *light_quad,
                                                 GLight *glights, GQuad *gquads) {
    const uint32_t l = blockIdx.x * kBlk + threadIdx.x;
    if (l >= n) return;
    const RrtLight L = lights[l];
    const uint32_t at = light_quad[l];
    glights[l] = light_record(L, at);
    if (L.kind == RRT_LIGHT_QUAD) gquads[at] = quad_record32(L.a, L.u, L.v);
}

// ---- constant media (rrt_scene_update_world, rrt_scene_refit_world) ------------------------------
static_assert(sizeof(RrtMedium) == 48 && sizeof(GMedium) == 32, "RrtMedium is 48 B, GMedium 32 B");
static_assert(kMaxUnbounded == 4u, "k_leaf_tables selects among four unbounded media");

// A lane loops over its medium's boundary quads (a make_box has 6).
__global__ __launch_bounds__(kBlk) void k_medium_boxes(uint32_t n, const RrtMedium *media, const RrtQuad *bquads,
                                                       uint32_t n_bquads, bvhb::Box6 *boxes) {
    const uint32_t m = blockIdx.x * kBlk + threadIdx.x;
    if (m >= n) return;
    const RrtMedium md = media[m];
    if (md.boundary_kind != RRT_BOUNDARY_SPHERE && ((uint64_t)md.first + md.count > n_bquads)) return;
    boxes[m] = medium_box(md, bquads);
}

__global__ __launch_bounds__(kBlk) void k_medium_records(uint32_t n, const RrtMedium *media, uint32_t n_quads,
                                                         GMedium *gmedia) {
    const uint32_t m = blockIdx.x * kBlk + threadIdx.x;
    if (m >= n) return;
    gmedia[m] = medium_record(media[m], n_quads);
}

// k_quad_records without the rows and the material: a boundary quad is no primitive of the scene.
__global__ __launch_bounds__(kBlk) void k_bquad_records(uint32_t n, const RrtQuad *bquads, GQuad *gquads) {
    const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
    if (k >= n) return;
    const Quv r = load_quv(bquads[k].q);
    gquads[k] = quad_record32(r.q, r.u, r.v);
}

}  // namespace

hipError_t launch_medium_boxes(uint32_t n, const void *d_media, const void *d_bquads, uint32_t n_bquads, void *d_boxes,
                               hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_medium_boxes, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtMedium *>(d_media), reinterpret_cast<const RrtQuad *>(d_bquads), n_bquads,
                       reinterpret_cast<bvhb::Box6 *>(d_boxes));
    return hipGetLastError();
}

hipError_t launch_medium_records(uint32_t n, const void *d_media, uint32_t n_quads, GMedium *gmedia, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_medium_records, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtMedium *>(d_media), n_quads, gmedia);
    return hipGetLastError();
}

hipError_t launch_bquad_records(uint32_t n, const void *d_bquads, GQuad *gquads, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bquad_records, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtQuad *>(d_bquads), gquads);
    return hipGetLastError();
}

hipError_t launch_quad_boxes(uint32_t n, const void *d_quads, void *d_boxes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_quad_boxes, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtQuad *>(d_quads), reinterpret_cast<bvhb::Box6 *>(d_boxes));
    return hipGetLastError();
}

hipError_t launch_quad_records(uint32_t n, const void *d_quads, GQuad *gquads, GQuad64 *gquads64, float4 *quad_rows,
                               uint32_t *quad_mat, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_quad_records, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtQuad *>(d_quads), gquads, gquads64, quad_rows, quad_mat);
    return hipGetLastError();
}

hipError_t launch_lights(uint32_t n, const void *d_lights, const uint32_t *light_quad, GLight *glights, GQuad *gquads,
                         hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lights, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtLight *>(d_lights), light_quad, glights, gquads);
    return hipGetLastError();
}

hipError_t launch_sphere_boxes(uint32_t n, const void *d_spheres, const float *d_motion, void *d_boxes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sphere_boxes, dim3((n + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, n,
                       reinterpret_cast<const RrtSphere *>(d_spheres), d_motion, reinterpret_cast<bvhb::Box6 *>(d_boxes));
    return hipGetLastError();
}

hipError_t launch_leaf_tables(const LeafTables &t, hipStream_t stream) {
    if (t.n_prims == 0) return hipSuccess;
    hipLaunchKernelGGL(k_leaf_tables, dim3((t.n_prims + kBlk - 1) / kBlk), dim3(kBlk), 0, stream, t);
    return hipGetLastError();
}

}  // namespace rrt
