// rrt_quad_form.h — everything a quad contributes to a scene, defined once for the host (scene
// creation, rrt_testing_quad_records, rrt_refit_bvh_binned_ex) and the device (rrt_scene_update.hip
// k_quad_boxes, k_quad_records, k_lights): its padded f64 box (quad.rs:43-47, aabb.rs:104-115), its
// derived plane in f64 (quad.rs:21-37: n = cross(u, v), normal = n * (1 / |n|), D = dot(normal, q),
// w = n * (1 / dot(n, n)); Vec3 / f64 is `(1 / rhs) * v`, vec3.rs:142-148), the f32 record the f32
// kernels read, its two leaf-table rows, and a book-3 light's record with a light quad's area
// (quad.rs:28). Both sides compile it with -ffp-contract=off; besides conversions, + - * /, and
// comparisons it calls sqrt(double), correctly rounded on either side, so an update on the device
// forms the bits scene creation forms on the host. A quad whose q, u, v are finite and whose u x v has
// a finite non-zero squared length produces no NaN here (quad_is_regular: what a geometry change
// accepts; a NaN formed on the host and one formed on the device need not share sign and payload).
#pragma once

#include <math.h>

#include "rrt_bvh_binned.h"
#include "rrt_internal.h"
#include "../../include/rrt_hip.h"

namespace rrt {

// The box of the four corners q, q + u + v, q + u, q + v, padded. min / max as std::min / std::max
// order their operands (the second only when strictly smaller / larger).
RRT_BB_HD bvhb::Box6 quad_box(const float *q3, const float *u3, const float *v3) {
    bvhb::Box6 b;
    for (int a = 0; a < 3; ++a) {
        const double q = q3[a], u = u3[a], v = v3[a];
        const double c0 = q, c1 = q + u + v, c2 = q + u, c3 = q + v;
        const double lo01 = c1 < c0 ? c1 : c0, lo23 = c3 < c2 ? c3 : c2;
        const double hi01 = c0 < c1 ? c1 : c0, hi23 = c2 < c3 ? c3 : c2;
        double mn = lo23 < lo01 ? lo23 : lo01;
        double mx = hi01 < hi23 ? hi23 : hi01;
        const double delta = 0.0001;
        if (mx - mn < delta) mn = mn - delta / 2.0, mx = mx + delta / 2.0;
        b.mn[a] = mn;
        b.mx[a] = mx;
    }
    return b;
}

// cross(u, v) in f64 from the f32 edges
RRT_BB_HD void quad_cross(const float *u3, const float *v3, double *n) {
    const double ux = u3[0], uy = u3[1], uz = u3[2], vx = v3[0], vy = v3[1], vz = v3[2];
    n[0] = uy * vz - uz * vy;
    n[1] = uz * vx - ux * vz;
    n[2] = ux * vy - uy * vx;
}

// The unrounded record (the f64 kernel's book-2 class reads it).
RRT_BB_HD GQuad64 quad_record64(const float *q3, const float *u3, const float *v3) {
    GQuad64 g;
    double n[3];
    quad_cross(u3, v3, n);
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double inv_len = 1.0 / sqrt(nn), inv_nn = 1.0 / nn;
    for (int a = 0; a < 3; ++a) {
        g.q[a] = q3[a];
        g.u[a] = u3[a];
        g.v[a] = v3[a];
        g.n[a] = n[a] * inv_len;
        g.w[a] = n[a] * inv_nn;
    }
    g.D = g.n[0] * g.q[0] + g.n[1] * g.q[1] + g.n[2] * g.q[2];
    return g;
}

// The f32 record: the f32 inputs as they are, the derived plane rounded once from f64.
RRT_BB_HD GQuad quad_record32(const float *q3, const float *u3, const float *v3) {
    const GQuad64 g64 = quad_record64(q3, u3, v3);
    GQuad g;
    g.q = make_float4(q3[0], q3[1], q3[2], (float)g64.D);
    g.u = make_float4(u3[0], u3[1], u3[2], 0.0f);
    g.v = make_float4(v3[0], v3[1], v3[2], 0.0f);
    g.n = make_float4((float)g64.n[0], (float)g64.n[1], (float)g64.n[2], 0.0f);
    g.w = make_float4((float)g64.w[0], (float)g64.w[1], (float)g64.w[2], 0.0f);
    return g;
}

// Quad j's leaf-table rows: (q, tag -(j + 1)) in the primitive slot, (normal, D) in the motion slot.
RRT_BB_HD float4 quad_row_cr(const GQuad &g, uint32_t j) { return make_float4(g.q.x, g.q.y, g.q.z, -(float)(j + 1u)); }
RRT_BB_HD float4 quad_row_plane(const GQuad &g) { return make_float4(g.n.x, g.n.y, g.n.z, g.q.w); }

// q, u, v finite and dot(u x v, u x v) finite and non-zero.
RRT_BB_HD bool quad_is_regular(const float *q3, const float *u3, const float *v3) {
    for (int a = 0; a < 3; ++a)
        if (!bvhb::finite64((double)q3[a]) || !bvhb::finite64((double)u3[a]) || !bvhb::finite64((double)v3[a])) return false;
    double n[3];
    quad_cross(u3, v3, n);
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    return bvhb::finite64(nn) && nn != 0.0;
}

// A book-3 light's record: a sphere as it is (radius max(r, 0)); a quad also its area |u x v| (f64,
// rounded) and `quad`, the index of its GQuad (its place among the light quads after the scene's).
RRT_BB_HD GLight light_record(const RrtLight &L, uint32_t quad) {
    GLight g;
    g.sphere = make_float4(L.a[0], L.a[1], L.a[2], L.a[3] < 0.0f ? 0.0f : L.a[3]);
    g.kind = L.kind;
    g.quad = 0u;
    g.area = 0.0f;
    g._pad = 0u;
    if (L.kind == RRT_LIGHT_QUAD) {
        double n[3];
        quad_cross(L.u, L.v, n);
        g.quad = quad;
        g.area = (float)sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    }
    return g;
}

}  // namespace rrt
