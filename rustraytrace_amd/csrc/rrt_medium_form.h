// rrt_medium_form.h — everything a constant medium contributes to a scene, defined once for the host
// (scene creation's prim_boxes and GMedium loop, rrt_testing_medium_records,
// rrt_refit_bvh_binned_world) and the device (rrt_scene_update.hip k_medium_boxes, k_medium_records,
// k_leaf_tables): its box (the boundary's, constant_medium.rs bounding_box), its 32-B GMedium record
// and its leaf-table row. Which media are tested outside the tree (rrt_host.cpp unbounded_media) is
// not here: that is a property of the whole scene, decided on the host. Both sides compile this with
// -ffp-contract=off; it uses conversions, + - /, comparisons and rrt_quad_form.h's quad_box, so an
// update on the device forms the bits scene creation forms on the host. A medium whose sphere row
// and density are finite and whose boundary quads are regular (quad_is_regular) produces no NaN here.
#pragma once

#include "rrt_bvh_binned.h"
#include "rrt_internal.h"
#include "rrt_quad_form.h"
#include "rrt_sphere_box.h"
#include "../../include/rrt_hip.h"

namespace rrt {

// Sphere boundary: [c - max(r, 0), c + max(r, 0)] in f64 from the f32 row, padded — a static
// sphere's box. Quad boundary: the union of its boundary quads' padded boxes, started from the empty
// box and folded in range order as aabb.rs's Aabb::from_boxes does (interval.rs:44-49 keeps the first
// operand on ties), with the constructor's pad after every fold: an axis-aligned face's own pad can
// leave its thin axis a rounding short of delta, and the fold then pads it once more — the bits
// scene creation has always formed. No further pad follows the last fold. bquads: the scene's
// boundary quads; the caller has checked md.first + md.count against their number.
RRT_BB_HD bvhb::Box6 medium_box(const RrtMedium &md, const RrtQuad *bquads) {
    if (md.boundary_kind == RRT_BOUNDARY_SPHERE) return sphere_box(md.sphere, nullptr);
    const double inf = __builtin_huge_val();
    bvhb::Box6 b;
    for (int a = 0; a < 3; ++a) b.mn[a] = inf, b.mx[a] = -inf;
    for (uint32_t k = 0; k < md.count; ++k) {
        const RrtQuad &qd = bquads[md.first + k];
        const bvhb::Box6 q = quad_box(qd.q, qd.u, qd.v);
        for (int a = 0; a < 3; ++a) {
            double mn = b.mn[a] <= q.mn[a] ? b.mn[a] : q.mn[a];
            double mx = b.mx[a] >= q.mx[a] ? b.mx[a] : q.mx[a];
            const double delta = 0.0001;
            if (mx - mn < delta) mn = mn - delta / 2.0, mx = mx + delta / 2.0;
            b.mn[a] = mn;
            b.mx[a] = mx;
        }
    }
    return b;
}

// The record the kernels read: the sphere with max(r, 0), the boundary's kind, its quads' place in
// the GQuad array (boundary quads follow the scene's n_quads quads) and -1 / density formed in f64
// and rounded once (constant_medium.rs:24).
RRT_BB_HD GMedium medium_record(const RrtMedium &md, uint32_t n_quads) {
    GMedium g;
    g.sphere = make_float4(md.sphere[0], md.sphere[1], md.sphere[2], md.sphere[3] < 0.0f ? 0.0f : md.sphere[3]);
    g.kind = md.boundary_kind;
    g.first = n_quads + md.first;
    g.count = md.count;
    g.neg_inv_density = (float)(-1.0 / (double)md.density);
    return g;
}

// Medium m's leaf-table row: no geometry, the tag -(1 + n_quads + m) (the quads' tags end at -n_quads).
RRT_BB_HD float4 medium_row_cr(uint32_t n_quads, uint32_t m) {
    return make_float4(0.0f, 0.0f, 0.0f, -(float)(n_quads + m + 1u));
}

// The sphere row is finite (what a world change accepts of a sphere-bounded medium).
RRT_BB_HD bool medium_sphere_is_finite(const RrtMedium &md) {
    for (int a = 0; a < 4; ++a)
        if (!bvhb::finite64((double)md.sphere[a])) return false;
    return true;
}

}  // namespace rrt
