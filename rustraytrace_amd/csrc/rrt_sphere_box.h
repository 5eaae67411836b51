// rrt_sphere_box.h — a sphere's padded f64 bounding box, defined once for the host
// (rrt_testing_sphere_boxes) and the device (rrt_scene_update.hip k_sphere_boxes). It restates
// rrt_host.cpp prim_boxes and pad operation by operation (sphere.rs:16-21, aabb.rs:29-34 and
// 104-115; a moving sphere: the_next_week/sphere.rs:31-33), so the boxes an update forms on the
// device carry the bits scene creation forms on the host. Both sides compile it with
// -ffp-contract=off; it uses conversions, + - and comparisons only.
#pragma once

#include "rrt_bvh_binned.h"

namespace rrt {

// cr: center xyz and radius (f32); motion: center2 - center1 (xyz, f32) or null.
RRT_BB_HD bvhb::Box6 sphere_box(const float *cr, const float *motion) {
    const double r32 = (double)cr[3];
    const double r = r32 < 0.0 ? 0.0 : r32;  // max(radius, 0)
    bvhb::Box6 b;
    for (int a = 0; a < 3; ++a) {
        const double c = (double)cr[a];
        double mn = c - r, mx = c + r;
        if (motion) {  // center2 = center1 + motion, an f32 sum (the kernel's t = 1 end)
            const double c2 = (double)(cr[a] + motion[a]);
            const double mn2 = c2 - r, mx2 = c2 + r;
            mn = mn <= mn2 ? mn : mn2;  // interval.rs:44-49
            mx = mx >= mx2 ? mx : mx2;
        }
        const double delta = 0.0001;
        if (mx - mn < delta) mn = mn - delta / 2.0, mx = mx + delta / 2.0;
        b.mn[a] = mn;
        b.mx[a] = mx;
    }
    return b;
}

}  // namespace rrt
