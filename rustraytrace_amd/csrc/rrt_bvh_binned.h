// rrt_bvh_binned.h — the binned SAH builder behind RRT_FLAG_DEVICE_BVH, defined once for the host
// twin (rrt_host.cpp rrt_build_bvh_binned) and the device builder (rrt_bvh_build.hip). Every
// floating-point decision of the builder lives here; both sides compile it with -ffp-contract=off
// and it calls no library function (conversions, + - * / and comparisons only; unions and the
// roundings of the stored boxes work on integer bit patterns), so the two cannot diverge.
//
// Input: one padded f64 box per primitive (rrt_host.cpp prim_boxes: spheres with both motion ends,
// quads, bounded media), the primitives of the tree in their original order, max_leaf, node_cost.
//
// The build is top-down and level-synchronous. A *task* is a range objs[lo, hi) of span > 1 whose box
// and centroid bounds are known (the root's from a reduction, a child's from its parent's bins). Per
// level every task is binned, decided and, if it splits, partitioned:
//   bin      An axis is usable when cmax > cmin and the two bounds fall into different bins
//            (axis_usable: rules out differences that overflow or vanish in bin_index's scale). A
//            primitive's bin on an axis is bin_index(centroid, cmin, cmax): x = (c - cmin) * (16 /
//            (cmax - cmin)), truncated, 15 when x is not below 16. Each of the 16 bins per axis keeps
//            a count and the union of its primitives' boxes and centroids (Bin). Unions are taken
//            on the order-preserving integer key of the f64 bits (f64_key), a total order (-0 < +0),
//            so any reduction order gives the same bits. Primitive boxes are NaN-free by contract (a
//            NaN key simply orders above +inf or below -inf, the same on both sides).
//            A task with no usable axis (every centroid coincides) is binned by position instead:
//            axis 0, bin 0 = its first span / 2 primitives in current order, bin 1 = the rest.
//   decide   15 planes per usable axis, left = bins [0, p], right = (p, 15]; planes with an empty
//            side are skipped; cost = A(L) * nL + A(R) * nR with surface_area's operations and order.
//            The winner is the first candidate, replaced by every later one of strictly smaller cost,
//            in (axis, plane) order. Leaf rule (Builder::build's): leaf when span <= max_leaf &&
//            !(area > 0 && node_cost + cost / area < span). No usable axis: leaf when span <=
//            max_leaf, else split at lo + span / 2 in the current order (a cluster of n coincident
//            centroids is log2 n deep; the sweep builder chains it n deep).
//   split    stable: primitives with bin <= plane go left, relative order kept, so sibling leaves are
//            adjacent. A child of span 1 is a leaf at once; a larger child is a task of the next level.
// Only internal nodes are numbered, breadth-first: level by level, tasks left to right, root = 0. A
// root that decides "leaf" is stored as node 0 with child 0 = that leaf and child 1 never hit, depth 1
// (flatten2's root-leaf form). max_depth = levels holding an internal node, stack_need = max_depth + 1.
//
// Stored boxes are today's pipeline (rrt_host.cpp put_box / put_node2) in integer-step form: the
// subtree's union, BoxSlack growth from the root box, f32 rounded outward by one bit step where the
// nearest f32 lies inside, and for the 32-B node each plane rounded outward to f16 by integer
// arithmetic with subnormal results pushed out to 0 or the smallest normal.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RRT_BB_HD __host__ __device__ inline
#else
#define RRT_BB_HD inline
#endif

namespace rrt {
namespace bvhb {

constexpr int kBins = 16;
constexpr uint32_t kNoSlot = 0xffffffffu;  // Task::slot of the root
constexpr uint32_t kAxisMedian = 3u;       // Decision::axis of a split by position

RRT_BB_HD uint64_t f64_bits(double d) { return __builtin_bit_cast(uint64_t, d); }
RRT_BB_HD double bits_f64(uint64_t b) { return __builtin_bit_cast(double, b); }
RRT_BB_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
RRT_BB_HD float bits_f32(uint32_t b) { return __builtin_bit_cast(float, b); }

// Order-preserving key of an f64: a < b as doubles implies key(a) < key(b) as integers; -0 < +0.
RRT_BB_HD uint64_t f64_key(double d) {
    const uint64_t b = f64_bits(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
RRT_BB_HD double key_f64(uint64_t k) { return bits_f64((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }
constexpr uint64_t kKeyPosInf = 0xfff0000000000000ull;  // f64_key(+inf): identity of a min
constexpr uint64_t kKeyNegInf = 0x000fffffffffffffull;  // f64_key(-inf): identity of a max

// A primitive's padded box: 48 B.
struct Box6 {
    double mn[3], mx[3];
};

// Keys of a box and of centroid bounds: k[0..2] box min, k[3..5] box max, k[6..8] centroid min,
// k[9..11] centroid max. Slots 0-2 and 6-8 reduce by integer min, 3-5 and 9-11 by integer max.
struct Bounds {
    uint64_t k[12];
};
RRT_BB_HD bool key_is_min(int j) { return j < 3 || (j >= 6 && j < 9); }
RRT_BB_HD Bounds bounds_empty() {
    Bounds b;
    for (int j = 0; j < 12; ++j) b.k[j] = key_is_min(j) ? kKeyPosInf : kKeyNegInf;
    return b;
}
RRT_BB_HD void bounds_merge(Bounds &a, const Bounds &b) {
    for (int j = 0; j < 12; ++j) {
        const bool take = key_is_min(j) ? b.k[j] < a.k[j] : b.k[j] > a.k[j];
        if (take) a.k[j] = b.k[j];
    }
}
RRT_BB_HD double centroid(const Box6 &b, int axis) { return 0.5 * (b.mn[axis] + b.mx[axis]); }  // Builder::centroid
RRT_BB_HD Bounds bounds_of(const Box6 &b) {
    Bounds r;
    for (int a = 0; a < 3; ++a) {
        r.k[a] = f64_key(b.mn[a]);
        r.k[3 + a] = f64_key(b.mx[a]);
        r.k[6 + a] = r.k[9 + a] = f64_key(centroid(b, a));
    }
    return r;
}

// One bin of one axis: 104 B. The device reduces n by integer adds and b.k by 64-bit integer
// atomic min / max; the twin does the same sequentially.
struct Bin {
    uint64_t n;
    Bounds b;
};

RRT_BB_HD int bin_index(double c, double cmin, double cmax) {
    const double scale = (double)kBins / (cmax - cmin);
    const double x = (c - cmin) * scale;
    if (!(x < (double)kBins)) return kBins - 1;  // also a NaN x
    return x > 0.0 ? (int)x : 0;                 // c >= cmin: x >= 0
}
RRT_BB_HD bool axis_usable(double cmin, double cmax) {
    return cmax > cmin && bin_index(cmax, cmin, cmax) > bin_index(cmin, cmin, cmax);
}

struct Task {
    uint32_t lo, hi;  // objs[lo, hi), span > 1
    uint32_t slot;    // 2 * parent node + side, kNoSlot for the root
    uint32_t usable;  // bit a: axis a takes bins (task_finish); 0: the task is binned by position
    Bounds b;
};
// Completes a task whose lo, hi, slot and bounds are set.
RRT_BB_HD void task_finish(Task &t) {
    t.usable = 0;
    for (int a = 0; a < 3; ++a)
        if (axis_usable(key_f64(t.b.k[6 + a]), key_f64(t.b.k[9 + a]))) t.usable |= 1u << a;
}
// The bin of the task's primitive at position i (lo <= i < hi) on `axis`; -1 when the axis takes no
// bins. A by-position task uses axis 0, bins 0 and 1.
RRT_BB_HD int task_bin(const Task &t, int axis, uint32_t i, const Box6 &box) {
    if (t.usable == 0) return axis == 0 ? (i - t.lo < (t.hi - t.lo) / 2u ? 0 : 1) : -1;
    if (!((t.usable >> axis) & 1u)) return -1;
    return bin_index(centroid(box, axis), key_f64(t.b.k[6 + axis]), key_f64(t.b.k[9 + axis]));
}

RRT_BB_HD double box_area(const Bounds &b) {  // surface_area
    const double a = key_f64(b.k[3]) - key_f64(b.k[0]);
    const double c1 = key_f64(b.k[4]) - key_f64(b.k[1]);
    const double c2 = key_f64(b.k[5]) - key_f64(b.k[2]);
    return 2.0 * (a * c1 + a * c2 + c1 * c2);
}

struct Decision {
    uint32_t split;   // 0: the task is a leaf
    uint32_t axis;    // 0-2, or kAxisMedian
    uint32_t plane;   // left = bins [0, plane]
    uint32_t n_left;
    Bounds child[2];
};

// bins: [axis][bin], 3 x kBins, as filled for this task.
RRT_BB_HD Decision decide(const Task &t, const Bin *bins, uint32_t max_leaf, double node_cost) {
    Decision d;
    d.split = 0;
    d.axis = 0;
    d.plane = 0;
    d.n_left = 0;
    d.child[0] = bounds_empty();
    d.child[1] = bounds_empty();
    const uint32_t span = t.hi - t.lo;
    if (t.usable == 0) {
        if (span <= max_leaf) return d;
        d.split = 1;
        d.axis = kAxisMedian;
        d.n_left = span / 2u;
        d.child[0] = bins[0].b;
        d.child[1] = bins[1].b;
        return d;
    }
    bool found = false;
    double best = 0.0;
    for (int axis = 0; axis < 3; ++axis) {
        if (!((t.usable >> axis) & 1u)) continue;
        const Bin *ab = bins + axis * kBins;
        double right_area[kBins];
        uint64_t right_n[kBins];
        Bounds acc = bounds_empty();
        uint64_t n = 0;
        for (int i = kBins - 1; i >= 1; --i) {
            bounds_merge(acc, ab[i].b);
            n += ab[i].n;
            right_area[i] = box_area(acc);
            right_n[i] = n;
        }
        acc = bounds_empty();
        n = 0;
        for (int p = 0; p < kBins - 1; ++p) {
            bounds_merge(acc, ab[p].b);
            n += ab[p].n;
            if (n == 0 || right_n[p + 1] == 0) continue;
            const double cost = box_area(acc) * (double)n + right_area[p + 1] * (double)right_n[p + 1];
            if (!found || cost < best) {
                found = true;
                best = cost;
                d.axis = (uint32_t)axis;
                d.plane = (uint32_t)p;
                d.n_left = (uint32_t)n;
            }
        }
    }
    if (!found) return d;  // unreachable for a usable axis: its cmin and cmax primitives differ in bin
    const double area = box_area(t.b);
    const bool keep_leaf = span <= max_leaf && !(area > 0.0 && node_cost + best / area < (double)span);
    if (keep_leaf) return d;
    d.split = 1;
    const Bin *ab = bins + d.axis * kBins;
    for (int i = 0; i < kBins; ++i) bounds_merge(d.child[i <= (int)d.plane ? 0 : 1], ab[i].b);
    return d;
}

// Whether the task's primitive at position i with box `box` goes left under decision d.
RRT_BB_HD bool goes_left(const Task &t, const Decision &d, uint32_t i, const Box6 &box) {
    if (d.axis == kAxisMedian) return i - t.lo < d.n_left;
    const double cmin = key_f64(t.b.k[6 + d.axis]), cmax = key_f64(t.b.k[9 + d.axis]);
    return bin_index(centroid(box, (int)d.axis), cmin, cmax) <= (int)d.plane;
}

// An internal node before the format's roundings: both children's f64 boxes (mn xyz, mx xyz) and
// links (a node index, or first | count << 28 for a leaf). 112 B.
struct RawNode {
    double box[2][6];
    uint32_t link[2];
    uint32_t _pad[2];
};
constexpr uint32_t kLeafShift = 28;  // == rrt::kLinkCountShift

// ---- stored boxes ------------------------------------------------------------------------------
RRT_BB_HD double abs64(double x) { return bits_f64(f64_bits(x) & 0x7fffffffffffffffull); }
RRT_BB_HD bool finite64(double x) { return (f64_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// BoxSlack (rrt_host.cpp): o[a] = the root box's largest |coordinate| on axis a.
struct Slack {
    double o[3];
};
RRT_BB_HD Slack slack_of(const double *root_box /* mn xyz, mx xyz */) {
    Slack s;
    for (int a = 0; a < 3; ++a) {
        const double lo = abs64(root_box[a]), hi = abs64(root_box[3 + a]);
        const double m = lo > hi ? lo : hi;  // std::max(lo, hi); a NaN m fails the test below either way
        s.o[a] = (finite64(m) && m < 1e29) ? m : 0.0;
        if (lo != lo || hi != hi) s.o[a] = 0.0;
    }
    return s;
}
RRT_BB_HD double slack_grow(const Slack &s, int a, double p) { return 4.0 * 0x1.0p-24 * (2.0 * abs64(p) + 3.0 * s.o[a]); }

RRT_BB_HD float f32_step(float f, bool up) {  // the next f32 toward +inf (up) or -inf
    const uint32_t b = f32_bits(f);
    if ((b & 0x7fffffffu) == 0) return bits_f32(up ? 0x00000001u : 0x80000001u);
    const bool neg = (b >> 31) != 0;
    return bits_f32(neg == up ? b - 1u : b + 1u);
}
RRT_BB_HD float f32_down(double d) {
    float f = (float)d;
    if ((double)f > d) f = f32_step(f, false);
    return f;
}
RRT_BB_HD float f32_up(double d) {
    float f = (float)d;
    if ((double)f < d) f = f32_step(f, true);
    return f;
}

// put_box: lo / hi of one child box (6 doubles) with slack (null: none, the never-hit box).
RRT_BB_HD void round_box(const double *box, const Slack *slack, float *lo, float *hi) {
    for (int a = 0; a < 3; ++a) {
        double mn = box[a], mx = box[3 + a];
        if (slack && mn <= mx && finite64(mn) && finite64(mx) && mx < 1e29) {
            mn -= slack_grow(*slack, a, mn);
            mx += slack_grow(*slack, a, mx);
        }
        lo[a] = f32_down(mn);
        hi[a] = f32_up(mx);
    }
}
RRT_BB_HD void never_hit(double *box) {
    for (int j = 0; j < 6; ++j) box[j] = 1e30;
}
// A never-hit slot as the 32-B packers (pack_node32, rrt_host.cpp put_node2) recognise it after
// round_box: its lo is 1e30 rounded DOWN to f32, one step below 1e30f (which lies above 1e30), so the
// test is against a bound under both; real boxes stay below 1e29 (round_box).
constexpr float kNeverHitLo = 9e29f;

// f32 -> f16 bits rounded toward -inf (up = false) or +inf, subnormal results pushed outward to 0
// or the smallest normal (rrt_host.cpp f16_round, without the conversion instruction).
RRT_BB_HD uint16_t f16_round(float x, bool up) {
    const uint32_t u = f32_bits(x);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t mag = u & 0x7fffffffu;
    const bool neg = sign != 0;
    if (mag > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (mag == 0x7f800000u) return (uint16_t)(sign | 0x7c00u);
    const bool away = up != neg;  // round the magnitude up
    const uint32_t e = mag >> 23;
    uint32_t h;
    bool inexact;
    if (e >= 143u) {  // >= 2^16: past the largest finite f16
        h = 0x7bffu;
        inexact = true;
    } else if (e >= 113u) {
        h = ((e - 112u) << 10) | ((mag >> 13) & 0x3ffu);
        inexact = (mag & 0x1fffu) != 0;
    } else {  // below 2^-14: a multiple of 2^-24
        const uint32_t m = e ? ((mag & 0x7fffffu) | 0x800000u) : (mag & 0x7fffffu);
        const uint32_t shift = e ? 126u - e : 125u;
        if (shift >= 32u) {
            h = 0;
            inexact = mag != 0;
        } else {
            h = m >> shift;
            inexact = (m & ((1u << shift) - 1u)) != 0;
        }
    }
    if (away && inexact) h += 1u;
    uint32_t b = sign | h;
    if ((b & 0x7c00u) == 0 && (b & 0x03ffu) != 0) b = up ? (neg ? 0x8000u : 0x0400u) : (neg ? 0x8400u : 0x0000u);
    return (uint16_t)b;
}

// The two node formats (rrt_internal.h GNode, GNodeH) as 32-bit words.
RRT_BB_HD void pack_node80(const float lo[2][3], const float hi[2][3], const uint32_t link[2], uint32_t *w /* 20 */) {
    for (int c = 0; c < 2; ++c)
        for (int a = 0; a < 3; ++a) {
            w[9 * c + 3 * a] = f32_bits(lo[c][a]);
            w[9 * c + 3 * a + 1] = f32_bits(hi[c][a]);
            w[9 * c + 3 * a + 2] = f32_bits(lo[c][a]);
        }
    w[18] = link[0];
    w[19] = link[1];
}
RRT_BB_HD void pack_node32(const float lo[2][3], const float hi[2][3], const uint32_t link[2], uint32_t *w /* 8 */) {
    for (int c = 0; c < 2; ++c) {
        // (compared with 1e30f the slot became the box [65504, +inf)^3, which a ray into the positive
        // octant enters, and its link 0 is the root)
        const bool never = lo[c][0] >= kNeverHitLo;
        for (int a = 0; a < 3; ++a) {
            const uint32_t l = never ? 0x7bffu : f16_round(lo[c][a], false);
            const uint32_t h = never ? 0x7bffu : f16_round(hi[c][a], true);
            w[3 * c + a] = l | (h << 16);
        }
    }
    w[6] = link[0];
    w[7] = link[1];
}
// One stored node from its raw form: stride 80 or 32. The never-hit box (never_hit) takes no slack
// by round_box's own test, as in put_box.
RRT_BB_HD void pack_node(const RawNode &r, const Slack &slack, uint32_t stride, uint32_t *w) {
    float lo[2][3], hi[2][3];
    for (int c = 0; c < 2; ++c) round_box(r.box[c], &slack, lo[c], hi[c]);
    if (stride == 80u) pack_node80(lo, hi, r.link, w);
    else pack_node32(lo, hi, r.link, w);
}

// ---- refit -------------------------------------------------------------------------------------
// The boxes of a built tree recomputed bottom-up from moved primitives; links and leaf order stay.
// A link of 0 is the never-hit slot of the root-leaf form (a node link is never 0: the root is no
// child, and a leaf link has count > 0): its box is kept and it takes no part in a union. Unions are
// the builder's: integer min / max of f64_key (-0 < +0), so a refit over the boxes the tree was built
// from reproduces the builder's bytes, in any evaluation order.
RRT_BB_HD bool link_is_leaf(uint32_t link) { return (link >> kLeafShift) != 0; }
RRT_BB_HD void box6_merge_keys(uint64_t *k /* 6: mn xyz, mx xyz */, const double *mn, const double *mx) {
    for (int a = 0; a < 3; ++a) {
        const uint64_t lo = f64_key(mn[a]), hi = f64_key(mx[a]);
        if (lo < k[a]) k[a] = lo;
        if (hi > k[3 + a]) k[3 + a] = hi;
    }
}
// Child c of node k from the level below (a node link's two child boxes) or from its primitives.
RRT_BB_HD void refit_child(RawNode *raw, uint32_t k, int c, const uint32_t *order, const Box6 *boxes) {
    const uint32_t link = raw[k].link[c];
    if (link == 0u) return;
    uint64_t key[6] = {kKeyPosInf, kKeyPosInf, kKeyPosInf, kKeyNegInf, kKeyNegInf, kKeyNegInf};
    if (link_is_leaf(link)) {
        const uint32_t first = link & ((1u << kLeafShift) - 1u), count = link >> kLeafShift;
        for (uint32_t i = first; i < first + count; ++i) {
            const Box6 &b = boxes[order[i]];
            box6_merge_keys(key, b.mn, b.mx);
        }
    } else {
        for (int cc = 0; cc < 2; ++cc) box6_merge_keys(key, raw[link].box[cc], raw[link].box[cc] + 3);
    }
    for (int j = 0; j < 6; ++j) raw[k].box[c][j] = key_f64(key[j]);
}
// The sequential refit: children carry larger numbers than their parents, so k runs downward.
inline void refit_raw(RawNode *raw, uint32_t n_nodes, const uint32_t *order, const Box6 *boxes) {
    for (uint32_t k = n_nodes; k-- > 0;)
        for (int c = 0; c < 2; ++c) refit_child(raw, k, c, order, boxes);
}
// The root's box: the union of node 0's child boxes (without a never-hit slot).
RRT_BB_HD void root_box_of(const RawNode &root, double *out /* 6 */) {
    uint64_t key[6] = {kKeyPosInf, kKeyPosInf, kKeyPosInf, kKeyNegInf, kKeyNegInf, kKeyNegInf};
    for (int c = 0; c < 2; ++c)
        if (root.link[c] != 0u) box6_merge_keys(key, root.box[c], root.box[c] + 3);
    for (int j = 0; j < 6; ++j) out[j] = key_f64(key[j]);
}

// The tree's SAH cost: node k's term is w0 * A(box0) + w1 * A(box1), A = box_area's operations, w =
// a leaf child's primitive count or node_cost for a node child (0 for a never-hit slot); the cost is
// the terms summed for k = 0 .. n-1 in that order, divided by the root box's area.
RRT_BB_HD double box6_area(const double *box) {
    const double a = box[3] - box[0], c1 = box[4] - box[1], c2 = box[5] - box[2];
    return 2.0 * (a * c1 + a * c2 + c1 * c2);
}
RRT_BB_HD double sah_term(const RawNode &r, double node_cost) {
    double w[2];
    for (int c = 0; c < 2; ++c) w[c] = r.link[c] == 0u ? 0.0 : (link_is_leaf(r.link[c]) ? (double)(r.link[c] >> kLeafShift) : node_cost);
    return w[0] * box6_area(r.box[0]) + w[1] * box6_area(r.box[1]);
}
inline double sah_of_terms(const double *terms, uint32_t n_nodes, const RawNode &root) {
    double sum = 0.0;
    for (uint32_t k = 0; k < n_nodes; ++k) sum += terms[k];
    double rb[6];
    root_box_of(root, rb);
    return sum / box6_area(rb);
}

// What the build reports besides nodes and order.
struct Summary {
    uint32_t n_nodes, n_leaves, max_depth, max_leaf;  // max_leaf: the largest leaf's count
};

}  // namespace bvhb
}  // namespace rrt
