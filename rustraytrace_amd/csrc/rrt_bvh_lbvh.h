// rrt_bvh_lbvh.h — the fast builder behind RRT_FLAG_FAST_BVH, defined once for the host twin
// (rrt_host.cpp rrt_build_bvh_lbvh) and the device builder (rrt_bvh_build.hip): an LBVH. It decides
// the leaf order and the topology; every stored box comes from rrt_bvh_binned.h (refit_child over the
// numbered tree, slack_of, pack_node). Both sides compile it with -ffp-contract=off and it calls no
// library function, so the two cannot diverge.
//
// Input: the binned builder's: one padded f64 box per primitive, the tree's primitives objs[0, n) in
// source order, n >= 2.
//   bounds    the centroid bounds of the tree's primitives: unions on f64_key (bounds_of / bounds_merge).
//   code      10 bits per axis: cell = (c - cmin) * (1024 / (cmax - cmin)), truncated, 1023 when not
//             below 1024 (morton_cell). An axis is usable by axis_usable's rule; an unusable axis
//             contributes cell 0. The cells are interleaved x, y, z from the top: bit 3 b + 2 of the
//             code is bit b of the x cell, 3 b + 1 of y, 3 b of z.
//   key       code << 32 | position in objs. Keys are unique, so every correct sort gives one order:
//             the leaf order.
//   topology  Karras' construction over the sorted keys (karras_node): internal node i, 0 <= i < n - 1,
//             covers positions [first, last] with i one of the two, and splits after position `split`;
//             delta is the common-prefix length of two 64-bit keys, no special case for equal codes
//             (the index bits tell them apart). The root is i = 0. A node is at most 62 levels deep
//             (the keys differ in their low 62 bits only), so stack_need <= 63.
//   leaves    for max_leaf m, a node whose range holds > m primitives is kept; a child that holds
//             <= m (an internal node of fewer primitives, or a single primitive) is a leaf of its
//             range. A root that holds <= m is the binned builder's root-leaf form.
//   numbers   kept nodes only, breadth-first: by level (the count of a node's ancestors, the same in
//             every shape: the ancestors of a kept node hold more than it and are kept), within a level
//             by `first`: the order of the keys level << 56 | first << 28 | i (number_key).
#pragma once

#include "rrt_bvh_binned.h"

namespace rrt {
namespace lbvh {

using namespace bvhb;

constexpr uint32_t kCells = 1024;
constexpr uint32_t kLeafChild = 0x80000000u;  // KNode::child: a single primitive at position child & ~kLeafChild
constexpr uint32_t kNoParent = 0xffffffffu;
constexpr uint32_t kMaxLevels = 64;           // levels a tree can hold: 62 by the keys

RRT_BB_HD uint32_t morton_cell(double c, double cmin, double cmax) {
    const double scale = (double)kCells / (cmax - cmin);
    const double x = (c - cmin) * scale;
    if (!(x < (double)kCells)) return kCells - 1u;  // also a NaN x
    return x > 0.0 ? (uint32_t)x : 0u;
}
RRT_BB_HD uint32_t spread10(uint32_t v) {  // bit b of v to bit 3 b
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// usable: bit a set when axis a takes cells (usable_axes over the centroid bounds).
RRT_BB_HD uint32_t usable_axes(const Bounds &b) {
    uint32_t u = 0;
    for (int a = 0; a < 3; ++a)
        if (axis_usable(key_f64(b.k[6 + a]), key_f64(b.k[9 + a]))) u |= 1u << a;
    return u;
}
RRT_BB_HD uint32_t morton_code(const Box6 &box, const Bounds &b, uint32_t usable) {
    uint32_t cell[3];
    for (int a = 0; a < 3; ++a)
        cell[a] = ((usable >> a) & 1u) ? morton_cell(centroid(box, a), key_f64(b.k[6 + a]), key_f64(b.k[9 + a])) : 0u;
    return (spread10(cell[0]) << 2) | (spread10(cell[1]) << 1) | spread10(cell[2]);
}
RRT_BB_HD uint64_t sort_key(uint32_t code, uint32_t position) { return ((uint64_t)code << 32) | position; }

RRT_BB_HD int clz64(uint64_t x) { return __builtin_clzll(x); }  // x != 0; a compiler builtin on both sides
// Common-prefix length of keys i and j; -1 when j lies outside [0, n).
RRT_BB_HD int delta(const uint64_t *keys, uint32_t n, uint32_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)n) return -1;
    const uint64_t x = keys[i] ^ keys[j];
    return x ? clz64(x) : 64;  // unique keys: x != 0 for j != i
}

struct KNode {
    uint32_t first, last;  // positions, inclusive
    uint32_t child[2];     // an internal node's index, or kLeafChild | position
};
RRT_BB_HD KNode karras_node(const uint64_t *keys, uint32_t n, uint32_t i) {
    const int d = delta(keys, n, i, (int64_t)i + 1) > delta(keys, n, i, (int64_t)i - 1) ? 1 : -1;
    const int dmin = delta(keys, n, i, (int64_t)i - d);
    uint32_t lmax = 2;
    while (delta(keys, n, i, (int64_t)i + (int64_t)lmax * d) > dmin) lmax <<= 1;
    uint32_t l = 0;
    for (uint32_t t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, n, i, (int64_t)i + (int64_t)(l + t) * d) > dmin) l += t;
    const int64_t j = (int64_t)i + (int64_t)l * d;
    const int dnode = delta(keys, n, i, j);
    uint32_t s = 0;
    for (uint32_t div = 2;; div <<= 1) {
        const uint32_t t = (l + div - 1u) / div;  // ceil(l / div)
        if (delta(keys, n, i, (int64_t)i + (int64_t)(s + t) * d) > dnode) s += t;
        if (t <= 1u) break;
    }
    const int64_t split = (int64_t)i + (int64_t)s * d + (d < 0 ? -1 : 0);
    KNode k;
    k.first = (uint32_t)(d > 0 ? (int64_t)i : j);
    k.last = (uint32_t)(d > 0 ? j : (int64_t)i);
    k.child[0] = (uint32_t)split == k.first ? (kLeafChild | (uint32_t)split) : (uint32_t)split;
    k.child[1] = (uint32_t)split + 1u == k.last ? (kLeafChild | ((uint32_t)split + 1u)) : (uint32_t)split + 1u;
    return k;
}

RRT_BB_HD uint64_t number_key(uint32_t level, uint32_t first, uint32_t i) {
    return ((uint64_t)level << 56) | ((uint64_t)first << 28) | i;
}
constexpr uint32_t kNumberIndexMask = (1u << 28) - 1u;

// The link of child c of a kept node under leaf size m: ids[j] = the number of kept node j.
RRT_BB_HD uint32_t child_link(uint32_t child, const uint32_t *first, const uint32_t *last, const uint32_t *ids, uint32_t m) {
    if (child & kLeafChild) return (child & ~kLeafChild) | (1u << kLeafShift);
    const uint32_t count = last[child] - first[child] + 1u;
    return count <= m ? (first[child] | (count << kLeafShift)) : ids[child];
}
// The largest leaf that child makes under leaf size m (0: the child is a kept node).
RRT_BB_HD uint32_t child_leaf_count(uint32_t child, const uint32_t *first, const uint32_t *last, uint32_t m) {
    if (child & kLeafChild) return 1u;
    const uint32_t count = last[child] - first[child] + 1u;
    return count <= m ? count : 0u;
}

}  // namespace lbvh
}  // namespace rrt
