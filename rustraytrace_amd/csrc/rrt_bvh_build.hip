// rrt_bvh_build.hip — the scene's BVH built on the device (RRT_FLAG_DEVICE_BVH): the binned SAH
// builder of rrt_bvh_binned.h, level-synchronous and top-down. Every floating-point decision is the
// header's; this file only moves data: it fills the header's Bin records with integer atomics (adds
// for counts, 64-bit min / max on the order-preserving keys of the f64 bits), runs the header's
// decide() one lane per task, numbers nodes and next-level tasks by exclusive scans over the level's
// tasks, and partitions stably by a prefix sum of the "goes left" flags. The kernel boundary is the
// only synchronisation between workgroups: no spin waits, no look-back, no cooperative launch. The
// host reads one small LevelState per level (the next level's task count) with a blocking copy.
//
// Per level: bins_init, bin, decide, scan (one block), emit, flags (reduce), scan (one block),
// scatter. After the last level pack writes GNode / GNodeH records from the raw f64 nodes.
// Tasks of a level are ordered left to right by position, so the flags' prefix at a task's start
// is the exclusive scan of the tasks' left counts, and node ids come out breadth-first.
//
// The same builder object also holds the fast builder (RRT_FLAG_FAST_BVH): the LBVH of rrt_bvh_lbvh.h
// over the same boxes and tree storage, in a launch count that does not depend on the depth and with
// one blocking read per build (lbvh_build / lbvh_finish, further down).
#include "rrt_bvh_binned.h"
#include "rrt_bvh_lbvh.h"
#include "rrt_internal.h"

#include <rocprim/device/device_radix_sort.hpp>  // the fast builder's sort of 64-bit keys, nothing else

#include <algorithm>
#include <atomic>
#include <vector>

namespace rrt {

using namespace bvhb;

namespace {

constexpr int kBlk = 256;
constexpr int kScanBlk = 1024;
// Trees of at most this many nodes refit in one workgroup (k_refit_small); larger ones take one
// launch per level. Measured on MI355X: the single workgroup wins up to 16,384 nodes
// (0.180 against 0.197 ms for the whole refit) and loses at 32,402 (0.337 against 0.318 ms).
constexpr uint32_t kRefitSmallMaxNodes = 16384;
constexpr uint32_t kBinWords = 13;                       // u64 words of a Bin: n, k[12]
constexpr uint32_t kTaskWords = 3 * kBins * kBinWords;   // of a task's bins
static_assert(sizeof(Bin) == kBinWords * 8, "Bin is 13 packed u64");
static_assert(sizeof(Task) == 112 && sizeof(RawNode) == 112, "layouts");
static_assert(kLeafShift == kLinkCountShift, "leaf link encoding");

struct LevelState {
    uint32_t n_next;     // tasks of the next level
    uint32_t n_nodes;    // internal nodes so far
    uint32_t node_base;  // n_nodes before this level
    uint32_t n_split;    // tasks of this level that split
    uint32_t n_leaves;
    uint32_t max_leaf;
    uint32_t error;      // a scatter destination left its task's range (never expected)
    uint32_t _pad;
};

typedef unsigned long long u64;

__device__ __forceinline__ u64 word_identity(uint32_t w) {  // w = word of a Bin
    return w == 0 ? 0ull : (key_is_min((int)w - 1) ? kKeyPosInf : kKeyNegInf);
}
// Folds one primitive into a task's bins (words: LDS or global, kTaskWords of them).
__device__ __forceinline__ void bin_prim(u64 *words, const Task &t, uint32_t i, const Box6 &box) {
    const Bounds bo = bounds_of(box);
    for (int axis = 0; axis < 3; ++axis) {
        const int b = task_bin(t, axis, i, box);
        if (b < 0) continue;
        u64 *w = words + (uint32_t)(axis * kBins + b) * kBinWords;
        atomicAdd(w, 1ull);
        for (int j = 0; j < 12; ++j) {
            if (key_is_min(j)) atomicMin(w + 1 + j, (u64)bo.k[j]);
            else atomicMax(w + 1 + j, (u64)bo.k[j]);
        }
    }
}

// The root task's bounds: LDS reduction per block, then 12 atomics per block.
__global__ __launch_bounds__(kBlk) void k_root_bounds(uint32_t n, const uint32_t *order, const Box6 *boxes, Task *root) {
    __shared__ u64 s[12];
    if (threadIdx.x < 12) s[threadIdx.x] = key_is_min((int)threadIdx.x) ? kKeyPosInf : kKeyNegInf;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i < n) {
        const Bounds bo = bounds_of(boxes[order[i]]);
        for (int j = 0; j < 12; ++j) {
            if (key_is_min(j)) atomicMin(&s[j], (u64)bo.k[j]);
            else atomicMax(&s[j], (u64)bo.k[j]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        u64 *dst = (u64 *)&root->b.k[threadIdx.x];
        if (key_is_min((int)threadIdx.x)) atomicMin(dst, s[threadIdx.x]);
        else atomicMax(dst, s[threadIdx.x]);
    }
}
__global__ void k_root_finish(Task *root) { task_finish(*root); }

__global__ __launch_bounds__(kBlk) void k_bins_init(uint64_t n_words, u64 *words) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < n_words) words[i] = word_identity((uint32_t)(i % kBinWords));
}

// Each primitive of a live task bins into its task. A block whose 256 positions lie in one task
// (every block of the top levels) reduces in LDS first and issues one atomic per touched bin word.
__global__ __launch_bounds__(kBlk) void k_bin(uint32_t n, const uint32_t *order, const int32_t *ptask, const Task *tasks,
                                              const Box6 *boxes, Bin *bins) {
    __shared__ u64 s[kTaskWords];
    const uint32_t i0 = blockIdx.x * kBlk;
    if (i0 >= n) return;
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t last = min(i0 + (uint32_t)kBlk - 1u, n - 1u);
    const int32_t tf = ptask[i0];
    const bool uniform = tf >= 0 && tf == ptask[last];  // tasks are contiguous ranges
    if (uniform) {
        for (uint32_t w = threadIdx.x; w < kTaskWords; w += kBlk) s[w] = word_identity(w % kBinWords);
        __syncthreads();
        if (i <= last) bin_prim(s, tasks[tf], i, boxes[order[i]]);
        __syncthreads();
        u64 *g = (u64 *)(bins + (size_t)tf * (3 * kBins));
        for (uint32_t w = threadIdx.x; w < kTaskWords; w += kBlk) {
            const uint32_t k = w % kBinWords;
            const u64 v = s[w];
            if (v == word_identity(k)) continue;
            if (k == 0) atomicAdd(g + w, v);
            else if (key_is_min((int)k - 1)) atomicMin(g + w, v);
            else atomicMax(g + w, v);
        }
        return;
    }
    if (i > last) return;
    const int32_t t = ptask[i];
    if (t < 0) return;
    bin_prim((u64 *)(bins + (size_t)t * (3 * kBins)), tasks[t], i, boxes[order[i]]);
}

// One lane per task: the header's decide(), and the three scan inputs.
__global__ __launch_bounds__(64) void k_decide(uint32_t n_tasks, const Task *tasks, const Bin *bins, uint32_t max_leaf,
                                               double node_cost, Decision *dec, uint32_t *s_node, uint32_t *s_child,
                                               uint32_t *s_left) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n_tasks) return;
    const Task tk = tasks[t];
    const Decision d = decide(tk, bins + (size_t)t * (3 * kBins), max_leaf, node_cost);
    dec[t] = d;
    const uint32_t span = tk.hi - tk.lo;
    s_node[t] = d.split;
    s_child[t] = d.split ? (d.n_left > 1u ? 1u : 0u) + (span - d.n_left > 1u ? 1u : 0u) : 0u;
    s_left[t] = d.split ? d.n_left : 0u;
}

// Exclusive scan, in place, of up to three arrays of n entries by one block; totals[c] = the sum
// of array c.
__global__ __launch_bounds__(kScanBlk) void k_excl_scan(uint32_t n, uint32_t *a0, uint32_t *a1, uint32_t *a2,
                                                        uint32_t *totals) {
    __shared__ uint32_t s[3][kScanBlk];
    uint32_t *a[3] = {a0, a1, a2};
    uint32_t carry[3] = {0u, 0u, 0u};
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < n; base += kScanBlk) {
        const uint32_t i = base + tid;
        uint32_t own[3];
        for (int c = 0; c < 3; ++c) {
            own[c] = (a[c] && i < n) ? a[c][i] : 0u;
            s[c][tid] = own[c];
        }
        __syncthreads();
        for (uint32_t off = 1; off < (uint32_t)kScanBlk; off <<= 1) {
            uint32_t v[3];
            for (int c = 0; c < 3; ++c) v[c] = tid >= off ? s[c][tid - off] : 0u;
            __syncthreads();
            for (int c = 0; c < 3; ++c) s[c][tid] += v[c];
            __syncthreads();
        }
        for (int c = 0; c < 3; ++c) {
            if (a[c] && i < n) a[c][i] = carry[c] + s[c][tid] - own[c];
            carry[c] += s[c][kScanBlk - 1];
        }
        __syncthreads();
    }
    if (tid == 0)
        for (int c = 0; c < 3; ++c) totals[c] = carry[c];
}

// After the task scan: the level's totals into the state (one thread).
__global__ void k_level_totals(const uint32_t *totals, LevelState *st) {
    st->node_base = st->n_nodes;
    st->n_split = totals[0];
    st->n_nodes += totals[0];
    st->n_next = totals[1];
}

// One lane per task: the task's link in its parent, its raw node, its leaf children and the next
// level's tasks.
__global__ __launch_bounds__(64) void k_emit(uint32_t n_tasks, const Task *tasks, const Decision *dec, const uint32_t *s_node,
                                             const uint32_t *s_child, LevelState *st, RawNode *raw, uint32_t raw_cap,
                                             Task *next, uint32_t next_cap) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n_tasks) return;
    const Task tk = tasks[t];
    const uint32_t span = tk.hi - tk.lo;
    const bool split = dec[t].split != 0;
    if (!split) {
        const uint32_t link = tk.lo | (span << kLeafShift);
        if (tk.slot == kNoSlot) {  // the root is a leaf: child 0 = the leaf, child 1 never hit
            RawNode r;
            for (int a = 0; a < 3; ++a) {
                r.box[0][a] = key_f64(tk.b.k[a]);
                r.box[0][3 + a] = key_f64(tk.b.k[3 + a]);
            }
            never_hit(r.box[1]);
            r.link[0] = link;
            r.link[1] = 0u;
            r._pad[0] = r._pad[1] = 0u;
            raw[0] = r;
            st->n_nodes = 1u;
        } else if ((tk.slot >> 1) < raw_cap) {
            raw[tk.slot >> 1].link[tk.slot & 1u] = link;
        }
        atomicAdd(&st->n_leaves, 1u);
        atomicMax(&st->max_leaf, span);
        return;
    }
    const uint32_t id = st->node_base + s_node[t];
    if (id >= raw_cap) {
        atomicOr(&st->error, 2u);
        return;
    }
    const Decision &d = dec[t];
    for (int c = 0; c < 2; ++c)
        for (int a = 0; a < 3; ++a) {
            raw[id].box[c][a] = key_f64(d.child[c].k[a]);
            raw[id].box[c][3 + a] = key_f64(d.child[c].k[3 + a]);
        }
    raw[id]._pad[0] = raw[id]._pad[1] = 0u;
    if (tk.slot != kNoSlot && (tk.slot >> 1) < raw_cap) raw[tk.slot >> 1].link[tk.slot & 1u] = id;
    uint32_t ci = s_child[t];
    const uint32_t first[2] = {tk.lo, tk.lo + d.n_left}, count[2] = {d.n_left, span - d.n_left};
    for (int c = 0; c < 2; ++c) {
        if (count[c] <= 1u) {
            raw[id].link[c] = first[c] | (count[c] << kLeafShift);
            atomicAdd(&st->n_leaves, 1u);
            atomicMax(&st->max_leaf, count[c]);
            continue;
        }
        raw[id].link[c] = 0u;  // set by the child's own level
        if (ci >= next_cap) {
            atomicOr(&st->error, 4u);
            continue;
        }
        Task nt;
        nt.lo = first[c];
        nt.hi = first[c] + count[c];
        nt.slot = 2u * id + (uint32_t)c;
        nt.b = d.child[c];
        task_finish(nt);
        next[ci++] = nt;
    }
}

__device__ __forceinline__ bool left_flag(uint32_t i, const uint32_t *order, const int32_t *ptask, const Task *tasks,
                                          const Decision *dec, const Box6 *boxes) {
    const int32_t t = ptask[i];
    if (t < 0 || !dec[t].split) return false;
    return goes_left(tasks[t], dec[t], i, boxes[order[i]]);
}

// Partition pass 1: the flags and their count per block of 256 positions.
__global__ __launch_bounds__(kBlk) void k_flags(uint32_t n, const uint32_t *order, const int32_t *ptask, const Task *tasks,
                                                const Decision *dec, const Box6 *boxes, uint8_t *flag, uint32_t *block_sum) {
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    const bool f = i < n && left_flag(i, order, ptask, tasks, dec, boxes);
    if (i < n) flag[i] = f ? 1u : 0u;
    const int c = __syncthreads_count(f ? 1 : 0);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = (uint32_t)c;
}

// Partition pass 3 (pass 2 is k_excl_scan over block_sum): each position's stable destination.
// F = flags before position i; inside a split task [lo, hi) with n_left lefts, rel = F - F(lo):
// a left goes to lo + rel, a right to lo + n_left + (i - lo - rel).
__global__ __launch_bounds__(kBlk) void k_scatter(uint32_t n, const uint32_t *order, const int32_t *ptask, const Task *tasks,
                                                  const Decision *dec, const uint32_t *s_child, const uint32_t *s_left,
                                                  const uint8_t *flag, const uint32_t *block_off, uint32_t *order_out,
                                                  int32_t *ptask_out, LevelState *st) {
    __shared__ uint32_t s[kBlk];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kBlk + tid;
    const uint32_t f = i < n ? flag[i] : 0u;
    s[tid] = f;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t)kBlk; off <<= 1) {
        const uint32_t v = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    if (i >= n) return;
    const uint32_t F = block_off[blockIdx.x] + s[tid] - f;
    const int32_t t = ptask[i];
    if (t < 0 || !dec[t].split) {  // outside the level's tasks, or in a task that became a leaf
        order_out[i] = order[i];
        ptask_out[i] = -1;
        return;
    }
    const uint32_t lo = tasks[t].lo, hi = tasks[t].hi, n_left = dec[t].n_left;
    const uint32_t rel = F - s_left[t];
    const uint32_t dest = f ? lo + rel : lo + n_left + (i - lo - rel);
    if (dest < lo || dest >= hi || dest >= n) {
        atomicOr(&st->error, 1u);
        return;
    }
    const uint32_t ci = s_child[t];
    const bool task0 = n_left > 1u, task1 = hi - lo - n_left > 1u;
    order_out[dest] = order[i];
    ptask_out[dest] = f ? (task0 ? (int32_t)ci : -1) : (task1 ? (int32_t)(ci + (task0 ? 1u : 0u)) : -1);
}

__global__ __launch_bounds__(kBlk) void k_pack(uint32_t n_nodes, const RawNode *raw, Slack slack, uint32_t stride,
                                               uint32_t *out) {
    const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
    if (k >= n_nodes) return;
    uint32_t w[20];
    pack_node(raw[k], slack, stride, w);
    const uint32_t words = stride / 4u;
    for (uint32_t j = 0; j < words; ++j) out[(size_t)k * words + j] = w[j];
}

// k_pack with the slack read from device memory (the refit never brings the root box to the host).
__global__ __launch_bounds__(kBlk) void k_pack_dev(uint32_t n_nodes, const RawNode *raw, const Slack *slack, uint32_t stride,
                                                   uint32_t *out) {
    const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
    if (k >= n_nodes) return;
    uint32_t w[20];
    pack_node(raw[k], *slack, stride, w);
    const uint32_t words = stride / 4u;
    for (uint32_t j = 0; j < words; ++j) out[(size_t)k * words + j] = w[j];
}

// ---- refit: the header's refit_child, one lane per (node, child) -------------------------------
// A link the build wrote stays inside the tree; a lane that finds another one (never expected) leaves
// its box alone instead of reading outside the arrays.
__device__ __forceinline__ void refit_lane(RawNode *raw, uint32_t n_nodes, uint32_t n_tree, uint32_t k, int c,
                                           const uint32_t *order, const Box6 *boxes) {
    const uint32_t link = raw[k].link[c];
    if (link_is_leaf(link)) {
        const uint32_t first = link & ((1u << kLeafShift) - 1u), count = link >> kLeafShift;
        if (first + count > n_tree) return;
    } else if (link <= k || link >= n_nodes) {
        return;  // 0: the never-hit slot
    }
    refit_child(raw, k, c, order, boxes);
}

// The per-level form: the nodes [base, end) of one level. The level below is complete (the kernel
// boundary on the stream), and lanes of one level write disjoint boxes and read none of their level.
__global__ __launch_bounds__(kBlk) void k_refit_level(uint32_t base, uint32_t end, RawNode *raw, uint32_t n_nodes,
                                                      uint32_t n_tree, const uint32_t *order, const Box6 *boxes) {
    const uint32_t lane = blockIdx.x * kBlk + threadIdx.x;
    const uint32_t k = base + (lane >> 1);
    if (k >= end) return;
    refit_lane(raw, n_nodes, n_tree, k, (int)(lane & 1u), order, boxes);
}

__device__ __forceinline__ void write_slack(const RawNode *raw, Slack *slack) {
    double rb[6];
    root_box_of(raw[0], rb);
    *slack = slack_of(rb);
}
__global__ void k_refit_slack(const RawNode *raw, Slack *slack) { write_slack(raw, slack); }

// The single-workgroup form: every level in one launch, deepest first, a barrier between levels (one
// workgroup's global stores are visible to its own waves after __syncthreads), then the slack.
__global__ __launch_bounds__(kScanBlk) void k_refit_small(uint32_t n_levels, const uint32_t *level_base, RawNode *raw,
                                                          uint32_t n_nodes, uint32_t n_tree, const uint32_t *order,
                                                          const Box6 *boxes, Slack *slack) {
    for (uint32_t l = n_levels; l-- > 0;) {
        const uint32_t base = level_base[l], end = level_base[l + 1u];
        for (uint32_t lane = threadIdx.x; lane < 2u * (end - base); lane += kScanBlk)
            refit_lane(raw, n_nodes, n_tree, base + (lane >> 1), (int)(lane & 1u), order, boxes);
        __syncthreads();
    }
    if (threadIdx.x == 0) write_slack(raw, slack);
}

// The SAH terms (rrt_scene_tree_cost): one lane per node.
__global__ __launch_bounds__(kBlk) void k_sah_terms(uint32_t n_nodes, const RawNode *raw, double node_cost, double *terms,
                                                    RawNode *root_out) {
    const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
    if (k >= n_nodes) return;
    terms[k] = sah_term(raw[k], node_cost);
    if (k == 0) *root_out = raw[0];
}

// ---- the fast builder (RRT_FLAG_FAST_BVH): rrt_bvh_lbvh.h, one lane per primitive or per node ----
// Phases: centroid bounds, keys, sort, Karras' nodes with parent links, levels and the per-level node
// counts of both candidate shapes, a sort of the numbering keys, then (one blocking read later, for
// the shape the host keeps) numbers, links and the level table, and the binned builder's level-ordered
// refit for the boxes. Every phase is a device function taking one element, called by a kernel per
// phase (any size; the sorts are rocPRIM's) or, for small trees, by one workgroup that loops over the
// elements with __syncthreads() between phases and sorts in LDS. Out-of-range values set an error
// bit instead of an address.
using namespace lbvh;

constexpr uint32_t kLbvhSmallMax = 2048;  // primitives the single workgroup takes (its LDS sort buffer)
enum : uint32_t { kLbvhErrLevel = 1u, kLbvhErrChild = 2u, kLbvhErrId = 4u };

struct LbvhState {  // read once per build
    uint32_t error;
    uint32_t finished;              // the shape the single workgroup finished in its launch
    uint32_t max_leaf[2];           // per shape: the largest leaf
    uint32_t hist[2][kMaxLevels];   // per shape: kept nodes per level
    Bounds b;
};

struct LbvhArgs {
    uint32_t n, cap;       // primitives of the tree; rows every array holds
    uint32_t leaf[2];      // the two shapes' leaf sizes
    const Box6 *boxes;
    const uint32_t *objs;  // the tree's primitives, source order
    uint64_t *keys[2];     // [0] unsorted, [1] sorted (n)
    uint64_t *nkeys[2];    // numbering keys, [0] unsorted, [1] sorted (n - 1)
    uint32_t *first, *last, *child, *parent, *ids, *scan;  // per Karras node (child: 2 each)
    uint32_t *order;
    RawNode *raw;
    uint32_t *level_base;
    LbvhState *st;
};

__device__ __forceinline__ void lbvh_state_init(LbvhState *st, uint32_t t) {  // t < 128
    st->hist[t >> 6][t & 63u] = 0u;
    if (t < 12) st->b.k[t] = key_is_min((int)t) ? kKeyPosInf : kKeyNegInf;
    if (t == 0) st->error = 0u, st->finished = 0u;
    if (t < 2) st->max_leaf[t] = 1u;
}
__device__ __forceinline__ void lbvh_key(const LbvhArgs &a, const Bounds &b, uint32_t usable, uint32_t i, uint64_t *keys) {
    keys[i] = sort_key(morton_code(a.boxes[a.objs[i]], b, usable), i);
}
// Position i's primitive and, for i < n - 1, Karras node i over the sorted keys.
__device__ __forceinline__ void lbvh_topology(const LbvhArgs &a, const uint64_t *keys, uint32_t i) {
    a.order[i] = a.objs[(uint32_t)keys[i] < a.n ? (uint32_t)keys[i] : 0u];
    if (i + 1u >= a.n) return;
    const KNode k = karras_node(keys, a.n, i);
    a.first[i] = k.first;
    a.last[i] = k.last;
    if (i == 0) a.parent[0] = kNoParent;
    for (int c = 0; c < 2; ++c) {
        uint32_t ch = k.child[c];
        const uint32_t limit = (ch & kLeafChild) ? a.n : a.n - 1u;
        if ((ch & ~kLeafChild) >= limit || ch == 0u) {  // never expected: keep every later index in range
            atomicOr(&a.st->error, kLbvhErrChild);
            ch = kLeafChild;
        }
        a.child[2u * i + (uint32_t)c] = ch;
        if (!(ch & kLeafChild)) a.parent[ch] = i;
    }
}
// Node i's level and numbering key; hist / max_leaf: the block's LDS counters ([2][kMaxLevels], [2]).
__device__ __forceinline__ void lbvh_level(const LbvhArgs &a, uint32_t i, uint64_t *nkeys, uint32_t *hist, uint32_t *max_leaf) {
    uint32_t level = 0;
    for (uint32_t p = a.parent[i]; p != kNoParent && level < kMaxLevels; p = p < a.n - 1u ? a.parent[p] : kNoParent) ++level;
    if (level >= kMaxLevels) {
        atomicOr(&a.st->error, kLbvhErrLevel);
        level = kMaxLevels - 1u;
    }
    nkeys[i] = number_key(level, a.first[i], i);
    const uint32_t count = a.last[i] - a.first[i] + 1u;
    for (int s = 0; s < 2; ++s) {
        if (count <= a.leaf[s]) continue;
        atomicAdd(&hist[s * kMaxLevels + level], 1u);
        for (int c = 0; c < 2; ++c) {
            const uint32_t lc = child_leaf_count(a.child[2u * i + (uint32_t)c], a.first, a.last, a.leaf[s]);
            if (lc > 1u) atomicMax(&max_leaf[s], lc);
        }
    }
}
__device__ __forceinline__ bool lbvh_kept(const LbvhArgs &a, uint32_t m, uint32_t s, uint32_t &i) {
    i = (uint32_t)a.nkeys[1][s] & kNumberIndexMask;
    if (i >= a.n - 1u) {
        i = 0;
        return false;
    }
    return a.last[i] - a.first[i] + 1u > m;
}
// The node at sorted position s: its number (scan: the exclusive scan of the kept flags, or null when
// every node is kept).
__device__ __forceinline__ void lbvh_id(const LbvhArgs &a, uint32_t m, const uint32_t *scan, uint32_t s) {
    uint32_t i;
    if (lbvh_kept(a, m, s, i)) a.ids[i] = scan ? scan[s] : s;
}
__device__ __forceinline__ void lbvh_links(const LbvhArgs &a, uint32_t m, uint32_t s) {
    uint32_t i;
    if (!lbvh_kept(a, m, s, i)) return;
    const uint32_t id = a.ids[i];
    if (id >= a.cap) {
        atomicOr(&a.st->error, kLbvhErrId);
        return;
    }
    for (int c = 0; c < 2; ++c) a.raw[id].link[c] = child_link(a.child[2u * i + (uint32_t)c], a.first, a.last, a.ids, m);
    a.raw[id]._pad[0] = a.raw[id]._pad[1] = 0u;
}
// One thread: the level table of shape `shape` (the first node of every level, then the node count)
// and, for a root that fits a leaf, the root-leaf form. Returns the levels.
__device__ __forceinline__ uint32_t lbvh_level_table(const LbvhArgs &a, int shape) {
    if (a.n <= a.leaf[shape]) {
        RawNode &r = a.raw[0];
        never_hit(r.box[0]);
        never_hit(r.box[1]);
        r.link[0] = a.n << kLeafShift;
        r.link[1] = 0u;
        r._pad[0] = r._pad[1] = 0u;
        a.level_base[0] = 0u;
        a.level_base[1] = 1u;
        return 1u;
    }
    uint32_t base = 0, l = 0;
    for (; l < kMaxLevels && a.st->hist[shape][l] != 0u; ++l) {
        a.level_base[l] = base;
        base += a.st->hist[shape][l];
    }
    a.level_base[l] = base;
    return l;
}

__global__ __launch_bounds__(128) void k_lbvh_init(LbvhState *st) { lbvh_state_init(st, threadIdx.x); }
__global__ __launch_bounds__(kBlk) void k_lbvh_bounds(LbvhArgs a) {
    __shared__ u64 s[12];
    if (threadIdx.x < 12) s[threadIdx.x] = key_is_min((int)threadIdx.x) ? kKeyPosInf : kKeyNegInf;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i < a.n) {
        const Bounds bo = bounds_of(a.boxes[a.objs[i]]);
        for (int j = 6; j < 12; ++j) {
            if (key_is_min(j)) atomicMin(&s[j], (u64)bo.k[j]);
            else atomicMax(&s[j], (u64)bo.k[j]);
        }
    }
    __syncthreads();
    if (threadIdx.x >= 6 && threadIdx.x < 12) {
        u64 *dst = (u64 *)&a.st->b.k[threadIdx.x];
        if (key_is_min((int)threadIdx.x)) atomicMin(dst, s[threadIdx.x]);
        else atomicMax(dst, s[threadIdx.x]);
    }
}
__global__ __launch_bounds__(kBlk) void k_lbvh_keys(LbvhArgs a) {
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i >= a.n) return;
    const Bounds b = a.st->b;
    lbvh_key(a, b, usable_axes(b), i, a.keys[0]);
}
__global__ __launch_bounds__(kBlk) void k_lbvh_topology(LbvhArgs a) {
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i < a.n) lbvh_topology(a, a.keys[1], i);
}
__global__ __launch_bounds__(kBlk) void k_lbvh_levels(LbvhArgs a) {
    __shared__ uint32_t hist[2 * kMaxLevels], max_leaf[2];
    if (threadIdx.x < 2 * kMaxLevels) hist[threadIdx.x] = 0u;
    if (threadIdx.x < 2) max_leaf[threadIdx.x] = 1u;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlk + threadIdx.x;
    if (i + 1u < a.n) lbvh_level(a, i, a.nkeys[0], hist, max_leaf);
    __syncthreads();
    if (threadIdx.x < 2 * kMaxLevels && hist[threadIdx.x]) atomicAdd(&a.st->hist[threadIdx.x >> 6][threadIdx.x & 63u], hist[threadIdx.x]);
    if (threadIdx.x < 2 && max_leaf[threadIdx.x] > 1u) atomicMax(&a.st->max_leaf[threadIdx.x], max_leaf[threadIdx.x]);
}
__global__ __launch_bounds__(kBlk) void k_lbvh_flags(LbvhArgs a, uint32_t m) {
    const uint32_t s = blockIdx.x * kBlk + threadIdx.x;
    uint32_t i;
    if (s + 1u < a.n) a.scan[s] = lbvh_kept(a, m, s, i) ? 1u : 0u;
}
__global__ __launch_bounds__(kBlk) void k_lbvh_ids(LbvhArgs a, uint32_t m, uint32_t scanned) {
    const uint32_t s = blockIdx.x * kBlk + threadIdx.x;
    if (s + 1u < a.n) lbvh_id(a, m, scanned ? a.scan : nullptr, s);
}
__global__ __launch_bounds__(kBlk) void k_lbvh_links(LbvhArgs a, int shape) {
    const uint32_t s = blockIdx.x * kBlk + threadIdx.x;
    if (s + 1u < a.n) lbvh_links(a, a.leaf[shape], s);
    if (s == 0) (void)lbvh_level_table(a, shape);
}

// The single workgroup's sort: bitonic over p keys in LDS (p a power of two, padded with ~0).
__device__ __forceinline__ void lbvh_lds_sort(uint64_t *s, uint32_t p) {
    for (uint32_t k = 2; k <= p; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < p / 2u; t += kScanBlk) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
                const uint64_t x = s[i], y = s[l];
                if ((x > y) == ((i & k) == 0u)) s[i] = y, s[l] = x;
            }
            __syncthreads();
        }
}
// k_excl_scan's scan by the calling workgroup, in place over a[0, n).
__device__ __forceinline__ void lbvh_block_scan(uint32_t n, uint32_t *a, uint32_t *s /* kScanBlk */) {
    uint32_t carry = 0;
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < n; base += kScanBlk) {
        const uint32_t i = base + tid;
        const uint32_t own = i < n ? a[i] : 0u;
        s[tid] = own;
        __syncthreads();
        for (uint32_t off = 1; off < (uint32_t)kScanBlk; off <<= 1) {
            const uint32_t v = tid >= off ? s[tid - off] : 0u;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        if (i < n) a[i] = carry + s[tid] - own;
        carry += s[kScanBlk - 1];
        __syncthreads();
    }
}

// The single-workgroup form, n <= kLbvhSmallMax. front: every phase up to the sorted numbering keys
// and the state; then one shape is finished: numbers, links, level table, boxes (k_refit_small's
// loop), slack. Which: shape 0 when its node count is at most fit_nodes (the host's prediction of its
// own choice: the count up to which the LDS shape fits), else shape 1. front = 0 finishes `shape` of
// the same build (the host kept the other one after all).
__global__ __launch_bounds__(kScanBlk) void k_lbvh_small(LbvhArgs a, uint32_t front, int shape, uint32_t fit_nodes,
                                                         uint32_t p /* pow2 >= n */, Slack *slack) {
    __shared__ uint64_t s_keys[kLbvhSmallMax];
    __shared__ u64 s_b[12];
    __shared__ uint32_t s_hist[2 * kMaxLevels], s_max[2], s_scan[kScanBlk], s_levels;
    const uint32_t tid = threadIdx.x, n = a.n, nk = a.n - 1u;
    if (n < 2u || n > kLbvhSmallMax || p > kLbvhSmallMax || p < n) return;
    if (front) {
        if (tid < 128) lbvh_state_init(a.st, tid);
        if (tid < 2 * kMaxLevels) s_hist[tid] = 0u;
        if (tid < 2) s_max[tid] = 1u;
        if (tid < 12) s_b[tid] = key_is_min((int)tid) ? kKeyPosInf : kKeyNegInf;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kScanBlk) {
            const Bounds bo = bounds_of(a.boxes[a.objs[i]]);
            for (int j = 6; j < 12; ++j) {
                if (key_is_min(j)) atomicMin(&s_b[j], (u64)bo.k[j]);
                else atomicMax(&s_b[j], (u64)bo.k[j]);
            }
        }
        __syncthreads();
        Bounds b;
        for (int j = 0; j < 12; ++j) b.k[j] = s_b[j];
        const uint32_t usable = usable_axes(b);
        for (uint32_t i = tid; i < p; i += kScanBlk) {
            if (i < n) lbvh_key(a, b, usable, i, s_keys);
            else s_keys[i] = ~0ull;
        }
        __syncthreads();
        lbvh_lds_sort(s_keys, p);
        for (uint32_t i = tid; i < n; i += kScanBlk) lbvh_topology(a, s_keys, i);
        __syncthreads();
        for (uint32_t i = tid; i < p; i += kScanBlk) {
            if (i < nk) lbvh_level(a, i, s_keys, s_hist, s_max);
            else s_keys[i] = ~0ull;
        }
        __syncthreads();
        lbvh_lds_sort(s_keys, p);
        for (uint32_t i = tid; i < nk; i += kScanBlk) a.nkeys[1][i] = s_keys[i];
        if (tid < 2 * kMaxLevels) a.st->hist[tid >> 6][tid & 63u] = s_hist[tid];
        if (tid < 2) a.st->max_leaf[tid] = s_max[tid];
        if (tid < 12) a.st->b.k[tid] = s_b[tid];
        __syncthreads();
        uint32_t nodes0 = 0;
        for (uint32_t l = 0; l < kMaxLevels; ++l) nodes0 += s_hist[l];
        if (n <= a.leaf[0]) nodes0 = 1u;
        shape = nodes0 <= fit_nodes ? 0 : 1;
        if (tid == 0) a.st->finished = (uint32_t)shape;
    }
    const uint32_t m = a.leaf[shape];
    const bool scanned = m > 1u;
    if (scanned) {
        uint32_t i;
        for (uint32_t s = tid; s < nk; s += kScanBlk) a.scan[s] = lbvh_kept(a, m, s, i) ? 1u : 0u;
        __syncthreads();
        lbvh_block_scan(nk, a.scan, s_scan);
    }
    for (uint32_t s = tid; s < nk; s += kScanBlk) lbvh_id(a, m, scanned ? a.scan : nullptr, s);
    __syncthreads();
    for (uint32_t s = tid; s < nk; s += kScanBlk) lbvh_links(a, m, s);
    if (tid == 0) s_levels = lbvh_level_table(a, shape);
    __syncthreads();
    const uint32_t n_levels = s_levels, n_nodes = a.level_base[n_levels];
    if (n_nodes > a.cap) return;
    for (uint32_t l = n_levels; l-- > 0;) {
        const uint32_t base = a.level_base[l], end = a.level_base[l + 1u];
        for (uint32_t lane = tid; lane < 2u * (end - base); lane += kScanBlk)
            refit_lane(a.raw, n_nodes, n, base + (lane >> 1), (int)(lane & 1u), a.order, a.boxes);
        __syncthreads();
    }
    if (tid == 0) write_slack(a.raw, slack);
}

uint32_t blocks_of(uint32_t n, uint32_t b) { return (n + b - 1u) / b; }

template <class T>
hipError_t grow(T *&p, size_t &cap, size_t need, uint64_t &n_alloc) {
    if (need <= cap) return hipSuccess;
    ++n_alloc;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = std::max(need, (size_t)64);
    const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
}

}  // namespace

struct DeviceBvhBuilder::Impl {
    uint32_t n_tree = 0;
    uint32_t cap = 0;  // primitives every array is sized for (upload's n_boxes): n_tree <= cap
    Box6 *d_boxes = nullptr;
    uint32_t *d_order[2] = {nullptr, nullptr};
    int32_t *d_ptask[2] = {nullptr, nullptr};
    uint32_t *d_order0 = nullptr;  // the initial order, kept for the second shape
    Task *d_tasks[2] = {nullptr, nullptr};
    size_t tasks_cap[2] = {0, 0};
    Decision *d_dec = nullptr;
    size_t dec_cap = 0;
    Bin *d_bins = nullptr;
    size_t bins_cap = 0;
    uint32_t *d_scan = nullptr;  // 3 x scan_cap
    size_t scan_cap = 0;
    RawNode *d_raw = nullptr;
    uint8_t *d_flag = nullptr;
    uint32_t *d_block = nullptr;
    uint32_t *d_totals = nullptr;  // 3 task totals, 3 block totals
    LevelState *d_state = nullptr;
    int cur = 0;
    Slack slack{};
    Summary sum{};
    uint32_t levels = 0;
    uint64_t n_alloc = 0;  // hipMalloc calls so far (allocations())
    // refit: the first node of every level that holds nodes, then n_nodes (host and device), the
    // kept build's node price, the slack on the device, and the SAH terms
    std::vector<uint32_t> level_base;
    uint32_t *d_level_base = nullptr;  // cap + 1 entries
    double node_cost = 0.0;
    Slack *d_slack = nullptr;
    double *d_terms = nullptr;
    size_t terms_cap = 0;
    std::vector<double> terms;
    // the last build's cost: its terms and root node are set aside on the device by the first refit
    // after it (before any box changes) and summed when tree_cost() first asks
    double *d_terms_build = nullptr;
    size_t terms_build_cap = 0;
    RawNode *d_root_build = nullptr;
    bool build_captured = false, build_sah_known = false;
    double build_sah = 0.0;
    uint64_t refits = 0;  // since the last build
        uint32_t last_refit_launches = 0, last_refit_form = 0;

    // the fast builder's workspace (lbvh_build), each sized for cap primitives, and the last read
    uint64_t *d_lkeys[2] = {nullptr, nullptr}, *d_nkeys[2] = {nullptr, nullptr};
    uint32_t *d_lnode = nullptr;  // 7 x cap: first, last, child (2), parent, ids, scan
    LbvhState *d_lstate = nullptr;
    void *d_sort_tmp = nullptr;
    size_t lkeys_cap = 0, sort_tmp_bytes = 0;
    LbvhState lstate{};
    uint32_t lbvh_leaf[2] = {0u, 0u};
    int lbvh_finished = -1;   // the shape the tree on the device is finished for
    bool lbvh_small = false;  // the current build's form
    bool slack_on_device = false;  // the held tree's slack is d_slack's (a fast build), not `slack`
    // the last shape choice (stats_begin .. ): rrt_testing_scene_build_stats
    BuildStats stats{};
    LbvhArgs lbvh_args();

    hipError_t grow_scan(size_t n_tasks) {
        if (n_tasks <= scan_cap) return hipSuccess;
        (void)hipFree(d_scan);
        d_scan = nullptr;
        scan_cap = 0;
        ++n_alloc;
        const hipError_t e = hipMalloc((void **)&d_scan, n_tasks * 3 * 4);
        if (e == hipSuccess) scan_cap = n_tasks;
        return e;
    }

    ~Impl() {
        (void)hipFree(d_boxes);
        for (int k = 0; k < 2; ++k) {
            (void)hipFree(d_order[k]);
            (void)hipFree(d_ptask[k]);
            (void)hipFree(d_tasks[k]);
        }
        (void)hipFree(d_order0);
        (void)hipFree(d_dec);
        (void)hipFree(d_bins);
        (void)hipFree(d_scan);
        (void)hipFree(d_raw);
        (void)hipFree(d_flag);
        (void)hipFree(d_block);
        (void)hipFree(d_totals);
        (void)hipFree(d_state);
        (void)hipFree(d_level_base);
        (void)hipFree(d_slack);
        (void)hipFree(d_terms);
        (void)hipFree(d_terms_build);
        (void)hipFree(d_root_build);
        for (int k = 0; k < 2; ++k) {
            (void)hipFree(d_lkeys[k]);
            (void)hipFree(d_nkeys[k]);
        }
        (void)hipFree(d_lnode);
        (void)hipFree(d_lstate);
        (void)hipFree(d_sort_tmp);
    }
};

DeviceBvhBuilder::DeviceBvhBuilder() : impl_(new Impl) {}
DeviceBvhBuilder::~DeviceBvhBuilder() { delete impl_; }

#define BB_TRY(expr)                       \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

hipError_t DeviceBvhBuilder::upload(const Box6 *boxes, uint32_t n_boxes, const uint32_t *objs, uint32_t n_tree) {
    Impl &m = *impl_;
    if (n_tree < 2u || n_tree > n_boxes || m.cap) return hipErrorInvalidValue;
    for (uint32_t i = 0; i < n_tree; ++i)
        if (objs[i] >= n_boxes) return hipErrorInvalidValue;
    m.n_tree = n_tree;
    m.cap = n_boxes;
    const size_t cap = n_boxes;  // n_tree may grow up to it (set_objects)
    const uint32_t nb = blocks_of(n_boxes, kBlk);
    BB_TRY(hipMalloc((void **)&m.d_boxes, cap * sizeof(Box6)));
    BB_TRY(hipMemcpy(m.d_boxes, boxes, cap * sizeof(Box6), hipMemcpyHostToDevice));
    BB_TRY(hipMalloc((void **)&m.d_order0, cap * 4));
    BB_TRY(hipMemcpy(m.d_order0, objs, (size_t)n_tree * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; ++k) {
        BB_TRY(hipMalloc((void **)&m.d_order[k], cap * 4));
        BB_TRY(hipMalloc((void **)&m.d_ptask[k], cap * 4));
    }
    BB_TRY(hipMalloc((void **)&m.d_raw, cap * sizeof(RawNode)));  // internal nodes <= n_tree - 1
    BB_TRY(hipMalloc((void **)&m.d_flag, cap));
    BB_TRY(hipMalloc((void **)&m.d_block, (size_t)nb * 4));
    BB_TRY(hipMalloc((void **)&m.d_totals, 6 * 4));
    BB_TRY(hipMalloc((void **)&m.d_state, sizeof(LevelState)));
    BB_TRY(hipMalloc((void **)&m.d_level_base, (cap + 1) * 4));  // a level holds a node: <= n_tree - 1 levels
    BB_TRY(hipMalloc((void **)&m.d_slack, sizeof(Slack)));
    m.n_alloc += 12;
    return hipSuccess;
}

hipError_t DeviceBvhBuilder::set_objects(const uint32_t *objs, uint32_t n_tree) {
    Impl &m = *impl_;
    if (!m.cap || !objs || n_tree < 2u || n_tree > m.cap) return hipErrorInvalidValue;
    for (uint32_t i = 0; i < n_tree; ++i)
        if (objs[i] >= m.cap) return hipErrorInvalidValue;
    BB_TRY(hipMemcpy(m.d_order0, objs, (size_t)n_tree * 4, hipMemcpyHostToDevice));
    m.n_tree = n_tree;
    return hipSuccess;
}
uint32_t DeviceBvhBuilder::n_tree() const { return impl_->n_tree; }

// Tasks are disjoint ranges of span >= 2, so a level holds at most n_tree / 2 <= cap / 2 of them.
hipError_t DeviceBvhBuilder::reserve() {
    Impl &m = *impl_;
    if (m.n_tree < 2u) return hipErrorInvalidValue;
    const size_t max_tasks = m.cap / 2u;
    for (int k = 0; k < 2; ++k) BB_TRY(grow(m.d_tasks[k], m.tasks_cap[k], max_tasks, m.n_alloc));
    BB_TRY(grow(m.d_dec, m.dec_cap, max_tasks, m.n_alloc));
    BB_TRY(grow(m.d_bins, m.bins_cap, max_tasks * (3 * kBins), m.n_alloc));
    return m.grow_scan(max_tasks);
}

Box6 *DeviceBvhBuilder::device_boxes() { return impl_->d_boxes; }
const uint32_t *DeviceBvhBuilder::device_order() const { return impl_->d_order[impl_->cur]; }
uint64_t DeviceBvhBuilder::allocations() const { return impl_->n_alloc; }

hipError_t DeviceBvhBuilder::build(uint32_t max_leaf, double node_cost, Summary *out) {
    Impl &m = *impl_;
    const uint32_t n = m.n_tree;
    if (n < 2u) return hipErrorInvalidValue;
    const uint32_t nb = blocks_of(n, kBlk);
    m.cur = 0;
    m.slack_on_device = false;
    m.lbvh_finished = -1;
    m.stats.builder = 0, m.stats.form = 0;
    m.stats.shape_attempts++;
    m.stats.launches += 2, m.stats.blocking_reads += 1;  // the root's bounds
    BB_TRY(hipMemcpy(m.d_order[0], m.d_order0, (size_t)n * 4, hipMemcpyDeviceToDevice));
    BB_TRY(hipMemset(m.d_ptask[0], 0, (size_t)n * 4));  // every primitive in task 0, the root
    BB_TRY(hipMemset(m.d_state, 0, sizeof(LevelState)));
    BB_TRY(grow(m.d_tasks[0], m.tasks_cap[0], 1, m.n_alloc));
    Task root;
    root.lo = 0;
    root.hi = n;
    root.slot = kNoSlot;
    root.usable = 0;
    root.b = bounds_empty();
    BB_TRY(hipMemcpy(m.d_tasks[0], &root, sizeof(Task), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_root_bounds, dim3(nb), dim3(kBlk), 0, 0, n, m.d_order[0], m.d_boxes, m.d_tasks[0]);
    hipLaunchKernelGGL(k_root_finish, dim3(1), dim3(1), 0, 0, m.d_tasks[0]);
    BB_TRY(hipGetLastError());
    BB_TRY(hipMemcpy(&root, m.d_tasks[0], sizeof(Task), hipMemcpyDeviceToHost));
    double root_box[6];
    for (int j = 0; j < 6; ++j) root_box[j] = key_f64(root.b.k[j]);
    m.slack = slack_of(root_box);

    uint32_t n_tasks = 1, level = 0, max_depth = 0;
    LevelState st{};
    m.level_base.clear();
    m.node_cost = node_cost;
    m.build_captured = m.build_sah_known = false;
    m.refits = 0;
    while (n_tasks > 0) {
        if (level > n) return hipErrorUnknown;  // every split leaves two non-empty sides: depth < n
        const int c = m.cur, o = 1 - m.cur;
        const uint32_t next_cap = std::min<uint64_t>(2ull * n_tasks, n / 2u);
        BB_TRY(grow(m.d_tasks[o], m.tasks_cap[o], std::max<size_t>(next_cap, 1), m.n_alloc));
        BB_TRY(grow(m.d_dec, m.dec_cap, n_tasks, m.n_alloc));
        BB_TRY(grow(m.d_bins, m.bins_cap, (size_t)n_tasks * (3 * kBins), m.n_alloc));
        BB_TRY(m.grow_scan(n_tasks));
        uint32_t *s_node = m.d_scan, *s_child = m.d_scan + m.scan_cap, *s_left = m.d_scan + 2 * m.scan_cap;
        const uint64_t bin_words = (uint64_t)n_tasks * kTaskWords;
        const uint32_t tb = blocks_of(n_tasks, 64u);
        hipLaunchKernelGGL(k_bins_init, dim3((uint32_t)((bin_words + kBlk - 1) / kBlk)), dim3(kBlk), 0, 0, bin_words,
                           (u64 *)m.d_bins);
        hipLaunchKernelGGL(k_bin, dim3(nb), dim3(kBlk), 0, 0, n, m.d_order[c], m.d_ptask[c], m.d_tasks[c], m.d_boxes,
                           m.d_bins);
        hipLaunchKernelGGL(k_decide, dim3(tb), dim3(64), 0, 0, n_tasks, m.d_tasks[c], m.d_bins, max_leaf, node_cost,
                           m.d_dec, s_node, s_child, s_left);
        hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(kScanBlk), 0, 0, n_tasks, s_node, s_child, s_left, m.d_totals);
        hipLaunchKernelGGL(k_level_totals, dim3(1), dim3(1), 0, 0, m.d_totals, m.d_state);
        hipLaunchKernelGGL(k_emit, dim3(tb), dim3(64), 0, 0, n_tasks, m.d_tasks[c], m.d_dec, s_node, s_child, m.d_state,
                           m.d_raw, n, m.d_tasks[o], next_cap);
        hipLaunchKernelGGL(k_flags, dim3(nb), dim3(kBlk), 0, 0, n, m.d_order[c], m.d_ptask[c], m.d_tasks[c], m.d_dec,
                           m.d_boxes, m.d_flag, m.d_block);
        hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(kScanBlk), 0, 0, nb, m.d_block, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, m.d_totals + 3);
        hipLaunchKernelGGL(k_scatter, dim3(nb), dim3(kBlk), 0, 0, n, m.d_order[c], m.d_ptask[c], m.d_tasks[c], m.d_dec,
                           s_child, s_left, m.d_flag, m.d_block, m.d_order[o], m.d_ptask[o], m.d_state);
        BB_TRY(hipGetLastError());
        BB_TRY(hipMemcpy(&st, m.d_state, sizeof(LevelState), hipMemcpyDeviceToHost));  // the per-level blocking read
        m.stats.launches += 9, m.stats.blocking_reads += 1;
        if (st.error || st.n_next > next_cap) return hipErrorUnknown;
        if (st.n_split) {
            max_depth = level + 1;
            m.level_base.push_back(st.node_base);
        }
        m.cur = o;
        n_tasks = st.n_next;
        ++level;
    }
    m.levels = level;
    m.sum.n_nodes = st.n_nodes;
    m.sum.n_leaves = st.n_leaves;
    m.sum.max_depth = std::max(max_depth, 1u);  // a root leaf: depth 1
    m.sum.max_leaf = st.max_leaf;
    if (m.sum.n_nodes == 0 || m.sum.n_nodes > n) return hipErrorUnknown;
    if (m.level_base.empty()) m.level_base.push_back(0u);  // the root-leaf form: node 0 alone
    m.level_base.push_back(m.sum.n_nodes);
    if (m.level_base.size() > (size_t)n + 1) return hipErrorUnknown;
    BB_TRY(hipMemcpy(m.d_level_base, m.level_base.data(), m.level_base.size() * 4, hipMemcpyHostToDevice));
    if (out) *out = m.sum;
    return hipSuccess;
}

namespace {
std::atomic<int> g_refit_form{-1};  // rrt_testing_refit_form
}
bool set_refit_form(int form) {
    if (form < -1 || form > 1) return false;
    g_refit_form.store(form);
    return true;
}

bool DeviceBvhBuilder::refit_form_ok() const { return g_refit_form.load() != 1 || impl_->sum.n_nodes <= kRefitSmallMaxNodes; }
uint32_t DeviceBvhBuilder::refit_small_max_nodes() { return kRefitSmallMaxNodes; }

hipError_t DeviceBvhBuilder::refit(hipStream_t stream) {
    Impl &m = *impl_;
    const uint32_t n_nodes = m.sum.n_nodes;
    if (n_nodes == 0 || m.level_base.size() < 2) return hipErrorInvalidValue;
    const int forced = g_refit_form.load();
    if (forced == 1 && n_nodes > kRefitSmallMaxNodes) return hipErrorInvalidValue;
    const bool small = forced < 0 ? n_nodes <= kRefitSmallMaxNodes : forced == 1;
    const uint32_t n_levels = (uint32_t)m.level_base.size() - 1u;
    const uint32_t *order = m.d_order[m.cur];
    uint32_t launches = 0;
    if (!m.build_captured) {  // the build's cost terms and root, while the tree still holds them
        if (m.terms_build_cap < n_nodes || !m.d_root_build) return hipErrorInvalidValue;  // reserve_refit() first
        hipLaunchKernelGGL(k_sah_terms, dim3(blocks_of(n_nodes, kBlk)), dim3(kBlk), 0, stream, n_nodes, m.d_raw, m.node_cost,
                           m.d_terms_build, m.d_root_build);
        BB_TRY(hipGetLastError());
        m.build_captured = true;
        launches = 1;
    }
    if (small) {
        hipLaunchKernelGGL(k_refit_small, dim3(1), dim3(kScanBlk), 0, stream, n_levels, m.d_level_base, m.d_raw, n_nodes,
                           m.n_tree, order, m.d_boxes, m.d_slack);
        m.last_refit_launches = launches + 1u;
    } else {
        for (uint32_t l = n_levels; l-- > 0;) {
            const uint32_t base = m.level_base[l], end = m.level_base[l + 1];
            hipLaunchKernelGGL(k_refit_level, dim3(blocks_of(2u * (end - base), kBlk)), dim3(kBlk), 0, stream, base, end,
                               m.d_raw, n_nodes, m.n_tree, order, m.d_boxes);
        }
        hipLaunchKernelGGL(k_refit_slack, dim3(1), dim3(1), 0, stream, m.d_raw, m.d_slack);
        m.last_refit_launches = launches + n_levels + 1u;
    }
    m.last_refit_form = small ? 1u : 0u;
    m.refits++;
    return hipGetLastError();
}

hipError_t DeviceBvhBuilder::emit_refit(uint32_t stride, uint8_t *d_nodes, size_t cap_bytes, hipStream_t stream) {
    Impl &m = *impl_;
    if ((stride != 80u && stride != 32u) || m.sum.n_nodes == 0 || !d_nodes ||
        (size_t)m.sum.n_nodes * stride > cap_bytes)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pack_dev, dim3(blocks_of(m.sum.n_nodes, kBlk)), dim3(kBlk), 0, stream, m.sum.n_nodes, m.d_raw,
                       m.d_slack, stride, (uint32_t *)d_nodes);
    return hipGetLastError();
}

uint32_t DeviceBvhBuilder::refit_launches() const { return impl_->last_refit_launches; }
uint32_t DeviceBvhBuilder::refit_form() const { return impl_->last_refit_form; }

hipError_t DeviceBvhBuilder::reserve_cost() {
    Impl &m = *impl_;
    BB_TRY(grow(m.d_terms, m.terms_cap, (size_t)m.cap, m.n_alloc));
    if (!m.d_root_build) {
        ++m.n_alloc;
        BB_TRY(hipMalloc((void **)&m.d_root_build, 2 * sizeof(RawNode)));  // [0]: the build's root, [1]: the current one
    }
    return hipSuccess;
}
hipError_t DeviceBvhBuilder::reserve_refit() {
    Impl &m = *impl_;
    BB_TRY(reserve_cost());
    return grow(m.d_terms_build, m.terms_build_cap, (size_t)m.cap, m.n_alloc);
}
uint64_t DeviceBvhBuilder::refits_since_build() const { return impl_->refits; }

// The SAH cost of the tree held now (rrt_bvh_binned.h): the terms by one launch on the default
// stream, copied back and summed here in node order. The caller has synchronised the device.
hipError_t DeviceBvhBuilder::tree_cost(double *sah, double *sah_at_build) {
    Impl &m = *impl_;
    const uint32_t n_nodes = m.sum.n_nodes;
    if (n_nodes == 0 || !sah || !sah_at_build) return hipErrorInvalidValue;
    BB_TRY(reserve_cost());
    hipLaunchKernelGGL(k_sah_terms, dim3(blocks_of(n_nodes, kBlk)), dim3(kBlk), 0, 0, n_nodes, m.d_raw, m.node_cost,
                       m.d_terms, m.d_root_build + 1);
    BB_TRY(hipGetLastError());
    m.terms.resize(n_nodes);
    RawNode root;
    BB_TRY(hipMemcpy(m.terms.data(), m.d_terms, (size_t)n_nodes * 8, hipMemcpyDeviceToHost));
    BB_TRY(hipMemcpy(&root, m.d_root_build + 1, sizeof(RawNode), hipMemcpyDeviceToHost));
    *sah = sah_of_terms(m.terms.data(), n_nodes, root);
    if (!m.build_sah_known) {
        if (m.build_captured) {  // refitted since: the terms set aside by the first refit
            BB_TRY(hipMemcpy(m.terms.data(), m.d_terms_build, (size_t)n_nodes * 8, hipMemcpyDeviceToHost));
            BB_TRY(hipMemcpy(&root, m.d_root_build, sizeof(RawNode), hipMemcpyDeviceToHost));
            m.build_sah = sah_of_terms(m.terms.data(), n_nodes, root);
        } else {
            m.build_sah = *sah;
        }
        m.build_sah_known = true;
    }
    *sah_at_build = m.build_sah;
    return hipSuccess;
}

hipError_t DeviceBvhBuilder::emit(uint32_t stride, uint8_t **d_nodes_out, uint32_t *order_out) {
    Impl &m = *impl_;
    if ((stride != 80u && stride != 32u) || m.sum.n_nodes == 0) return hipErrorInvalidValue;
    uint8_t *d = nullptr;
    ++m.n_alloc;
    BB_TRY(hipMalloc((void **)&d, (size_t)m.sum.n_nodes * stride));
    const hipError_t e = emit_into(stride, d, (size_t)m.sum.n_nodes * stride, order_out);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return e;
    }
    *d_nodes_out = d;
    return hipSuccess;
}

hipError_t DeviceBvhBuilder::emit_into(uint32_t stride, uint8_t *d_nodes, size_t cap_bytes, uint32_t *order_out) {
    Impl &m = *impl_;
    if ((stride != 80u && stride != 32u) || m.sum.n_nodes == 0 || !d_nodes ||
        (size_t)m.sum.n_nodes * stride > cap_bytes)
        return hipErrorInvalidValue;
    if (m.slack_on_device)  // a fast build never brings the root box to the host
        hipLaunchKernelGGL(k_pack_dev, dim3(blocks_of(m.sum.n_nodes, kBlk)), dim3(kBlk), 0, 0, m.sum.n_nodes, m.d_raw,
                           m.d_slack, stride, (uint32_t *)d_nodes);
    else
        hipLaunchKernelGGL(k_pack, dim3(blocks_of(m.sum.n_nodes, kBlk)), dim3(kBlk), 0, 0, m.sum.n_nodes, m.d_raw, m.slack,
                           stride, (uint32_t *)d_nodes);
    BB_TRY(hipGetLastError());
    return hipMemcpy(order_out, m.d_order[m.cur], (size_t)m.n_tree * 4, hipMemcpyDeviceToHost);
}

uint32_t DeviceBvhBuilder::levels() const { return impl_->levels; }

// ---- the fast builder ----------------------------------------------------------------------------
namespace {
std::atomic<int> g_lbvh_form{-1};  // rrt_testing_lbvh_form
}
bool set_lbvh_form(int form) {
    if (form < -1 || form > 1) return false;
    g_lbvh_form.store(form);
    return true;
}
uint32_t DeviceBvhBuilder::lbvh_small_max() { return kLbvhSmallMax; }
void DeviceBvhBuilder::stats_begin() { impl_->stats = BuildStats{}; }
BuildStats DeviceBvhBuilder::stats() const { return impl_->stats; }

hipError_t DeviceBvhBuilder::reserve_lbvh() {
    Impl &m = *impl_;
    if (!m.cap) return hipErrorInvalidValue;
    const size_t cap = m.cap;
    if (m.lkeys_cap < cap) {
        if (m.lkeys_cap) return hipErrorInvalidValue;  // cap is fixed by upload()
        for (int k = 0; k < 2; ++k) {
            BB_TRY(hipMalloc((void **)&m.d_lkeys[k], cap * 8));
            BB_TRY(hipMalloc((void **)&m.d_nkeys[k], cap * 8));
        }
        BB_TRY(hipMalloc((void **)&m.d_lnode, cap * 7 * 4));
        BB_TRY(hipMalloc((void **)&m.d_lstate, sizeof(LbvhState)));
        size_t t0 = 0, t1 = 0;
        BB_TRY(rocprim::radix_sort_keys(nullptr, t0, m.d_lkeys[0], m.d_lkeys[1], (uint32_t)cap, 0u, 62u, (hipStream_t)0));
        BB_TRY(rocprim::radix_sort_keys(nullptr, t1, m.d_nkeys[0], m.d_nkeys[1], (uint32_t)cap, 28u, 62u, (hipStream_t)0));
        m.sort_tmp_bytes = std::max<size_t>(std::max(t0, t1), 64);
        BB_TRY(hipMalloc(&m.d_sort_tmp, m.sort_tmp_bytes));
        m.n_alloc += 7;
        m.lkeys_cap = cap;
    }
    return hipSuccess;
}

namespace {
// rocPRIM's radix sort of bits [lo, hi) of n keys, its temporary storage the builder's.
hipError_t lbvh_sort(void *tmp, size_t tmp_bytes, uint64_t *in, uint64_t *out, uint32_t n, unsigned lo, unsigned hi) {
    size_t need = 0;
    BB_TRY(rocprim::radix_sort_keys(nullptr, need, in, out, n, lo, hi, (hipStream_t)0));
    if (need > tmp_bytes) return hipErrorOutOfMemory;  // sized for cap keys: never expected
    return rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n, lo, hi, (hipStream_t)0);
}
}  // namespace

LbvhArgs DeviceBvhBuilder::Impl::lbvh_args() {
    Impl &m = *this;
    LbvhArgs a{};
    a.n = m.n_tree, a.cap = m.cap;
    a.leaf[0] = m.lbvh_leaf[0], a.leaf[1] = m.lbvh_leaf[1];
    a.boxes = m.d_boxes, a.objs = m.d_order0;
    for (int k = 0; k < 2; ++k) a.keys[k] = m.d_lkeys[k], a.nkeys[k] = m.d_nkeys[k];
    const size_t cap = m.cap;
    a.first = m.d_lnode, a.last = m.d_lnode + cap, a.child = m.d_lnode + 2 * cap, a.parent = m.d_lnode + 4 * cap;
    a.ids = m.d_lnode + 5 * cap, a.scan = m.d_lnode + 6 * cap;
    a.order = m.d_order[0];
    a.raw = m.d_raw, a.level_base = m.d_level_base, a.st = m.d_lstate;
    return a;
}

namespace {
uint32_t pow2_at_least(uint32_t n) {
    uint32_t p = 2;
    while (p < n) p <<= 1;
    return p;
}
// What the state says of shape s.
Summary lbvh_summary(const LbvhState &st, uint32_t n, uint32_t leaf, int s, std::vector<uint32_t> *level_base) {
    Summary sum{};
    if (level_base) level_base->clear();
    if (n <= leaf) {
        sum.n_nodes = 1, sum.n_leaves = 1, sum.max_depth = 1, sum.max_leaf = n;
        if (level_base) level_base->push_back(0u), level_base->push_back(1u);
        return sum;
    }
    uint32_t l = 0;
    for (; l < kMaxLevels && st.hist[s][l] != 0u; ++l) {
        if (level_base) level_base->push_back(sum.n_nodes);
        sum.n_nodes += st.hist[s][l];
    }
    if (level_base) level_base->push_back(sum.n_nodes);
    sum.max_depth = l;
    sum.n_leaves = sum.n_nodes + 1u;
    sum.max_leaf = st.max_leaf[s];
    return sum;
}
}  // namespace

// The phases up to the one blocking read. Launches of the per-phase form: init, bounds, keys, sort,
// topology, levels, sort (7, a sort counted once); the single workgroup: 1, which also finishes the
// shape fit_nodes predicts.
hipError_t DeviceBvhBuilder::lbvh_build(uint32_t leaf_a, uint32_t leaf_b, uint32_t fit_nodes, Summary out[2]) {
    Impl &m = *impl_;
    const uint32_t n = m.n_tree;
    if (n < 2u || leaf_a == 0 || leaf_b == 0) return hipErrorInvalidValue;
    const int forced = g_lbvh_form.load();
    if (forced == 1 && n > kLbvhSmallMax) return hipErrorInvalidValue;
    BB_TRY(reserve_lbvh());
    m.lbvh_small = forced < 0 ? n <= kLbvhSmallMax : forced == 1;
    m.lbvh_leaf[0] = leaf_a, m.lbvh_leaf[1] = leaf_b;
    m.lbvh_finished = -1;
    m.cur = 0;
    m.sum = Summary{};
    m.level_base.clear();
    m.build_captured = m.build_sah_known = false;
    m.refits = 0;
    m.levels = 0;
    m.stats.builder = 1, m.stats.form = m.lbvh_small ? 1u : 0u;
    const LbvhArgs a = m.lbvh_args();
    const uint32_t nb = blocks_of(n, kBlk);
    if (m.lbvh_small) {
        hipLaunchKernelGGL(k_lbvh_small, dim3(1), dim3(kScanBlk), 0, 0, a, 1u, 0, fit_nodes, pow2_at_least(n), m.d_slack);
        BB_TRY(hipGetLastError());
        m.stats.launches += 1;
        m.stats.shape_attempts += 1;
    } else {
        hipLaunchKernelGGL(k_lbvh_init, dim3(1), dim3(128), 0, 0, m.d_lstate);
        hipLaunchKernelGGL(k_lbvh_bounds, dim3(nb), dim3(kBlk), 0, 0, a);
        hipLaunchKernelGGL(k_lbvh_keys, dim3(nb), dim3(kBlk), 0, 0, a);
        BB_TRY(hipGetLastError());
        BB_TRY(lbvh_sort(m.d_sort_tmp, m.sort_tmp_bytes, m.d_lkeys[0], m.d_lkeys[1], n, 0u, 62u));
        hipLaunchKernelGGL(k_lbvh_topology, dim3(nb), dim3(kBlk), 0, 0, a);
        hipLaunchKernelGGL(k_lbvh_levels, dim3(nb), dim3(kBlk), 0, 0, a);
        BB_TRY(hipGetLastError());
        BB_TRY(lbvh_sort(m.d_sort_tmp, m.sort_tmp_bytes, m.d_nkeys[0], m.d_nkeys[1], n - 1u, 28u, 62u));
        m.stats.launches += 7;
    }
    BB_TRY(hipMemcpy(&m.lstate, m.d_lstate, sizeof(LbvhState), hipMemcpyDeviceToHost));  // the build's one blocking read
    m.stats.blocking_reads += 1;
    if (m.lstate.error) return hipErrorUnknown;
    for (int s = 0; s < 2; ++s) {
        out[s] = lbvh_summary(m.lstate, n, m.lbvh_leaf[s], s, nullptr);
        if (out[s].n_nodes == 0 || out[s].n_nodes >= n) return hipErrorUnknown;
    }
    if (m.lbvh_small) m.lbvh_finished = m.lstate.finished ? 1 : 0;
    return hipSuccess;
}

// Shape `shape` of the last lbvh_build becomes the held tree: numbers, links, level table and boxes,
// with no read. Launches of the per-phase form: flags and scan (leaves over 1 only), ids, links (4),
// then the box pass: the refit's single workgroup (1), or one per level and the slack.
hipError_t DeviceBvhBuilder::lbvh_finish(int shape, double node_cost, Summary *out) {
    Impl &m = *impl_;
    const uint32_t n = m.n_tree;
    if (shape < 0 || shape > 1 || !m.lbvh_leaf[0]) return hipErrorInvalidValue;
    m.sum = lbvh_summary(m.lstate, n, m.lbvh_leaf[shape], shape, &m.level_base);
    m.levels = m.sum.max_depth;
    m.node_cost = node_cost;
    m.slack_on_device = true;
    if (out) *out = m.sum;
    if (m.lbvh_finished == shape) return hipSuccess;
    const LbvhArgs a = m.lbvh_args();
    m.stats.shape_attempts += 1;
    if (m.lbvh_small) {
        hipLaunchKernelGGL(k_lbvh_small, dim3(1), dim3(kScanBlk), 0, 0, a, 0u, shape, 0u, pow2_at_least(n), m.d_slack);
        m.stats.launches += 1;
    } else {
        const uint32_t nkb = blocks_of(n - 1u, kBlk), leaf = m.lbvh_leaf[shape];
        if (leaf > 1u) {
            hipLaunchKernelGGL(k_lbvh_flags, dim3(nkb), dim3(kBlk), 0, 0, a, leaf);
            hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(kScanBlk), 0, 0, n - 1u, a.scan, (uint32_t *)nullptr,
                               (uint32_t *)nullptr, m.d_totals);
            m.stats.launches += 2;
        }
        hipLaunchKernelGGL(k_lbvh_ids, dim3(nkb), dim3(kBlk), 0, 0, a, leaf, leaf > 1u ? 1u : 0u);
        hipLaunchKernelGGL(k_lbvh_links, dim3(nkb), dim3(kBlk), 0, 0, a, shape);
        m.stats.launches += 2;
        const uint32_t n_nodes = m.sum.n_nodes, n_levels = (uint32_t)m.level_base.size() - 1u;
        if (n_nodes <= kRefitSmallMaxNodes) {
            hipLaunchKernelGGL(k_refit_small, dim3(1), dim3(kScanBlk), 0, 0, n_levels, m.d_level_base, m.d_raw, n_nodes, n,
                               m.d_order[0], m.d_boxes, m.d_slack);
            m.stats.launches += 1;
        } else {
            for (uint32_t l = n_levels; l-- > 0;) {
                const uint32_t base = m.level_base[l], end = m.level_base[l + 1];
                hipLaunchKernelGGL(k_refit_level, dim3(blocks_of(2u * (end - base), kBlk)), dim3(kBlk), 0, 0, base, end, m.d_raw,
                                   n_nodes, n, m.d_order[0], m.d_boxes);
            }
            hipLaunchKernelGGL(k_refit_slack, dim3(1), dim3(1), 0, 0, m.d_raw, m.d_slack);
            m.stats.launches += n_levels + 1u;
        }
    }
    BB_TRY(hipGetLastError());
    m.lbvh_finished = shape;
    return hipSuccess;
}

}  // namespace rrt
