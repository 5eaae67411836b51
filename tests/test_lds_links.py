"""The link rule of the f32 kernel's LDS staging (rrt_internal.h lds_node_link, through the test-only
export rrt_testing_lds_node_link) on the host: no device needed.

The kernel stages a scene's 80-B BVH2 nodes at LDS offset 0 and rewrites every inner link (count
field 0) from a node index to the node's byte offset, so the node step reads its planes and links at
the link itself; leaf links (first primitive | count << 28) stay what they are. A staged scene is at
most 40 KB (kLdsSceneBudget), so every offset must fit the 16-bit stack entries.
"""
import numpy as np

from rustraytrace_amd import _lib

NODE_BYTES = 80          # sizeof(GNode)
BUDGET = 40 * 1024       # rrt_internal.h kLdsSceneBudget: nodes + primitives of a staged scene
COUNT_SHIFT = 28         # rrt_internal.h kLinkCountShift


def _link(words):
    f = _lib.load().rrt_testing_lds_node_link
    return np.array([f(int(w)) for w in words], dtype=np.uint64)


def test_inner_links_become_byte_offsets_for_every_node_count_up_to_the_budget():
    n_max = BUDGET // NODE_BYTES  # a scene of nodes alone: no staged scene has more
    idx = np.arange(n_max + 1, dtype=np.uint64)
    off = _link(idx)
    assert np.array_equal(off, idx * NODE_BYTES)
    assert np.all(off % 16 == 0)
    assert np.all(off < 65536)
    assert off[0] == 0  # the root's offset is the root's index


def test_leaf_links_are_returned_unchanged():
    firsts = np.array([0, 1, 2, 79, 80, 511, 512, 819, 65535, 65536, (1 << COUNT_SHIFT) - 1], dtype=np.uint64)
    for count in range(1, 16):  # every non-zero value of the 4-bit count field (two leaves: up to 14)
        words = firsts | np.uint64(count << COUNT_SHIFT)
        assert np.array_equal(_link(words), words), f"count {count}"
