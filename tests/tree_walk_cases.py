"""Inputs for the shared compaction (csrc/mnv_tree_walk.hip behind mnv_tree_truncate and mnv_tree_cut) whose predicate arrays disagree with
the tree: depth words and keep bytes that were edited by hand, and a few links that leave the tree.  The entry points check none of that;
what they answer is the behaviour, restated by view_lod_ref.cut.  tests/test_tree_walk_ref.py asserts that every situation occurs."""
import numpy as np

import lod_ref
import view_lod_ref
from test_lod_gpu import _random_tree as random_tree

MAX_DEPTH = 3
TREES = {5: (31, 5, 5, 0.5), 13: (32, 5, 13, 0.45)}       # data_dim -> (seed, levels, data_dim, p)


def _parents(child):
    """parent chunk of every chunk that a link inside [1, cap) leads to (-1: none)"""
    cap = child.shape[0]
    rows, cols = np.nonzero(child)
    target = rows + child[rows, cols].astype(np.int64)
    ok = (target >= 1) & (target < cap)
    parent = np.full(cap, -1, np.int64)
    parent[target[ok]] = rows[ok]
    return parent


def disagreeing(dd):
    """dict(data, child, counts, words, keep, max_depth): a random tree of depth 5; `words` are its chunk depths and `keep` the bytes of
    words in [1, max_depth], both after the edits below; three links of kept chunks lead outside [1, cap)."""
    data, child = random_tree(*TREES[dd])
    child = child.copy()
    cap = child.shape[0]
    rng = np.random.default_rng(dd)
    depth, _ = lod_ref.chunk_depths(child)
    parent = _parents(child)
    words = depth.astype(np.int32).copy()
    has_child = np.zeros(cap, bool)
    has_child[parent[parent >= 0]] = True
    at = lambda d, inner: [int(c) for c in np.nonzero((depth == d) & (has_child == inner))[0]]
    two, four = at(2, True), at(4, False) + at(4, True)
    words[two[0]] = 0                                     # a dropped chunk under the kept root; its children (depth 3) stay as orphans
    words[two[1]] = MAX_DEPTH + 4                         # ... and one whose word is above max_depth
    words[four[0]] = 2                                    # within range under a parent whose word is max_depth: an orphan of the truncation
    words[four[1]] = MAX_DEPTH                            # ... and under the same rule with the word max_depth itself
    keep = ((words >= 1) & (words <= MAX_DEPTH)).astype(np.uint8)
    keep[keep != 0] = rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), size=int(keep.sum()))      # any non-zero byte keeps
    # links that leave the tree, in leaf voxels of three kept chunks: to chunk 0, to chunk cap, far below 0
    hosts = [c for c in np.nonzero(keep)[0] if c >= 1 and (child[c] == 0).any()][:3]
    for c, target in zip(hosts, (0, cap, -5 * cap)):
        child[c, int(np.nonzero(child[c] == 0)[0][0])] = target - c
    counts = rng.integers(-100, 3000, size=(cap, 8)).astype(np.int16)
    return dict(data=data, child=child, counts=counts, words=words, keep=keep, max_depth=MAX_DEPTH)


def census(case):
    """how often each situation occurs: dict of counts"""
    child, words, keep, D = case["child"], case["words"], case["keep"] != 0, case["max_depth"]
    cap = child.shape[0]
    parent = _parents(child)
    rows, cols = np.nonzero(child)
    target = rows + child[rows, cols].astype(np.int64)
    inside = (target >= 1) & (target < cap)
    r, t = rows[inside], target[inside]
    has_parent = parent >= 0
    return dict(
        kept_under_dropped=int((keep & has_parent & ~keep[np.where(has_parent, parent, 0)]).sum()),
        dropped_under_kept=int((keep[r] & ~keep[t]).sum()),
        links_outside=int((keep[rows] & ~inside).sum()),
        word_out_of_range_under_shallow_parent=int((((words[t] > D) | (words[t] == 0)) & (words[r] >= 1) & (words[r] < D)).sum()),
        word_in_range_under_parent_at_max_depth=int(((words[t] >= 1) & (words[t] <= D) & (words[r] == D)).sum()))


def expected(case):
    """(what mnv_tree_truncate answers, what mnv_tree_cut answers): view_lod_ref.cut, for the truncation on links that end at max_depth"""
    cut_links = case["child"].copy()
    cut_links[case["words"] == case["max_depth"]] = 0
    return (view_lod_ref.cut(case["data"], cut_links, case["keep"], case["counts"]),
            view_lod_ref.cut(case["data"], case["child"], case["keep"], case["counts"]))
