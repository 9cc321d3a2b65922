"""What the passes over a tree share (csrc/mnv_tree_walk.hip): one compaction behind mnv_tree_truncate and mnv_tree_cut, one level walk with
one per-device scratch behind mnv_tree_mip_rows and mnv_tree_cull.  Every comparison is on bits, against the numpy restatements."""
import numpy as np
import pytest

import lod_ref
import test_lod_gpu as L
import test_view_lod_gpu as V
import test_visibility_gpu as G
import tree_walk_cases as cases
import visibility_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dd", sorted(cases.TREES))
def test_truncate_and_cut_on_arrays_that_disagree_with_the_tree(mnv, torch_gpu, dd):
    torch = torch_gpu
    case = cases.disagreeing(dd)
    assert all(n >= 1 for n in cases.census(case).values())
    want_truncate, want_cut = cases.expected(case)
    n = want_cut["capacity"]
    data_t, child_t, sc_t = L._dev(torch, case["data"]), L._dev(torch, case["child"]), L._dev(torch, case["counts"])
    words_t, keep_t = L._dev(torch, case["words"]), torch.from_numpy(case["keep"]).cuda()
    view = V._view(mnv, data_t, child_t, dd, counts_t=sc_t)
    a, b = V._outputs(torch, n, dd), V._outputs(torch, n, dd)
    mnv.tree_truncate(view, words_t, case["max_depth"], n, a["child"], a["data"], a["parent"], a["sample_counts"])      # no refusal
    mnv.tree_cut(view, keep_t, n, b["child"], b["data"], b["parent"], b["sample_counts"])
    torch.cuda.synchronize()
    for name, o, want in (("truncate", a, want_truncate), ("cut", b, want_cut)):
        got, clean = V._host(o, n)
        assert clean, name                                                        # nothing at or beyond new_capacity
        for k in ("child", "data", "parent", "sample_counts"):
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, (name, k, bad[:5])
    assert np.array_equal(L._host16(data_t), case["data"]) and np.array_equal(child_t.cpu().numpy(), case["child"])
    assert np.array_equal(words_t.cpu().numpy(), case["words"]) and np.array_equal(keep_t.cpu().numpy(), case["keep"])


def test_walk_scratch_is_shared_and_reused(mnv, torch_gpu):
    torch = torch_gpu
    large, small = L._random_tree(71, 6, 13, 0.45), L._random_tree(72, 4, 5, 0.5)
    assert 700 < large[1].shape[0] < 1600 and 40 < small[1].shape[0] < 200
    rng = np.random.default_rng(73)
    words = {id(t): G._words(rng, t[1].shape[0] * 8) for t in (large, small)}

    def mip(tree, want_depth):
        want, _, want_counts = lod_ref.mip_rows(*tree)
        out, _, counts = L._mip(mnv, torch, *tree, want_depth=want_depth)
        assert np.array_equal(counts, want_counts) and np.array_equal(out, want)

    def cull(tree):
        G._check_cull(mnv, torch, *tree, words[id(tree)])

    mip(large, True)        # the scratch grows to the large tree
    cull(small)             # ... and is used by the other pass, with stale lists and depth words behind the small tree's
    cull(large)
    mip(small, False)       # the walk's own depth words
    # a refused call leaves nothing behind: a leaf voxel of the last chunk links to a chunk that has a parent already
    data, child = large
    bad = child.copy()
    c = child.shape[0] - 1
    bad[c, int(np.nonzero(bad[c] == 0)[0][0])] = 1 - c
    with pytest.raises(ValueError, match="invalid"):
        visibility_ref.tree_cull(data, bad, words[id(large)], 0.0)
    with pytest.raises(mnv.MnvError, match="reached twice") as e:
        L._mip(mnv, torch, data, bad, want_depth=False)
    assert e.value.code == mnv.MNV_E_INVALID
    cull(large)
    mip(large, False)
    mip(small, True)
