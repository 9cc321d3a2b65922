"""The inputs of tests/test_tree_walk_gpu.py hold what they are there for (no GPU needed): every way in which the predicate arrays of a
compaction can disagree with the tree occurs, and the restatement answers each as the contract says."""
import numpy as np
import pytest

import tree_walk_cases as cases


@pytest.mark.parametrize("dd", sorted(cases.TREES))
def test_the_disagreeing_arrays_hold_every_situation(dd):
    case = cases.disagreeing(dd)
    cap = case["child"].shape[0]
    assert 100 <= cap <= 1600 and case["data"].shape == (cap, 8, dd) and case["counts"].shape == (cap, 8)
    census = cases.census(case)
    assert all(n >= 1 for n in census.values()), census
    assert census["links_outside"] == 3
    assert len(set(case["keep"].tolist())) > 2                                    # more than one non-zero byte value keeps
    truncated, cut = cases.expected(case)
    n = int((case["keep"] != 0).sum())
    assert truncated["capacity"] == cut["capacity"] == n and 8 < n < cap
    for want in (truncated, cut):
        assert want["parent"][0] == -1 and (want["parent"][1:] == -1).sum() >= census["kept_under_dropped"]       # orphans stay, parent -1
        assert np.array_equal(want["data"], case["data"][case["keep"] != 0])
    # the truncation drops the links out of chunks at max_depth, so it orphans more chunks than the cut and carries fewer links
    assert (truncated["parent"] == -1).sum() >= (cut["parent"] == -1).sum() + census["word_in_range_under_parent_at_max_depth"]
    assert np.count_nonzero(truncated["child"]) < np.count_nonzero(cut["child"])
