"""The level-of-detail contracts of include/mnv.h (mnv_tree_mip_rows, mnv_tree_truncate) pinned on the host: tests/lod_ref.py restates them
in numpy; these tests hold the restatement to hand-computed halfs and to the properties the contracts promise.  tests/test_lod_gpu.py
compares the device code with the same restatement, bit for bit."""
import numpy as np
import pytest

import lod_ref

H = dict(zero=0x0000, one=0x3C00, two=0x4000, four=0x4400, six=0x4600, hundred=0x5640, minus_one=0xBC00, half=0x3800, three_eighths=0x3600,
         third=0x3555)


def _two_level_tree():
    """Root chunk 0 with voxel 0 -> chunk 1 and voxel 3 -> chunk 2; rows are (colour, sigma)."""
    child = np.zeros((3, 8), np.int32)
    child[0, 0], child[0, 3] = 1, 2
    data = np.zeros((3, 8, 2), np.uint16)
    data[0, :, 0] = 0x1234   # stale interior rows and leaf rows of the root
    data[0, :, 1] = 0x2345
    colour = ["two", "four", "hundred", "hundred", "six", "zero", "zero", "zero"]
    sigma = ["one", "two", "zero", "minus_one", "one", "zero", "zero", "zero"]
    data[1, :, 0] = [H[c] for c in colour]
    data[1, :, 1] = [H[s] for s in sigma]
    data[2, :, 0] = [H["one"]] + [H["zero"]] * 7
    data[2, :, 1] = [H["one"]] * 3 + [H["zero"]] * 5
    return data, child


def test_hand_computed_two_level_tree():
    data, child = _two_level_tree()
    out, depth, counts = lod_ref.mip_rows(data, child)
    assert depth.tolist() == [1, 2, 2] and counts[1] == 1 and counts[2] == 2 and counts.sum() == 3
    # chunk 1: w = (1, 2, 0, 0, 1, 0, 0, 0), W = 4, sigma' = 4 / 8 = 0.5; S = 1*2 + 2*4 + 0*100 + 0*100 + 1*6 = 16, 16 / 4 = 4
    assert out[0, 0].tolist() == [H["four"], H["half"]]
    # chunk 2: W = 3, sigma' = 0.375; S = 1, float32(1 / 3) rounds to the binary16 0x3555
    assert out[0, 3].tolist() == [H["third"], H["three_eighths"]]
    # every other row is a leaf row: copied
    leaf = np.ones((3, 8), bool)
    leaf[0, 0] = leaf[0, 3] = False
    assert np.array_equal(out[leaf], data[leaf])


def test_eight_equal_children_mip_to_that_row():
    rng = np.random.default_rng(0)
    for _ in range(50):
        row = rng.uniform(-4, 4, size=6).astype(np.float16)
        row[5] = np.float16(rng.uniform(0.01, 60))   # sigma > 0
        rows = np.repeat(row.view(np.uint16)[None, None, :], 8, axis=1)
        assert np.array_equal(lod_ref.mip_parent_rows(rows)[0], row.view(np.uint16))


def test_empty_child_chunk_gives_a_zero_row():
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 0x7C00, size=(1, 8, 5), dtype=np.uint16)
    rows[0, :, 4] = [0x0000, 0x8000, 0xBC00, 0x7C00, 0x7E00, 0xFC00, 0x8001, 0x0000]   # nothing positive and finite
    assert lod_ref.mip_parent_rows(rows)[0].tolist() == [0] * 5


def test_special_halfs_read_as_the_contract_says():
    v = lod_ref.half_value(np.array([0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8000, 0x3C00], np.uint16))
    assert v[:3].tolist() == [0.0, 0.0, 0.0] and not np.signbit(v[:3]).any()
    assert v[3] == np.float32(2.0 ** -24) and v[4] == 0 and np.signbit(v[4]) and v[5] == 1


def _random_tree(seed, levels=5, dd=4):
    rng = np.random.default_rng(seed)
    child_rows, front, n = [np.zeros(8, np.int32)], [0], 1
    for _ in range(levels - 1):
        nxt = []
        for c in front:
            for j in range(8):
                if rng.uniform() < 0.3:
                    child_rows[c][j] = n - c
                    child_rows.append(np.zeros(8, np.int32))
                    nxt.append(n)
                    n += 1
        front = nxt
    child = np.stack(child_rows)
    data = rng.uniform(-2, 8, size=(n, 8, dd)).astype(np.float16).view(np.uint16)
    return data, child


def test_truncation_at_or_beyond_the_depth_keeps_child_and_leaf_rows():
    data, child = _random_tree(2)
    mipped, depth, counts = lod_ref.mip_rows(data, child)
    levels = int(depth.max())
    assert levels >= 3
    for d in (levels, levels + 1, 23, 1000):
        t = lod_ref.truncate(mipped, child, depth, d)
        assert t["capacity"] == child.shape[0] and np.array_equal(t["child"], child)
        assert np.array_equal(t["data"][child == 0], data[child == 0]) and np.array_equal(t["data"], mipped)
        assert t["parent"][0] == -1
        for c in range(1, child.shape[0]):
            p = t["parent"][c]
            assert p // 8 + child[p // 8, p % 8] == c


def test_truncation_at_depth_one_leaves_one_chunk_of_leaves():
    data, child = _random_tree(3)
    mipped, depth, _ = lod_ref.mip_rows(data, child)
    t = lod_ref.truncate(mipped, child, depth, 1)
    assert t["capacity"] == 1 and not t["child"].any() and t["parent"].tolist() == [-1]
    assert np.array_equal(t["data"][0], mipped[0])
    with pytest.raises(ValueError):
        lod_ref.truncate(mipped, child, depth, 0)


def test_truncation_in_between_links_the_survivors():
    data, child = _random_tree(4, levels=6)
    counts_in = np.arange(child.size, dtype=np.int16).reshape(-1, 8)
    mipped, depth, counts = lod_ref.mip_rows(data, child)
    for d in range(1, int(depth.max())):
        t = lod_ref.truncate(mipped, child, depth, d, counts_in)
        assert t["capacity"] == counts[1:d + 1].sum()
        again_depth, again_counts = lod_ref.chunk_depths(t["child"])   # an ordinary tree, every chunk reached, d levels
        assert again_depth.min() >= 1 and np.array_equal(again_counts[1:d + 1], counts[1:d + 1]) and again_counts[d + 1:].sum() == 0
        old = np.nonzero(depth <= d)[0]
        assert np.array_equal(t["data"], mipped[old]) and np.array_equal(t["sample_counts"], counts_in[old])


def test_the_walk_refuses_what_is_not_a_tree():
    data, child = _random_tree(5)
    leaf = np.argwhere(child[1:] == 0)[0]
    c, j = int(leaf[0]) + 1, int(leaf[1])
    for link in (-c, child.shape[0] - c, 1 - c if c != 1 else 2 - c):   # chunk 0, capacity, a chunk that already has a parent
        bad = child.copy()
        bad[c, j] = link
        with pytest.raises(ValueError, match="invalid"):
            lod_ref.chunk_depths(bad)
