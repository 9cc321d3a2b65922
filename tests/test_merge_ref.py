"""tests/merge_ref.py, the numpy restatement of the merge contract of include/mnv.h, held to properties that do not depend on it: what
merging with the empty tree must leave alone, what the canonical numbering means, what the two modes share, and tests/points_ref.py's
trees of a cloud and of its parts.  No GPU."""
import numpy as np
import pytest

import lod_ref
import merge_ref as mr
import points_ref as pr
from view_lod_cases import random_tree, renumbered, with_unreached

F = np.float32


def tree(seed, levels, dd, p=0.4):
    data, child = random_tree(seed, levels, dd, p)
    return dict(data=data, child=child)


def check_tree(t):
    """Breadth first, every chunk but the root linked once, parents consistent."""
    child, parent, cap = t["child"], t["parent"], t["capacity"]
    depth, counts = lod_ref.chunk_depths(child)
    assert (depth >= 1).all() and counts.sum() == cap and (np.diff(depth) >= 0).all()
    assert parent[0] == -1
    rows, cols = np.nonzero(child)
    target = rows + child[rows, cols]
    assert np.array_equal(np.sort(target), np.arange(1, cap)) and np.array_equal(parent[target], rows * 8 + cols)
    assert (np.diff(target) > 0).all()                       # ascending by (parent chunk, j)


def leaves(data, child):
    """{(depth, Morton code): row bytes} of every leaf voxel reached from the root: what a march can see of a tree."""
    out, front = {}, [(0, 1, 0)]
    while front:
        c, d, code = front.pop()
        for j in range(8):
            if child[c, j]:
                front.append((c + int(child[c, j]), d + 1, code * 8 + j))
            else:
                out[(d, code * 8 + j)] = data[c, j].tobytes()
    return out


@pytest.mark.parametrize("form", ["breadth_first", "renumbered", "unreached"])
def test_merging_with_the_empty_tree_is_the_same_tree_in_canonical_order(mnv, orc, form):
    """The result is isomorphic to A with A's rows, its oracle frame is A's bit for bit, and merging it again changes no byte."""
    data, child = random_tree(3, 5, 4, 0.4)
    if form == "renumbered":
        data, child = renumbered(data, child)
    if form == "unreached":
        data, child = with_unreached(data, child)
    a = dict(data=data, child=child)
    m = mr.merge(a, mr.empty_tree(4))
    check_tree(m)
    assert m["capacity"] == int((lod_ref.chunk_depths(child)[0] > 0).sum())
    assert mr.structure(m["child"]) == mr.structure(child) and leaves(m["data"], m["child"]) == leaves(data, child)
    assert m["stats"]["rows_from_a"] == 8 * m["capacity"] and m["stats"]["pushed_a"] == m["stats"]["rows_blended"] == 0
    assert m["stats"]["pushed_b"] == 8 * (m["capacity"] - 1)  # the empty tree's leaves cover everything below the root
    again = mr.merge(m, mr.empty_tree(4))
    for k in ("child", "data", "parent", "sample_counts"):
        assert np.array_equal(again[k], m[k]), k
    if form == "breadth_first":                               # random_tree numbers breadth first by (parent, j): already canonical
        assert np.array_equal(m["child"], child) and np.array_equal(m["data"], data)
    cam = mnv.orbit_camera(32, 24, 26.6, 2.6, 22.5, 20.0)
    opt = mnv.RenderOptions.cli_defaults()
    frames = []
    for d, c in ((data, child), (m["data"], m["child"])):
        t = mnv.N3Tree.from_arrays(d, c, data_format="RGBA")
        frames.append(orc.render(orc.tree_from_view(t.host_view()), cam.c, opt)["rgba"].view(np.uint32).copy())
    assert np.array_equal(frames[0], frames[1]) and (frames[0].view(np.float32)[..., 3] > 0).any()


@pytest.mark.parametrize("mode", [mr.OVER, mr.ADD])
def test_over_of_a_tree_with_itself_keeps_every_row(mode):
    a = tree(4, 5, 7)
    m = mr.merge(a, a, mode=mode)
    assert np.array_equal(m["child"], a["child"]) and m["stats"]["pushed_a"] == m["stats"]["pushed_b"] == 0
    assert np.array_equal(m["src_a"], m["src_b"]) and np.array_equal(m["src_a"], np.arange(m["capacity"] * 8).reshape(-1, 8))
    if mode == mr.OVER:
        assert np.array_equal(m["data"], a["data"])
    else:                                                     # the blend of a row with itself doubles sigma where sigma is positive
        sig = lod_ref.half_value(a["data"][..., 6])
        want = np.where(sig > 0, mr.sat_half((sig + sig).astype(F)), a["data"][..., 6])
        assert np.array_equal(m["data"][..., 6], want) and m["stats"]["rows_blended"] == int((sig > 0).sum()) > 0


def test_add_commutes_in_structure_and_in_blended_sigma():
    a, b = tree(5, 5, 4, 0.45), tree(6, 6, 4, 0.35)
    ab, ba = mr.merge(a, b, mode=mr.ADD), mr.merge(b, a, mode=mr.ADD)
    for k in ("child", "parent"):
        assert np.array_equal(ab[k], ba[k]), k
    assert np.array_equal(ab["src_a"], ba["src_b"]) and np.array_equal(ab["src_b"], ba["src_a"])
    assert ab["stats"]["rows_blended"] == ba["stats"]["rows_blended"] > 0 and ab["stats"]["pushed_a"] == ba["stats"]["pushed_b"] > 0
    _, _, kind = mr.rows(a["data"], b["data"], ab["src_a"], ab["src_b"], mr.ADD)
    blended = (kind == 2).reshape(-1, 8)
    assert np.array_equal(ab["data"][..., 3][blended], ba["data"][..., 3][blended])
    check_tree(ab)


CUBE = (np.array([0.5, 0.5, 0.5], F), np.array([1.0, 1.0, 1.0], F))


def dyadic_cloud(n, seed, bits=10):
    """Points k * 2^-bits - 0.5 (k integer): offset 0.5 + 1 * p and every 2^level multiple of it are exact in binary32."""
    rng = np.random.default_rng(seed)
    xyz = (rng.integers(0, 1 << bits, size=(n, 3)).astype(np.float64) / (1 << bits) - 0.5).astype(F)
    return xyz, rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def test_the_structure_of_two_clouds_merged_is_the_structure_of_their_union():
    (p1, c1), (p2, c2) = dyadic_cloud(300, 1), dyadic_cloud(500, 2)
    p2 = (p2 * F(0.5)).astype(F)                              # a denser middle
    t1, t2 = pr.build(p1, c1, CUBE[0], CUBE[1], 6), pr.build(p2, c2, CUBE[0], CUBE[1], 6)
    both = pr.build(np.concatenate([p1, p2]), np.concatenate([c1, c2]), CUBE[0], CUBE[1], 6)
    for mode in (mr.OVER, mr.ADD):
        m = mr.merge(t1, t2, mode=mode)
        assert np.array_equal(m["child"], both["child"]) and np.array_equal(m["parent"], both["parent"])
        assert m["stats"]["chunks_at_depth"] == both["stats"]["chunks_at_depth"]
    occupied = lod_ref.half_value(m["data"][..., 3]) > 0
    assert np.array_equal(occupied, both["counts"] > 0)


@pytest.mark.parametrize("fmt", ["RGBA", "SH4"])
def test_eight_octant_tiles_merged_are_the_tree_of_the_whole_cloud(fmt):
    """Eight trees of depth D - 1, each built from the whole cloud with the transform voxel_cube gives for its octant (so each keeps the
    points of its octant), merged one after the other at level 1 into the empty tree, equal the tree of the whole cloud at depth D byte for
    byte: links, parents, rows and sample counts.  The coordinates are dyadic (multiples of 2^-10 in [-0.5, 0.5)) and the cube is offset
    0.5, scale 1, so that every product and sum of the point-to-voxel map -- q = 0.5 + 1 * p for the whole, q' = (1 - c) + 2 * p for a
    tile -- is exact: a tile and the whole then put every point into the same voxel, which rounding would not promise."""
    D = 5
    xyz, rgb = dyadic_cloud(4000, 7)
    whole = pr.build(xyz, rgb, CUBE[0], CUBE[1], D, fmt, 1, 60.0)
    dd = pr.data_dim(fmt)
    merged = mr.empty_tree(dd)
    for j in range(8):
        corner = (j >> 2, (j >> 1) & 1, j & 1)
        offset, scale = mr.voxel_cube(CUBE[0], CUBE[1], 1, corner)
        assert np.array_equal(offset, F(1.0) - np.asarray(corner, F)) and np.array_equal(scale, np.full(3, 2.0, F))
        tile = pr.build(xyz, rgb, offset, scale, D - 1, fmt, 1, 60.0)
        assert 0 < tile["stats"]["accepted"] < 4000
        merged = mr.merge(merged, tile, level=1, corner=corner)
    assert merged["capacity"] == whole["capacity"]
    for k in ("child", "parent", "data", "sample_counts"):
        assert np.array_equal(merged[k], whole[k]), k


def test_placement_path_and_pushed_leaves():
    """B two levels down in a one-chunk A: the path forces two chunks, A's leaves are pushed down along it and under B."""
    a = dict(data=np.arange(8 * 4, dtype=np.uint16).reshape(1, 8, 4) + 0x3C00, child=np.zeros((1, 8), np.int32))
    b = tree(8, 3, 4, 0.5)
    m = mr.merge(a, b, level=2, corner=(3, 0, 2))
    check_tree(m)
    cap_b = b["child"].shape[0]
    assert m["capacity"] == 2 + cap_b and m["stats"]["chunks_at_depth"][1:4] == [1, 1, 1]
    j1, j2 = 4 * 1 + 0 + 1, 4 * 1 + 0 + 0                     # the bits of (3, 0, 2), most significant first
    assert m["child"][0, j1] == 1 and (m["child"][0] != 0).sum() == 1 and m["child"][1, j2] == 1
    assert (m["src_a"][1:] == j1).all() and (m["src_b"][:2] == -1).all()
    assert np.array_equal(m["src_b"][2:], np.arange(cap_b * 8).reshape(-1, 8)) and np.array_equal(m["child"][2:], b["child"])
    assert m["stats"]["pushed_a"] == 8 * (m["capacity"] - 1) and m["stats"]["pushed_b"] == 0
    empty_b = ~mr.pos(b["data"][..., 3])
    assert (m["data"][2:][empty_b] == a["data"][0, j1]).all()  # where B is empty, A's covering leaf shows


def test_the_restatement_refuses_what_the_entry_point_refuses():
    a = tree(9, 4, 4)
    with pytest.raises(ValueError, match="invalid"):
        mr.walk(a["child"], a["child"], 2, (4, 0, 0))
    with pytest.raises(ValueError, match="invalid"):
        mr.merge(a, tree(9, 4, 5))
    bad = a["child"].copy()
    bad[0, int(np.nonzero(bad[0])[0][0])] = bad.shape[0]
    with pytest.raises(ValueError, match="invalid"):
        mr.walk(bad, a["child"])
    def chain(n):
        links = np.zeros((n, 8), np.int32)
        links[:n - 1, 0] = 1
        return links

    cyc = np.zeros((3, 8), np.int32)
    cyc[0, 1], cyc[1, 2], cyc[2, 5] = 1, 1, -1                # chunk 2 links back to chunk 1
    with pytest.raises(ValueError, match="invalid|unsupported"):
        mr.walk(cyc, chain(2))
    assert mr.walk(chain(23), chain(2))["chunks_at_depth"][23] == 1 and mr.walk(chain(2), chain(22), 1, (1, 1, 1))["chunks_at_depth"][23] == 1
    with pytest.raises(ValueError, match="unsupported"):
        mr.walk(chain(2), chain(23), 1, (0, 0, 0))
