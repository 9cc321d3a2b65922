"""tests/view_lod_ref.py, the numpy restatement of mnv_tree_select_cut / mnv_tree_cut, against identities it must satisfy, a tie computed by
hand and the conditions every "mixed cut" scene of tests/test_view_lod_gpu.py has to meet.  No device, no tolerance."""
import numpy as np
import pytest

import lod_ref
import view_lod_ref as ref
from view_lod_cases import MIXED, TWO_VIEWS, random_tree, tie_chain

f32 = np.float32


def parent_closed(child, keep):
    """Every kept chunk but the root is the child of a voxel of a kept chunk."""
    child = np.asarray(child, np.int64).reshape(-1, 8)
    rows, cols = np.nonzero(child)
    target = rows + child[rows, cols]
    above = np.full(child.shape[0], -1, np.int64)
    above[target] = rows
    kept = np.nonzero(keep)[0]
    return bool(keep[0]) and all(above[c] >= 0 and keep[above[c]] for c in kept if c != 0)


def partial_depths(depth, keep):
    """The depths at which some but not all chunks are kept."""
    return [d for d in range(1, int(depth.max()) + 1) if 0 < int(keep[depth == d].sum()) < int((depth == d).sum())]


@pytest.mark.parametrize("max_depth", [1, 3, 5, 7, 23])
def test_zero_pixels_is_the_depth_predicate_and_cut_is_truncate(max_depth):
    data, child = random_tree(2, 7, 4, 0.35)
    depth, counts = lod_ref.chunk_depths(child)
    keep, kept = ref.select_cut(child, (0.5,) * 3, (1.0,) * 3, [((9.0, -4.0, 2.0), 10.0)], 0.0, 1, max_depth)
    assert np.array_equal(keep != 0, (depth >= 1) & (depth <= max_depth))
    assert np.array_equal(kept[1:], np.where(np.arange(1, 24) <= max_depth, counts[1:], 0))
    assert parent_closed(child, keep)
    sc = np.random.default_rng(1).integers(-9, 900, size=child.shape).astype(np.int16)
    a, b = ref.cut(data, child, keep, sc), lod_ref.truncate(data, child, depth, max_depth, sc)
    assert a["capacity"] == b["capacity"]
    for k in ("child", "data", "parent", "sample_counts"):
        assert np.array_equal(a[k], b[k]), k


def test_a_far_eye_keeps_exactly_the_minimum_depth():
    _, child = random_tree(2, 7, 4, 0.35)
    depth, _ = lod_ref.chunk_depths(child)
    keep, kept = ref.select_cut(child, (0.5,) * 3, (1.0,) * 3, [((40.0, 0.0, 0.0), 64.0)], 8.0, 2, 23)
    assert np.array_equal(keep != 0, (depth >= 1) & (depth <= 2)) and kept[3:].sum() == 0 and parent_closed(child, keep)


def test_the_tie_refines():
    """Offset 0, scale 1, eye (0.5, 0, 0), focal_px / pixels == 1.  The chain's voxel of depth 3 is [0.625, 0.75] x [0, 0.125]^2: its gap
    to the eye is 0.125 along x and 0 along y and z, so D2 = 2^-6, and R2[3] = ((4 * 2^-3) / 4)^2 = 2^-6: equal.  `<=` keeps the chunk
    of depth 4 under it, `<` would not.  One level down the gap is still 0.125 and R is 2^-4: the chunk of depth 5 goes."""
    _, child, offset, scale, views, pixels = tie_chain()
    q, R2 = ref.view_tables(offset, scale, views, pixels)
    assert q[0].tolist() == [0.5, 0.0, 0.0] and R2[0, 3] == f32(2.0 ** -6) and R2[0, 4] == f32(2.0 ** -8)
    ix = np.array([[5, 0, 0]], np.int64)
    lo = ix.astype(f32) * f32(0.125)
    g = np.maximum(np.maximum(lo - q[0], q[0] - (lo + f32(0.125))), f32(0))
    D2 = (g[0, 0] * g[0, 0] + g[0, 1] * g[0, 1]) + g[0, 2] * g[0, 2]
    assert D2 == R2[0, 3]                                   # the tie really occurs
    assert ref.refines(ix, 3, q, R2, scale).tolist() == [True]
    assert ref.refines(ix, 3, q, np.nextafter(R2, f32(0)), scale).tolist() == [False]
    keep, kept = ref.select_cut(child, offset, scale, views, pixels, 1, 23)
    assert keep.tolist() == [1, 1, 1, 1, 0, 0] and kept[1:6].tolist() == [1, 1, 1, 1, 0]
    assert parent_closed(child, keep)


@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_cuts_are_mixed(name):
    case = MIXED[name]
    _, child = random_tree(*case["tree"])
    depth, _ = lod_ref.chunk_depths(child)
    keep, kept = ref.select_cut(child, (0.5,) * 3, case["scale"], case["views"], case["pixels"], case["min_depth"], 23)
    n, floor = int(keep.sum()), int((depth <= case["min_depth"]).sum())
    partial = partial_depths(depth, keep)
    print(name, "kept", n, "of", child.shape[0], "floor", floor, "partial depths", partial)
    assert child.shape[0] == case["total"]
    assert floor < n < child.shape[0] and len(partial) >= 3
    assert parent_closed(child, keep) and kept.sum() == n
    assert n == case["kept"] and partial == case["partial"]      # the counts this restatement gives (the conditions above are the claim)


def test_a_second_view_adds_chunks():
    _, child = random_tree(2, 7, 4, 0.35)
    both, _ = ref.select_cut(child, (0.5,) * 3, (1.0,) * 3, TWO_VIEWS["views"], TWO_VIEWS["pixels"], 1, 23)
    first, _ = ref.select_cut(child, (0.5,) * 3, (1.0,) * 3, TWO_VIEWS["views"][:1], TWO_VIEWS["pixels"], 1, 23)
    second, _ = ref.select_cut(child, (0.5,) * 3, (1.0,) * 3, TWO_VIEWS["views"][1:], TWO_VIEWS["pixels"], 1, 23)
    print("two views", int(both.sum()), "first alone", int(first.sum()), "second alone", int(second.sum()))
    assert np.array_equal(both, first | second)             # "some view": the union (a chunk's ancestors pass for the same view)
    assert both.sum() > first.sum() and both.sum() > second.sum()
    assert (int(both.sum()), int(first.sum())) == (TWO_VIEWS["kept"], TWO_VIEWS["kept_first"])
    assert parent_closed(child, both)


def test_the_restatement_refuses_what_the_entry_point_refuses():
    _, child = random_tree(2, 5, 4, 0.35)
    view = [((0.0, 0.0, 0.0), 64.0)]
    for kw in (dict(min_depth=0), dict(max_depth=1, min_depth=2), dict(pixels=-1.0), dict(pixels=float("nan")), dict(views=[]),
               dict(views=[((0.0, float("inf"), 0.0), 64.0)]), dict(views=[((0.0, 0.0, 0.0), 0.0)]), dict(scale=(1.0, 0.0, 1.0))):
        args = dict(offset=(0.5,) * 3, scale=(1.0,) * 3, views=view, pixels=1.0, min_depth=1, max_depth=23)
        args.update(kw)
        with pytest.raises(ValueError, match="invalid"):
            ref.select_cut(child, **args)
    bad = child.copy()
    bad[0, np.nonzero(child[0])[0][0]] = child.shape[0]
    with pytest.raises(ValueError, match="leaves the tree"):
        ref.select_cut(bad, (0.5,) * 3, (1.0,) * 3, view, 0.0, 1, 23)
    keep = np.ones(child.shape[0], np.uint8)
    keep[0] = 0
    with pytest.raises(ValueError, match="root"):
        ref.cut(np.zeros(child.shape + (4,), np.uint16), child, keep)
