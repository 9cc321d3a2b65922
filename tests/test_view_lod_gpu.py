"""View-dependent levels of detail on the device (csrc/mnv_lod_view.hip: mnv_tree_select_cut, mnv_tree_cut; N3Tree.make_view_lod,
Renderer.set_view_lod, mnv_render --lod_pixels) against tests/view_lod_ref.py, the numpy restatement of the two contracts in include/mnv.h.
No tolerance anywhere: every comparison is on bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import lod_ref
import test_lod_gpu as L
import view_lod_ref as ref
from view_lod_cases import MIXED, TWO_VIEWS, chain, random_tree, renumbered, tie_chain, with_unreached

pytestmark = pytest.mark.gpu
W, H, EXE, POSES = L.W, L.H, L.EXE, L.POSES
GUARD = 64          # elements behind every output that must keep their pattern
HALF = (0.5, 0.5, 0.5)
ONE = (1.0, 1.0, 1.0)


# ---------------------------------------------------------------------------------------------------- device calls

def _view(mnv, data_t, child_t, dd, offset=HALF, scale=ONE, counts_t=None):
    v = L._view(mnv, data_t, child_t, dd, counts_t)
    for i in range(3):
        v.offset[i], v.scale[i] = offset[i], scale[i]
    return v


def _select(mnv, torch, child, offset, scale, views, pixels, min_depth, max_depth):
    """(keep, kept_at_depth) of mnv_tree_select_cut; the links must come back unchanged and nothing is written behind keep[capacity)."""
    cap = child.shape[0]
    data_t, child_t = torch.zeros((cap, 8, 8), dtype=torch.int16, device="cuda"), L._dev(torch, child)
    keep_t = torch.full((cap + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    kept = mnv.tree_select_cut(_view(mnv, data_t, child_t, 8, offset, scale), views, pixels, min_depth, max_depth, keep_t)
    keep = keep_t.cpu().numpy()
    assert (keep[cap:] == 0x55).all() and np.array_equal(child_t.cpu().numpy(), child)
    return keep[:cap], kept


def _check_select(mnv, torch, child, offset, scale, views, pixels, min_depth=1, max_depth=23):
    want, want_kept = ref.select_cut(child, offset, scale, views, pixels, min_depth, max_depth)
    keep, kept = _select(mnv, torch, child, offset, scale, views, pixels, min_depth, max_depth)
    assert np.array_equal(kept, want_kept), (kept, want_kept)
    bad = np.nonzero(keep != want)[0]
    assert bad.size == 0, (bad[:8], keep[bad[:8]], want[bad[:8]])
    return want, want_kept


# ---------------------------------------------------------------------------------------------------- mnv_tree_select_cut

@pytest.mark.parametrize("name", sorted(MIXED))
def test_select_cut_on_the_mixed_scenes(mnv, torch_gpu, name):
    case = MIXED[name]
    _, child = random_tree(*case["tree"])
    keep, kept = _check_select(mnv, torch_gpu, child, HALF, case["scale"], case["views"], case["pixels"], case["min_depth"])
    assert int(keep.sum()) == case["kept"] and [d for d in range(1, 24) if kept[d]][-1] == case["partial"][-1]


def test_select_cut_takes_the_union_over_views(mnv, torch_gpu):
    _, child = random_tree(*TWO_VIEWS["tree"])
    both, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, TWO_VIEWS["views"], TWO_VIEWS["pixels"])
    first, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, TWO_VIEWS["views"][:1], TWO_VIEWS["pixels"])
    assert (int(both.sum()), int(first.sum())) == (TWO_VIEWS["kept"], TWO_VIEWS["kept_first"])


@pytest.mark.parametrize("scale", [ONE, (0.5, 1.0, 2.0)])
def test_select_cut_when_only_the_last_of_64_views_passes(mnv, torch_gpu, scale):
    """More views than a wavefront has lanes; 63 eyes far away along x, then the one every kept chunk below min_depth is kept for."""
    _, child = random_tree(2, 7, 4, 0.35)
    last = ((-0.25, 0.125, 0.0), 64.0)
    views = [((400.0 + 3 * i, 0.0, 0.0), 64.0) for i in range(63)] + [last]
    keep, _ = _check_select(mnv, torch_gpu, child, HALF, scale, views, 8.0)
    far, _ = ref.select_cut(child, HALF, scale, views[:63], 8.0, 1, 23)
    alone, _ = ref.select_cut(child, HALF, scale, [last], 8.0, 1, 23)
    assert far.sum() == 1 and np.array_equal(keep, alone) and keep.sum() > 100


def test_select_cut_keeps_the_tie(mnv, torch_gpu):
    _, child, offset, scale, views, pixels = tie_chain()
    keep, kept = _check_select(mnv, torch_gpu, child, offset, scale, views, pixels)
    assert keep.tolist() == [1, 1, 1, 1, 0, 0] and kept[1:6].tolist() == [1, 1, 1, 1, 0]


def _voxel_above(child, n):
    """(integer corner, depth) of the voxel whose child chunk is n."""
    path = []
    while n != 0:
        c, j = np.argwhere((np.arange(child.shape[0])[:, None] + child == n) & (child != 0))[0]
        path.append(int(j))
        n = int(c)
    corner = np.zeros(3, np.int64)
    for j in reversed(path):
        corner = corner * 2 + np.array([j >> 2, (j >> 1) & 1, j & 1])
    return corner, len(path)


def test_select_cut_with_an_eye_inside_the_tree(mnv, torch_gpu):
    _, child = random_tree(3, 8, 4, 0.30)
    corner, d = _voxel_above(child, child.shape[0] - 1)                                         # a voxel of depth 7 above a chunk of leaves
    assert d == 7
    for scale in (ONE, (0.5, 1.0, 2.0)):
        eye = tuple(np.float32(x) for x in ((corner + 0.5) / 2.0 ** d - 0.5) / np.array(scale))  # its centre, in world space
        keep, kept = _check_select(mnv, torch_gpu, child, HALF, scale, [(eye, 48.0)], 12.0)
        assert 8 < keep.sum() < child.shape[0] and kept[8] > 0 and keep[-1] == 1                 # the leaves around the eye stay


def test_select_cut_without_a_threshold_and_with_one_depth(mnv, torch_gpu):
    _, child = random_tree(2, 7, 4, 0.35)
    depth, _ = lod_ref.chunk_depths(child)
    view = [((40.0, 0.0, 0.0), 64.0)]
    for max_depth in (1, 4, 7, 23):
        keep, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, view, 0.0, 1, max_depth)      # pixels 0: the depth predicate
        assert np.array_equal(keep != 0, depth <= max_depth)
    keep, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, view, 8.0, 3, 3)                  # min_depth == max_depth
    assert np.array_equal(keep != 0, depth <= 3)
    keep, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, view, 8.0, 2, 23)                 # a far eye: the floor alone
    assert np.array_equal(keep != 0, depth <= 2)


def test_select_cut_does_not_rely_on_chunk_order(mnv, torch_gpu):
    case = MIXED["anisotropic"]
    data, child = random_tree(*case["tree"])
    _, moved = renumbered(data, child)
    assert (moved[1:][moved[1:] != 0] < 0).all()
    keep, _ = _check_select(mnv, torch_gpu, moved, HALF, case["scale"], case["views"], case["pixels"])
    assert int(keep.sum()) == case["kept"]


def test_select_cut_leaves_unreached_chunks_out(mnv, torch_gpu):
    _, child = with_unreached(*random_tree(22, 5, 28))
    keep, kept = _check_select(mnv, torch_gpu, child, HALF, ONE, [((0.0, 0.0, 0.0), 64.0)], 0.0)
    assert keep[-3:].tolist() == [0, 0, 0] and keep[:-3].all() and kept.sum() == child.shape[0] - 3


def test_select_cut_of_a_single_chunk_and_of_a_chain_fourteen_deep(mnv, torch_gpu):
    _, child = random_tree(0, 1, 4)
    keep, kept = _check_select(mnv, torch_gpu, child, HALF, ONE, [((0.0, 0.0, 0.0), 64.0)], 1.0)
    assert keep.tolist() == [1] and kept.tolist() == [0, 1] + [0] * 22
    _, child = chain()
    keep, kept = _check_select(mnv, torch_gpu, child, HALF, ONE, [((9.0, 9.0, 9.0), 1.0)], 0.0)
    assert keep.all() and kept[1:15].tolist() == [1] * 14
    # the eye in the chain's deepest voxel: every voxel above it contains the eye, D2 == 0 on the whole way down
    corner = np.zeros(3, np.int64)
    for c in range(14):
        corner = corner * 2 + np.array([(c % 8) >> 2, ((c % 8) >> 1) & 1, (c % 8) & 1])
    eye = tuple((corner + 0.5) / 2.0 ** 14 - 0.5)
    keep, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, [(eye, 1e-3)], 1e6)
    assert keep.all()
    keep, _ = _check_select(mnv, torch_gpu, child, HALF, ONE, [((9.0, 9.0, 9.0), 1e-3)], 1e6)
    assert keep.sum() == 1


# ---------------------------------------------------------------------------------------------------- mnv_tree_cut

def _outputs(torch, n, dd, parent=True, counts=True):
    o = dict(child=torch.full((n + GUARD, 8), 0x55555555, dtype=torch.int32, device="cuda"),
             data=torch.full((n + GUARD, 8, dd), 0x5555, dtype=torch.int16, device="cuda"),
             parent=torch.full((n + GUARD,), 0x55555555, dtype=torch.int32, device="cuda") if parent else None,
             sample_counts=torch.full((n + GUARD, 8), 0x5555, dtype=torch.int16, device="cuda") if counts else None)
    return o


def _host(o, n):
    """(the first n chunks of every output, whether everything behind them kept its pattern)"""
    got, clean = {}, True
    for k, t in o.items():
        if t is None:
            continue
        a = t.cpu().numpy()
        a = a.view(np.uint16) if k == "data" else a
        got[k] = a[:n]
        clean = clean and bool((a[n:] == (0x5555 if a.dtype.itemsize == 2 else 0x55555555)).all())
    return got, clean


@pytest.mark.parametrize("dd", [4, 28, 76])
def test_cut_against_the_restatement(mnv, torch_gpu, dd):
    torch = torch_gpu
    data, child = random_tree(60 + dd, 6, dd, 0.45)
    cap = child.shape[0]
    assert 250 < cap < 1600
    sc = np.random.default_rng(7).integers(-100, 3000, size=(cap, 8)).astype(np.int16)
    keep, _ = ref.select_cut(child, HALF, ONE, MIXED["isotropic"]["views"], 8.0, 1, 23)
    want = ref.cut(data, child, keep, sc)
    n = want["capacity"]
    assert 8 < n < cap
    data_t, child_t, keep_t, sc_t = L._dev(torch, data), L._dev(torch, child), torch.from_numpy(keep).cuda(), L._dev(torch, sc)
    with_counts, without_counts = _view(mnv, data_t, child_t, dd, counts_t=sc_t), _view(mnv, data_t, child_t, dd)
    for variant in ("all", "no_parent", "no_counts", "neither", "view_without_counts"):
        o = _outputs(torch, n, dd, parent=variant not in ("no_parent", "neither"), counts=variant not in ("no_counts", "neither"))
        mnv.tree_cut(without_counts if variant == "view_without_counts" else with_counts, keep_t, n, o["child"], o["data"], o["parent"], o["sample_counts"])
        torch.cuda.synchronize()
        got, clean = _host(o, n)
        assert clean, variant                                # nothing at or beyond new_capacity
        for k, a in got.items():
            if k == "sample_counts" and variant == "view_without_counts":
                assert (a == 0x5555).all()                   # skipped: the input has none
            else:
                assert np.array_equal(a, want[k]), (variant, k)
    assert np.array_equal(L._host16(data_t), data) and np.array_equal(child_t.cpu().numpy(), child) and np.array_equal(keep_t.cpu().numpy(), keep)


@pytest.mark.parametrize("name", ["renumbered", "unreached"])
def test_cut_along_a_depth_is_truncate(mnv, torch_gpu, name):
    torch = torch_gpu
    data, child = renumbered(*random_tree(50, 6, 13)) if name == "renumbered" else with_unreached(*random_tree(51, 5, 5))
    cap, _, dd = data.shape
    sc = np.random.default_rng(8).integers(-100, 3000, size=(cap, 8)).astype(np.int16)
    depth, counts = lod_ref.chunk_depths(child)
    data_t, child_t, depth_t, sc_t = L._dev(torch, data), L._dev(torch, child), L._dev(torch, depth), L._dev(torch, sc)
    view = _view(mnv, data_t, child_t, dd, counts_t=sc_t)
    for d in range(1, int(depth.max()) + 2):
        keep = ((depth >= 1) & (depth <= d)).astype(np.uint8)
        n = int(keep.sum())
        a, b = _outputs(torch, n, dd), _outputs(torch, n, dd)
        mnv.tree_truncate(view, depth_t, d, n, a["child"], a["data"], a["parent"], a["sample_counts"])
        mnv.tree_cut(view, torch.from_numpy(keep).cuda(), n, b["child"], b["data"], b["parent"], b["sample_counts"])
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (d, k)           # guard regions included
        want = ref.cut(data, child, keep, sc)
        got, _ = _host(b, n)
        for k in got:
            assert np.array_equal(got[k], want[k]), (d, k)


# ---------------------------------------------------------------------------------------------------- refusals

def test_select_cut_and_cut_refuse_what_the_contract_lists(mnv, torch_gpu):
    torch = torch_gpu
    lib = mnv.lib()
    data, child = random_tree(41, 5, 4, 0.5)
    cap = child.shape[0]
    assert cap > 100
    data_t, child_t = L._dev(torch, data), L._dev(torch, child)
    keep_t = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
    kept = (C.c_int64 * 24)()
    good = mnv.lod_views([((0.0, 0.0, 0.0), 64.0), ((1.0, 2.0, 3.0), 32.0)])

    def select(v=None, views=good, n=None, pixels=1.0, lo=1, hi=23, keep=keep_t.data_ptr(), counts=kept):
        v = _view(mnv, data_t, child_t, 4) if v is None else v
        table = None if views is None else np.ascontiguousarray(views, np.float32)
        return lib.mnv_tree_select_cut(C.byref(v) if v != "null" else None, None if table is None else table.ctypes.data,
                                       (0 if table is None else table.shape[0]) if n is None else n, pixels, lo, hi, keep, counts, None)

    assert select() == 0
    for kw in (dict(v="null"), dict(views=None, n=1), dict(keep=None), dict(counts=None),                 # a null argument
               dict(n=0), dict(views=np.zeros((4097, 4), np.float32) + 1, n=4097),                        # n_views outside [1, 4096]
               dict(pixels=-1.0), dict(pixels=float("nan")), dict(pixels=float("inf")),
               dict(lo=0), dict(lo=3, hi=2)):
        assert select(**kw) == mnv.MNV_E_INVALID, kw
    for i, bad in ((0, float("nan")), (1, float("inf")), (2, float("-inf")), (3, float("nan")), (3, float("inf")), (3, 0.0), (3, -64.0)):
        views = good.copy()
        views[1, i] = bad                                                                                 # an eye / a focal length
        assert select(views=views) == mnv.MNV_E_INVALID, (i, bad)
    for k, bad in ((0, 0.0), (1, -1.0), (2, float("inf")), (0, float("nan"))):
        v = _view(mnv, data_t, child_t, 4)
        v.scale[k] = bad
        assert select(v=v) == mnv.MNV_E_INVALID, (k, bad)
    v = _view(mnv, data_t, child_t, 4)
    v.N = 3
    assert select(v=v) == mnv.MNV_E_UNSUPPORTED
    host_child = np.ascontiguousarray(child)
    v = _view(mnv, data_t, child_t, 4)
    v.child = host_child.ctypes.data                                                                      # host arrays in the view
    assert select(v=v) == mnv.MNV_E_INVALID
    # links the walk follows: chunk 0, capacity, a chunk that has a parent already -- refused where the voxel refines, not where it does not
    leaf = np.argwhere(child[2:] == 0)[0]
    c, j = int(leaf[0]) + 2, int(leaf[1])
    for link in (-c, cap - c, 1 - c):
        bad = child.copy()
        bad[c, j] = link
        bad_t = L._dev(torch, bad)
        v = _view(mnv, data_t, bad_t, 4)
        assert select(v=v, pixels=0.0) == mnv.MNV_E_INVALID, link
        with pytest.raises(ValueError, match="invalid"):
            ref.select_cut(bad, HALF, ONE, [((0.0, 0.0, 0.0), 64.0)], 0.0, 1, 23)
        assert select(v=v, pixels=0.0, hi=1) == 0                                                        # the walk never meets the link
    deep = chain(levels=24)[1]
    deep_t = L._dev(torch, deep)
    v = _view(mnv, torch.zeros((24, 8, 4), dtype=torch.int16, device="cuda"), deep_t, 4)
    deep_keep = torch.zeros((24,), dtype=torch.uint8, device="cuda")
    assert select(v=v, pixels=0.0, hi=24, keep=deep_keep.data_ptr()) == mnv.MNV_E_UNSUPPORTED              # more than 23 levels
    assert select(v=v, pixels=0.0, hi=23, keep=deep_keep.data_ptr()) == 0 and deep_keep.cpu().numpy().tolist() == [1] * 23 + [0]

    # mnv_tree_cut
    v = _view(mnv, data_t, child_t, 4)
    o_child = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    o_data = torch.zeros((cap * 8 * 4 + 8,), dtype=torch.int16, device="cuda")
    ones = torch.ones((cap,), dtype=torch.uint8, device="cuda")

    def cut(view=v, keep=ones.data_ptr(), n=cap, links=o_child.data_ptr(), rows=o_data.data_ptr()):
        return lib.mnv_tree_cut(C.byref(view) if view is not None else None, keep, n, links, rows, None, None, None)

    assert cut() == 0
    rootless = ones.clone()
    rootless[0] = 0
    for kw in (dict(view=None), dict(keep=None), dict(links=None), dict(rows=None), dict(keep=rootless.data_ptr()), dict(n=0), dict(n=cap + 1),
               dict(rows=o_data.data_ptr() + 2), dict(keep=np.ones(cap, np.uint8).ctypes.data)):
        assert cut(**kw) == mnv.MNV_E_INVALID, kw
    v3 = _view(mnv, data_t, child_t, 4)
    v3.N = 3
    assert cut(view=v3) == mnv.MNV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(L._host16(data_t), data) and np.array_equal(child_t.cpu().numpy(), child)


# ---------------------------------------------------------------------------------------------------- frames

EYE, BACK, FX = POSES[0][0], POSES[0][1], 224.0


def _march(mnv, torch, tree, cam, opt, packed=True):
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    if packed:
        mnv.render_voxels_accel(tree.accel, cam, opt, rgba=out)
    else:
        mnv.render_voxels(tree.device_view(), cam, opt, rgba=out)
    torch.cuda.synchronize()
    return cases.bits(out.cpu().numpy()).copy()


@pytest.mark.parametrize("fmt,depth,pixels", [("SH1", 5, 16.0), ("SH9", 6, 4.0), ("RGBA", 5, 12.0)])
def test_frames_of_the_view_cut_three_ways(mnv, orc, torch_gpu, fmt, depth, pixels):
    torch = torch_gpu
    if fmt == "RGBA":
        tree = mnv.N3Tree.synth_random(depth=depth, basis_dim=-1, fmt=mnv.FORMAT_RGBA, seed=depth)
    else:
        tree = mnv.N3Tree.synth_random(depth=depth, basis_dim=int(fmt[2:]), seed=depth)
    data, child, _ = tree.host_arrays()
    hv = tree.host_view()
    views = [(EYE, FX)]
    want = ref.make_view_lod(data, child, tuple(hv.offset), tuple(hv.scale), views, pixels)
    chunk_depth, _ = lod_ref.chunk_depths(child)
    assert int((chunk_depth <= 1).sum()) < want["capacity"] < child.shape[0]
    tree.move_to_device(need_parent=True, need_sample_counts=True)
    cut, kept = tree.make_view_lod(views, pixels, return_counts=True)
    assert np.array_equal(kept, want["kept_at_depth"]) and cut.capacity == want["capacity"] and cut.data_format == tree.data_format
    got_data, got_child, got_parent = cut.host_arrays()
    assert np.array_equal(got_child, want["child"]) and np.array_equal(got_data, want["data"]) and np.array_equal(got_parent, want["parent"])
    cv = cut.host_view()
    assert list(cv.offset) == list(hv.offset) and list(cv.scale) == list(hv.scale)
    cam = mnv.Camera(W, H, FX).set_pose(EYE, BACK)
    opt = mnv.RenderOptions.cli_defaults()
    if hv.basis_dim > 0:
        opt.basis_minmax[0], opt.basis_minmax[1] = 0, hv.basis_dim - 1
    host = mnv.N3Tree.from_arrays(want["data"], want["child"], data_format=tree.data_format, offset=tuple(hv.offset), scale=tuple(hv.scale))
    oracle = cases.bits(orc.render(orc.tree_from_view(host.host_view()), cam.c, opt)["rgba"])
    assert np.array_equal(_march(mnv, torch, cut, cam, opt), oracle)
    assert np.array_equal(_march(mnv, torch, cut, cam, opt, packed=False), oracle)
    full = _march(mnv, torch, tree, cam, opt)
    assert not np.array_equal(full, oracle)                                    # the cut is visible
    # no threshold and no depth limit: the whole tree, and interior rows are never seen
    whole = tree.make_view_lod(views, 0.0, 1, depth)
    assert whole.capacity == tree.capacity
    assert np.array_equal(_march(mnv, torch, whole, cam, opt), full)
    assert np.array_equal(_march(mnv, torch, whole, cam, opt, packed=False), full)
    assert np.array_equal(_march(mnv, torch, tree, cam, opt), full)            # ... and the source tree is what it was


# ---------------------------------------------------------------------------------------------------- Renderer.set_view_lod

VIEWS = [(c, FX) for c, _ in POSES] + [(L.ORTHO_POSE[0], 18.0)]
PIXELS = 8.0


def test_renderer_with_a_view_cut_equals_a_renderer_of_the_cut_tree(mnv, torch_gpu):
    spec = cases.CASES["sh4_d6"]["tree"]
    tree, source = cases.make_tree(mnv, spec), cases.make_tree(mnv, spec)
    source.move_to_device()
    cut = source.make_view_lod(VIEWS, PIXELS)
    assert 300 < cut.capacity < tree.capacity
    a = L._renderer(mnv, tree, tree.capacity)
    b = L._renderer(mnv, cut, cut.capacity)
    before = L._walk(mnv, a, 3)
    a.set_view_lod(VIEWS, PIXELS)
    for in_flight in (3, 1):
        got, want = L._walk(mnv, a, in_flight), L._walk(mnv, b, in_flight)
        assert len(got) == len(want) == len(POSES) + 4
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (in_flight, i)
    assert not all(np.array_equal(x, y) for x, y in zip(got, before))
    # other parameters: another tree, grid included
    coarse = source.make_view_lod(VIEWS[:1], 16.0, 2, 5)
    assert coarse.capacity < cut.capacity
    c = L._renderer(mnv, coarse, coarse.capacity)
    a.set_view_lod(VIEWS[:1], 16.0, 2, 5)
    for i, (g, w) in enumerate(zip(L._walk(mnv, a, 3), L._walk(mnv, c, 3))):
        assert np.array_equal(g, w), i
    a.set_view_lod([])                                                          # off: byte for byte what it was
    after = L._walk(mnv, a, 3)
    for i, (x, y) in enumerate(zip(after, before)):
        assert np.array_equal(x, y), i
    # a new tree drops the cut one: the same views now cut the new tree
    other = mnv.N3Tree.synth_random(depth=6, basis_dim=4, seed=77)
    other_source = mnv.N3Tree.synth_random(depth=6, basis_dim=4, seed=77)
    other_source.move_to_device()
    other_cut = other_source.make_view_lod(VIEWS, PIXELS)
    a.set_view_lod(VIEWS, PIXELS)
    a.set(other, other.capacity)
    d = L._renderer(mnv, other_cut, other_cut.capacity)
    for r in (a, d):
        r.options.basis_minmax[0], r.options.basis_minmax[1] = 0, 3
        r.set_camera(*POSES[0], fx=FX)
        r.render()
    assert np.array_equal(cases.bits(a.download_slot(a.last_slot())), cases.bits(d.download_slot(d.last_slot())))


def test_renderer_refuses_a_view_cut_with_what_edits_the_tree_or_cuts_it_twice(mnv, torch_gpu):
    tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    r = L._renderer(mnv, tree, tree.capacity)
    r.set_camera(*POSES[0], fx=FX)
    r.set_view_lod(VIEWS, PIXELS)
    r.render()
    good = cases.bits(r.download_slot(r.last_slot())).copy()

    def refused(word):
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == mnv.MNV_E_INVALID and word in str(e.value)

    r.options.use_splitting = True
    refused("set_view_lod")
    r.options.use_splitting = False
    r.options.use_guided_sampling = True
    refused("set_view_lod")
    r.options.use_guided_sampling = False
    r.set_lod(3)
    refused("set_view_lod")
    r.set_lod(0)
    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)         # one rank through RCCL
    try:
        r.set_ranks(comm)
        refused("set_view_lod")
        r.set_ranks(None)
    finally:
        r.set_ranks(None)
        comm.close()
    for bad in (dict(pixels=-1.0), dict(pixels=float("nan")), dict(min_depth=0), dict(min_depth=4, max_depth=3),
                dict(views=[((0.0, float("inf"), 0.0), FX)]), dict(views=[((0.0, 0.0, 0.0), 0.0)]), dict(views=[((0.0, 0.0, 0.0), 1.0)] * 4097)):
        args = dict(views=VIEWS, pixels=PIXELS, min_depth=1, max_depth=23)
        args.update(bad)
        with pytest.raises(mnv.MnvError) as e:
            r.set_view_lod(**args)
        assert e.value.code == mnv.MNV_E_INVALID, bad
    r.render()                                               # the same call renders once the obstacle is gone; refused settings changed nothing
    assert np.array_equal(cases.bits(r.download_slot(r.last_slot())), good)
    host_only = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    with pytest.raises(mnv.MnvError) as e:
        host_only.make_view_lod(VIEWS, PIXELS)               # not on the device
    assert e.value.code == mnv.MNV_E_INVALID


# ---------------------------------------------------------------------------------------------------- mnv_render --lod_pixels

def test_mnv_render_lod_pixels_orbit_and_save_lod(mnv, torch_gpu, tmp_path):
    """One pose: the saved tree and the frame are make_view_lod's for that eye.  An orbit: the poses are the CLI's own, so the saved tree is
    checked through what it must do -- reload, and render the frames the run wrote, pose for pose -- and through the counts the run printed."""
    torch = torch_gpu
    assert os.path.exists(EXE), "mnv_render not built"
    tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    npz, saved, out = str(tmp_path / "scene.npz"), str(tmp_path / "cut.npz"), str(tmp_path / "frame")
    tree.save_npz(npz)
    pose = ["-w", str(W), "-h", str(H), "--fx", "224", "--center", ",".join(map(str, EYE)), "--back", ",".join(map(str, BACK))]
    common = [EXE, npz] + pose

    def run(cmd):
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120)

    r = run(common + ["--out", out, "--raw", "--frames", "1", "--lod_pixels", "8", "--save_lod", saved])
    assert r.returncode == 0, r.stderr + r.stdout
    tree.move_to_device()
    cut, kept = tree.make_view_lod([(EYE, FX)], 8.0, return_counts=True)
    assert 8 < cut.capacity < tree.capacity
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("lod_pixels:")]
    assert len(line) == 1 and line[0].split("kept per depth:")[1].split() == [str(int(k)) for k in kept[1:] if k]
    back_in = mnv.N3Tree.open(saved)
    for x, y in zip(back_in.host_arrays(), cut.host_arrays()):
        assert np.array_equal(x, y)
    assert back_in.data_format == cut.data_format and list(back_in.host_view().scale) == list(cut.host_view().scale)
    cam = mnv.Camera(W, H, FX).set_pose(EYE, BACK)
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, 3
    got = np.fromfile(out + "_0000.f32", dtype=np.float32).reshape(H, W, 4)
    assert np.array_equal(cases.bits(got), _march(mnv, torch, cut, cam, opt))

    orbit_saved, orbit_out, again = str(tmp_path / "orbit.npz"), str(tmp_path / "orbit"), str(tmp_path / "again")
    r = run(common + ["--out", orbit_out, "--raw", "--frames", "4", "--orbit", "60", "--lod_pixels", "8", "--lod_min", "2", "--lod_max", "6", "--save_lod", orbit_saved])
    assert r.returncode == 0, r.stderr + r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("lod_pixels:")]
    assert len(line) == 1 and "4 view(s)" in line[0]
    counts = [int(x) for x in line[0].split("kept per depth:")[1].split()]
    orbit_tree = mnv.N3Tree.open(orbit_saved)
    depth, at_depth = lod_ref.chunk_depths(orbit_tree.host_arrays()[1])
    assert at_depth[1:len(counts) + 1].tolist() == counts and at_depth.sum() == orbit_tree.capacity == sum(counts)
    assert cut.capacity < orbit_tree.capacity < tree.capacity                  # four eyes keep more than the first of them alone
    r = run([EXE, orbit_saved] + pose + ["--out", again, "--raw", "--frames", "4", "--orbit", "60"])
    assert r.returncode == 0, r.stderr + r.stdout
    for f in range(4):
        a, b = np.fromfile(f"{orbit_out}_{f:04d}.f32", dtype=np.uint32), np.fromfile(f"{again}_{f:04d}.f32", dtype=np.uint32)
        assert a.size == W * H * 4 and np.array_equal(a, b), f

    for extra in (["--lod", "4"], ["--gpus", "1"], ["--use_splitting"], ["--use_guided_sampling"]):
        bad = run(common + ["--lod_pixels", "8"] + extra)
        assert bad.returncode != 0 and "--lod_pixels" in bad.stderr, extra
    for extra in (["--lod_min", "2"], ["--lod_pixels", "-1"], ["--lod_pixels", "8", "--lod_min", "5", "--lod_max", "4"]):
        bad = run(common + extra)
        assert bad.returncode != 0 and "--lod_pixels" in bad.stderr, extra
