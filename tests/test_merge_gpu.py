"""Merging two trees on the device (csrc/mnv_merge.hip: mnv_tree_merge_plan / write; N3Tree.merge, mnv_render --merge) against
tests/merge_ref.py, the numpy restatement of the contract in include/mnv.h.  No tolerance anywhere: the six arrays and the stats are
compared byte for byte, frames bit for bit.  Every output has 64 guard elements behind it that must keep their pattern, and the inputs
must come back unchanged."""
import os
import subprocess

import numpy as np
import pytest

import cases
import merge_ref as mr
import points_ref as pr
from view_lod_cases import random_tree, renumbered, with_unreached

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")
W, H = 64, 48
GUARD = 64
F = np.float32
KEYS = ("child", "data", "parent", "sample_counts", "src_a", "src_b")


# ---------------------------------------------------------------------------------------------------- trees

def tree(seed, levels, dd, p=0.4, counts=False):
    data, child = random_tree(seed, levels, dd, p)
    t = dict(data=data, child=child)
    if counts:
        t["sample_counts"] = np.random.default_rng(seed + 1000).integers(-20000, 30000, size=child.shape).astype(np.int16)
    return t


def one_chunk(dd, seed=0, sigma=None):
    """A root chunk of eight leaves with random finite rows (sigma: all eight sigma halfs)."""
    rng = np.random.default_rng(seed)
    data = rng.uniform(0.1, 9, size=(1, 8, dd)).astype(np.float16).view(np.uint16)
    if sigma is not None:
        data[..., dd - 1] = sigma
    return dict(data=np.ascontiguousarray(data), child=np.zeros((1, 8), np.int32))


def chain(n, dd=4):
    """n chunks, chunk c's voxel c % 8 leads to chunk c + 1: the deepest voxels have depth n."""
    child = np.zeros((n, 8), np.int32)
    for c in range(n - 1):
        child[c, c % 8] = 1
    data = np.random.default_rng(n).uniform(0.1, 9, size=(n, 8, dd)).astype(np.float16).view(np.uint16)
    return dict(data=np.ascontiguousarray(data), child=child)


def trimmed(t, n):
    """The tree with all but the first n links into its first level of more than n chunks cut (what hung under them is left unreached):
    that level then has exactly n chunks."""
    import lod_ref

    depth, at = lod_ref.chunk_depths(t["child"])
    d = int(np.nonzero(at > n)[0][0])
    child = t["child"].copy()
    rows, cols = np.nonzero(np.where((depth == d - 1)[:, None], child, 0))
    child[rows[n:], cols[n:]] = 0
    assert lod_ref.chunk_depths(child)[1][d] == n
    return dict(t, child=child)


# ---------------------------------------------------------------------------------------------------- device calls

def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _upload(mnv, torch, t):
    """(device tensors, view) of a tree dict"""
    dev = {k: _dev(torch, t[k]) for k in ("data", "child", "sample_counts") if t.get(k) is not None}
    v = mnv.TreeView()
    v.data, v.child = dev["data"].data_ptr(), dev["child"].data_ptr()
    v.sample_counts = dev["sample_counts"].data_ptr() if "sample_counts" in dev else None
    for i in range(3):
        v.offset[i] = v.scale[i] = 0.5
    v.N, v.data_dim, v.format, v.basis_dim, v.capacity = 2, t["data"].shape[-1], mnv.FORMAT_RGBA, -1, t["child"].shape[0]
    return dev, v


def _unchanged(dev, t):
    for k, x in dev.items():
        got = x.cpu().numpy()
        assert np.array_equal(got.view(np.uint16) if k == "data" else got, t[k]), k


def _outputs(torch, cap, dd, nulls=()):
    shapes = dict(child=((cap + GUARD, 8), torch.int32), data=((cap + GUARD, 8, dd), torch.int16), parent=((cap + GUARD,), torch.int32),
                  sample_counts=((cap + GUARD, 8), torch.int16), src_a=((cap + GUARD, 8), torch.int32), src_b=((cap + GUARD, 8), torch.int32))
    return {k: None if k in nulls else torch.full(s, 0x5555 if dt == torch.int16 else 0x55555555, dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}


def _write(torch, plan, out, stream=0):
    plan.write(out["child"], out["data"], out["parent"], out["sample_counts"], out["src_a"], out["src_b"], stream=stream)


def _host(out, cap):
    """the first cap chunks of every output; everything behind them must have kept its pattern"""
    got = {}
    for k, x in out.items():
        if x is None:
            continue
        a = x.cpu().numpy()
        a = a.view(np.uint16) if k == "data" else a
        assert (a[cap:] == (0x5555 if a.dtype.itemsize == 2 else 0x55555555)).all(), k
        got[k] = a[:cap]
    return got


def _merge(mnv, torch, a, b, level=0, corner=(0, 0, 0), mode="over", nulls=()):
    dev_a, va = _upload(mnv, torch, a)
    dev_b, vb = _upload(mnv, torch, b)
    torch.cuda.synchronize()
    plan = mnv.TreeMerge(va, vb, level, corner, mode)
    cap = int(plan.stats.capacity)
    out = _outputs(torch, cap, a["data"].shape[-1], nulls)
    torch.cuda.synchronize()
    _write(torch, plan, out)
    torch.cuda.synchronize()
    got = _host(out, cap)
    got["stats"] = plan.stats.as_dict()
    _unchanged(dev_a, a)
    _unchanged(dev_b, b)
    return got


def _same(got, ref, nulls=()):
    assert got["stats"] == ref["stats"], (got["stats"], ref["stats"])
    for k in KEYS:
        if k in nulls:
            assert k not in got
            continue
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (k, got[k].shape, ref[k].shape, got[k].dtype, ref[k].dtype)
        bad = np.argwhere(got[k] != ref[k])
        assert bad.size == 0, (k, bad[:5], got[k][tuple(bad[0])], ref[k][tuple(bad[0])])


def _check(mnv, torch, a, b, level=0, corner=(0, 0, 0), mode="over", nulls=()):
    ref = mr.merge(a, b, level, corner, mr.ADD if mode == "add" else mr.OVER)
    _same(_merge(mnv, torch, a, b, level, corner, mode, nulls), ref, nulls)
    return ref


# ---------------------------------------------------------------------------------------------------- structure

@pytest.mark.parametrize("mode", ["over", "add"])
def test_interior_over_leaf_leaf_over_interior_and_both_interior(mnv, torch_gpu, mode):
    big, other, leaf = tree(21, 4, 4, 0.5), tree(22, 5, 4, 0.35), one_chunk(4, 1)
    ref = _check(mnv, torch_gpu, big, leaf, mode=mode)
    assert ref["stats"]["pushed_b"] == 8 * (ref["capacity"] - 1) and ref["stats"]["pushed_a"] == 0 and ref["capacity"] == big["child"].shape[0]
    ref = _check(mnv, torch_gpu, leaf, big, mode=mode)
    assert ref["stats"]["pushed_a"] == 8 * (ref["capacity"] - 1) and ref["stats"]["pushed_b"] == 0
    ref = _check(mnv, torch_gpu, big, other, mode=mode)
    assert ref["stats"]["pushed_a"] > 0 and ref["stats"]["pushed_b"] > 0 and max(big["child"].shape[0], other["child"].shape[0]) < ref["capacity"]
    assert (ref["stats"]["rows_blended"] > 0) == (mode == "add")


def test_a_leaf_pushed_down_four_levels(mnv, torch_gpu):
    a = tree(23, 2, 4, 0.5)
    b = tree(24, 6, 4, 0.3)
    ref = _check(mnv, torch_gpu, a, b, mode="add")
    assert np.nonzero(ref["stats"]["chunks_at_depth"])[0].max() == 6 and ref["stats"]["pushed_a"] > 8 * sum(ref["stats"]["chunks_at_depth"][4:])


def test_chains_to_the_depth_bound(mnv, torch_gpu):
    """The deepest legal tree has 23 levels.  A chain of 23 chunks merges with a single chunk either way round; a chain of 22 placed one
    level down still fits; the chain of 23 placed one level down would have 24 levels: MNV_E_UNSUPPORTED."""
    torch = torch_gpu
    single = one_chunk(4, 2)
    ref = _check(mnv, torch, chain(23), single)
    assert ref["stats"]["chunks_at_depth"][1:] == [1] * 23 and ref["capacity"] == 23
    _check(mnv, torch, single, chain(23), mode="add")
    _check(mnv, torch, chain(22), single, 1, (1, 0, 1))
    ref = _check(mnv, torch, single, chain(22), 1, (1, 1, 0))
    assert ref["stats"]["chunks_at_depth"][23] == 1
    dev_a, va = _upload(mnv, torch, single)
    dev_b, vb = _upload(mnv, torch, chain(23))
    with pytest.raises(mnv.MnvError) as e:
        mnv.TreeMerge(va, vb, 1, (0, 0, 0))
    assert e.value.code == mnv.MNV_E_UNSUPPORTED
    with pytest.raises(ValueError, match="unsupported"):
        mr.merge(single, chain(23), 1, (0, 0, 0))


def test_links_that_leave_a_tree_and_cycles_end_in_an_error(mnv, torch_gpu):
    torch = torch_gpu
    good = tree(25, 4, 4)
    bad = dict(good, child=good["child"].copy())
    j = int(np.nonzero(bad["child"][0])[0][0])
    bad["child"][0, j] = bad["child"].shape[0]
    cyc = one_chunk(4, 3)
    cyc = dict(data=np.repeat(cyc["data"], 3, axis=0), child=np.zeros((3, 8), np.int32))
    cyc["child"][0, 1], cyc["child"][1, 2], cyc["child"][2, 5] = 1, 1, -1
    for a, b in ((bad, good), (good, bad), (cyc, good), (good, cyc)):
        dev_a, va = _upload(mnv, torch, a)
        dev_b, vb = _upload(mnv, torch, b)
        with pytest.raises(mnv.MnvError) as e:
            mnv.TreeMerge(va, vb)
        assert e.value.code in (mnv.MNV_E_INVALID, mnv.MNV_E_UNSUPPORTED)
        with pytest.raises(ValueError):
            mr.merge(a, b)
    negative = dict(good, child=good["child"].copy())
    negative["child"][0, j] = -1
    dev_a, va = _upload(mnv, torch, negative)
    dev_b, vb = _upload(mnv, torch, good)
    with pytest.raises(mnv.MnvError) as e:
        mnv.TreeMerge(va, vb)
    assert e.value.code == mnv.MNV_E_INVALID


# ---------------------------------------------------------------------------------------------------- placement

@pytest.mark.parametrize("level,corner", [(0, (0, 0, 0)), (1, (0, 1, 0)), (1, (1, 1, 1)), (3, (5, 2, 6)), (3, (7, 7, 7)), (3, (0, 0, 0))])
@pytest.mark.parametrize("base", ["leaf", "shallow", "deep"])
def test_placement(mnv, torch_gpu, level, corner, base):
    """A one-chunk base is a leaf above B's cube (the path forces the chunks); the shallow and the deep base end above, at or below the
    placement level, depending on the corner."""
    a = dict(leaf=one_chunk(4, 4), shallow=tree(26, 3, 4, 0.4), deep=tree(27, 6, 4, 0.62))[base]
    b = tree(28, 4, 4, 0.45)
    for mode in ("over", "add"):
        ref = _check(mnv, torch_gpu, a, b, level, corner, mode)
    assert ref["stats"]["rows_from_b"] + ref["stats"]["rows_blended"] > 0
    if base == "leaf" and level > 0:
        assert ref["capacity"] == level + b["child"].shape[0]


def test_a_base_deeper_than_the_placement_along_the_path(mnv, torch_gpu):
    a, b = tree(27, 6, 4, 0.62), tree(28, 4, 4, 0.45)
    child = a["child"]

    def height(c):
        return 1 + max([height(c + child[c, j]) for j in range(8) if child[c, j]] or [0])

    c, corner = 0, [0, 0, 0]
    for _ in range(3):                                        # three levels down along the tallest subtree
        j = max(range(8), key=lambda j: height(c + child[c, j]) if child[c, j] else 0)
        assert child[c, j]
        corner = [2 * corner[0] + (j >> 2), 2 * corner[1] + ((j >> 1) & 1), 2 * corner[2] + (j & 1)]
        c += child[c, j]
    s = mr.walk(child, b["child"], 3, corner)
    assert ((s["b_vox"] >= 0) & s["a_exact"]).sum() > 8 and ((s["b_vox"] >= 0) & ~s["a_exact"]).any() and (~s["b_exact"] & (s["b_vox"] >= 0)).any()
    for mode in ("over", "add"):
        _check(mnv, torch_gpu, a, b, 3, tuple(corner), mode)


# ---------------------------------------------------------------------------------------------------- level sizes

@pytest.mark.parametrize("n", [7, 8, 9, 31, 32, 33])
def test_levels_at_the_wavefront_and_workgroup_edges(mnv, torch_gpu, n):
    a = trimmed(tree(30, 5, 4, 0.62), n)
    ref = _check(mnv, torch_gpu, a, one_chunk(4, 5), mode="add")
    assert n in ref["stats"]["chunks_at_depth"]
    ref = _check(mnv, torch_gpu, one_chunk(4, 6), a, 1, (1, 0, 0))           # the same levels one depth down
    assert n in ref["stats"]["chunks_at_depth"]


def test_a_level_of_five_thousand_chunks(mnv, torch_gpu):
    a = trimmed(tree(32, 7, 4, 0.55), 5000)
    ref = _check(mnv, torch_gpu, a, tree(33, 5, 4, 0.4), mode="add")
    assert max(ref["stats"]["chunks_at_depth"]) >= 5000 and ref["capacity"] < 40000


# ---------------------------------------------------------------------------------------------------- input forms

@pytest.mark.parametrize("form_a,form_b", [("renumbered", "plain"), ("plain", "renumbered"), ("unreached", "unreached"), ("renumbered", "unreached")])
def test_inputs_that_are_not_breadth_first_or_hold_unreached_chunks(mnv, torch_gpu, form_a, form_b):
    def shaped(t, form):
        data, child = t["data"], t["child"]
        if form == "renumbered":
            data, child = renumbered(data, child)
        if form == "unreached":
            data, child = with_unreached(data, child)
        return dict(data=data, child=child)

    a, b = shaped(tree(34, 5, 4, 0.45), form_a), shaped(tree(35, 5, 4, 0.4), form_b)
    plain = mr.merge(tree(34, 5, 4, 0.45), tree(35, 5, 4, 0.4), 1, (0, 1, 1), mr.ADD)
    ref = _check(mnv, torch_gpu, a, b, 1, (0, 1, 1), "add")
    for k in ("child", "data", "parent"):                     # the numbering is canonical: the input's order does not show
        assert np.array_equal(ref[k], plain[k]), k


@pytest.mark.parametrize("counts_a,counts_b", [(True, True), (True, False), (False, True), (False, False)])
def test_sample_counts_on_both_sides_one_side_and_neither(mnv, torch_gpu, counts_a, counts_b):
    a, b = tree(36, 4, 4, 0.5, counts=counts_a), tree(37, 4, 4, 0.5, counts=counts_b)
    ref = _check(mnv, torch_gpu, a, b, mode="add")
    if counts_a and counts_b:
        assert (ref["sample_counts"] == 32767).any() and (ref["sample_counts"] == -32768).any()      # the blended sum is clamped
    if not counts_a and not counts_b:
        assert set(np.unique(ref["sample_counts"]).tolist()) == {8, 16}
    _check(mnv, torch_gpu, a, b, mode="over", nulls=("parent", "sample_counts", "src_a", "src_b"))
    _check(mnv, torch_gpu, a, b, mode="over", nulls=("src_b",))


# ---------------------------------------------------------------------------------------------------- rows

SIGMAS = np.array([0x0000, 0x8000, 0xBC00, 0xC900, 0x0001, 0x03FF, 0x8001, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x78E2, 0x3C00, 0x4D00, 0x5640], np.uint16)
COEFFS = np.array([0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF, 0x8000, 0x0000], np.uint16)


def special_pair(dd, seed):
    """Two trees of one structure whose sigmas come from SIGMAS (+0, -0, negative, subnormal, 65504, infinities, NaNs, 40000 = 0x78E2 and
    ordinary values) and whose other columns hold special halfs here and there: every pairing of the two sides occurs, so chunks mix rows
    of A, rows of B and blended rows."""
    rng = np.random.default_rng(seed)
    a, b = tree(seed, 4, dd, 0.5), tree(seed, 4, dd, 0.5)
    b["data"] = np.ascontiguousarray(rng.uniform(-3, 12, size=b["data"].shape).astype(np.float16).view(np.uint16))
    for t in (a, b):
        t["data"][..., dd - 1] = rng.choice(SIGMAS, size=t["child"].shape)
        hit = rng.uniform(size=t["data"].shape) < 0.1
        hit[..., dd - 1] = False
        t["data"][hit] = rng.choice(COEFFS, size=int(hit.sum()))
    a["data"][1, :, dd - 1] = 0x78E2                          # 40000 + 40000 saturates
    b["data"][1, :, dd - 1] = 0x78E2
    a["data"][2, :, dd - 1] = 0x3C00                          # a chunk blended throughout, with infinite coefficients that read as 0
    b["data"][2, :, dd - 1] = 0x4000
    a["data"][2, :, 0] = 0x7C00
    b["data"][2, :, 1] = 0xFC00
    return a, b


@pytest.mark.parametrize("dd", [4, 28, 49, 76])
@pytest.mark.parametrize("mode", ["over", "add"])
def test_rows_with_special_halfs_and_mixed_chunks(mnv, torch_gpu, dd, mode):
    a, b = special_pair(dd, 40 + dd)
    assert a["child"].shape[0] > 8
    ref = _check(mnv, torch_gpu, a, b, mode=mode)
    st = ref["stats"]
    assert st["rows_from_a"] > 0 and st["rows_from_b"] > 0
    if mode == "add":
        assert st["rows_blended"] > 0 and (ref["data"][1, :, dd - 1] == 0x7BFF).all()
        kinds = mr.rows(a["data"], b["data"], ref["src_a"], ref["src_b"], mr.ADD)[2].reshape(-1, 8)
        assert any(len(set(row.tolist())) == 3 for row in kinds)                                   # a chunk with all three kinds of row
        hb = mr.half_value(b["data"][2, :, 0])               # chunk 2: wa = 1, wb = 2, W = 3; A's infinite coefficient reads as 0
        want0 = mr.sat_half(((F(1.0) * F(0.0) + (F(2.0) * hb).astype(F)).astype(F) / F(3.0)).astype(F))
        assert np.array_equal(ref["data"][2, :, 0], want0) and np.array_equal(ref["data"][2, :, dd - 1], np.full(8, 0x4200, np.uint16))
    # the same rows under a placement: B's chunks sit one level down, most merged chunks take A's pushed leaf on one side
    _check(mnv, torch_gpu, a, b, 1, (1, 0, 1), mode)


# ---------------------------------------------------------------------------------------------------- handles and streams

def test_two_handles_on_two_streams_give_the_bytes_of_handles_used_one_at_a_time(mnv, torch_gpu):
    torch = torch_gpu
    a, b, c = tree(50, 6, 28, 0.5), tree(51, 6, 28, 0.45), tree(52, 5, 28, 0.5)
    alone = [_merge(mnv, torch, a, b, mode="add"), _merge(mnv, torch, c, a, 1, (1, 1, 0), "over")]
    (dev_a, va), (dev_b, vb), (dev_c, vc) = (_upload(mnv, torch, t) for t in (a, b, c))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    p1 = mnv.TreeMerge(va, vb, 0, (0, 0, 0), "add", stream=s1.cuda_stream)
    p2 = mnv.TreeMerge(vc, va, 1, (1, 1, 0), "over", stream=s2.cuda_stream)
    outs = [_outputs(torch, int(p.stats.capacity), 28) for p in (p1, p2)]
    torch.cuda.synchronize()
    for _ in range(3):                                        # the two writes interleave; a handle is written from more than once
        _write(torch, p1, outs[0], stream=s1.cuda_stream)
        _write(torch, p2, outs[1], stream=s2.cuda_stream)
    torch.cuda.synchronize()
    for p, out, want in zip((p1, p2), outs, alone):
        got = _host(out, int(p.stats.capacity))
        assert p.stats.as_dict() == want["stats"]
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------- frames

OUTSIDE = ((-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48))
INSIDE = ((0.3, -0.2, 0.1), (-0.6, 0.64, 0.48))
FX = 224.0


def _march(mnv, torch, t, cam, opt, packed=True):
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    if packed:
        mnv.render_voxels_accel(t.accel, cam, opt, rgba=out)
    else:
        mnv.render_voxels(t.device_view(), cam, opt, rgba=out)
    torch.cuda.synchronize()
    return cases.bits(out.cpu().numpy()).copy()


def _arrays(t):
    data, child, _ = t.host_arrays()
    return dict(data=data.copy(), child=child.copy())


@pytest.mark.parametrize("mode", ["over", "add"])
def test_frames_of_a_merged_tree_are_the_oracles(mnv, orc, torch_gpu, mode):
    torch = torch_gpu
    a = mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=3)
    b = mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=4, sigma_max=80.0)
    hv = a.host_view()
    want = mr.merge(_arrays(a), _arrays(b), 1, (1, 0, 1), mr.ADD if mode == "add" else mr.OVER)
    a.move_to_device(need_parent=True, need_sample_counts=True)
    b.move_to_device()
    before = _arrays(a)
    merged, st = a.merge(b, level=1, corner=(1, 0, 1), mode=mode, return_stats=True)
    assert st.as_dict() == want["stats"] and merged.capacity == want["capacity"] and merged.data_format == a.data_format
    got_data, got_child, got_parent = merged.host_arrays()
    assert np.array_equal(got_child, want["child"]) and np.array_equal(got_data, want["data"]) and np.array_equal(got_parent, want["parent"])
    mv = merged.host_view()
    assert list(mv.offset) == list(hv.offset) and list(mv.scale) == list(hv.scale)
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, 3
    host = mnv.N3Tree.from_arrays(want["data"], want["child"], data_format=a.data_format, offset=tuple(hv.offset), scale=tuple(hv.scale))
    shows = False
    for eye, back in (OUTSIDE, INSIDE):
        cam = mnv.Camera(W, H, FX).set_pose(eye, back)
        oracle = cases.bits(orc.render(orc.tree_from_view(host.host_view()), cam.c, opt)["rgba"])
        assert np.array_equal(_march(mnv, torch, merged, cam, opt), oracle)
        assert np.array_equal(_march(mnv, torch, merged, cam, opt, packed=False), oracle)
        shows = shows or not np.array_equal(_march(mnv, torch, a, cam, opt), oracle)
    assert shows                                              # B is in the picture
    after = _arrays(a)
    assert np.array_equal(before["data"], after["data"]) and np.array_equal(before["child"], after["child"])


def test_merging_with_the_empty_tree_renders_what_the_tree_renders(mnv, torch_gpu):
    torch = torch_gpu
    a = mnv.N3Tree.synth_random(depth=5, basis_dim=1, seed=5)
    data, child, _ = a.host_arrays()
    data, child = renumbered(data.copy(), child.copy())       # not breadth first
    hv = a.host_view()
    a = mnv.N3Tree.from_arrays(data, child, data_format="SH1", offset=tuple(hv.offset), scale=tuple(hv.scale))
    empty = mnv.N3Tree.from_arrays(np.zeros((1, 8, 4), np.uint16), np.zeros((1, 8), np.int32), data_format="SH1")
    a.move_to_device(need_parent=True, need_sample_counts=True)
    empty.move_to_device()
    merged = a.merge(empty)
    want = mr.merge(dict(data=data, child=child), mr.empty_tree(4))
    assert np.array_equal(merged.host_arrays()[0], want["data"]) and np.array_equal(merged.host_arrays()[1], want["child"])
    assert not np.array_equal(want["child"], child)
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, 0
    for eye, back in (OUTSIDE, INSIDE):
        cam = mnv.Camera(W, H, FX).set_pose(eye, back)
        frame = _march(mnv, torch, a, cam, opt)
        assert np.array_equal(_march(mnv, torch, merged, cam, opt), frame) and np.array_equal(_march(mnv, torch, merged, cam, opt, packed=False), frame)
        assert (frame.view(np.float32)[..., 3] > 0).any()


# ---------------------------------------------------------------------------------------------------- tiles of a point cloud

def test_octant_tiles_from_points_merged_are_the_tree_of_the_whole_cloud(mnv, torch_gpu):
    """tests/test_merge_ref.py's tile case on the device, through N3Tree.from_points and N3Tree.merge: dyadic coordinates, offset 0.5 and
    scale 1, so that every product and sum of the point-to-voxel map is exact for the tiles and for the whole."""
    D = 6
    rng = np.random.default_rng(9)
    xyz = (rng.integers(0, 1 << 10, size=(20000, 3)).astype(np.float64) / (1 << 10) - 0.5).astype(F)
    rgb = rng.integers(0, 256, size=(20000, 3), dtype=np.uint8)
    cube = (np.array([0.5, 0.5, 0.5], F), np.array([1.0, 1.0, 1.0], F))
    for fmt in ("RGBA", "SH4"):
        whole = mnv.N3Tree.from_points(xyz, rgb, depth=D, sigma=60.0, data_format=fmt, cube=cube)
        ref = pr.build(xyz, rgb, cube[0], cube[1], D, fmt, 1, 60.0)
        dd = pr.data_dim(fmt)
        merged = mnv.N3Tree.from_arrays(np.zeros((1, 8, dd), np.uint16), np.zeros((1, 8), np.int32), data_format=fmt, offset=tuple(cube[0]), scale=tuple(cube[1]))
        merged.move_to_device(need_parent=True, need_sample_counts=True)
        for j in range(8):
            corner = (j >> 2, (j >> 1) & 1, j & 1)
            tile = mnv.N3Tree.from_points(xyz, rgb, depth=D - 1, sigma=60.0, data_format=fmt, cube=merged.voxel_cube(1, corner))
            merged = merged.merge(tile, level=1, corner=corner)
        for got, dev, want in zip(merged.host_arrays(), whole.host_arrays(), (ref["data"], ref["child"], ref["parent"])):
            assert np.array_equal(got, want) and np.array_equal(got, dev)


# ---------------------------------------------------------------------------------------------------- mnv_render --merge

def test_mnv_render_merge_and_save_lod(mnv, torch_gpu, tmp_path):
    torch = torch_gpu
    assert os.path.exists(EXE), "mnv_render not built"
    a = mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=6)
    hv = a.host_view()
    offset, scale = mnv.tree_voxel_cube(tuple(hv.offset), tuple(hv.scale), 2, (1, 3, 2))
    b = mnv.N3Tree.synth_random(depth=3, basis_dim=4, seed=7, sigma_max=90.0, offset=tuple(offset), scale=tuple(scale))
    c = mnv.N3Tree.synth_random(depth=3, basis_dim=4, seed=8, offset=(0.4, 0.5, 0.5), scale=tuple(scale))   # no voxel of A's cube
    npz_a, npz_b, npz_c, saved, out = (str(tmp_path / n) for n in ("a.npz", "b.npz", "c.npz", "merged.npz", "frame"))
    a.save_npz(npz_a), b.save_npz(npz_b), c.save_npz(npz_c)
    pose = ["-w", str(W), "-h", str(H), "--fx", "224", "--center", ",".join(map(str, OUTSIDE[0])), "--back", ",".join(map(str, OUTSIDE[1]))]

    def run(cmd):
        return subprocess.run([EXE] + cmd + pose, capture_output=True, text=True, timeout=120)

    a.move_to_device(need_parent=True, need_sample_counts=True)
    b.move_to_device()
    c.move_to_device()
    once = a.merge(b, level=2, corner=(1, 3, 2))
    r = run([npz_a, "--merge", npz_b, "--save_lod", saved, "--out", out, "--raw", "--frames", "1"])
    assert r.returncode == 0, r.stderr + r.stdout
    assert "merge: " in r.stdout and " at 2:1,3,2 (over)" in r.stdout
    back_in = mnv.N3Tree.open(saved)
    for x, y in zip(back_in.host_arrays(), once.host_arrays()):
        assert np.array_equal(x, y)
    assert back_in.data_format == a.data_format and list(back_in.host_view().scale) == list(hv.scale) and list(back_in.host_view().offset) == list(hv.offset)
    cam = mnv.Camera(W, H, FX).set_pose(*OUTSIDE)
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, 3
    frame = np.fromfile(out + "_0000.f32", dtype=np.float32).reshape(H, W, 4)
    assert np.array_equal(cases.bits(frame), _march(mnv, torch, once, cam, opt))
    # a fold of two merges, each with its own placement and mode
    twice = once.merge(c, level=1, corner=(0, 1, 0), mode="add")
    r = run([npz_a, "--merge", npz_b, "--merge", npz_c, "--merge_at", "1:0,1,0", "--merge_mode", "add", "--save_lod", saved, "--frames", "0"])
    assert r.returncode == 0, r.stderr + r.stdout
    back_in = mnv.N3Tree.open(saved)                           # (host_arrays are views: the tree must outlive them)
    for x, y in zip(back_in.host_arrays(), twice.host_arrays()):
        assert np.array_equal(x, y)
    # ... and under a level of detail: the merge comes first
    r = run([npz_a, "--merge", npz_b, "--lod", "3", "--save_lod", saved, "--frames", "0"])
    assert r.returncode == 0, r.stderr + r.stdout
    back_in, coarse = mnv.N3Tree.open(saved), once.make_lod(3)
    assert coarse.capacity < once.capacity
    for x, y in zip(back_in.host_arrays(), coarse.host_arrays()):
        assert np.array_equal(x, y)
    bad = run([npz_a, "--merge", npz_c, "--frames", "0"])
    assert bad.returncode != 0 and "--merge_at" in bad.stderr
