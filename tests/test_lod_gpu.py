"""Levels of detail on the device (csrc/mnv_lod.hip: mnv_tree_mip_rows, mnv_tree_truncate; N3Tree.make_lod, Renderer.set_lod, mnv_render --lod)
against tests/lod_ref.py, the numpy restatement of the two contracts in include/mnv.h.  No tolerance anywhere: every comparison is on bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import lod_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")
W, H = 64, 48


# ---------------------------------------------------------------------------------------------------- trees

def _random_tree(seed, levels, dd, p=0.4):
    """Chunks in breadth-first order, random finite halfs with a third of the sigmas zero or negative."""
    rng = np.random.default_rng(seed)
    child_rows, front, n = [np.zeros(8, np.int32)], [0], 1
    for _ in range(levels - 1):
        nxt = []
        for c in front:
            for j in range(8):
                if rng.uniform() < p:
                    child_rows[c][j] = n - c
                    child_rows.append(np.zeros(8, np.int32))
                    nxt.append(n)
                    n += 1
        front = nxt
    child = np.stack(child_rows)
    vals = rng.uniform(-3, 12, size=(n, 8, dd)).astype(np.float16)
    vals[..., dd - 1] = np.where(rng.uniform(size=(n, 8)) < 0.33, rng.uniform(-5, 0, size=(n, 8)) * (rng.uniform(size=(n, 8)) < 0.5),
                                 rng.uniform(0, 300, size=(n, 8))).astype(np.float16)
    return np.ascontiguousarray(vals.view(np.uint16)), child


def _synth(mnv, depth, fmt):
    if fmt == "RGBA":
        t = mnv.N3Tree.synth_random(depth=depth, basis_dim=-1, fmt=mnv.FORMAT_RGBA, seed=depth)
    else:
        t = mnv.N3Tree.synth_random(depth=depth, basis_dim=int(fmt[2:]), seed=depth)
    data, child, _ = t.host_arrays()
    return data.copy(), child.copy()


def _chain(levels=14, dd=4):
    """One interior voxel per level: chunk c's voxel c % 8 leads to chunk c + 1.  Only the deepest-first order makes the top rows right."""
    rng = np.random.default_rng(14)
    child = np.zeros((levels, 8), np.int32)
    for c in range(levels - 1):
        child[c, c % 8] = 1
    data = rng.uniform(0.1, 9, size=(levels, 8, dd)).astype(np.float16).view(np.uint16)
    return np.ascontiguousarray(data), child


def _renumbered(data, child):
    """The same tree with chunk c >= 1 stored at capacity - c: children precede their parents in memory."""
    cap = child.shape[0]
    new = np.concatenate([[0], cap - np.arange(1, cap)]).astype(np.int64)
    d2, c2 = np.empty_like(data), np.zeros_like(child)
    d2[new] = data
    rows, cols = np.nonzero(child)
    c2[new[rows], cols] = (new[rows + child[rows, cols]] - new[rows]).astype(np.int32)
    return d2, c2


def _patched(data, child):
    """Special halfs all over: negative, infinite and NaN sigmas, infinite and NaN colours, subnormals, -0; one all-leaf chunk whose first
    colour column is -0 under positive sigmas (the sum of eight -0 terms)."""
    rng = np.random.default_rng(99)
    data = data.copy()
    dd = data.shape[2]
    special = np.array([0xBC00, 0xC900, 0x7C00, 0x7E00, 0xFC00, 0xFE01, 0x0001, 0x03FF, 0x8001, 0x83FF, 0x8000, 0x0000, 0x7BFF, 0xFBFF], np.uint16)
    hit = rng.uniform(size=data.shape) < 0.3
    data[hit] = rng.choice(special, size=int(hit.sum()))
    depth, _ = lod_ref.chunk_depths(child)
    k = int(np.nonzero((depth == depth.max()))[0][0])
    data[k, :, 0] = 0x8000
    data[k, :, dd - 1] = 0x3C00
    return data


def _with_unreached(data, child):
    """Three trailing chunks nothing links to (one of them links to the next)."""
    rng = np.random.default_rng(5)
    extra = rng.integers(0, 0x7BFF, size=(3,) + data.shape[1:], dtype=np.uint16)
    links = np.zeros((3, 8), np.int32)
    links[0, 2] = 1
    return np.concatenate([data, extra]), np.concatenate([child, links])


# ---------------------------------------------------------------------------------------------------- device calls

def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


def _view(mnv, data_t, child_t, dd, counts_t=None, fmt=None, basis=-1):
    v = mnv.TreeView()
    v.data, v.child = data_t.data_ptr(), child_t.data_ptr()
    v.sample_counts = counts_t.data_ptr() if counts_t is not None else None
    for i in range(3):
        v.offset[i] = v.scale[i] = 0.5
    v.N, v.data_dim, v.format, v.basis_dim, v.capacity = 2, dd, mnv.FORMAT_RGBA if fmt is None else fmt, basis, int(child_t.shape[0])
    return v


def _mip(mnv, torch, data, child, want_depth=True):
    """(data_out, chunk_depth, chunks_at_depth) of mnv_tree_mip_rows; the input arrays must come back unchanged."""
    cap, _, dd = data.shape
    data_t, child_t = _dev(torch, data), _dev(torch, child)
    out_t = torch.full((cap, 8, dd), 0x5555, dtype=torch.int16, device="cuda")
    depth_t = torch.full((cap,), -7, dtype=torch.int32, device="cuda") if want_depth else None
    counts = mnv.tree_mip_rows(_view(mnv, data_t, child_t, dd), out_t, depth_t)
    assert np.array_equal(_host16(data_t), data) and np.array_equal(child_t.cpu().numpy(), child)
    return _host16(out_t), (depth_t.cpu().numpy() if want_depth else None), counts


def _check_mip(mnv, torch, data, child):
    ref, ref_depth, ref_counts = lod_ref.mip_rows(data, child)
    out, depth, counts = _mip(mnv, torch, data, child)
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(depth, ref_depth)
    bad = np.argwhere(out != ref)
    assert bad.size == 0, (bad[:5], out[tuple(bad[0])], ref[tuple(bad[0])])
    return ref, ref_depth, ref_counts


# ---------------------------------------------------------------------------------------------------- mnv_tree_mip_rows

@pytest.mark.parametrize("depth,fmt", [(2, "SH1"), (3, "SH4"), (4, "SH9"), (5, "SH16"), (6, "SH25"), (4, "RGBA"), (6, "SH9"), (5, "SH1")])
def test_mip_rows_of_synthetic_trees(mnv, torch_gpu, depth, fmt):
    data, child = _synth(mnv, depth, fmt)
    _, ref_depth, _ = _check_mip(mnv, torch_gpu, data, child)
    assert 2 <= ref_depth.max() <= depth and child.shape[0] < 20000


def test_mip_rows_of_a_single_chunk_are_the_input(mnv, torch_gpu):
    data, child = _random_tree(0, 1, 28)
    out, depth, counts = _mip(mnv, torch_gpu, data, child)
    assert np.array_equal(out, data) and depth.tolist() == [1] and counts.tolist() == [0, 1] + [0] * 22


def test_mip_rows_of_a_chain_fourteen_deep(mnv, torch_gpu):
    data, child = _chain()
    ref, _, counts = _check_mip(mnv, torch_gpu, data, child)
    assert counts[1:15].tolist() == [1] * 14 and not np.array_equal(ref[0, 0], data[0, 0])


def test_mip_rows_do_not_rely_on_chunk_order(mnv, torch_gpu):
    data, child = _renumbered(*_random_tree(21, 6, 13))
    assert (child[1:][child[1:] != 0] < 0).all()          # every link below the root points backwards
    _check_mip(mnv, torch_gpu, data, child)


@pytest.mark.parametrize("fmt", ["SH4", "RGBA"])
def test_mip_rows_with_special_halfs(mnv, torch_gpu, fmt):
    data, child = _synth(mnv, 5, fmt)
    data = _patched(data, child)
    ref, _, _ = _check_mip(mnv, torch_gpu, data, child)
    assert (ref[child != 0] == 0x8000).any()              # a -0 survived the mip somewhere


def test_mip_rows_copy_unreached_chunks(mnv, torch_gpu):
    data, child = _with_unreached(*_random_tree(22, 5, 28))
    ref, ref_depth, ref_counts = _check_mip(mnv, torch_gpu, data, child)
    assert ref_depth[-3:].tolist() == [0, 0, 0] and np.array_equal(ref[-3:], data[-3:]) and ref_counts.sum() == child.shape[0] - 3
    out, _, _ = _mip(mnv, torch_gpu, data, child, want_depth=False)      # chunk_depth_out may be NULL
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("dd", [2, 5, 76, 129])
def test_mip_rows_with_rows_that_have_no_sh_meaning(mnv, torch_gpu, dd):
    data, child = _random_tree(30 + dd, 5, dd)
    assert child.shape[0] > 100
    _check_mip(mnv, torch_gpu, data, child)


def test_mip_rows_over_more_than_one_launch_block(mnv, torch_gpu):
    data, child = _random_tree(40, 7, 4, p=0.5)
    assert child.shape[0] > 3000
    _check_mip(mnv, torch_gpu, data, child)


def test_mip_rows_refuse_what_is_not_a_tree(mnv, torch_gpu):
    torch = torch_gpu
    data, child = _random_tree(41, 5, 4, p=0.5)
    cap = child.shape[0]
    assert cap > 100
    leaf = np.argwhere(child[2:] == 0)[0]
    c, j = int(leaf[0]) + 2, int(leaf[1])
    data_t = _dev(torch, data)
    out_t = torch.zeros((cap, 8, 4), dtype=torch.int16, device="cuda")
    counts = (C.c_int64 * 24)()
    lib = mnv.lib()
    for link in (-c, cap - c, 1 - c):                      # chunk 0, capacity, a chunk that has a parent already
        bad = child.copy()
        bad[c, j] = link
        child_t = _dev(torch, bad)
        v = _view(mnv, data_t, child_t, 4)
        assert lib.mnv_tree_mip_rows(C.byref(v), out_t.data_ptr(), None, counts, None) == mnv.MNV_E_INVALID, link
    child_t = _dev(torch, child)
    v = _view(mnv, data_t, child_t, 4)
    assert lib.mnv_tree_mip_rows(C.byref(v), data_t.data_ptr(), None, counts, None) == mnv.MNV_E_INVALID      # data_out aliases the tree
    assert lib.mnv_tree_mip_rows(C.byref(v), None, None, counts, None) == mnv.MNV_E_INVALID
    assert lib.mnv_tree_mip_rows(None, out_t.data_ptr(), None, counts, None) == mnv.MNV_E_INVALID
    v.N = 3
    assert lib.mnv_tree_mip_rows(C.byref(v), out_t.data_ptr(), None, counts, None) == mnv.MNV_E_UNSUPPORTED
    deep_data, deep_child = _chain(levels=24)
    dt, ct = _dev(torch, deep_data), _dev(torch, deep_child)
    v = _view(mnv, dt, ct, 4)
    deep_out = torch.zeros((24, 8, 4), dtype=torch.int16, device="cuda")
    assert lib.mnv_tree_mip_rows(C.byref(v), deep_out.data_ptr(), None, counts, None) == mnv.MNV_E_UNSUPPORTED
    assert np.array_equal(_host16(data_t), data)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- mnv_tree_truncate

def _truncation_trees(mnv):
    a = _synth(mnv, 5, "SH9")
    b = _renumbered(*_random_tree(50, 6, 13))
    c = _with_unreached(*_random_tree(51, 5, 5))
    return dict(synth_sh9=a, renumbered=b, unreached=c)


@pytest.mark.parametrize("name", ["synth_sh9", "renumbered", "unreached"])
def test_truncate_at_every_depth(mnv, torch_gpu, name):
    torch = torch_gpu
    data, child = _truncation_trees(mnv)[name]
    cap, _, dd = data.shape
    sc = np.random.default_rng(7).integers(-100, 3000, size=(cap, 8)).astype(np.int16)
    mipped, depth, counts = lod_ref.mip_rows(data, child)
    out, dev_depth, dev_counts = _mip(mnv, torch, data, child)
    assert np.array_equal(out, mipped) and np.array_equal(dev_depth, depth)
    mip_t, child_t, depth_t, sc_t = _dev(torch, mipped), _dev(torch, child), _dev(torch, depth), _dev(torch, sc)
    with_counts, without_counts = _view(mnv, mip_t, child_t, dd, sc_t), _view(mnv, mip_t, child_t, dd)
    levels = int(depth.max())
    for d in range(1, levels + 2):
        ref = lod_ref.truncate(mipped, child, depth, d, sc)
        n = int(dev_counts[1:min(d, 23) + 1].sum())
        assert n == ref["capacity"]
        for variant in ("all", "no_parent", "no_counts", "view_without_counts"):
            o_child = torch.full((n, 8), 0x55555555, dtype=torch.int32, device="cuda")
            o_data = torch.full((n, 8, dd), 0x5555, dtype=torch.int16, device="cuda")
            o_parent = None if variant == "no_parent" else torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
            o_sc = None if variant == "no_counts" else torch.full((n, 8), 0x5555, dtype=torch.int16, device="cuda")
            view = without_counts if variant == "view_without_counts" else with_counts
            mnv.tree_truncate(view, depth_t, d, n, o_child, o_data, o_parent, o_sc)
            torch.cuda.synchronize()
            assert np.array_equal(o_child.cpu().numpy(), ref["child"]), (d, variant)
            assert np.array_equal(_host16(o_data), ref["data"]), (d, variant)
            if o_parent is not None:
                assert np.array_equal(o_parent.cpu().numpy(), ref["parent"]), (d, variant)
            if o_sc is not None and variant != "view_without_counts":
                assert np.array_equal(o_sc.cpu().numpy(), ref["sample_counts"]), (d, variant)
            if variant == "view_without_counts":
                assert (o_sc.cpu().numpy() == 0x5555).all()      # skipped: the input has none
    assert np.array_equal(_host16(mip_t), mipped) and np.array_equal(child_t.cpu().numpy(), child)
    lib = mnv.lib()
    one = torch.zeros((cap, 8, dd), dtype=torch.int16, device="cuda")
    links = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    assert lib.mnv_tree_truncate(C.byref(with_counts), depth_t.data_ptr(), 0, 1, links.data_ptr(), one.data_ptr(), None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_tree_truncate(C.byref(with_counts), None, 1, 1, links.data_ptr(), one.data_ptr(), None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_tree_truncate(C.byref(with_counts), depth_t.data_ptr(), 1, cap + 1, links.data_ptr(), one.data_ptr(), None, None, None) == mnv.MNV_E_INVALID


# ---------------------------------------------------------------------------------------------------- frames

def _frame_case(mnv, which):
    if which == "shell":
        tree = mnv.N3Tree.synth_shell(depth=7, basis_dim=9, radius=0.35, half_thickness=1.5 / 128, seed=0)
        cam = mnv.orbit_camera(W, H, 53.2, 2.6, 22.5, 20.0)
    else:
        tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
        cam = mnv.Camera(W, H, 224.0).set_pose((-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48))
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, tree.host_view().basis_dim - 1
    return tree, cam, opt


@pytest.mark.parametrize("which", ["shell", "sh4_d6"])
@pytest.mark.parametrize("lod", [3, 5])
def test_frames_of_the_truncated_tree_three_ways(mnv, orc, torch_gpu, which, lod):
    torch = torch_gpu
    tree, cam, opt = _frame_case(mnv, which)
    data, child, _ = tree.host_arrays()
    ref = lod_ref.make_lod(data, child, lod)
    tree.move_to_device(need_parent=True, need_sample_counts=True)
    cut = tree.make_lod(lod)
    got_data, got_child, got_parent = cut.host_arrays()
    assert cut.capacity == ref["capacity"] < tree.capacity and cut.data_format == tree.data_format
    assert np.array_equal(got_child, ref["child"]) and np.array_equal(got_data, ref["data"]) and np.array_equal(got_parent, ref["parent"])
    hv, cv = tree.host_view(), cut.host_view()
    assert list(cv.offset) == list(hv.offset) and list(cv.scale) == list(hv.scale)
    frames = {}
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(cut.accel, cam, opt, rgba=out)
    torch.cuda.synchronize()
    frames["accel"] = out.cpu().numpy()
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels(cut.device_view(), cam, opt, rgba=out)
    torch.cuda.synchronize()
    frames["ref_layout"] = out.cpu().numpy()
    host = mnv.N3Tree.from_arrays(ref["data"], ref["child"], data_format=tree.data_format, offset=tuple(hv.offset), scale=tuple(hv.scale))
    frames["oracle"] = orc.render(orc.tree_from_view(host.host_view()), cam.c, opt)["rgba"]
    assert np.array_equal(cases.bits(frames["accel"]), cases.bits(frames["oracle"]))
    assert np.array_equal(cases.bits(frames["ref_layout"]), cases.bits(frames["oracle"]))
    full = orc.render(orc.tree_from_view(hv), cam.c, opt)["rgba"]
    assert not np.array_equal(cases.bits(full), cases.bits(frames["oracle"]))      # the level of detail is visible
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels(tree.device_view(), cam, opt, rgba=out)                      # ... and the source tree is what it was
    torch.cuda.synchronize()
    assert np.array_equal(cases.bits(out.cpu().numpy()), cases.bits(full))


# ---------------------------------------------------------------------------------------------------- Renderer.set_lod

POSES = [((-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48)), ((-2.0, 1.9, 1.5), (-0.62, 0.6, 0.5)), ((1.2, -2.3, 1.4), (0.4, -0.78, 0.48)),
         ((2.5, 0.4, -1.2), (0.89, 0.14, -0.43)), ((0.3, 2.6, 1.0), (0.1, 0.93, 0.36))]
ORTHO_POSE = ((-1.35, 0.9, 2.25), (-0.45, 0.3, 0.75))


def _renderer(mnv, tree, capacity):
    r = mnv.Renderer()
    r.resize(W, H)
    r.set(tree, capacity)
    opt = mnv.RenderOptions.cli_defaults()
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    r.options.grid_max_depth = 3
    return r


def _walk(mnv, r, in_flight):
    """Plain frames with `in_flight` frames in flight, a grid frame, anti-aliased frames, orthographic frames: every frame's bits."""
    frames = []
    r.set_frames_in_flight(in_flight)
    r.set_antialiasing(1)
    r.set_projection(mnv.PROJ_PINHOLE)
    pending = []
    for c, b in POSES:
        r.set_camera(c, b, fx=224.0)
        r.render()
        pending.append(r.last_slot())
        if len(pending) == in_flight:
            frames.append(r.download_slot(pending.pop(0)))
    while pending:
        frames.append(r.download_slot(pending.pop(0)))
    r.options.show_grid = True
    r.render()
    frames.append(r.download_slot(r.last_slot()))
    r.options.show_grid = False
    r.set_antialiasing(4)
    for c, b in POSES[:2]:
        r.set_camera(c, b, fx=224.0)
        r.render()
        frames.append(r.download_slot(r.last_slot()))
    r.set_antialiasing(1)
    r.set_projection(mnv.PROJ_ORTHO)
    r.set_camera(*ORTHO_POSE, fx=18.0)
    r.render()
    frames.append(r.download_slot(r.last_slot()))
    r.set_projection(mnv.PROJ_PINHOLE)
    return [cases.bits(f).copy() for f in frames]


@pytest.mark.parametrize("lod", [3, 5])
def test_renderer_with_a_level_of_detail_equals_a_renderer_of_the_truncated_tree(mnv, torch_gpu, lod):
    spec = cases.CASES["sh4_d6"]["tree"]
    tree, source = cases.make_tree(mnv, spec), cases.make_tree(mnv, spec)
    source.move_to_device()
    cut = source.make_lod(lod)
    a = _renderer(mnv, tree, tree.capacity)
    b = _renderer(mnv, cut, cut.capacity)
    before = _walk(mnv, a, 3)
    a.set_lod(lod)
    for in_flight in (3, 1):
        got, want = _walk(mnv, a, in_flight), _walk(mnv, b, in_flight)
        assert len(got) == len(want) == len(POSES) + 4
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (in_flight, i)
    assert not all(np.array_equal(x, y) for x, y in zip(got, before))
    a.set_lod(0)
    after = _walk(mnv, a, 3)
    for i, (x, y) in enumerate(zip(after, before)):
        assert np.array_equal(x, y), i
    # a new tree drops the truncated ones: the same depth is now cut from the new tree
    other = mnv.N3Tree.synth_random(depth=6, basis_dim=4, seed=77)
    other_source = mnv.N3Tree.synth_random(depth=6, basis_dim=4, seed=77)
    other_source.move_to_device()
    other_cut = other_source.make_lod(lod)
    a.set(other, other.capacity)
    a.set_lod(lod)
    c = _renderer(mnv, other_cut, other_cut.capacity)
    for r in (a, c):
        r.options.basis_minmax[0], r.options.basis_minmax[1] = 0, 3
        r.set_camera(*POSES[0], fx=224.0)
        r.render()
    assert np.array_equal(cases.bits(a.download_slot(a.last_slot())), cases.bits(c.download_slot(c.last_slot())))


def test_renderer_refuses_a_level_of_detail_with_what_edits_the_tree(mnv, torch_gpu):
    tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    r = _renderer(mnv, tree, tree.capacity)
    r.set_camera(*POSES[0], fx=224.0)
    r.set_lod(3)
    r.render()
    good = cases.bits(r.download_slot(r.last_slot())).copy()

    def refused(word):
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == mnv.MNV_E_INVALID and word in str(e.value)

    r.options.use_splitting = True
    refused("set_lod")
    r.options.use_splitting = False
    r.options.use_guided_sampling = True
    refused("set_lod")
    r.options.use_guided_sampling = False
    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)         # one rank through RCCL
    try:
        r.set_ranks(comm)
        refused("set_lod")
        r.set_ranks(None)
    finally:
        r.set_ranks(None)
        comm.close()
    with pytest.raises(mnv.MnvError) as e:
        r.set_lod(-1)
    assert e.value.code == mnv.MNV_E_INVALID
    r.render()                                               # the same call renders once the obstacle is gone
    assert np.array_equal(cases.bits(r.download_slot(r.last_slot())), good)
    host_only = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    with pytest.raises(mnv.MnvError) as e:
        host_only.make_lod(3)                                # not on the device
    assert e.value.code == mnv.MNV_E_INVALID


# ---------------------------------------------------------------------------------------------------- mnv_render --lod

def test_mnv_render_lod_and_save_lod(mnv, torch_gpu, tmp_path):
    torch = torch_gpu
    assert os.path.exists(EXE), "mnv_render not built"
    tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    npz, saved, out = str(tmp_path / "scene.npz"), str(tmp_path / "lod4.npz"), str(tmp_path / "frame")
    tree.save_npz(npz)
    center, back = POSES[0]
    common = [EXE, npz, "-w", str(W), "-h", str(H), "--fx", "224", "--center", ",".join(map(str, center)), "--back", ",".join(map(str, back))]
    r = subprocess.run(common + ["--out", out, "--raw", "--frames", "1", "--lod", "4", "--save_lod", saved], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    tree.move_to_device()
    cut = tree.make_lod(4)
    back_in = mnv.N3Tree.open(saved)
    for x, y in zip(back_in.host_arrays(), cut.host_arrays()):
        assert np.array_equal(x, y)
    assert back_in.data_format == cut.data_format and list(back_in.host_view().scale) == list(cut.host_view().scale)
    cam = mnv.Camera(W, H, 224.0).set_pose(center, back)
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, 3
    want = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(cut.accel, cam, opt, rgba=want)
    torch.cuda.synchronize()
    got = np.fromfile(out + "_0000.f32", dtype=np.float32).reshape(H, W, 4)
    assert np.array_equal(cases.bits(got), cases.bits(want.cpu().numpy()))
    for extra in (["--gpus", "1"], ["--use_splitting"], ["--use_guided_sampling"]):
        bad = subprocess.run(common + ["--lod", "4"] + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--lod" in bad.stderr, extra
    bad = subprocess.run(common + ["--save_lod", saved], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--lod" in bad.stderr
