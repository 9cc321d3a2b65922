"""A tree from a coloured point cloud on the device (csrc/mnv_points.hip: mnv_point_tree_create / add / finish / write; N3Tree.from_points,
mnv_render --points) against tests/points_ref.py, the numpy restatement of the contract in include/mnv.h.  No tolerance anywhere: the five
arrays and the stats are compared byte for byte, frames bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import points_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")
W, H = 64, 48
F = np.float32
HALF = (np.array([0.5, 0.5, 0.5], F), np.array([0.5, 0.5, 0.5], F))      # the cube [-1, 1)^3
UNIT = (np.array([0.0, 0.0, 0.0], F), np.array([1.0, 1.0, 1.0], F))      # the cube [0, 1)^3: p == q


# ---------------------------------------------------------------------------------------------------- device calls

def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).cuda()


def _build(mnv, torch, xyz, rgb, depth, fmt="RGBA", min_points=1, sigma=100.0, cube=HALF, splits=None, nulls=(), stream=0, handle=None):
    """create, add (once, or per (begin, end) of `splits`), finish, write into arrays pre-filled with 0x55: dict like points_ref.build's."""
    xyz, rgb = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    pt = handle or mnv.PointTree(cube[0], cube[1], depth, sigma, min_points, fmt)
    x, c = _dev(torch, xyz), _dev(torch, rgb)
    torch.cuda.synchronize()
    for a, b in (splits if splits is not None else [(0, xyz.shape[0])]):
        pt.add(x[a:b], c[a:b], n=b - a, stream=stream)
    return _finish_and_write(mnv, torch, pt, nulls, stream)


def _finish_and_write(mnv, torch, pt, nulls=(), stream=0):
    st = pt.finish(stream=stream)
    cap, dd = st.capacity, pt.data_dim
    out = dict(child=torch.full((cap, 8), 0x55555555, dtype=torch.int32, device="cuda"),
               data=torch.full((cap, 8, dd), 0x5555, dtype=torch.int16, device="cuda"),
               parent=torch.full((cap,), 0x55555555, dtype=torch.int32, device="cuda"),
               sample_counts=torch.full((cap, 8), 0x5555, dtype=torch.int16, device="cuda"),
               counts=torch.full((cap, 8), 0x55555555, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    pt.write(out["child"], out["data"], None if "parent" in nulls else out["parent"], None if "sample_counts" in nulls else out["sample_counts"],
             None if "counts" in nulls else out["counts"], stream=stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["data"], got["counts"] = got["data"].view(np.uint16), got["counts"].view(np.uint32)
    got["stats"], got["capacity"] = st.as_dict(), cap
    return got


def _same(got, ref, nulls=()):
    st = dict(got["stats"])
    assert st.pop("capacity") == ref["capacity"] == got["capacity"]
    assert st == ref["stats"], (st, ref["stats"])
    for k in ("child", "data", "parent", "sample_counts", "counts"):
        if k in nulls:
            assert (got[k].view(np.uint8) == 0x55).all(), k            # left alone
            continue
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        bad = np.argwhere(got[k] != ref[k])
        assert bad.size == 0, (k, bad[:5], got[k][tuple(bad[0])], ref[k][tuple(bad[0])])


def _check(mnv, torch, xyz, rgb, depth, fmt="RGBA", min_points=1, sigma=100.0, cube=HALF, **kw):
    ref = pr.build(xyz, rgb, cube[0], cube[1], depth, fmt, min_points, sigma)
    got = _build(mnv, torch, xyz, rgb, depth, fmt, min_points, sigma, cube, **kw)
    _same(got, ref, kw.get("nulls", ()))
    return ref


def _random_cloud(n, seed, spread=0.9):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, size=(n, 3)).astype(F), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def _cell_points(cells, depth):
    """The centre of depth-`depth` cells (integer triples) in the world of UNIT: exact."""
    return ((np.asarray(cells, np.float64) + 0.5) / 2.0 ** depth).astype(F)


def shell_cloud(n=200_000, seed=11):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    xyz = (v * 0.7 * (1 + 0.004 * rng.normal(size=(n, 1)))).astype(F)
    rgb = np.clip(128 + 120 * v + rng.normal(size=(n, 3)) * 6, 0, 255).astype(np.uint8)
    return xyz, rgb


@pytest.fixture(scope="module")
def shell():
    """The 200 k point sphere shell at D = 8 and its restated trees, computed once."""
    xyz, rgb = shell_cloud()
    return dict(xyz=xyz, rgb=rgb, RGBA=pr.build(xyz, rgb, HALF[0], HALF[1], 8, "RGBA", 1, 100.0), SH9=pr.build(xyz, rgb, HALF[0], HALF[1], 8, "SH9", 1, 100.0))


# ---------------------------------------------------------------------------------------------------- sizes and runs

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025])
def test_wavefront_workgroup_and_tile_edges(mnv, torch_gpu, n):
    xyz, rgb = _random_cloud(n, 100 + n)
    ref = _check(mnv, torch_gpu, xyz, rgb, 4)
    assert ref["stats"]["accepted"] == n
    ref = _check(mnv, torch_gpu, xyz, rgb, 2, min_points=2)          # long runs: at most 64 voxels
    assert ref["stats"]["distinct_voxels"] <= 64


def test_a_run_that_spans_blocks_between_short_runs(mnv, torch_gpu):
    rng = np.random.default_rng(5)
    big = np.repeat(_cell_points([(9, 3, 4)], 5), 5000, axis=0)
    rgb = rng.integers(0, 256, size=(5002, 3), dtype=np.uint8)
    ref = _check(mnv, torch_gpu, big, rgb[:5000], 5, cube=UNIT)
    assert ref["stats"]["distinct_voxels"] == 1 and ref["counts"].max() == 5000
    before, after = _cell_points([(1, 0, 0)], 5), _cell_points([(30, 30, 30)], 5)      # a smaller and a larger code
    xyz = np.concatenate([big[:2500], after, big[2500:], before])
    ref = _check(mnv, torch_gpu, xyz, rgb, 5, cube=UNIT)
    assert sorted(ref["counts"][ref["counts"] > 0].tolist()) == [1, 1, 5000]
    cells = rng.integers(0, 2, size=(100_000, 3)) * 7                                   # 100 k points into the eight corner voxels of D = 3
    ref = _check(mnv, torch_gpu, _cell_points(cells, 3), rng.integers(0, 256, size=(100_000, 3), dtype=np.uint8), 3, cube=UNIT)
    assert ref["stats"]["distinct_voxels"] == 8 and ref["counts"].sum() == 100_000


# ---------------------------------------------------------------------------------------------------- structure

def test_every_voxel_of_depth_three(mnv, torch_gpu):
    cells = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    rgb = (cells * 36).astype(np.uint8)
    ref = _check(mnv, torch_gpu, _cell_points(cells, 3), rgb, 3, cube=UNIT)
    assert ref["capacity"] == 73 and ref["stats"]["chunks_at_depth"][1:4] == [1, 8, 64] and (ref["child"][:9] != 0).all()


def test_depth_one_and_depth_two_with_one_point(mnv, torch_gpu):
    xyz, rgb = _random_cloud(300, 3)
    ref = _check(mnv, torch_gpu, xyz, rgb, 1)
    assert ref["capacity"] == 1 and (ref["counts"] > 0).all()
    ref = _check(mnv, torch_gpu, xyz, rgb, 1, min_points=40)          # D == 1 below min_points: counts stay, rows do not
    assert ref["counts"].sum() == 300 and 0 < (ref["data"][..., 3] != 0).sum() < 8
    ref = _check(mnv, torch_gpu, np.array([[0.3, -0.6, 0.9]], F), np.array([[1, 2, 3]], np.uint8), 2)
    assert ref["capacity"] == 2 and ref["parent"].tolist() == [-1, 4 * 1 + 2 * 0 + 1]


def _chain_cells():
    base = np.array([0x155554, 0x0AAAA8, 0x13333C], np.int64)        # the low two bits of each axis clear
    return np.stack([base, base + [1, 0, 0], base + [0, 2, 0]])


def test_a_chain_twenty_one_deep_with_a_fork(mnv, torch_gpu):
    xyz = _cell_points(_chain_cells(), 21)
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    for fmt in ("RGBA", "SH4"):
        ref = _check(mnv, torch_gpu, xyz, rgb, 21, fmt, cube=UNIT)
        assert ref["capacity"] == 22 and ref["stats"]["chunks_at_depth"][1:22] == [1] * 20 + [2]
        assert (ref["counts"] > 0).sum() == 3 and (ref["child"] != 0).sum() == 21


# ---------------------------------------------------------------------------------------------------- the voxel of a point

def test_points_on_voxel_faces_cube_faces_and_outside(mnv, torch_gpu):
    D = 6
    k = np.arange(0, 64, 7, dtype=np.float64)
    on_faces = np.stack([k, k[::-1], (k * 3) % 64], -1) / 64.0                       # q = k * 2^-D exactly
    below_one = np.float32(1) - np.float32(2.0 ** -24)                               # the largest float below 1
    xyz = np.concatenate([on_faces, [[0, 0, 0], [below_one, 0, below_one], [1, 0.5, 0.5], [0.5, -0.25, 0.5], [-1e-30, 0.5, 0.5],
                                     [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0.25, 0.25, 0.25]]]).astype(F)
    rgb = np.arange(xyz.size, dtype=np.uint8).reshape(-1, 3)
    ref = _check(mnv, torch_gpu, xyz, rgb, D, cube=UNIT)
    assert ref["stats"]["dropped"] == 6 and ref["stats"]["accepted"] == xyz.shape[0] - 6
    # through offset + scale * p: 1 - 2^-24 becomes q == 1.0f (dropped), 1 - 2^-23 the largest q below 1 (the last cell)
    edge = np.array([[np.float32(1) - np.float32(2.0 ** -24), 0, 0], [np.float32(1) - np.float32(2.0 ** -23), 0, 0], [-1, -1, -1]], F)
    ref = _check(mnv, torch_gpu, edge, rgb[:3], D)
    assert ref["stats"]["dropped"] == 1 and ref["stats"]["accepted"] == 2
    code, ok = pr.voxel_codes(edge, HALF[0], HALF[1], D)
    assert ok.tolist() == [False, True, True] and int(code[2]) == 0 and int(code[1]) >> (3 * D - 3) == 4 + 2 + 1
    # a dropped point first, in the middle and last of a batch; a batch of dropped points alone
    xyz, rgb = _random_cloud(200, 8)
    for where in (0, 100, 199):
        bad = xyz.copy()
        bad[where] = [np.nan, 5.0, -np.inf]
        ref = _check(mnv, torch_gpu, bad, rgb, 4)
        assert ref["stats"]["dropped"] == 1
    ref = _check(mnv, torch_gpu, np.full((70, 3), 3.0, F), rgb[:70], 4)
    assert ref["capacity"] == 1 and ref["stats"]["dropped"] == 70 and ref["stats"]["distinct_voxels"] == 0
    # ... and beside points of the largest code, with which dropped points sort
    xyz = np.concatenate([np.full((3, 3), 0.99, F), np.full((5, 3), np.nan, F), np.full((2, 3), 0.99, F)])
    ref = _check(mnv, torch_gpu, xyz, rgb[:10], 4)
    assert ref["stats"]["dropped"] == 5 and ref["counts"].max() == 5 and ref["stats"]["distinct_voxels"] == 1


def test_unequal_scales_and_an_offset(mnv, torch_gpu):
    rng = np.random.default_rng(21)
    cube = (np.array([0.4, 0.55, 0.5], F), np.array([0.5, 0.125, 0.03], F))
    xyz = (rng.uniform(-1, 1, size=(4000, 3)) * [1.1, 4.2, 17.0]).astype(F)
    ref = _check(mnv, torch_gpu, xyz, rng.integers(0, 256, size=(4000, 3), dtype=np.uint8), 7, "SH4", cube=cube)
    assert ref["stats"]["dropped"] > 100 and ref["stats"]["accepted"] > 2000


def test_min_points_on_counts_one_four_five_six(mnv, torch_gpu):
    cells = [(1, 1, 1)] * 1 + [(2, 5, 3)] * 4 + [(7, 0, 6)] * 5 + [(4, 4, 0)] * 6
    xyz = _cell_points(cells, 3)
    rgb = np.random.default_rng(2).integers(0, 256, size=(16, 3), dtype=np.uint8)
    for mp, occupied in ((1, 4), (2, 3), (5, 2), (6, 1)):
        ref = _check(mnv, torch_gpu, xyz, rgb, 3, min_points=mp, cube=UNIT)
        assert ref["stats"]["occupied_voxels"] == occupied and ref["stats"]["distinct_voxels"] == 4
    ref = _check(mnv, torch_gpu, xyz, rgb, 3, min_points=7, cube=UNIT)                 # above every count
    assert ref["capacity"] == 1 and not ref["counts"].any() and not ref["data"].any()


def test_colour_means_that_land_on_a_half(mnv, torch_gpu):
    cells = [(0, 0, 0)] * 2 + [(1, 0, 0)] * 2 + [(2, 0, 0)] * 2 + [(3, 0, 0)] * 3 + [(4, 0, 0)] * 3
    rgb = np.array([[0, 1, 0], [1, 0, 0], [1, 2, 3], [2, 1, 0], [0, 255, 127], [255, 0, 128], [0, 0, 0], [0, 0, 0], [0, 0, 0],
                    [255, 255, 255], [255, 255, 255], [255, 255, 255]], np.uint8)
    for fmt in ("RGBA", "SH1"):
        ref = _check(mnv, torch_gpu, _cell_points(cells, 3), rgb, 3, fmt, cube=UNIT)
        t = pr.colour_table(fmt)
        rows = ref["data"][ref["data"][..., 3] != 0]
        assert sorted(map(tuple, rows[:, :3].tolist())) == sorted([(t[1], t[1], t[0]), (t[2], t[2], t[2]), (t[128], t[128], t[128]), (t[0],) * 3, (t[255],) * 3])


@pytest.mark.parametrize("fmt", ["RGBA", "SH1", "SH9", "SH25"])
def test_row_formats(mnv, torch_gpu, fmt):
    xyz, rgb = _random_cloud(3000, 31)
    ref = _check(mnv, torch_gpu, xyz, rgb, 5, fmt, sigma=37.5)
    dd = pr.data_dim(fmt)
    lit = ref["data"][..., dd - 1] != 0
    assert lit.sum() > 2000 and (ref["data"][lit][:, dd - 1] == np.float16(37.5).view(np.uint16)).all()
    assert np.array_equal(mnv.points_colour_table(fmt), pr.colour_table(fmt))           # (the table the device was given)


# ---------------------------------------------------------------------------------------------------- order, calls, handles

def test_shell_cloud_in_any_order_and_any_split(mnv, torch_gpu, shell):
    torch = torch_gpu
    xyz, rgb, ref = shell["xyz"], shell["rgb"], shell["RGBA"]
    n = xyz.shape[0]
    assert ref["capacity"] > 10_000 and ref["stats"]["chunks_at_depth"][8] > 5_000 and ref["stats"]["accepted"] == n
    _same(_build(mnv, torch, xyz, rgb, 8), ref)
    perm = np.random.default_rng(1).permutation(n)
    _same(_build(mnv, torch, xyz[perm], rgb[perm], 8), ref)
    _same(_build(mnv, torch, xyz, rgb, 8, splits=[(0, 70_001), (70_001, 70_001), (70_001, n)]), ref)       # three calls, one of them empty
    cuts = [0, 1, 64, 5_000, 5_513, 99_999, 100_000, n]
    _same(_build(mnv, torch, xyz, rgb, 8, splits=list(zip(cuts[:-1], cuts[1:]))), ref)                     # seven calls of unequal sizes
    _same(_build(mnv, torch, xyz, rgb, 8, "SH9"), shell["SH9"])


def test_add_after_finish(mnv, torch_gpu):
    torch = torch_gpu
    xyz, rgb = _random_cloud(5000, 41)
    pt = mnv.PointTree(HALF[0], HALF[1], 6, 100.0, 2, "RGBA")
    lib = mnv.lib()
    one = torch.zeros((64, 8, 4), dtype=torch.int16, device="cuda")
    links = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
    assert lib.mnv_point_tree_write(pt._h, links.data_ptr(), one.data_ptr(), None, None, None, None) == mnv.MNV_E_INVALID      # before finish
    first = _build(mnv, torch, xyz[:2000], rgb[:2000], 6, handle=pt)
    _same(first, pr.build(xyz[:2000], rgb[:2000], HALF[0], HALF[1], 6, "RGBA", 2))
    x, c = _dev(torch, xyz[2000:]), _dev(torch, rgb[2000:])
    pt.add(x, c)
    assert lib.mnv_point_tree_write(pt._h, links.data_ptr(), one.data_ptr(), None, None, None, None) == mnv.MNV_E_INVALID      # a finish is due again
    _same(_finish_and_write(mnv, torch, pt), pr.build(xyz, rgb, HALF[0], HALF[1], 6, "RGBA", 2))
    # refusals that need a handle
    st = mnv.PointsStats()
    assert lib.mnv_point_tree_add(pt._h, x.data_ptr(), c.data_ptr(), -1, None) == mnv.MNV_E_INVALID
    assert lib.mnv_point_tree_add(pt._h, None, c.data_ptr(), 4, None) == mnv.MNV_E_INVALID
    assert lib.mnv_point_tree_add(pt._h, x.data_ptr(), None, 4, None) == mnv.MNV_E_INVALID
    host = np.zeros((4, 3), F)
    assert lib.mnv_point_tree_add(pt._h, host.ctypes.data, c.data_ptr(), 4, None) == mnv.MNV_E_INVALID                          # a host pointer
    assert lib.mnv_point_tree_finish(pt._h, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_point_tree_finish(pt._h, C.byref(st), None) == mnv.MNV_OK
    big = torch.zeros((st.capacity * 8 * 4 + 8,), dtype=torch.int16, device="cuda")
    links = torch.zeros((st.capacity, 8), dtype=torch.int32, device="cuda")
    assert lib.mnv_point_tree_write(pt._h, links.data_ptr(), big.data_ptr() + 2, None, None, None, None) == mnv.MNV_E_INVALID   # misaligned rows
    assert lib.mnv_point_tree_write(pt._h, None, big.data_ptr(), None, None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_point_tree_write(pt._h, links.data_ptr(), big.data_ptr(), None, None, None, None) == mnv.MNV_OK
    torch.cuda.synchronize()


def test_two_handles_on_two_streams(mnv, torch_gpu):
    torch = torch_gpu
    a_xyz, a_rgb = _random_cloud(20_000, 51)
    b_xyz, b_rgb = _random_cloud(30_000, 52, spread=0.5)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = mnv.PointTree(HALF[0], HALF[1], 6, 100.0, 1, "RGBA")
    b = mnv.PointTree(HALF[0], HALF[1], 7, 60.0, 2, "SH4")
    ax, ac, bx, bc = _dev(torch, a_xyz), _dev(torch, a_rgb), _dev(torch, b_xyz), _dev(torch, b_rgb)
    torch.cuda.synchronize()
    for lo in range(0, 30_000, 10_000):
        if lo < 20_000:
            a.add(ax[lo:lo + 10_000], ac[lo:lo + 10_000], stream=s1.cuda_stream)
        b.add(bx[lo:lo + 10_000], bc[lo:lo + 10_000], stream=s2.cuda_stream)
    _same(_finish_and_write(mnv, torch, b, stream=s2.cuda_stream), pr.build(b_xyz, b_rgb, HALF[0], HALF[1], 7, "SH4", 2, 60.0))
    _same(_finish_and_write(mnv, torch, a, stream=s1.cuda_stream), pr.build(a_xyz, a_rgb, HALF[0], HALF[1], 6, "RGBA", 1, 100.0))


@pytest.mark.parametrize("null", ["counts", "parent", "sample_counts"])
def test_optional_outputs(mnv, torch_gpu, null):
    xyz, rgb = _random_cloud(2000, 61)
    _check(mnv, torch_gpu, xyz, rgb, 5, "SH4", nulls=(null,))


# ---------------------------------------------------------------------------------------------------- frames

def _frame_pair(mnv, orc, torch, tree, cam):
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(tree.host_view().basis_dim - 1, 0)
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(tree.accel, cam, opt, rgba=out)
    torch.cuda.synchronize()
    want = orc.render(orc.tree_from_view(tree.host_view()), cam.c, opt)["rgba"]
    return out.cpu().numpy(), want


CAMERAS = dict(outside=lambda mnv: mnv.orbit_camera(W, H, 53.2, 2.6, 22.5, 20.0),
               inside=lambda mnv: mnv.Camera(W, H, 40.0).set_pose((0.1, -0.05, 0.15), (-0.6, 0.64, 0.48)))


@pytest.mark.parametrize("which", ["full_d3", "shell_rgba", "shell_sh9", "chain_d21"])
def test_frames_of_a_built_tree_equal_the_oracle(mnv, orc, torch_gpu, shell, which):
    torch = torch_gpu
    if which == "full_d3":
        cells = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
        xyz, rgb, depth, fmt, sigma = _cell_points(cells, 3) * 2 - 1, (cells * 36).astype(np.uint8), 3, "RGBA", 3.0
    elif which == "chain_d21":
        xyz, rgb, depth, fmt, sigma = _cell_points(_chain_cells(), 21) * 2 - 1, np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8), 21, "SH4", 60000.0
    else:
        xyz, rgb, depth, fmt, sigma = shell["xyz"], shell["rgb"], 8, which[6:].upper(), 100.0
    tree, st = mnv.N3Tree.from_points(xyz, rgb, depth=depth, sigma=sigma, data_format=fmt, cube=HALF, return_stats=True)
    ref = shell[fmt] if which.startswith("shell") else pr.build(xyz, rgb, HALF[0], HALF[1], depth, fmt, 1, sigma)
    data, child, parent = tree.host_arrays()
    assert np.array_equal(data, ref["data"]) and np.array_equal(child, ref["child"]) and np.array_equal(parent, ref["parent"])
    assert st.capacity == tree.capacity == ref["capacity"] and tree.data_format == fmt
    seen = 0
    for name, make in CAMERAS.items():
        got, want = _frame_pair(mnv, orc, torch, tree, make(mnv))
        assert np.array_equal(cases.bits(got), cases.bits(want)), name
        seen += int((want[..., 3] > 0).sum())
    assert seen > 0 or which == "chain_d21"                 # (three voxels of 2^-21 are not in every picture)


def test_lod_and_surface_of_the_shell_tree(mnv, torch_gpu, shell):
    tree = mnv.N3Tree.from_points(shell["xyz"], shell["rgb"], depth=8, sigma=100.0, data_format="SH9", cube=HALF)
    lod = tree.make_lod(6)
    at = shell["SH9"]["stats"]["chunks_at_depth"]
    assert lod.capacity == sum(at[1:7])
    surface = mnv.extract_surface(lod.accel, 6, 1.0)
    vert, faces = surface.vertices(), surface.faces().astype(np.int64).reshape(-1, 3)
    assert vert.shape[0] > 1000 and faces.shape[0] > 2000
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])              # closed: every directed edge has its reverse
    nv = vert.shape[0]
    assert np.array_equal(np.sort(e[:, 0] * nv + e[:, 1]), np.sort(e[:, 1] * nv + e[:, 0]))


# ---------------------------------------------------------------------------------------------------- round trip

def _leaves(data, child):
    """(depth, cell, chunk, j) of every voxel without a child, and the set of (depth, cell above) of every chunk."""
    out, chunks, todo = [], set(), [(0, 1, (0, 0, 0))]
    while todo:
        c, d, corner = todo.pop()
        chunks.add((d, corner))
        for j in range(8):
            cell = (2 * corner[0] + (j >> 2), 2 * corner[1] + ((j >> 1) & 1), 2 * corner[2] + (j & 1))
            if child[c, j]:
                todo.append((c + child[c, j], d + 1, cell))
            else:
                out.append((d, cell, c, j))
    return out, chunks


def test_round_trip_through_the_leaf_centres_of_a_shell_tree(mnv, torch_gpu):
    src = mnv.N3Tree.synth_shell(depth=5, basis_dim=4, radius=0.3, half_thickness=0.04)
    data, child, _ = src.host_arrays()
    dd = data.shape[2]
    leaves, _ = _leaves(data, child)
    lit = [(d, cell) for d, cell, c, j in leaves if data[c, j, dd - 1].view(np.float16) > 0]
    assert len(lit) > 500 and all(d == 5 for d, _ in lit)          # the shell is at full depth
    hv = src.host_view()
    offset, scale = np.array(hv.offset[:], F), np.array(hv.scale[:], F)
    u = _cell_points([cell for _, cell in lit], 5)
    xyz = ((u - offset) / scale).astype(F)
    assert np.array_equal(offset + scale * xyz, u)                  # the way back is exact
    tree, st = mnv.N3Tree.from_points(xyz, None, depth=5, sigma=50.0, data_format="SH4", cube=(offset, scale), return_stats=True)
    got_data, got_child, _ = tree.host_arrays()
    got_leaves, got_chunks = _leaves(got_data, got_child)
    got_lit = {(d, cell) for d, cell, c, j in got_leaves if got_data[c, j, dd - 1] != 0}
    assert got_lit == set(lit) and st.occupied_voxels == len(lit) == st.accepted
    # a chunk of the built tree exists exactly where the source has a chunk with a lit leaf beneath
    want_chunks = {(1, (0, 0, 0))}
    for d, cell in lit:
        for up in range(1, d):
            want_chunks.add((d - up + 1, tuple(x >> up for x in cell)))
    assert got_chunks == want_chunks
    white = pr.colour_table("SH4")[255]
    rows = got_data[got_data[..., dd - 1] != 0]
    assert (rows[:, [0, 4, 8]] == white).all()


# ---------------------------------------------------------------------------------------------------- Python level, command line

def test_from_points_save_and_open(mnv, torch_gpu, tmp_path):
    torch = torch_gpu
    xyz, rgb = _random_cloud(20_000, 71)
    tree, st = mnv.N3Tree.from_points(torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda(), depth=6, sigma=80.0, min_points=2, data_format="SH9",
                                      cube=HALF, return_stats=True)
    ref = pr.build(xyz, rgb, HALF[0], HALF[1], 6, "SH9", 2, 80.0)
    st = st.as_dict()
    assert st.pop("capacity") == ref["capacity"] and st == ref["stats"]
    path = str(tmp_path / "built.npz")
    tree.save_npz(path)
    back = mnv.N3Tree.open(path)
    for x, y, z in zip(back.host_arrays(), tree.host_arrays(), (ref["data"], ref["child"], ref["parent"])):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert back.data_format == tree.data_format == "SH9" and list(back.host_view().scale) == [0.5, 0.5, 0.5]
    dv = tree.device_view()
    assert dv.parent and dv.sample_counts and tree.accel
    empty = mnv.N3Tree.from_points(np.zeros((0, 3), F), depth=4)                       # no point at all: the one-chunk tree
    assert empty.capacity == 1 and not empty.host_arrays()[0].any()
    with pytest.raises(mnv.MnvError) as e:
        mnv.N3Tree.from_points(xyz, rgb, depth=22)
    assert e.value.code == mnv.MNV_E_INVALID


def test_mnv_render_points(mnv, torch_gpu, tmp_path):
    torch = torch_gpu
    assert os.path.exists(EXE), "mnv_render not built"
    xyz, rgb = shell_cloud(30_000, seed=81)
    cloud, saved, out = str(tmp_path / "cloud.npz"), str(tmp_path / "out.npz"), str(tmp_path / "frame")
    np.savez(cloud, points=xyz, colors=rgb)
    center, back = (-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48)
    common = ["-w", str(W), "-h", str(H), "--fx", "60", "--center", ",".join(map(str, center)), "--back", ",".join(map(str, back))]
    r = subprocess.run([EXE, "--points", cloud, "--points_depth", "6", "--save_lod", saved, "--out", out, "--raw", "--frames", "1"] + common,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "points: 30000 point(s), 30000 accepted, 0 dropped" in r.stdout and "per depth: 1 8 " in r.stdout
    tree = mnv.N3Tree.from_points(xyz, rgb, depth=6)                                   # the same defaults: the cloud's own cube
    back_in = mnv.N3Tree.open(saved)
    for x, y in zip(back_in.host_arrays(), tree.host_arrays()):
        assert np.array_equal(x, y)
    assert list(back_in.host_view().scale) == list(tree.host_view().scale) and list(back_in.host_view().offset) == list(tree.host_view().offset)
    cam = mnv.Camera(W, H, 60.0).set_pose(center, back)
    opt = mnv.RenderOptions.cli_defaults()
    want = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(tree.accel, cam, opt, rgba=want)
    torch.cuda.synchronize()
    got = np.fromfile(out + "_0000.f32", dtype=np.float32).reshape(H, W, 4)
    assert np.array_equal(cases.bits(got), cases.bits(want.cpu().numpy())) and (got[..., 3] > 0.5).sum() > 100
    # an .obj cloud: v x y z r g b, float colours to 8 bits
    obj = str(tmp_path / "cloud.obj")
    with open(obj, "w") as f:
        for p, c in zip(xyz[:500], rgb[:500]):
            f.write("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % (p[0], p[1], p[2], c[0] / 255.0, c[1] / 255.0, c[2] / 255.0))
    saved2 = str(tmp_path / "out2.npz")
    r = subprocess.run([EXE, "--points", obj, "--points_depth", "5", "--points_format", "SH4", "--points_min", "2", "--points_cube", "0.5,0.5,0.5,0.5,0.5,0.5",
                        "--save_lod", saved2, "--frames", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    ref = pr.build(xyz[:500], rgb[:500], HALF[0], HALF[1], 5, "SH4", 2, 100.0)
    from_obj = mnv.N3Tree.open(saved2)                                                 # (host_arrays are views: the tree must outlive them)
    data, child, parent = from_obj.host_arrays()
    assert np.array_equal(data, ref["data"]) and np.array_equal(child, ref["child"]) and np.array_equal(parent, ref["parent"])
