"""The points contract of include/mnv.h pinned on the host: tests/points_ref.py restates it in numpy; these tests hold the restatement to
what any tree has (links, one parent per chunk), to a brute-force dictionary of voxels, and its colour tables to their formulas.  No GPU."""
import numpy as np
import pytest

import points_ref as pr

F = np.float32
OFFSET, SCALE = np.array([0.5, 0.5, 0.5], F), np.array([0.5, 0.5, 0.5], F)


def shell_cloud(n, seed=0, radius=0.7):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    xyz = (v * radius * (1 + 0.01 * rng.normal(size=(n, 1)))).astype(F)
    rgb = np.clip(128 + 120 * v, 0, 255).astype(np.uint8)
    return xyz, rgb


def check_tree(t):
    """Every link lies in [1, capacity), every chunk but the root is reached exactly once, parent mirrors child."""
    child, parent, cap = t["child"], t["parent"], t["capacity"]
    rows, cols = np.nonzero(child)
    target = rows + child[rows, cols]
    assert ((target >= 1) & (target < cap)).all()
    assert np.array_equal(np.sort(target), np.arange(1, cap))
    assert parent[0] == -1 and np.array_equal(parent[target], rows * 8 + cols)
    assert (child[rows, cols] > 0).all()                      # breadth first: children come after their parents
    assert sum(t["stats"]["chunks_at_depth"]) == cap


@pytest.mark.parametrize("depth,fmt,min_points", [(1, "RGBA", 1), (2, "SH1", 1), (4, "RGBA", 2), (6, "SH9", 1), (8, "SH25", 3)])
def test_restated_tree_is_a_tree_and_its_voxels_are_the_brute_force_ones(depth, fmt, min_points):
    xyz, rgb = shell_cloud(3000, seed=depth)
    xyz[::97] = np.nan
    xyz[5::131] *= 3.0                                           # outside the cube
    t = pr.build(xyz, rgb, OFFSET, SCALE, depth, fmt, min_points, 50.0)
    check_tree(t)
    brute = pr.brute_force_voxels(xyz, OFFSET, SCALE, depth)
    st = t["stats"]
    assert st["accepted"] == sum(brute.values()) and st["accepted"] + st["dropped"] == xyz.shape[0] and st["dropped"] > 0
    assert st["distinct_voxels"] == len(brute)
    want = sorted(pr.code_of_cell(c, depth) for c, n in brute.items() if n >= min_points)
    assert [int(c) for c in t["occupied"]] == want and st["occupied_voxels"] == len(want)
    # the rows: sigma exactly where a depth-D voxel is occupied; counts where a chunk exists
    dd = pr.data_dim(fmt)
    lit = t["data"][..., dd - 1] != 0
    assert lit.sum() == len(want) and (t["counts"][lit] >= min_points).all()
    assert (t["data"][~lit] == 0).all() and t["counts"].sum() <= st["accepted"]
    if min_points == 1:
        assert t["counts"].sum() == st["accepted"]
    # walk down to every occupied voxel by its digits
    for code in want[:50]:
        c = 0
        for level in range(depth - 1):
            j = (code >> (3 * (depth - 1 - level))) & 7
            assert t["child"][c, j] != 0
            c += t["child"][c, j]
        assert lit[c, code & 7]


def test_restated_empty_clouds_are_one_chunk():
    for xyz in (np.zeros((0, 3), F), np.full((4, 3), np.nan, F), np.full((4, 3), 7.0, F)):
        t = pr.build(xyz, np.zeros(xyz.shape, np.uint8), OFFSET, SCALE, 5)
        assert t["capacity"] == 1 and not t["child"].any() and not t["data"].any() and t["parent"].tolist() == [-1]
        assert t["stats"]["chunks_at_depth"][1:3] == [1, 0]
    t = pr.build(np.zeros((3, 3), F), np.zeros((3, 3), np.uint8), OFFSET, SCALE, 5, min_points=4)
    assert t["capacity"] == 1 and t["stats"]["distinct_voxels"] == 1 and t["stats"]["occupied_voxels"] == 0 and not t["counts"].any()
    t = pr.build(np.zeros((3, 3), F), np.zeros((3, 3), np.uint8), OFFSET, SCALE, 1, min_points=4)     # D == 1: the root's voxels are the leaves
    assert t["capacity"] == 1 and t["counts"].sum() == 3 and not t["data"].any()


def test_restated_means_round_half_up():
    xyz = np.zeros((2, 3), F)
    for a, b, want in ((0, 1, 1), (1, 2, 2), (0, 255, 128), (255, 255, 255), (0, 0, 0), (7, 7, 7)):
        rgb = np.array([[a, a, a], [b, b, b]], np.uint8)
        t = pr.build(xyz, rgb, OFFSET, SCALE, 1, "RGBA")
        assert t["data"][0, 7, 0] == pr.colour_table("RGBA")[want] and t["data"][0, 7, 3] == np.float16(100.0).view(np.uint16)


def test_colour_tables():
    rgba = pr.colour_table("RGBA")
    assert np.array_equal(rgba, np.float16(np.float32(np.arange(256)) / np.float32(255)).view(np.uint16))
    assert rgba[0] == 0 and rgba[255] == 0x3C00
    sh = pr.colour_table("SH9").view(np.float16).astype(np.float64)
    assert np.array_equal(pr.colour_table("SH9"), pr.colour_table("SH1"))
    lo, hi = int(np.ceil(255 / 512)), int(np.floor(255 * 511 / 512))     # the means the clamp leaves alone
    assert (np.diff(sh[lo:hi + 1]) > 0).all() and sh[0] == sh[lo - 1] and sh[255] == sh[hi + 1]
    back = 1.0 / (1.0 + np.exp(-pr.C0 * sh))                      # the march's sigmoid of C0 * coefficient
    assert np.abs(back[lo:hi + 1] * 255 - np.arange(lo, hi + 1)).max() < 0.5


def test_the_oracle_renders_a_restated_tree(mnv, orc):
    xyz, rgb = shell_cloud(20000, seed=3)
    for fmt in ("RGBA", "SH4"):
        t = pr.build(xyz, rgb, OFFSET, SCALE, 5, fmt, 1, 200.0)
        check_tree(t)
        tree = mnv.N3Tree.from_arrays(t["data"], t["child"], data_format=fmt, offset=tuple(OFFSET), scale=tuple(SCALE))
        cam = mnv.orbit_camera(32, 24, 26.6, 2.6, 22.5, 20.0)
        opt = mnv.RenderOptions.cli_defaults()
        opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(tree.host_view().basis_dim - 1, 0)
        frame = orc.render(orc.tree_from_view(tree.host_view()), cam.c, opt)["rgba"]
        assert np.isfinite(frame).all() and (frame[..., 3] > 0.5).sum() > 50          # the shell is in the picture, opaque
