"""N3Tree::gen_wireframe on the host (reference n3tree.cpp:249-329): the vertex list of the grid overlay, in the reference's order and float
arithmetic, through the C ABI (mnv_n3tree_gen_wireframe) and the binding."""
import ctypes as C

import numpy as np
import pytest

import cases
import wireframe_ref


def _check_tree(mnv, tree, depths):
    v = tree.host_view()
    _, child, _ = tree.host_arrays()
    tree_depth = 0
    for d in depths:
        got = tree.gen_wireframe(d)
        want = wireframe_ref.gen_wireframe(child, list(v.offset), list(v.scale), d)
        assert got.dtype == np.float32 and got.shape == want.shape and got.shape[1] == 9, (d, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), d
        level, _ = wireframe_ref.wireframe_cubes(child, d)
        tree_depth = max(tree_depth, int(level.max()))
    return tree_depth


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_gen_wireframe_equals_the_restatement_on_random_trees(mnv, depth):
    tree = mnv.N3Tree.synth_random(depth=depth, basis_dim=1, refine_prob=0.6, empty_prob=0.5, seed=40 + depth,
                                   offset=(0.45, 0.5, 0.55), scale=(0.6, 0.5, 0.4))
    full = _check_tree(mnv, tree, [-1, 0, 1, 3, depth, depth + 3])
    assert full == depth - 1   # a depth-`depth` tree has chunks on levels 0 .. depth - 1
    assert np.array_equal(tree.gen_wireframe(-1), tree.gen_wireframe(0))          # a negative max_depth acts like 0
    assert np.array_equal(tree.gen_wireframe(), tree.gen_wireframe(depth + 3))    # the default draws every leaf


@pytest.mark.parametrize("name", ["sh9_d7_aniso", "terrain_d7_aniso"])
def test_gen_wireframe_on_the_anisotropic_trees(mnv, name):
    tree = cases.make_tree(mnv, cases.CASES[name]["tree"])
    _check_tree(mnv, tree, [-1, 0, 1, 3, 7, 100000])


def test_one_chunk_tree_by_hand(mnv):
    """synth_random(depth=1): the root chunk only, eight cubes of half the unit cube; offset / scale 0.5 map it to [-1, 1]^3."""
    tree = mnv.N3Tree.synth_random(depth=1, basis_dim=1, seed=3)
    assert tree.capacity == 1
    got = tree.gen_wireframe(4)
    assert got.shape == (8 * 24, 9)
    want = []
    for c in range(8):
        i, j, k = c >> 2, (c >> 1) & 1, c & 1
        lo = [-1.0 + i, -1.0 + j, -1.0 + k]
        hi = [lo[0] + 1.0, lo[1] + 1.0, lo[2] + 1.0]
        bb = lo + hi
        for a in range(2):
            for b in range(2):
                for sel in [(0, a, b), (1, a, b), (a, 0, b), (a, 1, b), (a, b, 0), (a, b, 1)]:
                    want.append([bb[sel[0] * 3], bb[sel[1] * 3 + 1], bb[sel[2] * 3 + 2], 0, 0, 0, 0, 0, 1])
    assert np.array_equal(got, np.float32(want))


def test_c_abi_error_paths(mnv):
    lib = mnv.lib()
    tree = mnv.N3Tree.synth_random(depth=3, basis_dim=1, seed=5)
    need = tree.gen_wireframe(2).size
    n = C.c_int64(-1)
    assert lib.mnv_n3tree_gen_wireframe(tree._h, 2, None, 0, C.byref(n)) == mnv.MNV_OK and n.value == need
    small = np.zeros(need - 1, np.float32)
    n = C.c_int64(-1)
    assert lib.mnv_n3tree_gen_wireframe(tree._h, 2, small.ctypes.data, small.size, C.byref(n)) == mnv.MNV_E_INVALID
    assert n.value == need                                  # the size it needs
    assert not small.any()                                  # nothing written
    assert lib.mnv_n3tree_gen_wireframe(None, 2, None, 0, C.byref(n)) == mnv.MNV_E_INVALID
    assert lib.mnv_n3tree_gen_wireframe(tree._h, 2, None, 5, C.byref(n)) == mnv.MNV_E_INVALID


def test_wireframe_entry_points_refuse_null_arguments(mnv):
    lib = mnv.lib()
    cam = mnv.Camera(16, 16, 20.0)
    opt = mnv.RenderOptions.defaults()
    assert lib.mnv_render_wireframe(None, C.byref(cam.c), C.byref(opt), mnv.Rect(0, 0, 16, 16), None, None, None) == mnv.MNV_E_INVALID
    n = C.c_int64(-1)
    assert lib.mnv_wireframe_segments(None, None, 0, C.byref(n), None) == mnv.MNV_E_INVALID
    assert lib.mnv_wireframe_update(None, None, 0, None) == mnv.MNV_E_INVALID
    out = C.c_void_p()
    assert lib.mnv_wireframe_create(None, 0, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_wireframe_cube_count(None) == 0 and lib.mnv_renderer_wireframe(None) is None
    assert lib.mnv_wireframe_set_method(None, mnv.WIREFRAME_BINNED) == mnv.MNV_E_INVALID
    assert lib.mnv_renderer_camera(None, None) == mnv.MNV_E_INVALID
    del out


def test_a_child_link_outside_the_tree_is_invalid(mnv):
    """The same status as the device walk (mnv_wireframe_create): MNV_E_INVALID, not an I/O error."""
    child = np.zeros((2, 8), np.int32)
    child[0, 3] = 1
    child[1, 5] = 7                     # chunk 8 does not exist
    data = np.zeros((2, 8, 4), np.float16)
    # parents given: from_arrays derives missing parents from the child links, which a link outside the tree cannot give
    tree = mnv.N3Tree.from_arrays(data, child, data_format="SH1", parent=np.int32([-1, 3]))
    with pytest.raises(mnv.MnvError) as e:
        tree.gen_wireframe(10)
    assert e.value.code == mnv.MNV_E_INVALID
    assert tree.gen_wireframe(0).shape == (8 * 24, 9)   # the walk stops above the bad link
