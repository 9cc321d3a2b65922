"""The host half of the mesh pass (no GPU): mnv_model_matrix against a double-precision Rodrigues formula, the OBJ reader against
hand-written fixtures, the numpy restatement of the raster contract on line meshes against the grid pass's restatement, and the argument
checks of the device entry points."""
import ctypes as C

import numpy as np
import pytest

import cases
import mesh_ref
import wireframe_ref


# ------------------------------------------------------------------------------------------------ the model matrix

def test_model_matrix_equals_rodrigues_in_double(mnv):
    """Bound 1e-6: the matrix is computed in double and rounded once; its entries are at most scale <= 10 in magnitude (translations are
    copied), and one float rounding of a value <= 10 is at most 2^-24 * 16 = 9.5e-7 (6e-7 for values below 8)."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for i in range(200):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = [1.1e-3, 0.5, np.pi / 2, 3.0, np.pi][i % 5] if i < 10 else rng.uniform(1.1e-3, np.pi)
        rot = np.float32(axis * angle)
        tr = np.float32(rng.uniform(-5, 5, size=3))
        scale = [1.0, 10.0, 0.01][i % 3] if i < 9 else float(rng.uniform(0.01, 10.0))
        got = mnv.model_matrix(rot, tr, scale)
        want = mesh_ref.model_matrix(rot, tr, scale)
        assert got.dtype == np.float32 and got.shape == (3, 4)
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        assert np.array_equal(got[:, 3], tr)
    assert worst <= 1e-6, worst


def test_model_matrix_below_the_threshold_is_identity_times_scale(mnv):
    for rot in [(0, 0, 0), (9e-4, 0, 0), (5e-4, 5e-4, 5e-4), (0, -9.99e-4, 0)]:
        for scale in (1.0, 2.5, 10.0):
            got = mnv.model_matrix(rot, (1.0, -2.0, 3.0), scale)
            want = np.zeros((3, 4), np.float32)
            want[0, 0] = want[1, 1] = want[2, 2] = np.float32(scale)
            want[:, 3] = (1.0, -2.0, 3.0)
            assert np.array_equal(got, want), (rot, scale)
    assert mnv.model_matrix((1.1e-3, 0, 0), (0, 0, 0), 1.0)[1, 2] != 0      # just above: a rotation
    assert mnv.lib().mnv_model_matrix(None, None, 1.0, None) == mnv.MNV_E_INVALID


# ------------------------------------------------------------------------------------------------ the OBJ reader

OBJ_NORMALS = """# a quad and a triangle, every f form that carries a normal
v 0 0 0
v 1 0 0 0.25 0.5 0.75
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
vn 0 1 0
f 1//1 2//1 3//1 4//1
f -4/1/2 -3/1/2 3//1
"""


def test_obj_with_normals_is_indexed_and_fanned(mnv, tmp_path):
    p = tmp_path / "a.obj"
    p.write_text(OBJ_NORMALS)
    vert, faces, fs = mnv.obj_read(str(p), color=(0.5, 0.25, 1.0))
    d = [0.5, 0.25, 1.0]
    P = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
    col = [d, [0.25, 0.5, 0.75], d, d]
    # (v, vn) pairs in order of first use: (1,1) (2,1) (3,1) (4,1) (1,2) (2,2)
    want = [P[0] + col[0] + [0, 0, 1], P[1] + col[1] + [0, 0, 1], P[2] + col[2] + [0, 0, 1], P[3] + col[3] + [0, 0, 1],
            P[0] + col[0] + [0, 1, 0], P[1] + col[1] + [0, 1, 0]]
    assert fs == 3 and np.array_equal(vert, np.float32(want))
    assert np.array_equal(faces, np.uint32([[0, 1, 2], [0, 2, 3], [4, 5, 2]]))   # the quad fanned, then -4 -> v1, -3 -> v2


OBJ_PLAIN = """v 0 0 0
v 2 0 0
v 2 2 0
v 0 2 0
vt 0.5 0.5
f 1 2 3 4
f 1/1 3/1 2/1
"""


def test_obj_without_normals_gets_face_normals_and_unshared_vertices(mnv, tmp_path):
    p = tmp_path / "b.obj"
    p.write_text(OBJ_PLAIN)
    vert, faces, fs = mnv.obj_read(str(p))
    assert fs == 3 and faces is None and vert.shape == (9, 9)
    P = np.float32([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]])
    order = [0, 1, 2, 0, 2, 3, 0, 2, 1]
    assert np.array_equal(vert[:, 0:3], P[order])
    assert np.array_equal(vert[:, 3:6], np.ones((9, 3), np.float32))              # the default colour is white
    assert np.array_equal(vert[:6, 6:9], np.float32([[0, 0, 1]] * 6)) and np.array_equal(vert[6:, 6:9], np.float32([[0, 0, -1]] * 3))


def test_obj_polylines_and_points(mnv, tmp_path):
    p = tmp_path / "c.obj"
    p.write_text("v 0 0 0 1 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 1\nl 1 2 3\nl -1 1\n")
    vert, faces, fs = mnv.obj_read(str(p), color=(0.0, 0.0, 0.0))
    assert fs == 2 and vert.shape == (4, 9)
    assert np.array_equal(faces, np.uint32([[0, 1], [1, 2], [3, 0]]))
    assert np.array_equal(vert[:, 6:9], np.float32([[0, 0, 1]] * 4)) and np.array_equal(vert[0, 3:6], np.float32([1, 0, 0]))
    assert np.array_equal(vert[1:, 3:6], np.zeros((3, 3), np.float32))
    q = tmp_path / "d.obj"
    q.write_text("v 1 2 3\nv 4 5 6\n")
    vert, faces, fs = mnv.obj_read(str(q))
    assert fs == 1 and faces is None and np.array_equal(vert[:, 0:3], np.float32([[1, 2, 3], [4, 5, 6]]))


@pytest.mark.parametrize("text, line", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4),            # an index outside the file
    ("v 0 0 0\nv 1 0 x\n", 2),                               # a malformed number
    ("v 0 0 0\nv 1 0 0\n\n# c\nf 1 2\n", 5),                 # a face with two corners
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nl 1 2\n", 5),      # faces and polylines in one file
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//2\n", 5),   # a normal index outside the file
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", 4),             # index 0
])
def test_obj_malformed_input_names_the_line(mnv, tmp_path, text, line):
    p = tmp_path / "bad.obj"
    p.write_text(text)
    with pytest.raises(mnv.MnvError) as e:
        mnv.obj_read(str(p))
    assert e.value.code == mnv.MNV_E_IO and f"line {line}:" in str(e.value), str(e.value)


def test_obj_read_size_query_and_missing_file(mnv, tmp_path):
    lib = mnv.lib()
    p = tmp_path / "a.obj"
    p.write_text(OBJ_NORMALS)
    nf, ni, fs = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    assert lib.mnv_obj_read(str(p).encode(), None, None, 0, C.byref(nf), None, 0, C.byref(ni), C.byref(fs)) == mnv.MNV_OK
    assert (nf.value, ni.value, fs.value) == (54, 9, 3)
    small = np.zeros(53, np.float32)
    idx = np.zeros(9, np.uint32)
    assert lib.mnv_obj_read(str(p).encode(), None, small.ctypes.data, 53, C.byref(nf), idx.ctypes.data, 9, C.byref(ni), C.byref(fs)) == mnv.MNV_E_INVALID
    assert not small.any() and nf.value == 54
    assert lib.mnv_obj_read(str(tmp_path / "none.obj").encode(), None, None, 0, C.byref(nf), None, 0, C.byref(ni), C.byref(fs)) == mnv.MNV_E_IO
    assert lib.mnv_obj_read(None, None, None, 0, None, None, 0, None, None) == mnv.MNV_E_INVALID


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("name, tile", [("sh4_d6", None), ("terrain_d7_aniso", (37, 21, 75, 53)), ("camera_inside", None)])
def test_mesh_ref_on_line_meshes_equals_the_wireframe_restatement(mnv, name, tile):
    spec = cases.CASES[name]
    tree = cases.make_tree(mnv, spec["tree"])
    cam = cases.make_camera(mnv, spec["camera"])
    tile = tile or (0, 0, cam.width, cam.height)
    total = 0
    for depth in (0, 3):
        verts = tree.gen_wireframe(depth)
        for bg in (0.0, 0.5):
            want_t, want_i = wireframe_ref.raster(wireframe_ref.segments_from_vertices(verts), cam.c, tile, bg)
            got_t, got_i = mesh_ref.render([mesh_ref.RefMesh(verts, None, 2, unlit=True)], cam.c, tile, bg)
            assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)) and np.array_equal(got_i, want_i), (depth, bg)
            total += int((want_t != np.float32(1e9)).sum())
    assert total > 500


# ------------------------------------------------------------------------------------------------ argument checks

def _tri():
    v = np.zeros((3, 9), np.float32)
    v[:, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    return v


def test_mesh_entry_points_check_their_arguments_before_the_device(mnv):
    lib = mnv.lib()
    v = _tri()
    h = C.c_void_p()
    idx = np.uint32([0, 1, 2])

    def create(vert, n_verts, faces, n_idx, fs):
        return lib.mnv_mesh_create(vert.ctypes.data if vert is not None else None, n_verts, faces.ctypes.data if faces is not None else None, n_idx, fs, 0,
                                   C.byref(h))

    for fs in (0, 4, -1):
        assert create(v, 3, idx, 3, fs) == mnv.MNV_E_INVALID                    # another face_size
    assert create(v, 3, np.uint32([0, 1, 3]), 3, 3) == mnv.MNV_E_INVALID        # an index >= n_verts
    assert create(v, 3, np.uint32([0, 1, 2, 0]), 4, 3) == mnv.MNV_E_INVALID     # an index count that is no multiple of face_size
    assert create(v, 3, None, 0, 2) == mnv.MNV_E_INVALID                        # a vertex count that is no multiple of face_size
    assert create(None, 3, idx, 3, 3) == mnv.MNV_E_INVALID                      # null vertices
    assert create(v, 3, None, 3, 3) == mnv.MNV_E_INVALID                        # a count without indices
    assert create(v, 0, None, 0, 3) == mnv.MNV_E_INVALID
    assert lib.mnv_mesh_create(v.ctypes.data, 3, None, 0, 3, 0, None) == mnv.MNV_E_INVALID
    assert h.value is None
    rc = create(v, 3, idx, 3, 3)                                                # valid arrays: the device is the only thing missing
    if mnv.device_count() == 0:
        assert rc == mnv.MNV_E_NO_DEVICE and h.value is None
    else:
        assert rc == mnv.MNV_OK
        lib.mnv_mesh_destroy(h)
    # null handles
    assert lib.mnv_mesh_update(None, v.ctypes.data, 3, None, 0, 3, 0) == mnv.MNV_E_INVALID
    assert lib.mnv_mesh_model_matrix(None, None) == mnv.MNV_E_INVALID and lib.mnv_mesh_show(None, 1) == mnv.MNV_E_INVALID
    assert lib.mnv_mesh_vertex_count(None) == 0 and lib.mnv_mesh_face_count(None) == 0 and lib.mnv_mesh_face_size(None) == 0
    assert lib.mnv_mesh_visible(None) == 0
    lib.mnv_mesh_destroy(None)
    assert lib.mnv_renderer_add_mesh(None, None) == mnv.MNV_E_INVALID and lib.mnv_renderer_clear_meshes(None) == mnv.MNV_E_INVALID
    assert lib.mnv_renderer_mesh_count(None) == 0
    # the pass
    cam = mnv.Camera(16, 16, 20.0)
    opt = mnv.RenderOptions.defaults()
    rect = mnv.Rect(0, 0, 16, 16)
    assert lib.mnv_render_meshes(None, 1, C.byref(cam.c), C.byref(opt), rect, None, None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_render_meshes(None, 0, None, C.byref(opt), rect, None, None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_render_meshes(None, 0, C.byref(cam.c), None, rect, None, None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_render_meshes(None, 0, C.byref(cam.c), C.byref(opt), mnv.Rect(0, 0, -1, 4), None, None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_render_meshes(None, 0, C.byref(cam.c), C.byref(opt), rect, None, None, C.c_void_p(2), None) == mnv.MNV_E_INVALID   # unaligned image
    one = (C.c_void_p * 1)(None)
    assert lib.mnv_render_meshes(one, 1, C.byref(cam.c), C.byref(opt), rect, None, None, None, None) == mnv.MNV_E_INVALID            # a null mesh
    if mnv.device_count() == 0:
        assert lib.mnv_render_meshes(None, 0, C.byref(cam.c), C.byref(opt), rect, None, None, None, None) == mnv.MNV_E_NO_DEVICE
        with pytest.raises(mnv.MnvError) as e:
            mnv.Mesh(v)
        assert e.value.code == mnv.MNV_E_NO_DEVICE

