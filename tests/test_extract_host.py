"""The surface contract of include/mnv.h (mnv_extract_surface) pinned on the host: tests/extract_ref.py restates it in numpy; these tests
hold the restatement to the properties a closed, consistently oriented surface has, and check the OBJ writer against the reader.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import extract_ref as xr

F = np.float32


def tree_arrays(mnv, tree):
    v = tree.host_view()
    data, child, _ = tree.host_arrays()
    basis = v.basis_dim if (v.format == mnv.FORMAT_SH and v.basis_dim >= 0) else -1
    return data, child, np.array(v.offset[:], F), np.array(v.scale[:], F), basis


@pytest.fixture(scope="module")
def shell(mnv):
    tree = mnv.N3Tree.synth_shell(depth=5, basis_dim=4, radius=0.3, half_thickness=0.04)
    data, child, offset, scale, basis = tree_arrays(mnv, tree)
    vert, faces, info = xr.extract(data, child, offset, scale, 5, 10.0, colour=True, basis_dim=basis)
    return dict(tree=tree, vert=vert, faces=faces, info=info, offset=offset, scale=scale)


def test_shell_surface_is_closed_oriented_and_two_spheres(shell):
    vert, faces, info = shell["vert"], shell["faces"].astype(np.int64), shell["info"]
    ins = info["inside"]
    assert not (ins[0].any() or ins[-1].any() or ins[:, 0].any() or ins[:, -1].any() or ins[:, :, 0].any() or ins[:, :, -1].any())
    assert vert.shape[0] > 1000 and faces.shape[0] > 2000
    # every directed edge a -> b occurs as often as b -> a
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    nv = vert.shape[0]
    fwd = np.sort(e[:, 0] * nv + e[:, 1])
    rev = np.sort(e[:, 1] * nv + e[:, 0])
    assert np.array_equal(fwd, rev)
    # Euler characteristic 4: the outer and the inner sphere
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * nv + np.maximum(e[:, 0], e[:, 1]))
    assert np.unique(faces).size == nv                      # every vertex is used
    assert nv - und.size + faces.shape[0] == 4
    # outward orientation: the signed volume is the shell's, positive
    p = vert[:, 0:3].astype(np.float64)
    v0, v1, v2 = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    assert np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0 > 0.0
    # face normals agree with the vertex normals (both point from inside to outside)
    fn = np.cross(v1 - v0, v2 - v0)
    vn = vert[:, 6:9].astype(np.float64)
    agree = (np.einsum("ij,ij->i", fn, vn[faces[:, 0]] + vn[faces[:, 1]] + vn[faces[:, 2]]) > 0).mean()
    assert agree > 0.95, agree
    assert np.allclose(np.linalg.norm(vn, axis=1), 1.0, atol=1e-5)
    assert np.isfinite(vert).all() and (vert[:, 3:6] > 0).all() and (vert[:, 3:6] < 1).all()   # sigmoid colours


def test_every_vertex_lies_in_its_dual_cell(shell):
    info, vert, offset, scale = shell["info"], shell["vert"], shell["offset"], shell["scale"]
    local, cells = info["local"], info["cells"]
    assert (local >= 0).all() and (local <= 1).all()
    n = 32
    u = vert[:, 0:3].astype(np.float64) * scale + offset    # back to tree space
    lo, hi = (cells + 0.5) / n, (cells + 1.5) / n
    assert (u >= lo - 1e-6).all() and (u <= hi + 1e-6).all()
    # cells in the canonical order: by brick, then inside the brick
    nb = n // 8
    key = (((cells[:, 0] >> 3) * nb + (cells[:, 1] >> 3)) * nb + (cells[:, 2] >> 3)) * 512 + ((cells[:, 0] & 7) * 8 + (cells[:, 1] & 7)) * 8 + (cells[:, 2] & 7)
    assert (np.diff(key) > 0).all()


def test_iso_above_every_sigma_gives_nothing(mnv, shell):
    data, child, offset, scale, basis = tree_arrays(mnv, shell["tree"])
    top = float(xr.pr.half_bits_to_float(data[..., -1]).max())
    vert, faces, _ = xr.extract(data, child, offset, scale, 5, top, colour=True, basis_dim=basis)   # S > iso is strict
    assert vert.shape == (0, 9) and faces.shape == (0, 3)
    vert, faces, _ = xr.extract(data, child, offset, scale, 4, top + 1.0, colour=False)
    assert vert.shape == (0, 9) and faces.shape == (0, 3)


def test_reference_descent_matches_the_lattice_by_integer_path(mnv):
    """A sample of the lattice deeper trees refine lies on a corner of finer voxels: the float descent takes the voxel with the larger
    coordinates (path bits of 2 i + 1, then zeros), which is what the device's integer descent assumes."""
    tree = mnv.N3Tree.synth_random(depth=6, basis_dim=1, seed=3)
    data, child, _ = tree.host_arrays()
    level = 3
    _, vox = xr.lattice(data, child, level)
    n = 1 << level
    for (i, j, k) in [(0, 0, 0), (3, 5, 1), (7, 7, 7), (4, 0, 6)]:
        q = [2 * i + 1, 2 * j + 1, 2 * k + 1]
        chunk, d = 0, 1
        while True:
            sh = level + 1 - d
            c = 0 if sh < 0 else (((q[0] >> sh) & 1) << 2) | (((q[1] >> sh) & 1) << 1) | ((q[2] >> sh) & 1)
            if child[chunk, c] == 0:
                break
            chunk += int(child[chunk, c])
            d += 1
        assert vox[i, j, k] == chunk * 8 + c


def test_obj_round_trip_returns_the_same_bits(mnv, shell, tmp_path):
    vert, faces = shell["vert"], shell["faces"]
    path = str(tmp_path / "shell.obj")
    mnv.obj_write(path, vert, faces)
    v2, f2, fs = mnv.obj_read(path)
    rv, rf = xr.reindex_like_load_obj(vert, faces)
    assert fs == 3 and np.array_equal(f2, rf)
    assert np.array_equal(v2.view(np.uint32), rv.view(np.uint32))
    # a vertex no face uses, awkward values: denormal, negative zero, the largest float, a value that needs nine digits
    odd = np.array([[1e-45, -0.0, 3.4028235e38, 0.1, 0.2, 0.3, 0.0, 0.0, 1.0],
                    [1.0, 2.0, 3.0, 0.123456789, 1.0 / 3.0, 16777217.0, 0.6, 0.8, -0.0],
                    [-1.5, 2.5e-7, 7.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0],
                    [9.0, 9.0, 9.0, 0.5, 0.5, 0.5, 1.0, 0.0, 0.0]], F)
    tri = np.array([[3, 0, 1]], np.uint32)                  # vertex 2 is unused; first use order 3, 0, 1
    path = str(tmp_path / "odd.obj")
    mnv.obj_write(path, odd, tri)
    v2, f2, fs = mnv.obj_read(path)
    rv, rf = xr.reindex_like_load_obj(odd, tri)
    assert rv.shape[0] == 3 and np.array_equal(f2, rf) and np.array_equal(f2, [[0, 1, 2]])
    assert np.array_equal(v2.view(np.uint32), rv.view(np.uint32))
    text = open(path).read().splitlines()
    assert sum(t.startswith("v ") for t in text) == 4 and sum(t.startswith("vn ") for t in text) == 4 and text[-1] == "f 4//4 1//1 2//2"


def test_obj_write_refuses_what_is_no_mesh(mnv, tmp_path):
    v = np.zeros((3, 9), F)
    for faces, fs in (([[0, 1, 3]], 3), ([[0, 1]], 3), ([[0, 1, 2]], 4)):
        with pytest.raises(mnv.MnvError) as e:
            mnv.obj_write(str(tmp_path / "x.obj"), v, np.array(faces, np.uint32), fs)
        assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        mnv.obj_write(str(tmp_path / "no_such_dir" / "x.obj"), v, np.array([[0, 1, 2]], np.uint32))
    assert e.value.code == mnv.MNV_E_IO


def test_extraction_entry_points_fail_loudly_without_a_device(mnv):
    """No CPU fallback: argument errors first, then MNV_E_NO_DEVICE before the accel is looked at."""
    lib = mnv.lib()
    h = C.c_void_p()
    p = mnv.ExtractParams(5, 10.0, mnv.EXTRACT_COLOUR)
    assert lib.mnv_extract_surface(None, C.byref(p), None, C.byref(h)) == mnv.MNV_E_INVALID
    blank = C.create_string_buffer(1 << 16)                 # stands in for an accel that holds no tree
    for level in (2, 11):
        bad = mnv.ExtractParams(level, 10.0, 0)
        assert lib.mnv_extract_surface(blank, C.byref(bad), None, C.byref(h)) == mnv.MNV_E_INVALID
    assert lib.mnv_extract_surface(blank, C.byref(mnv.ExtractParams(5, float("nan"), 0)), None, C.byref(h)) == mnv.MNV_E_INVALID
    assert lib.mnv_extract_surface(blank, C.byref(mnv.ExtractParams(5, 1.0, 4)), None, C.byref(h)) == mnv.MNV_E_INVALID
    assert lib.mnv_accel_sample_points(None, None, 4, None, None, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_accel_sample_points(blank, None, -1, None, None, None, None) == mnv.MNV_E_INVALID
    expect = mnv.MNV_E_NO_DEVICE if mnv.device_count() == 0 else mnv.MNV_E_INVALID
    pts = np.zeros((4, 3), F)
    assert lib.mnv_extract_surface(blank, C.byref(p), None, C.byref(h)) == expect and not h.value
    assert lib.mnv_accel_sample_points(blank, pts.ctypes.data, 4, None, None, None, None) == expect
    if mnv.device_count() == 0:
        assert "HIP device" in lib.mnv_last_error().decode()
        t = mnv.N3Tree.synth_random(depth=2, basis_dim=1)
        with pytest.raises(mnv.MnvError):
            mnv.extract_surface(t.accel, 3, 1.0)           # no accel without a device
