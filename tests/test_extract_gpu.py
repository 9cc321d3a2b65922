"""mnv_accel_sample_points and mnv_extract_surface on the device against tests/extract_ref.py (the numpy restatement of the contract in
include/mnv.h): voxel, depth and sigma bits of the point query; the vertex array and the index array of a surface byte for byte.  No
tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import cases
import extract_ref as xr
import mesh_ref

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")


def tree_arrays(mnv, tree):
    v = tree.host_view()
    data, child, _ = tree.host_arrays()
    basis = v.basis_dim if (v.format == mnv.FORMAT_SH and v.basis_dim >= 0) else -1
    return data, child, np.array(v.offset[:], F), np.array(v.scale[:], F), basis


def two_leaf_tree(mnv):
    """One chunk: the root's eight children are leaves, all empty but child 4 (the +x, -y, -z octant), sigma 50."""
    data = np.zeros((1, 8, 4), np.float16)
    data[0, :, :3] = np.linspace(-1.0, 1.0, 24).reshape(8, 3)
    data[0, 4, 3] = 50.0
    return mnv.N3Tree.from_arrays(data, np.zeros((1, 8), np.int32), data_format="SH1", parent=np.array([-1], np.int32))


def patched_tree(mnv):
    """synth_random depth 4 with one inf and one NaN sigma half (both read as 0 by the extraction)."""
    src = mnv.N3Tree.synth_random(depth=4, basis_dim=4, refine_prob=0.7, empty_prob=0.3, sigma_max=30.0, seed=21)
    data, child, parent = (a.copy() for a in src.host_arrays())
    leaves = np.argwhere((child == 0) & (xr.pr.half_bits_to_float(data[..., -1]) > 5.0))
    data[leaves[3][0], leaves[3][1], -1] = 0x7C00
    data[leaves[11][0], leaves[11][1], -1] = 0x7E00
    v = src.host_view()
    return mnv.N3Tree.from_arrays(data, child, data_format=src.data_format, offset=v.offset[:], scale=v.scale[:], parent=parent)


def random_tree(depth, basis_dim, seed, **kw):
    return lambda mnv: mnv.N3Tree.synth_random(depth=depth, basis_dim=basis_dim, seed=seed, **kw)


def case_tree(name):
    return lambda mnv: cases.make_tree(mnv, cases.CASES[name]["tree"])


def a_leaf_sigma(data, child):
    """a density some leaf holds exactly (iso equal to it: that leaf is outside, S > iso is strict)"""
    s = xr.pr.half_bits_to_float(data[..., -1])[child == 0]
    s = np.sort(s[s > 0])
    return float(s[s.size // 2])


# name -> (tree, level, iso (a number, or a function of the host arrays), colour)
SURFACES = {
    "one_brick_l3": (random_tree(3, 1, 11), 3, 0.0, True),                        # one brick; the cells of index 7 do not exist
    "across_bricks_l4": (random_tree(4, 4, 12, empty_prob=0.3), 4, 6.0, True),  # quads across brick faces, dense to the boundary
    "shell_l5": (lambda m: m.N3Tree.synth_shell(depth=5, basis_dim=9, radius=0.3, half_thickness=0.04), 5, 10.0, True),
    "random_l6": (case_tree("sh4_d6"), 6, 12.0, True),
    "coarse_leaves_l4": (two_leaf_tree, 4, 25.0, True),                           # tree depth 1 below the level
    "coarse_leaves_l5": (two_leaf_tree, 5, 25.0, True),
    "deep_tree_l4": (case_tree("terrain_d7_aniso"), 4, 10.0, True),              # tree depth 7 above the level; anisotropic scale
    "terrain_l6": (case_tree("terrain_d7_aniso"), 6, 10.0, True),
    "aniso_random_l5": (case_tree("sh9_d7_aniso"), 5, 20.0, True),
    "iso_is_a_leaf_sigma": (random_tree(4, 4, 13, empty_prob=0.3), 4, a_leaf_sigma, True),
    "iso_above_all": (random_tree(4, 4, 13, empty_prob=0.3), 4, 1e4, True),     # nothing
    "no_colour": (random_tree(4, 9, 14), 4, 3.0, False),
    "rgba_l5": (case_tree("rgba_d5"), 5, 5.0, True),
    "sh1_l4": (case_tree("cfg1_sh1_d4"), 4, 5.0, True),
    "sh16_l4": (case_tree("sh16_d4"), 4, 5.0, True),
    "sh25_l4": (case_tree("sh25_d4"), 4, 5.0, True),
    "inf_nan_sigma": (patched_tree, 4, 5.0, True),
}


@pytest.mark.parametrize("name", sorted(SURFACES))
def test_extract_surface_equals_the_restatement_byte_for_byte(mnv, torch_gpu, name):
    make, level, iso, colour = SURFACES[name]
    tree = make(mnv)
    data, child, offset, scale, basis = tree_arrays(mnv, tree)
    if callable(iso):
        iso = iso(data, child)
    want_v, want_f, info = xr.extract(data, child, offset, scale, level, iso, colour=colour, basis_dim=basis)
    tree.move_to_device()
    s = mnv.extract_surface(tree.accel, level, iso, colour=colour)
    got_v, got_f = s.vertices(), s.faces()
    st = s.stats()
    print(name, "vertices", got_v.shape[0], "triangles", got_f.shape[0], "bricks", st["bricks"], "candidates", st["candidate_bricks"])
    assert s.counts() == (want_v.shape[0], want_f.size)
    assert got_v.tobytes() == want_v.tobytes()
    assert got_f.tobytes() == want_f.tobytes()
    assert st["bricks"] == 8 ** (level - 3) and 0 <= st["candidate_bricks"] <= st["bricks"]
    # the empty-space skip changes nothing, and neither does a second call
    every = mnv.extract_surface(tree.accel, level, iso, colour=colour, all_bricks=True)
    assert every.stats()["candidate_bricks"] == st["bricks"]
    assert every.vertices().tobytes() == got_v.tobytes() and every.faces().tobytes() == got_f.tobytes()
    again = mnv.extract_surface(tree.accel, level, iso, colour=colour)
    assert again.vertices().tobytes() == got_v.tobytes() and again.faces().tobytes() == got_f.tobytes()
    if name == "iso_above_all":
        assert got_v.shape == (0, 9) and got_f.shape == (0, 3)
        with pytest.raises(mnv.MnvError):
            s.to_mesh()
    elif name == "inf_nan_sigma":
        assert np.isfinite(got_v).all()
    else:
        assert got_v.shape[0] > 0
    if name == "iso_is_a_leaf_sigma":
        assert (info["samples"] == F(iso)).any()            # the case is what it says
    if name == "across_bricks_l4":
        ins = info["inside"]
        assert ins[0].any() and ins[-1].any()               # dense to the boundary: quads there are dropped
        used = np.zeros(got_v.shape[0], bool)
        used[got_f.reshape(-1)] = True
        assert not used.all()                               # active cells no face names
        b = info["cells"] >> 3
        brick = ((b[:, 0] * 2 + b[:, 1]) * 2 + b[:, 2])[got_f.astype(np.int64)]
        assert (brick.min(axis=1) != brick.max(axis=1)).any()   # triangles whose vertices lie in different bricks


def test_the_skip_removes_bricks_and_keeps_the_ones_a_neighbour_needs(mnv, torch_gpu):
    """two_leaf_tree at level 4: the bricks are the root's eight children.  Brick (1, 0, 0) is the dense leaf; brick (0, 0, 0) is one empty
    leaf and looks skippable, but its cells of x index 7 reach the samples of x index 8 in its +1 neighbour: both are candidates.  The other
    six bricks see only empty leaves in {b, b + 1}^3 (clamped) and are skipped."""
    tree = two_leaf_tree(mnv)
    data, child, offset, scale, basis = tree_arrays(mnv, tree)
    tree.move_to_device()
    s = mnv.extract_surface(tree.accel, 4, 25.0)
    st = s.stats()
    assert st["bricks"] == 8 and st["candidate_bricks"] == 2
    _, _, info = xr.extract(data, child, offset, scale, 4, 25.0, colour=True, basis_dim=basis)
    cells = info["cells"]
    in_first = ((cells >> 3) == 0).all(axis=1)
    assert in_first.any() and (cells[in_first][:, 0] == 7).all()      # brick 0's vertices exist only because of brick (1, 0, 0)
    assert s.vertices().shape[0] == cells.shape[0]
    # one level up the dense octant spans 2 x 2 x 2 bricks of 64: far fewer than all are visited
    st5 = mnv.extract_surface(tree.accel, 5, 25.0).stats()
    assert st5["bricks"] == 64 and st5["candidate_bricks"] < 64
    print("level 5 candidates", st5["candidate_bricks"])


def test_extract_surface_refuses_bad_arguments(mnv, torch_gpu):
    tree = two_leaf_tree(mnv).move_to_device()
    for level in (2, 11):
        with pytest.raises(mnv.MnvError) as e:
            mnv.extract_surface(tree.accel, level, 1.0)
        assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        mnv.extract_surface(tree.accel, 4, float("nan"))
    assert e.value.code == mnv.MNV_E_INVALID


def query_points(rng, depth, offset, scale):
    """4 096 world-space points: random ones, ones outside the cube on every side, exact cell boundaries k / 2^d, 1 - 1e-6 and 1.0 in
    tree space, a NaN and an inf row."""
    u = rng.uniform(0.0, 1.0, size=(4096, 3)).astype(F)
    u[100:400] = rng.uniform(-0.5, 1.5, size=(300, 3)).astype(F)
    for a in range(3):
        u[400 + 2 * a, a] = F(-0.25)
        u[401 + 2 * a, a] = F(1.25)
    k = rng.integers(0, (1 << depth) + 1, size=(600, 3))
    u[500:1100] = (k / F(1 << depth)).astype(F)              # exact in binary32
    u[1100:1400, 0] = (rng.integers(0, (1 << depth) + 1, size=300) / F(1 << depth)).astype(F)
    u[1400] = F(1.0) - F(1e-6)
    u[1401] = F(1.0)
    u[1402] = (F(1.0) - F(1e-6), F(0.0), F(1.0))
    u[1403] = F(0.0)
    p = ((u - offset[None, :]) / scale[None, :]).astype(F)   # world space (the round trip need not be exact: the reference sees p too)
    p[1500] = (np.nan, 0.1, 0.2)
    p[1501] = (0.1, np.inf, 0.2)
    p[1502] = (0.1, 0.2, -np.inf)
    return np.ascontiguousarray(p)


@pytest.mark.parametrize("name", ["random_d3", "random_d6", "terrain_d7_aniso"])
def test_sample_points_equals_the_numpy_descent(mnv, torch_gpu, name):
    torch = torch_gpu
    make, depth = {"random_d3": (random_tree(3, 1, 31), 3), "random_d6": (random_tree(6, 4, 32), 6),
                   "terrain_d7_aniso": (case_tree("terrain_d7_aniso"), 7)}[name]
    tree = make(mnv)
    data, child, offset, scale, _ = tree_arrays(mnv, tree)
    pts = query_points(np.random.default_rng(7), depth, offset, scale)
    want_v, want_d, want_s = xr.sample_points(data, child, offset, scale, pts)
    assert (want_v[1500:1503] == -1).all() and (want_d[1500:1503] == 0).all() and len(set(want_d.tolist())) > 2
    tree.move_to_device()
    dev = torch.from_numpy(pts).cuda()
    v, d, s = mnv.sample_points(tree.accel, dev)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), want_v)
    assert np.array_equal(d.cpu().numpy(), want_d)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
    # every output alone (the others NULL)
    for keep in range(3):
        flags = [i == keep for i in range(3)]
        out = mnv.sample_points(tree.accel, dev, *flags)
        torch.cuda.synchronize()
        assert [o is not None for o in out] == flags
        got = out[keep].cpu().numpy()
        want = (want_v, want_d, want_s)[keep]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert mnv.sample_points(tree.accel, dev, False, False, False) == (None, None, None)
    assert mnv.sample_points(tree.accel, dev[:0])[0].numel() == 0


@pytest.fixture(scope="module")
def shell_surface(mnv, torch_gpu):
    tree = mnv.N3Tree.synth_shell(depth=5, basis_dim=4, radius=0.3, half_thickness=0.04)
    tree.move_to_device()
    return tree, mnv.extract_surface(tree.accel, 5, 10.0)


def test_surface_mesh_draws_like_the_restatement_of_the_mesh_pass(mnv, torch_gpu, shell_surface):
    _, s = shell_surface
    cam = mnv.orbit_camera(96, 72, 80.0, 2.6, 22.5, 20.0)
    opt = mnv.RenderOptions.cli_defaults()
    vert, faces = s.vertices(), s.faces()
    for unlit in (False, True):
        mesh = s.to_mesh(unlit=unlit)
        assert (mesh.vertex_count, mesh.face_count, mesh.face_size) == (vert.shape[0], faces.shape[0], 3)
        tmax, rgba8 = mnv.render_meshes([mesh], cam, opt)
        torch_gpu.cuda.synchronize()
        want_t, want_c = mesh_ref.render([mesh_ref.RefMesh(vert, faces, 3, unlit=unlit)], cam.c, (0, 0, 96, 72), opt.background_brightness)
        assert np.array_equal(cases.bits(tmax.cpu().numpy()), cases.bits(want_t.reshape(72, 96)))
        assert np.array_equal(rgba8.cpu().numpy(), want_c.reshape(72, 96, 4))
        assert int((want_t.reshape(-1) < 1e8).sum()) > 500      # the shell shows
    dv, df = s.device_pointers()
    assert dv and df


def test_renderer_draws_an_extracted_surface(mnv, torch_gpu, shell_surface):
    tree, s = shell_surface
    r = mnv.Renderer()
    r.resize(96, 72)
    r.set(tree, tree.capacity)
    r.set_camera((2.0, 1.0, 1.2), (0.77, 0.385, 0.46), fx=80.0)
    r.render()
    plain, _ = r.download(want_rgba8=True)
    r.add_mesh(s.to_mesh())
    assert r.mesh_count == 1
    st = r.render()
    with_mesh, _ = r.download(want_rgba8=True)
    assert st["used_accel"] and np.isfinite(with_mesh).all()
    assert (cases.bits(with_mesh) != cases.bits(plain)).any()


def test_mnv_render_extract_mesh_writes_the_python_extraction(mnv, torch_gpu, shell_surface, tmp_path):
    tree, s = shell_surface
    npz, obj, out = str(tmp_path / "shell.npz"), str(tmp_path / "shell.obj"), str(tmp_path / "frame")
    tree.save_npz(npz)
    base = [EXE, npz, "-w", "96", "-h", "72", "--fx", "80", "--extract_mesh", obj, "--extract_level", "5", "--extract_iso", "10"]
    r = subprocess.run(base + ["--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"extract_mesh: {s.counts()[0]} vertices, {s.counts()[1] // 3} triangles" in r.stdout
    v2, f2, fs = mnv.obj_read(obj)
    rv, rf = xr.reindex_like_load_obj(s.vertices(), s.faces())
    assert fs == 3 and np.array_equal(f2, rf) and np.array_equal(v2.view(np.uint32), rv.view(np.uint32))
    with_mesh = open(out + "_0000.ppm", "rb").read()
    r = subprocess.run([a for a in base if a not in ("--extract_mesh", obj)] + ["--out", out + "_plain"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(out + "_plain_0000.ppm", "rb").read() != with_mesh       # the frame of the same run draws the mesh under the volume
    r = subprocess.run(base + ["--gpus", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--extract_mesh" in r.stderr
    os.remove(obj)
    r = subprocess.run(base + ["--frames", "0"], capture_output=True, text=True, timeout=300)     # the file alone
    assert r.returncode == 0 and os.path.exists(obj), r.stderr + r.stdout
