"""The host side of the point entry points through libmnv.so: arguments are judged before a device is touched, the cube helper and the
colour tables against tests/points_ref.py, and the command line refuses --points beside an input tree.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import points_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")
F = np.float32


def _params(mnv, **kw):
    p = mnv.PointsParams((C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.5, 0.5, 0.5), 5, mnv.FORMAT_RGBA, -1, 1, 100.0)
    for k, v in kw.items():
        if k in ("offset", "scale"):
            setattr(p, k, (C.c_float * 3)(*v))
        else:
            setattr(p, k, v)
    return p


def test_struct_layouts(mnv):
    assert C.sizeof(mnv.PointsParams) == 44 and C.sizeof(mnv.PointsStats) == 8 * 28
    assert mnv.PointsParams.depth.offset == 24 and mnv.PointsParams.sigma.offset == 40 and mnv.PointsStats.chunks_at_depth.offset == 32


def test_arguments_are_judged_without_a_device(mnv):
    lib = mnv.lib()
    h = C.c_void_p()
    inf, nan = float("inf"), float("nan")
    assert lib.mnv_point_tree_create(None, C.byref(h)) == mnv.MNV_E_INVALID
    assert lib.mnv_point_tree_create(C.byref(_params(mnv)), None) == mnv.MNV_E_INVALID
    bad = [dict(depth=0), dict(depth=22), dict(depth=-3), dict(min_points=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=inf), dict(sigma=nan),
           dict(scale=(0.5, 0.0, 0.5)), dict(scale=(0.5, 0.5, -0.5)), dict(scale=(inf, 0.5, 0.5)), dict(scale=(0.5, nan, 0.5)),
           dict(offset=(nan, 0.5, 0.5)), dict(offset=(0.5, 0.5, -inf))]
    for kw in bad:
        assert lib.mnv_point_tree_create(C.byref(_params(mnv, **kw)), C.byref(h)) == mnv.MNV_E_INVALID, kw
        assert not h.value
    for kw in (dict(format=2), dict(format=-1), dict(format=mnv.FORMAT_SH, basis_dim=2), dict(format=mnv.FORMAT_SH, basis_dim=-1),
               dict(format=mnv.FORMAT_SH, basis_dim=36)):
        assert lib.mnv_point_tree_create(C.byref(_params(mnv, **kw)), C.byref(h)) == mnv.MNV_E_UNSUPPORTED, kw
    assert lib.mnv_point_tree_add(None, None, None, 0, None) == mnv.MNV_E_INVALID
    st = mnv.PointsStats()
    assert lib.mnv_point_tree_finish(None, C.byref(st), None) == mnv.MNV_E_INVALID
    assert lib.mnv_point_tree_write(None, None, None, None, None, None, None) == mnv.MNV_E_INVALID
    lib.mnv_point_tree_destroy(None)
    out = C.c_void_p()
    assert lib.mnv_n3tree_from_points(None, None, None, 0, None, None, C.byref(out)) == mnv.MNV_E_INVALID
    assert lib.mnv_n3tree_from_points(C.byref(_params(mnv, depth=0)), None, None, 0, None, None, C.byref(out)) == mnv.MNV_E_INVALID
    assert lib.mnv_n3tree_from_points(C.byref(_params(mnv, format=7)), None, None, 0, None, None, C.byref(out)) == mnv.MNV_E_UNSUPPORTED
    assert not out.value
    if mnv.device_count() == 0:                                 # good arguments get as far as the device
        assert lib.mnv_point_tree_create(C.byref(_params(mnv)), C.byref(h)) == mnv.MNV_E_NO_DEVICE and not h.value


def test_bounds_to_cube_on_three_boxes(mnv):
    boxes = [((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), ((10.0, -3.0, 0.25), (12.5, 4.0, 0.75)), ((-7.25, 100.0, 3.0), (-7.0, 100.125, 35.0))]
    for lo, hi in boxes:
        lo, hi = np.array(lo, F), np.array(hi, F)
        offset, scale = mnv.points_bounds_to_cube(lo, hi)
        s = F(1) / (hi - lo).max()
        want_offset = F(0.5) - s * (F(0.5) * (lo + hi))
        assert scale.dtype == F and np.array_equal(scale, np.full(3, s, F)) and np.array_equal(offset, want_offset)
        q_lo, q_hi = offset + scale * lo, offset + scale * hi
        assert np.allclose(offset + scale * (0.5 * (lo + hi)), 0.5, atol=1e-6)
        assert (q_lo > -1e-5).all() and (q_hi < 1 + 1e-5).all() and np.isclose((q_hi - q_lo).max(), 1.0, atol=1e-5)
    offset, scale = mnv.points_bounds_to_cube((2.0, 2.0, 2.0), (2.0, 2.0, 2.0))     # a single point: an edge of 1
    assert scale.tolist() == [1.0, 1.0, 1.0] and offset.tolist() == [-1.5, -1.5, -1.5]
    lib = mnv.lib()
    lo, hi, o, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(), (C.c_float * 3)()
    assert lib.mnv_points_bounds_to_cube(None, hi, o, s) == mnv.MNV_E_INVALID and lib.mnv_points_bounds_to_cube(lo, hi, o, None) == mnv.MNV_E_INVALID
    assert lib.mnv_points_bounds_to_cube(hi, lo, o, s) == mnv.MNV_E_INVALID                          # hi < lo
    assert lib.mnv_points_bounds_to_cube(lo, (C.c_float * 3)(1, float("nan"), 1), o, s) == mnv.MNV_E_INVALID
    assert lib.mnv_points_bounds_to_cube(lo, hi, o, s) == mnv.MNV_OK


def test_colour_tables_against_the_restatement(mnv):
    assert np.array_equal(mnv.points_colour_table("RGBA"), pr.colour_table("RGBA"))
    for fmt in ("SH1", "SH4", "SH9", "SH16", "SH25"):
        got, want = mnv.points_colour_table(fmt), pr.colour_table(fmt)
        assert ((got ^ want) & 0x8000 == 0).all()                                                    # same signs
        assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1                      # one binary16 ulp: the host log's last bit
        vals = got.view(np.float16).astype(np.float64)
        assert (np.diff(vals[1:255]) > 0).all() and vals[0] <= vals[1] and vals[254] <= vals[255]
    lib = mnv.lib()
    out = np.zeros(256, np.uint16)
    assert lib.mnv_points_colour_table(mnv.FORMAT_RGBA, -1, None) == mnv.MNV_E_INVALID
    assert lib.mnv_points_colour_table(mnv.FORMAT_SH, 3, out.ctypes.data) == mnv.MNV_E_UNSUPPORTED
    assert lib.mnv_points_colour_table(5, 1, out.ctypes.data) == mnv.MNV_E_UNSUPPORTED


def test_mnv_render_refuses_points_beside_a_tree(mnv, tmp_path):
    assert os.path.exists(EXE), "mnv_render not built"
    cloud, tree = str(tmp_path / "cloud.npz"), str(tmp_path / "tree.npz")
    np.savez(cloud, points=np.zeros((4, 3), F))
    mnv.N3Tree.synth_random(depth=2, basis_dim=1).save_npz(tree)
    r = subprocess.run([EXE, tree, "--points", cloud], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--points" in r.stderr and "input tree" in r.stderr
    r = subprocess.run([EXE, "--points", cloud, "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--points" in r.stderr
    r = subprocess.run([EXE, tree, "--points_depth", "5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--points" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)                             # neither a tree nor --points: the usage text
    assert r.returncode == 2 and "--points" in r.stdout
