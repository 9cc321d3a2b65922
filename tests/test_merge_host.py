"""The host half of the merge entry points (include/mnv.h, "merging two trees"): mnv_tree_voxel_cube's values, the argument checks of
mnv_tree_merge_plan / write and N3Tree.merge that answer before a device is touched, and what mnv_render refuses around --merge.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")
F = np.float32


def test_voxel_cube_values(mnv):
    rng = np.random.default_rng(1)
    cases = [((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0, (0, 0, 0)), ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), 1, (1, 0, 1)), ((0.5, 0.25, 0.125), (0.5, 1.0, 2.0), 3, (7, 0, 5)),
             ((0.3, -0.7, 1e-3), (0.1, 0.2, 0.3), 5, (31, 0, 17)), ((0.1, 0.2, 0.3), (3.0, 3.0, 3.0), 22, ((1 << 22) - 1, 1, 12345))]
    for _ in range(20):
        k = int(rng.integers(0, 23))
        cases.append((tuple(rng.uniform(-1, 1, 3)), tuple(rng.uniform(0.01, 4, 3)), k, tuple(int(c) for c in rng.integers(0, 1 << k, 3))))
    for offset, scale, level, corner in cases:
        got_o, got_s = mnv.tree_voxel_cube(offset, scale, level, corner)
        want_o, want_s = mr.voxel_cube(F(offset), F(scale), level, corner)
        assert got_o.tobytes() == want_o.tobytes() and got_s.tobytes() == want_s.tobytes(), (offset, scale, level, corner)
    o, s = mnv.tree_voxel_cube((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 2, (3, 0, 1))
    assert o.tolist() == [-1.0, 2.0, 1.0] and s.tolist() == [2.0, 2.0, 2.0]
    # the octants of the unit cube [0, 1): a point of octant c lands in [0, 1) of its tile
    o, s = mnv.tree_voxel_cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1, (1, 0, 1))
    assert (o + s * F([0.75, 0.25, 0.5])).tolist() == [0.5, 0.5, 0.0]
    for level, corner in ((-1, (0, 0, 0)), (23, (0, 0, 0)), (2, (4, 0, 0)), (2, (0, -1, 0)), (0, (0, 0, 1))):
        with pytest.raises(mnv.MnvError) as e:
            mnv.tree_voxel_cube((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), level, corner)
        assert e.value.code == mnv.MNV_E_INVALID
    buf = (C.c_float * 3)(0, 0, 0)
    ints = (C.c_int32 * 3)(0, 0, 0)
    assert mnv.lib().mnv_tree_voxel_cube(None, buf, 0, ints, buf, buf) == mnv.MNV_E_INVALID
    assert mnv.lib().mnv_tree_voxel_cube(buf, buf, 0, ints, buf, None) == mnv.MNV_E_INVALID


def _view(mnv, data, child, dd=4, n=2, fmt=None, basis=-1):
    v = mnv.TreeView()
    v.data, v.child = data.ctypes.data, child.ctypes.data
    for i in range(3):
        v.offset[i] = v.scale[i] = 0.5
    v.N, v.data_dim, v.format, v.basis_dim, v.capacity = n, dd, mnv.FORMAT_RGBA if fmt is None else fmt, basis, child.shape[0]
    return v


def test_plan_and_write_refuse_bad_arguments_before_a_device_is_touched(mnv):
    """Host arrays throughout: a call that passed every argument check would end at "the tree views must hold device arrays", which is
    MNV_E_INVALID as well -- so the codes below are asserted together with the text of the check that is meant."""
    lib = mnv.lib()
    data = np.zeros(8 * 4 + 8, np.uint16)
    data = data[(-data.ctypes.data // 2) % 8:][:32]            # 16-byte aligned
    assert data.ctypes.data % 16 == 0
    child = np.zeros((1, 8), np.int32)
    a, b = _view(mnv, data, child), _view(mnv, data, child)

    def plan(a=a, b=b, p=None, level=0, corner=(0, 0, 0), mode=0, out=True, stats=True):
        h, st = C.c_void_p(), mnv.MergeStats()
        p = mnv.MergeParams(level, (C.c_int32 * 3)(*corner), mode, 0) if p is None else p
        rc = lib.mnv_tree_merge_plan(C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, C.byref(p) if p else None,
                                     C.byref(h) if out else None, C.byref(st) if stats else None, None)
        assert not h.value
        return rc, lib.mnv_last_error().decode()

    for kw in (dict(a=None), dict(b=None), dict(p=False), dict(out=False), dict(stats=False)):
        rc, text = plan(**kw)
        assert rc == mnv.MNV_E_INVALID and "null" in text, kw
    for kw, word in ((dict(level=-1), "level"), (dict(level=23), "level"), (dict(level=2, corner=(4, 0, 0)), "corner"), (dict(level=2, corner=(0, 0, -1)), "corner"),
                     (dict(corner=(0, 1, 0)), "corner"), (dict(mode=2), "mode"), (dict(mode=-1), "mode")):
        rc, text = plan(**kw)
        assert rc == mnv.MNV_E_INVALID and word in text, (kw, text)
    for bad, code, word in ((_view(mnv, data, child, n=3), mnv.MNV_E_UNSUPPORTED, "N == 2"), (_view(mnv, data, child, dd=1), mnv.MNV_E_INVALID, "data_dim"),
                            (_view(mnv, data, child, dd=1025), mnv.MNV_E_UNSUPPORTED, "data_dim"), (_view(mnv, data[1:], child), mnv.MNV_E_INVALID, "aligned")):
        for kw in (dict(a=bad), dict(b=bad)):
            rc, text = plan(**kw)
            assert rc == code and word in text, (kw, text)
    empty = _view(mnv, data, child)
    empty.capacity = 0
    rc, text = plan(b=empty)
    assert rc == mnv.MNV_E_INVALID and "root" in text
    for other in (_view(mnv, data, child, dd=2), _view(mnv, data, child, fmt=mnv.FORMAT_SH, basis=1)):
        rc, text = plan(b=other)
        assert rc == mnv.MNV_E_INVALID and "same" in text, text
    rc, text = plan()
    assert rc == mnv.MNV_E_INVALID and "device arrays" in text
    assert lib.mnv_tree_merge_write(None, child.ctypes.data, data.ctypes.data, None, None, None, None, None) == mnv.MNV_E_INVALID
    lib.mnv_tree_merge_destroy(None)
    with pytest.raises(mnv.MnvError) as e:
        mnv.merge_params(mode="under")
    assert e.value.code == mnv.MNV_E_INVALID


def test_n3tree_merge_refuses_trees_that_are_not_on_the_device(mnv):
    t = mnv.N3Tree.synth_random(depth=2, basis_dim=1)
    with pytest.raises(mnv.MnvError) as e:
        t.merge(t)
    assert e.value.code == mnv.MNV_E_INVALID and "device" in str(e.value)
    h = C.c_void_p()
    assert mnv.lib().mnv_n3tree_merge(t._h, t._h, None, None, C.byref(h)) == mnv.MNV_E_INVALID and not h.value


def test_mnv_render_refuses_what_merge_cannot_be_combined_with(mnv, tmp_path):
    assert os.path.exists(EXE), "mnv_render not built"
    npz = str(tmp_path / "scene.npz")
    mnv.N3Tree.synth_random(depth=2, basis_dim=1).save_npz(npz)

    def run(*extra):
        return subprocess.run([EXE, npz, "--frames", "0"] + list(extra), capture_output=True, text=True, timeout=60)

    for extra, word in ((["--merge", npz, "--gpus", "1"], "--gpus"), (["--merge", npz, "--use_splitting"], "--use_splitting"),
                        (["--merge_at", "0:0,0,0"], "--merge"), (["--merge_mode", "add"], "--merge"), (["--merge_at", "1:0,0,0", "--merge", npz], "--merge"),
                        (["--merge", npz, "--merge_at", "1:2,0,0"], "--merge_at"), (["--merge", npz, "--merge_at", "1,0,0,0"], "--merge_at"),
                        (["--merge", npz, "--merge_at", "23:0,0,0"], "--merge_at"), (["--merge", npz, "--merge_at", "1:0,0,0x"], "--merge_at"),
                        (["--merge", npz, "--merge_mode", "under"], "--merge_mode")):
        r = run(*extra)
        assert r.returncode != 0 and word in r.stderr and "usable HIP device" not in r.stderr, (extra, r.stderr)
