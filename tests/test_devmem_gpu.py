"""Nothing leaks and nothing is freed twice: every owner of device / pinned memory (csrc/mnv_devmem.h) is created, grown and destroyed in
a cycle that a child process on the test-hook build runs three times.  The owners count their live bytes (mnv_hook_live_bytes, test-hook
library only); process-lifetime caches (the refinement workspace, the mesh pass's scratch) fill in cycle 1, so cycles 2 and 3 must end
with exactly cycle 1's figures, device and pinned.  A leak shows as growth per cycle, a double free as a smaller number or a HIP error.

One cycle: the accel steps (create with a reserve, a refresh that appends chunks, a prune that allocates the spare set, a second refresh,
destroy) on N3Tree.synth_random(depth=4, basis_dim=4) and once more on a depth-7 tree -- the shallow tree has no second lookup grid, so
only the deep one reaches the patch items, the inline words and the brick records; a Wireframe and a two-triangle Mesh at two sizes;
extract_surface -> to_mesh (the one hand-over); an Mlp (w64_l1_min of tests/test_mlp_gpu.py, the smallest description the suite has) with
a small and a large query; a Renderer through every frame kind that owns buffers, at two sizes; and three refused calls, which must
leave both counters as they were."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import hooks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = 3


def test_three_cycles_end_with_the_same_live_bytes(mnv, torch_gpu):
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=hooks.hooks_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    ends = [tuple(int(x) for x in line.split()[3::2]) for line in r.stdout.splitlines() if line.startswith("cycle ")]
    print(r.stdout)
    assert len(ends) == CYCLES, r.stdout
    assert ends[0][0] > 0 and ends[0][1] > 0, ends        # the caches of cycle 1 are counted: the accessor is live
    assert ends[1] == ends[0] and ends[2] == ends[0], ends
    assert "refused calls ok" in r.stdout


# ---------------------------------------------------------------- the child process

def _refused(live, what, call):
    before = live()
    call()
    assert live() == before, (what, before, live())


def _accel_steps(m, torch, live, depth, refuse):
    from test_accel_edit_gpu import EditedTree, chunk_depths

    spec = dict(kind="random", depth=depth, basis_dim=4) if depth == 4 else dict(kind="random", depth=depth, basis_dim=4, refine_prob=0.45,
                                                                                 empty_prob=0.9, sigma_max=40.0, seed=31)
    et = EditedTree(m, torch, spec, reserve=64)
    try:
        if refuse:
            def too_small():
                h = C.c_void_p()
                assert m.lib().mnv_accel_create_reserved(C.byref(et.tv), et.cap - 1, None, C.byref(h)) != 0 and not h.value
            _refused(live, "accel_create below the tree", too_small)
        with_accel = live()
        rng = np.random.default_rng(5)
        L2 = m.accel_info(et.accel)["grid2_level"]
        wanted = [max(L2, 1), L2 + 1, L2 + 2, 2]
        added, _ = et.edit(rng, 24, 16, wanted)
        assert added > 0
        # marks that drop the sub-tree under the root's first inner voxel (closed under ancestors, as a track_visit frame leaves them)
        first = next(s for s in range(8) if et.child[0, s] != 0)
        gone, todo = set(), [int(et.child[0, first])]
        while todo:
            c = todo.pop()
            gone.add(c)
            todo += [c + int(o) for o in et.child[c] if o != 0]
        marks = np.ones(et.max_cap, np.int32)
        marks[sorted(gone)] = 0
        marks[et.cap:] = 0
        visited = torch.from_numpy(marks).cuda()
        v = et.tree.host_view()
        edit = m.tree_edit(et.d["child"], et.d["parent"], list(v.offset), list(v.scale), et.cap)
        new_cap, n_del = m.prune_tree(edit, et.d["data"], et.dd, et.d["counts"], visited, et.max_cap, accel=et.accel)
        assert n_del == len(gone) and new_cap == et.cap - n_del
        assert live()[0] > with_accel[0]                  # the spare set
        # the host copies follow the renumbering, then the loop goes on
        torch.cuda.synchronize()
        et.cap = new_cap
        et.data[:] = et.d["data"].cpu().numpy().view(np.float16)
        et.child[:] = et.d["child"].cpu().numpy()
        et.parent[:] = et.d["parent"].cpu().numpy()
        et.child[new_cap:], et.parent[new_cap:], et.depth[:] = 0, 0, 0
        et.depth[:new_cap] = chunk_depths(et.parent, new_cap)
        et.tv.capacity = new_cap
        added, _ = et.edit(rng, 24, 16, wanted)
        assert added > 0
        info = m.accel_info(et.accel)
        torch.cuda.synchronize()
    finally:
        et.close()
    return info


def _small_objects(m, torch, live, tree):
    from test_mlp_gpu import CONFIGS
    import mlp_cases

    opt = m.RenderOptions.cli_defaults()
    sizes = ((64, 48), (96, 64))
    cam = lambda w, h: m.Camera(w, h, 0.9 * w).set_pose((-2.5, 1.4, 1.8), (-0.74, 0.4, 0.54))   # noqa: E731
    wire = m.Wireframe(tree.device_view(), 100)
    assert wire.cube_count > 0
    for w, h in sizes:       # regrows the key image, the tile bins and the pair list
        for method in (m.WIREFRAME_BINNED, m.WIREFRAME_GLOBAL):
            wire.set_method(method)
            wire.render(cam(w, h), opt)
    vert = np.zeros((4, 9), np.float32)
    vert[:, :3] = [(-0.8, -0.8, 0.1), (0.8, -0.8, 0.1), (0.8, 0.8, 0.0), (-0.8, 0.8, 0.0)]
    vert[:, 3:6], vert[:, 8] = (0.9, 0.4, 0.1), 1.0
    faces = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    mesh = m.Mesh(vert, faces, 3)
    for i, (w, h) in enumerate(sizes):
        m.render_meshes([mesh], cam(w, h), opt)
        if i == 0:
            torch.cuda.synchronize()
            assert m.lib().mnv_mesh_update(mesh._h, vert.ctypes.data, 4, faces.ctypes.data, 6, 3, 0) == 0
    _refused(live, "mesh with face_size 4", lambda: _raises(m, lambda: m.Mesh(vert, np.arange(4, dtype=np.uint32), 4)))
    _refused(live, "extract_surface at level 2", lambda: _raises(m, lambda: m.extract_surface(tree.accel, 2, 1.0)))
    surface = m.extract_surface(tree.accel, 3, 1.0)
    n_verts, n_indices = surface.counts()
    assert n_verts > 0 and n_indices > 0
    adopted = surface.to_mesh()
    assert adopted.vertex_count == n_verts
    torch.cuda.synchronize()
    del surface, adopted, mesh, wire
    desc = m.mlp_desc(**CONFIGS["w64_l1_min"])
    mlp = m.Mlp(desc, mlp_cases.make_params(m, desc, seed=3))
    for n in (64, 4096):     # the scratch regrows
        x, cluster = mlp_cases.make_samples(desc, n, seed=4)
        out = torch.zeros((n, desc.out_dim), dtype=torch.float32, device="cuda")
        mlp.query(torch.from_numpy(cluster).cuda(), torch.from_numpy(x).cuda(), out)
    torch.cuda.synchronize()
    del mlp
    gc.collect()


def _raises(m, call):
    try:
        call()
    except m.MnvError:
        return
    raise AssertionError("the call was not refused")


def _renderer(m, torch, tree):
    r = m.Renderer()
    r.resize(64, 48)
    r.set(tree, 2 * tree.capacity)
    r.options.grid_max_depth = 3
    r.set_camera((-2.5, 1.4, 1.8), (-0.74, 0.4, 0.54), fx=60.0)

    def frames(w, h):
        r.render()                                        # plain
        r.set_antialiasing(4)
        r.render()
        r.set_antialiasing(1)
        r.set_projection(m.PROJ_EQUIRECT)
        r.render()
        r.set_projection(m.PROJ_PINHOLE)
        r.set_target(torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda"))
        r.render()
        assert r.metrics()["n_px"] > 0
        r.set_target(None)
        r.options.show_grid = True
        r.render()
        r.options.show_grid = False

    frames(64, 48)
    r.resize(96, 64)
    frames(96, 64)
    r.sync_tree()
    torch.cuda.synchronize()
    del r
    gc.collect()


def _cycle(m, torch, live, i):
    infos = [_accel_steps(m, torch, live, 4, refuse=True), _accel_steps(m, torch, live, 7, refuse=False)]
    assert infos[1]["grid2_level"] > 0 and infos[1]["brick_levels"] > 0, infos   # the deep tree reached the patch items and the inline words
    tree = m.N3Tree.synth_random(depth=4, basis_dim=4)
    tree.move_to_device()
    _small_objects(m, torch, live, tree)
    del tree
    tree = m.N3Tree.synth_random(depth=4, basis_dim=4)
    _renderer(m, torch, tree)
    del tree
    gc.collect()
    torch.cuda.synchronize()
    dev, pinned = live()
    print(f"cycle {i} device {dev} pinned {pinned}", flush=True)


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import mega_nerf_viewer_amd as mnv_

    assert os.environ.get("MNV_LIB_PATH", "").endswith(os.path.join("testhooks", "libmnv.so"))
    hooks_lib = mnv_.hooks_lib()
    live_ = lambda: (int(hooks_lib.mnv_hook_live_bytes(0)), int(hooks_lib.mnv_hook_live_bytes(1)))   # noqa: E731
    assert live_() == (0, 0)
    for k in range(CYCLES):
        _cycle(mnv_, torch, live_, k + 1)
    print("refused calls ok", flush=True)
