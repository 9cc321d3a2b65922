"""The grid overlay on the device: the edge list (mnv_wireframe) equals N3Tree::gen_wireframe's edges, mnv_render_wireframe equals the numpy
restatement of its raster contract bit for bit, and VolumeRenderer frames with show_grid equal the oracle's frame over those two images."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import wireframe_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mega-nerf-viewer_amd")


def _sorted_rows(a):
    a = np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 6)
    return a[np.lexsort(a.T[::-1])]


def _host_segments(tree, depth):
    return wireframe_ref.segments_from_vertices(tree.gen_wireframe(depth))


def _device_wireframe(mnv, tree, depth):
    try:
        tree.device_view()
    except mnv.MnvError:
        tree.move_to_device()
    return mnv.Wireframe(tree.device_view(), depth)


def _render(mnv, torch, w, cam, opt, tile=None):
    t, i = w.render(cam, opt, tile)
    torch.cuda.synchronize()
    return t.cpu().numpy(), i.cpu().numpy()


def _assert_raster(mnv, torch, tree, depth, cam, opt, tile=None):
    """Both raster methods (tile-binned LDS resolve, global key image) against the contract, twice each (the scratch is reused)."""
    w = _device_wireframe(mnv, tree, depth)
    tile = tile or (0, 0, cam.width, cam.height)
    want_t, want_i = wireframe_ref.raster(_host_segments(tree, depth), cam.c, tile, opt.background_brightness)
    for method in (mnv.WIREFRAME_BINNED, mnv.WIREFRAME_GLOBAL, mnv.WIREFRAME_AUTO, mnv.WIREFRAME_BINNED):
        w.set_method(method)
        got_t, got_i = _render(mnv, torch, w, cam, opt, tile)
        bad = (got_t.view(np.uint32) != want_t.view(np.uint32)) | (got_i != want_i).any(axis=-1)
        assert not bad.any(), f"method {method}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"
    hits = int((want_t != np.float32(1e9)).sum())
    return hits


@pytest.mark.parametrize("name", ["sh4_d6", "terrain_d7_aniso", "sh9_d7_aniso"])
def test_device_segments_equal_gen_wireframe(mnv, torch_gpu, name):
    tree = cases.make_tree(mnv, cases.CASES[name]["tree"])
    tree.move_to_device()
    for depth in (-1, 0, 2, 4, 100):
        w = mnv.Wireframe(tree.device_view(), depth)
        got = w.segments().cpu().numpy()
        want = _host_segments(tree, depth)
        assert got.shape == want.shape and w.cube_count * 12 == want.shape[0], depth
        assert np.array_equal(_sorted_rows(got), _sorted_rows(want)), depth
    w.update(tree.device_view(), 1)                                   # in place, another depth
    assert np.array_equal(_sorted_rows(w.segments().cpu().numpy()), _sorted_rows(_host_segments(tree, 1)))


def test_wireframe_refuses_n_other_than_2_and_host_arrays(mnv, torch_gpu):
    tree = mnv.N3Tree.synth_random(depth=3, basis_dim=1, seed=1)
    tree.move_to_device()
    v = tree.device_view()
    v.N = 3
    with pytest.raises(mnv.MnvError) as e:
        mnv.Wireframe(v, 2)
    assert e.value.code == mnv.MNV_E_UNSUPPORTED
    with pytest.raises(mnv.MnvError) as e:
        mnv.Wireframe(tree.host_view(), 2)
    assert e.value.code == mnv.MNV_E_INVALID


RASTER_CASES = {
    # name: (tree case, camera spec override or None = the case's camera, tile or None)
    "outside": ("sh4_d6", None, None),
    "oblique_aniso": ("sh9_d7_aniso", None, None),
    "inside": ("camera_inside", None, None),
    "odd_size_offcentre": ("sh4_d6", dict(width=201, height=147, fx=650.0, cx=93.25, cy=80.5, center=(-2.4, 1.1, 1.6), back=(-0.72, 0.33, 0.48)), None),
    "sub_tile": ("terrain_d7_aniso", None, (37, 21, 150, 90)),
}


@pytest.mark.parametrize("name", sorted(RASTER_CASES))
def test_raster_equals_the_contract(mnv, torch_gpu, name):
    base, cam_spec, tile = RASTER_CASES[name]
    spec = cases.CASES[base]
    tree = cases.make_tree(mnv, spec["tree"])
    cam = cases.make_camera(mnv, cam_spec or spec["camera"])
    opt = cases.make_options(mnv, spec["options"])
    total = 0
    for depth in (0, 1, 2, 3, 4, 100):
        for bg in (0.0, 0.5, 1.0):
            opt.background_brightness = bg
            total += _assert_raster(mnv, torch_gpu, tree, depth, cam, opt, tile)
    assert total > 1000


def test_raster_full_depth_of_a_depth6_tree(mnv, torch_gpu):
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    cam = cases.make_camera(mnv, spec["camera"])
    opt = cases.make_options(mnv, spec["options"])
    assert _assert_raster(mnv, torch_gpu, tree, 5, cam, opt) > 1000


def test_raster_cfg2_1080p_depth4(mnv, torch_gpu):
    tree = cases.make_tree(mnv, cases.CFG2_TREE)
    cam = cases.cfg2_camera(mnv)
    opt = mnv.RenderOptions.cli_defaults()
    assert _assert_raster(mnv, torch_gpu, tree, 4, cam, opt) > 50000


# ------------------------------------------------------------------------------------------------ the renderer

def _renderer(mnv, tree, spec, opt, **over):
    r = mnv.Renderer()
    cs = spec["camera"]
    r.resize(cs["width"], cs["height"])
    r.set(tree, tree.capacity)
    r.set_camera(cs["center"], cs["back"], fx=cs["fx"], up=cs.get("up", (0.0, 0.0, 1.0)))
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    for k, v in over.items():
        setattr(r.options, k, v)
    return r


def _grid_inputs(tree, cam, opt, depth):
    """T and I of the contract for camera struct `cam` (use the renderer's own: Renderer.last_camera())."""
    return wireframe_ref.raster(_host_segments(tree, depth), cam, (0, 0, cam.width, cam.height), opt.background_brightness)


def _grid_frame_oracle(mnv, orc, tree, cam, opt, depth):
    v = tree.host_view()
    t, img = _grid_inputs(tree, cam, opt, depth)
    return orc.render(orc.tree_from_view(v), cam, opt, want_rgba8=True, tmax_px=t, rgba8_init=img)


@pytest.mark.parametrize("name", ["sh9_d7_aniso", "terrain_d7_aniso"])
def test_renderer_grid_frame_equals_the_oracle(mnv, orc, torch_gpu, name):
    spec = cases.CASES[name]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    cam = cases.make_camera(mnv, spec["camera"])
    opt = cases.make_options(mnv, spec["options"])
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(v.basis_dim - 1, 0)
    for depth in (2, 4):
        for in_flight in (1, 3):      # slot 0's path and a slot in flight; three frames each, against the camera of every frame
            r = _renderer(mnv, tree, spec, opt, show_grid=True, grid_max_depth=depth)
            r.set_frames_in_flight(in_flight)
            for f in range(3):
                st = r.render()
                f32, u8 = r.download(want_rgba8=True)
                want = _grid_frame_oracle(mnv, orc, tree, r.last_camera(), opt, depth)
                assert st["used_accel"]
                assert np.array_equal(cases.bits(f32), cases.bits(want["rgba"])) and np.array_equal(u8, want["rgba8"]), (depth, in_flight, f)
    # the grid changes the frame
    want = _grid_frame_oracle(mnv, orc, tree, cam.c, opt, 3)
    got = orc.render(orc.tree_from_view(v), cam.c, opt, want_rgba8=True)
    assert int((cases.bits(got["rgba"]) != cases.bits(want["rgba"])).any(axis=-1).sum()) > 100   # the grid shows


def _model(mnv, v):
    import mlp_cases
    from test_renderer_refine_gpu import make_grid
    desc = mnv.mlp_desc(n_clusters=6, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=64, hidden_layers=2, out_dim=v.data_dim + 1)
    return desc, mlp_cases.make_params(mnv, desc, seed=21), make_grid(mnv)


def test_renderer_grid_tracker_and_guided_frames(mnv, orc, torch_gpu):
    """The grid's images reach the other frame kinds of VolumeRenderer::render: the refinement frame (trackers + visit marks on the packed
    accel, mnv_render_voxels_accel_visit_ex) equals the oracle's frame over T and I; the guided-sampling frame, fused and four-step, equals
    mnv_render_guided_fused called with the grid's depth image (the guided composite does not show the image)."""
    torch = torch_gpu
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    opt = cases.make_options(mnv, spec["options"])
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(v.basis_dim - 1, 0)
    desc, params, grid = _model(mnv, v)
    # refinement frame: the picture is drawn before the frame's tree edit
    r = _renderer(mnv, tree, spec, opt, show_grid=True, grid_max_depth=3)
    r.set(tree, v.capacity * 4)
    r.set_model(desc, params, grid)
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.show_grid, r.options.grid_max_depth = True, 3
    r.options.use_splitting, r.options.split_batch_size, r.options.max_depth = True, 64, 8
    st = r.render()
    f32, u8 = r.download(want_rgba8=True)
    assert st["used_accel"] and not st["fused"]
    cam = r.last_camera()
    want = orc.render(orc.tree_from_view(v), cam, opt, want_rgba8=True, tmax_px=_grid_inputs(tree, cam, opt, 3)[0],
                      rgba8_init=_grid_inputs(tree, cam, opt, 3)[1])
    assert np.array_equal(cases.bits(f32), cases.bits(want["rgba"])) and np.array_equal(u8, want["rgba8"])
    # guided sampling, fused and four-step, against the fused entry point with the same depth image
    tree = cases.make_tree(mnv, spec["tree"])
    for fused in (True, False):
        r = _renderer(mnv, tree, spec, opt, show_grid=True, grid_max_depth=3)
        r.set_model(desc, params, grid)
        r.options.use_guided_sampling, r.options.max_guided_samples = True, 16
        r.set_fused_guided(fused)
        st = r.render()
        assert bool(st["fused"]) == fused
        got = r.download()
        cam = r.last_camera()
        t, _ = _grid_inputs(tree, cam, opt, 3)
        opt2 = mnv.RenderOptions()
        C.memmove(C.byref(opt2), C.byref(r.options), C.sizeof(opt2))
        cam_obj = mnv.Camera(cam.width, cam.height, cam.fx)
        C.memmove(C.byref(cam_obj.c), C.byref(cam), C.sizeof(cam))
        out = torch.empty((cam.height, cam.width, 4), dtype=torch.float32, device="cuda")
        mnv.render_guided_fused(tree.accel, cam_obj, opt2, mnv.Mlp(desc, params), grid, rgba=out, tmax_px=torch.from_numpy(t).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(cases.bits(got), cases.bits(out.cpu().numpy())), f"guided frame (fused {fused})"
        mnv.render_guided_fused(tree.accel, cam_obj, opt2, mnv.Mlp(desc, params), grid, rgba=out)
        torch.cuda.synchronize()
        assert (cases.bits(got) != cases.bits(out.cpu().numpy())).any()   # the grid's depth image matters


def test_frames_in_flight_3_equal_1_with_the_grid(mnv, torch_gpu):
    spec = cases.CASES["terrain_d7_aniso"]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    opt = cases.make_options(mnv, spec["options"])
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(v.basis_dim - 1, 0)
    frames = {}
    for k in (1, 3):
        r = _renderer(mnv, tree, spec, opt, show_grid=True, grid_max_depth=3)
        r.set_frames_in_flight(k)
        out = []
        for f in range(6):
            r.options.grid_max_depth = 3 if f < 3 else 4      # a depth change regenerates between frames in flight
            r.render()
            out.append(r.download_slot(r.last_slot(), want_rgba8=True))
        frames[k] = out
    for (a, a8), (b, b8) in zip(frames[1], frames[3]):
        assert np.array_equal(cases.bits(a), cases.bits(b)) and np.array_equal(a8, b8)


@pytest.mark.parametrize("bg", [0.0, 1.0])
def test_uncovered_pixels_equal_the_frame_without_grid(mnv, torch_gpu, bg):
    spec = cases.CASES["sh9_d7_aniso"]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    cam = cases.make_camera(mnv, spec["camera"])
    opt = cases.make_options(mnv, spec["options"])
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(v.basis_dim - 1, 0)
    opt.background_brightness = bg
    plain = _renderer(mnv, tree, spec, opt)
    plain.render()
    p32, p8 = plain.download(want_rgba8=True)
    r = _renderer(mnv, tree, spec, opt, show_grid=True, grid_max_depth=3)
    r.render()
    g32, g8 = r.download(want_rgba8=True)
    t, _ = wireframe_ref.raster(_host_segments(tree, 3), cam.c, (0, 0, cam.width, cam.height), bg)
    free = t == np.float32(1e9)
    assert free.sum() > 1000 and (~free).sum() > 1000
    assert np.array_equal(cases.bits(g32[free]), cases.bits(p32[free])) and np.array_equal(g8[free], p8[free])
    assert (cases.bits(g32[~free]) != cases.bits(p32[~free])).any()


def test_show_grid_off_frames_are_unchanged(mnv, orc, torch_gpu):
    spec = cases.CASES["sh9_d7_aniso"]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    cam = cases.make_camera(mnv, spec["camera"])
    opt = cases.make_options(mnv, spec["options"])
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(v.basis_dim - 1, 0)
    want = orc.render(orc.tree_from_view(v), cam.c, opt, want_rgba8=True)
    r = _renderer(mnv, tree, spec, opt, show_grid=False, grid_max_depth=3)
    r.render()
    f32, u8 = r.download(want_rgba8=True)
    assert np.array_equal(cases.bits(f32), cases.bits(want["rgba"])) and np.array_equal(u8, want["rgba8"])
    assert r.wireframe() == 0


def test_grid_follows_a_split(mnv, torch_gpu):
    """A refinement frame with the grid on splits leaves; the next grid frame's edge list equals gen_wireframe of the synced tree."""
    import mlp_cases
    from test_renderer_refine_gpu import make_grid
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    opt = cases.make_options(mnv, spec["options"])
    desc = mnv.mlp_desc(n_clusters=6, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=64, hidden_layers=2, out_dim=v.data_dim + 1)
    params = mlp_cases.make_params(mnv, desc, seed=21)
    r = mnv.Renderer()
    cs = spec["camera"]
    r.resize(cs["width"], cs["height"])
    r.set(tree, v.capacity * 4)
    r.set_model(desc, params, make_grid(mnv))
    r.set_camera(cs["center"], cs["back"], fx=cs["fx"])
    r.options.show_grid, r.options.grid_max_depth = True, 100
    r.options.use_splitting = True
    r.options.split_batch_size = 64
    r.options.max_depth = 8
    cap0 = v.capacity
    added = 0
    for _ in range(3):
        added += r.render()["added"]
    assert added > 0
    r.options.use_splitting = False
    r.render()
    r.sync_tree()
    assert tree.capacity > cap0
    got = mnv.wireframe_segments(r.wireframe()).cpu().numpy()
    assert np.array_equal(_sorted_rows(got), _sorted_rows(_host_segments(tree, 100)))


def test_show_grid_refuses_frame_inputs_and_ranks(mnv, torch_gpu):
    torch = torch_gpu
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    opt = cases.make_options(mnv, spec["options"])
    r = _renderer(mnv, tree, spec, opt, show_grid=True)
    cs = spec["camera"]
    t = torch.zeros((cs["height"], cs["width"]), dtype=torch.float32, device="cuda")
    r.set_frame_inputs(t, None)
    with pytest.raises(mnv.MnvError) as e:
        r.render()
    assert e.value.code == mnv.MNV_E_INVALID and "show_grid" in str(e.value)
    r.set_frame_inputs(None, None)
    r.render()                                              # and fine without them
    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)         # one rank through RCCL
    try:
        r.set_ranks(comm)
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == mnv.MNV_E_INVALID and "set_ranks" in str(e.value)
        r.set_ranks(None)
        r.render()
    finally:
        r.set_ranks(None)
        comm.close()


def _run_cli(args, out):
    exe = os.path.join(PKG, "mnv_render")
    r = subprocess.run([exe] + args + ["--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_cli_grid(mnv, orc, torch_gpu, tmp_path):
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    path = str(tmp_path / "t.npz")
    tree.save_npz(path)
    base = [path, "-w", "96", "-h", "80", "--fx", "150", "--in_flight", "1"]
    _run_cli(base, str(tmp_path / "plain"))
    _run_cli(base + ["--grid", "3"], str(tmp_path / "grid"))
    plain, grid = _ppm(str(tmp_path / "plain_0000.ppm")), _ppm(str(tmp_path / "grid_0000.ppm"))
    assert (plain != grid).any()
    # the same frame through the Renderer (the CLI's default camera and options)
    t2 = mnv.N3Tree.open(path)
    opt = mnv.RenderOptions.cli_defaults()
    opt.show_grid, opt.grid_max_depth = True, 3
    r = mnv.Renderer()
    r.resize(96, 80)
    r.set(t2, t2.capacity)
    r.set_camera((-3.5, 0.0, 3.5), (-0.7071068, 0.0, 0.7071068), fx=150.0)
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    r.render()
    _, u8 = r.download(want_rgba8=True)
    assert np.array_equal(u8[..., :3], grid)
    # --bounds_only --grid 0: the root cube cut in eight, nothing else
    _run_cli(base + ["-b", "--grid", "0", "--bg", "1"], str(tmp_path / "bounds"))
    img = _ppm(str(tmp_path / "bounds_0000.ppm"))
    cam = mnv.Camera(96, 80, 150.0).set_pose((-3.5, 0.0, 3.5), (-0.7071068, 0.0, 0.7071068))
    v = tree.host_view()
    one = np.zeros((1, 8), np.int32)
    segs = wireframe_ref.segments_from_vertices(wireframe_ref.gen_wireframe(one, list(v.offset), list(v.scale), 0))
    assert segs.shape == (8 * 12, 6)
    _, want8 = wireframe_ref.raster(segs, cam.c, (0, 0, 96, 80), 1.0)
    assert np.array_equal(img, want8[..., :3])
    r = subprocess.run([os.path.join(PKG, "mnv_render"), path, "--grid", "2", "--gpus", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--grid" in r.stderr
