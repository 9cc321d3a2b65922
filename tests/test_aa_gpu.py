"""Anti-aliased frames on the device.  mnv_resolve_samples equals the numpy restatement of its contract (tests/aa_ref.py) bit for bit; a
Renderer with set_antialiasing(K, filter) equals that restatement applied to K frames rendered one at a time with the shifted cameras;
K = 1 is the renderer as it was; the combinations the renderer cannot serve are refused; mnv_render --aa writes the Renderer's frame.
No tolerance anywhere: the contract fixes the order of every float operation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aa_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mega-nerf-viewer_amd")

SHAPES = [(1, 1), (5, 3), (33, 9), (70, 37), (129, 65)]   # narrower than any halo, off every tile multiple (32 x 8), just past one
KS = [1, 2, 5, 16]
RADII = [0, 1, 2]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sub_frames(rng, k, w, h):
    sub = rng.random((k, h, w, 4), dtype=np.float32)
    pick = rng.random(sub.shape)
    sub[pick < 0.05] = 0.0
    sub[(pick >= 0.05) & (pick < 0.10)] = 1.0
    sub[(pick >= 0.10) & (pick < 0.15)] = 1.5            # both ends of the pack
    return sub


def _table(rng, k, r):
    d = 2 * r + 1
    w = (0.1 + 0.9 * rng.random((k, d, d))).astype(np.float32)
    flat = w.reshape(-1)
    flat[rng.permutation(flat.size)[:(flat.size + 1) // 3]] = 0.0          # a third of the entries, exactly 0 (none of a single weight)
    return w


def _resolve(mnv, torch, sub_t, w_np, r, want_f32=True, want_u8=True):
    k, h, w, _ = sub_t.shape
    f32 = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") if want_f32 else None
    u8 = torch.full((h, w, 4), 77, dtype=torch.uint8, device="cuda") if want_u8 else None
    mnv.resolve_samples(sub_t, w_np, r, rgba=f32, rgba8=u8)
    torch.cuda.synchronize()
    return (f32.cpu().numpy() if want_f32 else None), (u8.cpu().numpy() if want_u8 else None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resolve_kernel_equals_the_contract(mnv, torch_gpu, shape):
    torch = torch_gpu
    w, h = shape
    rng = np.random.default_rng(1000 * w + h)
    for k in KS:
        sub = _sub_frames(rng, k, w, h)
        sub_t = torch.from_numpy(sub).cuda()
        for r in RADII:
            table = _table(rng, k, r)
            assert int((table == 0).sum()) == (table.size + 1) // 3 and (table != 0).any()
            want_f32, want_u8 = aa_ref.resolve(sub, table, r)
            got_f32, got_u8 = _resolve(mnv, torch, sub_t, table, r)
            assert np.array_equal(bits(got_f32), bits(want_f32)), (shape, k, r)
            assert np.array_equal(got_u8, want_u8), (shape, k, r)
            # either output alone is the same output
            alone_f32, _ = _resolve(mnv, torch, sub_t, table, r, want_u8=False)
            _, alone_u8 = _resolve(mnv, torch, sub_t, table, r, want_f32=False)
            assert np.array_equal(bits(alone_f32), bits(want_f32)) and np.array_equal(alone_u8, want_u8), (shape, k, r)
            # no weight at all: wsum == 0, the frame is 0
            zero_f32, zero_u8 = _resolve(mnv, torch, sub_t, np.zeros_like(table), r)
            assert not bits(zero_f32).any() and not zero_u8.any(), (shape, k, r)


def test_resolve_with_the_library_s_own_tables(mnv, torch_gpu):
    """The box and tent tables of mnv_aa_weights through the kernel: the box resolve is the plain mean in sample order."""
    torch = torch_gpu
    rng = np.random.default_rng(7)
    for k in (4, 16, 64):
        sub = _sub_frames(rng, k, 70, 37)
        sub_t = torch.from_numpy(sub).cuda()
        off = mnv.aa_pattern(k)
        for filt, r in ((mnv.AA_BOX, 0), (mnv.AA_TENT, 1)):
            table = mnv.aa_weights(filt, off)
            assert table.shape[1] // 2 == r
            want_f32, want_u8 = aa_ref.resolve(sub, table, r)
            got_f32, got_u8 = _resolve(mnv, torch, sub_t, table, r)
            assert np.array_equal(bits(got_f32), bits(want_f32)) and np.array_equal(got_u8, want_u8), (k, filt)
        mean = np.zeros((37, 70, 4), np.float32)
        for s in sub:
            mean = mean + s
        mean = mean / np.float32(k)
        got_f32, _ = _resolve(mnv, torch, sub_t, mnv.aa_weights(mnv.AA_BOX, off), 0)
        assert np.array_equal(bits(got_f32), bits(mean))


def test_resolve_refuses_bad_arguments(mnv, torch_gpu):
    torch = torch_gpu
    lib = mnv.lib()
    sub = torch.zeros((2, 4, 8, 4), dtype=torch.float32, device="cuda")
    w = torch.ones((2, 25), dtype=torch.float32, device="cuda")
    f32 = torch.zeros((4, 8, 4), dtype=torch.float32, device="cuda")
    u8 = torch.zeros((4 * 8 * 4 + 8,), dtype=torch.uint8, device="cuda")
    s, wp, fp, up = sub.data_ptr(), w.data_ptr(), f32.data_ptr(), u8.data_ptr()
    assert up % 4 == 0
    bad = [
        (None, 2, 8, 4, wp, 1, fp, up),        # no sub-frames
        (s, 2, 8, 4, None, 1, fp, up),         # no weights
        (s, 2, 8, 4, wp, 1, None, None),       # no output
        (s, 0, 8, 4, wp, 1, fp, up),           # sample counts outside 1 .. MAX_BATCH
        (s, 65, 8, 4, wp, 1, fp, up),
        (s, 2, 8, 4, wp, -1, fp, up),          # radius outside 0 .. 2
        (s, 2, 8, 4, wp, 3, fp, up),
        (s, 2, 0, 4, wp, 1, fp, up),           # non-positive sizes
        (s, 2, 8, 0, wp, 1, fp, up),
        (s, 2, -8, 4, wp, 1, fp, up),
        (s, 2, 8, 4, wp, 1, fp, up + 2),       # rgba8_out not 4-byte aligned
        (s, 2, 8, 4, wp, 1, None, up + 1),
        (s + 4, 1, 8, 4, wp, 1, fp, up),       # the 16-byte loads and stores need aligned float arrays
        (s, 2, 8, 4, wp, 1, fp + 4, None),
    ]
    for a in bad:
        assert lib.mnv_resolve_samples(*a, None) == mnv.MNV_E_INVALID, a
    torch.cuda.synchronize()
    assert not f32.any().item() and not u8.any().item()          # nothing ran
    assert lib.mnv_resolve_samples(s, 2, 8, 4, wp, 1, fp, up, None) == mnv.MNV_OK
    assert lib.mnv_resolve_samples(s, 2, 8, 4, wp, 1, fp, up + 4, None) == mnv.MNV_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ whole frames

W, H, FX = 96, 64, 150.0
CENTER, BACK = (-3.5, 0.0, 3.5), (-0.7071068, 0.0, 0.7071068)


@pytest.fixture(scope="module")
def tree(mnv, torch_gpu):
    return mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=11)


def _renderer(mnv, tree, in_flight=None, **over):
    r = mnv.Renderer()
    r.resize(W, H)
    r.set(tree, tree.capacity)
    r.set_camera(CENTER, BACK, fx=FX)
    if in_flight is not None:
        r.set_frames_in_flight(in_flight)
    for k, v in over.items():
        setattr(r.options, k, v)
    return r


def _shifted(mnv, cam_struct, dx, dy):
    """The renderer's camera with the principal point moved by (-dx, -dy), in float32."""
    cam = mnv.Camera(cam_struct.width, cam_struct.height, cam_struct.fx)
    C.memmove(C.byref(cam.c), C.byref(cam_struct), C.sizeof(cam_struct))
    cam.c.cx = float(np.float32(cam_struct.cx) - np.float32(dx))
    cam.c.cy = float(np.float32(cam_struct.cy) - np.float32(dy))
    return cam


def _one_at_a_time(mnv, torch, tree, r, k, filt, grid_depth=None):
    """aa_ref.resolve of k frames of the renderer's last camera, each rendered alone with render_voxels_accel."""
    off = aa_ref.pattern(k)
    lc = r.last_camera()
    wire = mnv.Wireframe(tree.device_view(), grid_depth) if grid_depth is not None else None
    sub = np.empty((k, H, W, 4), np.float32)
    for i in range(k):
        cam = _shifted(mnv, lc, off[i, 0], off[i, 1])
        out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        if wire is not None:
            tmax, img = wire.render(cam, r.options)
            mnv.render_voxels_accel(tree.accel, cam, r.options, rgba=out, tmax_px=tmax, rgba8_init=img)
        else:
            mnv.render_voxels_accel(tree.accel, cam, r.options, rgba=out)
        torch.cuda.synchronize()
        sub[i] = out.cpu().numpy()
    assert not np.isnan(sub).any()
    table = aa_ref.weights(filt, off)
    return aa_ref.resolve(sub, table, table.shape[1] // 2), sub


@pytest.mark.parametrize("k,filt", [(4, aa_ref.AA_TENT), (5, aa_ref.AA_BOX), (16, aa_ref.AA_TENT)])
def test_renderer_frame_equals_the_resolve_of_single_frames(mnv, torch_gpu, tree, k, filt):
    r = _renderer(mnv, tree)
    r.set_antialiasing(k, filt)
    st = r.render()
    f32, u8 = r.download(want_rgba8=True)
    (want_f32, want_u8), sub = _one_at_a_time(mnv, torch_gpu, tree, r, k, filt)
    assert st["used_accel"]
    assert np.array_equal(bits(f32), bits(want_f32)) and np.array_equal(u8, want_u8)
    # the sub-frames differ from each other (the jitter moves the picture) and the frame is none of them
    assert (bits(sub[0]) != bits(sub[1])).any() and (bits(f32) != bits(sub[0])).any()
    assert f32[..., 3].max() > 0                                             # the volume is in view


def test_renderer_depth_frame(mnv, torch_gpu, tree):
    r = _renderer(mnv, tree, render_depth=True)
    r.set_antialiasing(4, mnv.AA_TENT)
    r.render()
    f32, u8 = r.download(want_rgba8=True)
    (want_f32, want_u8), _ = _one_at_a_time(mnv, torch_gpu, tree, r, 4, aa_ref.AA_TENT)
    assert np.array_equal(bits(f32), bits(want_f32)) and np.array_equal(u8, want_u8)
    plain = _renderer(mnv, tree)
    plain.set_antialiasing(4, mnv.AA_TENT)
    plain.render()
    assert (bits(plain.download()) != bits(f32)).any()                        # depth mode shows


@pytest.mark.parametrize("in_flight", [1, 3])
def test_renderer_grid_frame(mnv, torch_gpu, tree, in_flight):
    """show_grid: the sub-frames are issued one by one (grid pass + march per camera), on slot 0's stream and on a slot in flight."""
    r = _renderer(mnv, tree, in_flight=in_flight, show_grid=True, grid_max_depth=2, background_brightness=1.0)
    r.set_antialiasing(4, mnv.AA_TENT)
    for f in range(2):
        r.render()
        f32, u8 = r.download(want_rgba8=True)
        (want_f32, want_u8), _ = _one_at_a_time(mnv, torch_gpu, tree, r, 4, aa_ref.AA_TENT, grid_depth=2)
        assert np.array_equal(bits(f32), bits(want_f32)) and np.array_equal(u8, want_u8), f
    no_grid = _renderer(mnv, tree, background_brightness=1.0)
    no_grid.set_antialiasing(4, mnv.AA_TENT)
    no_grid.render()
    assert (bits(no_grid.download()) != bits(f32)).any()                      # the grid shows
    # its lines are filtered: pixels between the background and the line's black exist (a point-sampled grid frame over an empty
    # stretch of background has only the two)
    point = _renderer(mnv, tree, show_grid=True, grid_max_depth=2, background_brightness=1.0)
    point.render()
    empty = point.download()[..., 3] == 0
    assert empty.sum() > 100
    assert set(np.unique(point.download()[empty][:, 0]).tolist()) <= {0.0, 1.0}
    assert len(np.unique(f32[empty][:, 0])) > 2


def test_one_sample_is_the_renderer_as_it_was(mnv, torch_gpu, tree):
    plain = _renderer(mnv, tree)
    plain.render()
    want_f32, want_u8 = plain.download(want_rgba8=True)
    for filt in (mnv.AA_TENT, mnv.AA_BOX):
        r = _renderer(mnv, tree)
        r.set_antialiasing(1, filt)
        r.render()
        f32, u8 = r.download(want_rgba8=True)
        assert f32.tobytes() == want_f32.tobytes() and u8.tobytes() == want_u8.tobytes(), filt
    r = _renderer(mnv, tree)                    # ... also after anti-aliased frames (their buffers go)
    r.set_antialiasing(4, mnv.AA_TENT)
    r.render()
    assert r.download().tobytes() != want_f32.tobytes()
    r.set_antialiasing(1, mnv.AA_TENT)
    for _ in range(2):
        r.render()
        f32, u8 = r.download(want_rgba8=True)
        assert f32.tobytes() == want_f32.tobytes() and u8.tobytes() == want_u8.tobytes()


def _orbit(mnv, r, f):
    a = np.deg2rad(7.0 * f)
    c, s = float(np.cos(a)), float(np.sin(a))
    rot = lambda v: (c * v[0] - s * v[1], s * v[0] + c * v[1], v[2])
    r.set_camera(rot(CENTER), rot(BACK), fx=FX)


def test_frames_in_flight_do_not_change_the_frames(mnv, torch_gpu, tree):
    """Four frames of an orbit, three in flight (every slot owns its sub-frame buffer; the fourth frame reuses the first one's slot)
    against the same four on one stream."""
    frames = {}
    for in_flight in (3, 1):
        r = _renderer(mnv, tree, in_flight=in_flight)
        r.set_antialiasing(4, mnv.AA_TENT)
        got, slots = [], []
        for f in range(3):
            _orbit(mnv, r, f)
            r.render()
            slots.append(r.last_slot())
            if in_flight == 1:
                got.append(r.download_slot(slots[-1], want_rgba8=True))
        if in_flight == 3:
            assert len(set(slots)) == 3
            got.append(r.download_slot(slots[0], want_rgba8=True))       # before frame 3 takes its slot
        _orbit(mnv, r, 3)
        r.render()
        slots.append(r.last_slot())
        if in_flight == 3:
            assert slots[3] == slots[0]
            got += [r.download_slot(s, want_rgba8=True) for s in slots[1:]]
        else:
            assert set(slots) == {0}
            got.append(r.download_slot(0, want_rgba8=True))
        frames[in_flight] = got
    for f in range(4):
        assert frames[3][f][0].tobytes() == frames[1][f][0].tobytes() and frames[3][f][1].tobytes() == frames[1][f][1].tobytes(), f
    assert frames[1][0][0].tobytes() != frames[1][1][0].tobytes()         # the orbit moves
    # changing K and the filter between frames rebuilds the buffers and the table
    r = _renderer(mnv, tree, in_flight=3)
    for k, filt in ((4, mnv.AA_TENT), (16, mnv.AA_TENT), (16, mnv.AA_BOX), (2, mnv.AA_BOX)):
        r.set_antialiasing(k, filt)
        r.render()
        f32, u8 = r.download(want_rgba8=True)
        (want_f32, want_u8), _ = _one_at_a_time(mnv, torch_gpu, tree, r, k, filt)
        assert np.array_equal(bits(f32), bits(want_f32)) and np.array_equal(u8, want_u8), (k, filt)
    r.resize(W // 2, H // 2)                    # and a resize frees them
    r.render()
    assert r.download().shape == (H // 2, W // 2, 4)


def _model(mnv, v):
    import mlp_cases
    from test_renderer_refine_gpu import make_grid
    desc = mnv.mlp_desc(n_clusters=6, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=64, hidden_layers=2, out_dim=v.data_dim + 1)
    return desc, mlp_cases.make_params(mnv, desc, seed=21), make_grid(mnv)


def test_refusals(mnv, torch_gpu, tree):
    torch = torch_gpu
    plain = _renderer(mnv, tree)
    plain.render()
    want = plain.download().tobytes()

    def refused(r, word):
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == mnv.MNV_E_INVALID and word in str(e.value), str(e.value)

    # a depth image of the caller's fixed camera cannot follow the jitter
    r = _renderer(mnv, tree)
    t = torch.full((H, W), 1e9, dtype=torch.float32, device="cuda")
    r.set_frame_inputs(t, None)
    r.set_antialiasing(4, mnv.AA_TENT)
    refused(r, "set_frame_inputs")
    r.set_antialiasing(1, mnv.AA_TENT)
    r.render()
    r.download()
    r.set_frame_inputs(None, None)
    r.set_antialiasing(4, mnv.AA_TENT)
    r.render()
    # refinement votes per ray of one camera
    own = mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=11)           # (refinement frames edit their tree)
    r = _renderer(mnv, own)
    r.set_model(*_model(mnv, own.host_view()))
    r.set_antialiasing(4, mnv.AA_TENT)
    r.render()                                                             # a model alone is no obstacle
    r.options.use_guided_sampling = True
    refused(r, "use_guided_sampling")
    r.set_antialiasing(1, mnv.AA_BOX)
    r.render()
    r.options.use_guided_sampling = False
    r.options.use_splitting = True
    r.set_antialiasing(4, mnv.AA_TENT)
    refused(r, "use_splitting")
    r.set_antialiasing(1, mnv.AA_TENT)
    r.render()
    r.options.use_splitting = False
    r.set_antialiasing(4, mnv.AA_TENT)
    r.render()
    r.download()
    # more samples than one launch takes; no samples; an unknown filter
    r = _renderer(mnv, tree)
    for k in (65, 0, -3):
        r.set_antialiasing(k, mnv.AA_TENT)
        refused(r, "aa_samples")
    with pytest.raises(mnv.MnvError) as e:
        r.set_antialiasing(4, 2)
    assert e.value.code == mnv.MNV_E_INVALID
    r.set_antialiasing(1, mnv.AA_TENT)
    r.render()
    assert r.download().tobytes() == want
    r.set_antialiasing(64, mnv.AA_BOX)                                     # the largest count there is
    r.render()
    (want_f32, _), _ = _one_at_a_time(mnv, torch, tree, r, 64, aa_ref.AA_BOX)
    assert np.array_equal(bits(r.download()), bits(want_f32))
    # no tree
    r = mnv.Renderer()
    r.resize(W, H)
    r.set_antialiasing(4, mnv.AA_TENT)
    refused(r, "packed accel")
    r.set_antialiasing(1, mnv.AA_TENT)
    r.render()


def test_cli_writes_the_renderer_s_frame(mnv, torch_gpu, tree, tmp_path):
    path = str(tmp_path / "t.npz")
    tree.save_npz(path)
    exe = os.path.join(PKG, "mnv_render")
    out = str(tmp_path / "aa")
    p = subprocess.run([exe, path, "-w", str(W), "-h", str(H), "--aa", "4", "--aa_filter", "tent", "--out", out, "--raw"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = np.fromfile(out + "_0000.f32", np.float32).reshape(H, W, 4)
    # the same scene through the Renderer: the command line's default camera and options
    t2 = mnv.N3Tree.open(path)
    r = mnv.Renderer()
    r.resize(W, H)
    r.set(t2, t2.capacity)
    r.set_camera(CENTER, BACK, fx=1111.0)
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    opt = mnv.RenderOptions.cli_defaults()
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    r.set_antialiasing(4, mnv.AA_TENT)
    r.render()
    f32, u8 = r.download(want_rgba8=True)
    assert got.tobytes() == f32.tobytes()
    with open(out + "_0000.ppm", "rb") as f:
        ppm = np.frombuffer(f.read().split(b"\n", 3)[3], np.uint8).reshape(H, W, 3)
    assert np.array_equal(ppm, u8[..., :3])
    # ... and it is the anti-aliased frame: the box filter and the point-sampled frame are other frames
    for extra, name in ((["--aa", "4", "--aa_filter", "box"], "box"), ([], "point")):
        p = subprocess.run([exe, path, "-w", str(W), "-h", str(H), "--out", str(tmp_path / name), "--raw"] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert np.fromfile(str(tmp_path / name) + "_0000.f32", np.float32).tobytes() != got.tobytes(), name
    # one process per GPU gathers RGBA8 tiles: refused, with a message, before anything is forked
    p = subprocess.run([exe, path, "-w", str(W), "-h", str(H), "--aa", "4", "--gpus", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--aa" in p.stderr and "--gpus" in p.stderr
    p = subprocess.run([exe, path, "--aa", "4", "--aa_filter", "gauss"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--aa_filter" in p.stderr
