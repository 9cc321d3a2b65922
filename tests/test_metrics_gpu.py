"""Frame metrics on the device (csrc/mnv_metrics.hip) against the numpy restatement of the metric contract (tests/metrics_ref.py): every sums
word and both maps bit for bit, on shapes off every tile multiple, with every flag subset, either map, the standard and an asymmetric window;
masks; a frame against itself; the Renderer's per-slot scores for every frame kind; `mnv_render --target`.  All comparisons are exact."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import metrics_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mega-nerf-viewer_amd", "mnv_render")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(mnv, torch, frame, target8, flags, window=None, maps=("se", "ssim"), sums=None):
    """mnv_frame_metrics on host arrays -> (sums int64 [5], se_map or None, ssim_map or None); the maps start as 7.0 everywhere"""
    h, w = frame.shape[:2]
    f = torch.from_numpy(frame).cuda()
    t = torch.from_numpy(target8).cuda()
    se = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda") if "se" in maps else None
    has_win = w >= 11 and h >= 11
    ss = torch.full((h - 10, w - 10, 3), 7.0, dtype=torch.float32, device="cuda") if "ssim" in maps and has_win else None
    sums = mnv.frame_metrics(f, t, flags, window=window, sums=sums, se_map=se, ssim_map=ss)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), None if se is None else se.cpu().numpy(), None if ss is None else ss.cpu().numpy()


def check(mnv, torch, frame, target8, flags, window=None, want=None):
    """every sums word and both maps against the restatement, with both maps, either alone and none"""
    want = want or ref.frame_metrics(frame, target8, flags, window)
    for maps in (("se", "ssim"), ("se",), ("ssim",), ()):
        sums, se, ss = run(mnv, torch, frame, target8, flags, window, maps)
        assert sums.tolist() == want[0].tolist(), (flags, maps, sums.tolist(), want[0].tolist())
        if se is not None:
            assert np.array_equal(bits(se), bits(want[1])), (flags, maps, int((bits(se) != bits(want[1])).sum()))
        if ss is not None:
            if flags & ref.SSIM:
                assert np.array_equal(bits(ss), bits(want[2])), (flags, maps, int((bits(ss) != bits(want[2])).sum()))
            else:
                assert (ss == 7.0).all()            # without MNV_METRIC_SSIM the map is not touched
    return want


def asymmetric_window(rng):
    g = rng.random(11) + 0.05
    return (g / g.sum()).astype(np.float32)


SHAPES = [(1, 1), (5, 3), (11, 11), (12, 11), (30, 10), (43, 19), (70, 37), (129, 65)]    # (width, height)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_kernel_equals_the_contract(mnv, torch_gpu, shape):
    w, h = shape
    rng = np.random.default_rng(1000 * w + h)
    frame = ref.random_frame(rng, h, w)
    target8 = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    target8[..., 3][rng.random((h, w)) < 0.05] = 0
    assert np.isnan(frame).any() or w * h < 200
    g = asymmetric_window(rng)
    assert not np.array_equal(g, g[::-1])
    for flags in range(8):
        for window in (None, g):
            want = check(mnv, torch_gpu, frame, target8, flags, window)
            n_win = max(w - 10, 0) * max(h - 10, 0)
            if not flags & ref.SSIM or n_win == 0:
                assert want[0][2] == 0 and want[0][3] == 0
            elif not flags & ref.MASK_ALPHA:
                assert want[0][2] == n_win
            assert want[0][0] == (int((target8[..., 3] != 0).sum()) if flags & ref.MASK_ALPHA else w * h)


def test_more_tiles_than_workgroups(mnv, torch_gpu):
    """901 x 451: 841 SSIM tiles for a grid of at most 768 workgroups, 1588 blocks of pixels for a streaming grid of at most 1024 -- some
    workgroups take a second tile / a second stretch of pixels, and their sums and maps are still the restatement's"""
    rng = np.random.default_rng(61)
    frame = ref.random_frame(rng, 451, 901)
    target8 = rng.integers(0, 256, (451, 901, 4), dtype=np.uint8)
    target8[..., 3][rng.random((451, 901)) < 0.01] = 0
    for flags in (0, ref.MASK_ALPHA | ref.QUANTISED, ref.SSIM, ref.SSIM | ref.MASK_ALPHA | ref.QUANTISED):
        want = check(mnv, torch_gpu, frame, target8, flags)
        assert want[0][0] > 400000 and (not flags & ref.SSIM or want[0][2] > 1000)


def test_the_two_passes_are_not_interchangeable(mnv, torch_gpu):
    """what the asymmetric window is for: a transposed frame under it scores differently (under the symmetric window it cannot)"""
    rng = np.random.default_rng(3)
    frame, target8 = ref.random_frame(rng, 24, 24), rng.integers(0, 256, (24, 24, 4), dtype=np.uint8)
    g = asymmetric_window(rng)
    a = ref.frame_metrics(frame, target8, ref.SSIM, g)[2]
    b = ref.frame_metrics(np.ascontiguousarray(frame.transpose(1, 0, 2)), np.ascontiguousarray(target8.transpose(1, 0, 2)), ref.SSIM, g)[2]
    assert not np.array_equal(a, b.transpose(1, 0, 2))
    check(mnv, torch_gpu, frame, target8, ref.SSIM, g)


def test_masks(mnv, torch_gpu):
    rng = np.random.default_rng(11)
    frame = ref.random_frame(rng, 33, 33)
    target8 = rng.integers(0, 256, (33, 33, 4), dtype=np.uint8)
    flags = ref.SSIM | ref.MASK_ALPHA
    target8[..., 3] = 255
    full = check(mnv, torch_gpu, frame, target8, flags)
    assert full[0][0] == 33 * 33 and full[0][2] == 23 * 23
    one = target8.copy()
    one[16, 16, 3] = 0                              # one excluded pixel in the middle: exactly 1 pixel and the 121 windows over it
    got = check(mnv, torch_gpu, frame, one, flags)
    assert got[0][0] == 33 * 33 - 1 and got[0][2] == 23 * 23 - 121
    assert (got[2][6:17, 6:17] == 0).all() and np.count_nonzero((got[2] == 0).all(axis=2)) == 121
    check(mnv, torch_gpu, frame, one, ref.SSIM)     # without the flag the alpha byte means nothing
    rnd = target8.copy()
    rnd[..., 3][rng.random((33, 33)) < 0.05] = 0
    check(mnv, torch_gpu, frame, rnd, flags | ref.QUANTISED)
    none = target8.copy()
    none[..., 3] = 0
    zero = check(mnv, torch_gpu, frame, none, flags)
    assert zero[0].tolist() == [0, 0, 0, 0, 0] and not zero[1].any() and not zero[2].any()


def test_a_frame_against_itself(mnv, torch_gpu):
    rng = np.random.default_rng(21)
    frame = ref.random_frame(rng, 37, 70)
    target8 = ref.pack(frame)
    flags = ref.QUANTISED | ref.SSIM
    want = ref.frame_metrics(frame, target8, flags)
    n_win = 60 * 27
    assert want[0].tolist() == [70 * 37, 0, n_win, 3 * n_win << 32, 0]      # num and den are the same float expression: s == 1 exactly
    check(mnv, torch_gpu, frame, target8, flags, want=want)
    sums, _, _ = run(mnv, torch_gpu, frame, target8, flags, maps=())
    v = mnv.metrics_finish(sums)
    assert v["mse"] == 0.0 and v["psnr"] == math.inf and v["ssim"] == 1.0 and (v["n_px"], v["n_win"]) == (70 * 37, n_win)
    # without QUANTISED the frame's own values are compared: not the same image
    assert check(mnv, torch_gpu, frame, target8, ref.SSIM)[0][1] > 0


def test_sums_are_per_call(mnv, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(31)
    a, b = ref.random_frame(rng, 19, 43), ref.random_frame(rng, 19, 43)
    target8 = rng.integers(0, 256, (19, 43, 4), dtype=np.uint8)
    sums = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    first, _, _ = run(mnv, torch, a, target8, ref.SSIM, maps=(), sums=sums)
    second, _, _ = run(mnv, torch, b, target8, ref.SSIM, maps=(), sums=sums)
    assert first.tolist() == ref.frame_metrics(a, target8, ref.SSIM)[0].tolist()
    assert second.tolist() == ref.frame_metrics(b, target8, ref.SSIM)[0].tolist() and first.tolist() != second.tolist()
    third, _, _ = run(mnv, torch, b, target8, 0, maps=(), sums=sums)         # ... and the SSIM words of an earlier call do not stay
    assert third.tolist() == [43 * 19, second[1], 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the renderer

W, H = 70, 37
POSE = ((-3.5, 0.0, 3.5), (-0.7071068, 0.0, 0.7071068), 60.0)
ORTHO = ((-1.35, 0.9, 2.25), (-0.45, 0.3, 0.75), 16.0)
PANORAMA = ((0.1, -0.2, 0.05), (0.6, 0.64, 0.48), 60.0)


@pytest.fixture(scope="module")
def tree(mnv, torch_gpu):
    return mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=77)


def _renderer(mnv, tree, in_flight=None, pose=POSE, **options):
    r = mnv.Renderer()
    r.resize(W, H)
    r.set(tree, tree.capacity)
    opt = mnv.RenderOptions.cli_defaults()
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    for k, v in options.items():
        setattr(r.options, k, v)
    r.set_camera(pose[0], pose[1], fx=pose[2])
    if in_flight is not None:
        r.set_frames_in_flight(in_flight)
    return r


def _move(r, pose, f):
    c, b, fx = pose
    a = np.deg2rad(11.0 * f)
    cs, sn = float(np.cos(a)), float(np.sin(a))
    rot = lambda v: (cs * v[0] - sn * v[1], sn * v[0] + cs * v[1], v[2])
    r.set_camera(rot(c), rot(b), fx=fx)


def _targets(torch, n, seed):
    rng = np.random.default_rng(seed)
    host = [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(n)]
    return host, [torch.from_numpy(t).cuda() for t in host]


def test_renderer_scores_three_frames_in_flight(mnv, torch_gpu, tree):
    flags = ref.SSIM | ref.MASK_ALPHA
    host, dev = _targets(torch_gpu, 3, 41)
    r, plain = _renderer(mnv, tree, in_flight=3), _renderer(mnv, tree, in_flight=3)
    slots = []
    for f in range(3):                              # three poses issued before anything is collected, each against its own target
        for x in (r, plain):
            _move(x, POSE, f)
        r.set_target(dev[f], flags)
        r.render()
        plain.render()
        slots.append(r.last_slot())
        assert plain.last_slot() == slots[-1]
    assert len(set(slots)) == 3
    frames = []
    for f, slot in enumerate(slots):
        got = r.metrics(slot)
        f32, u8 = r.download_slot(slot, want_rgba8=True)
        want = ref.finish(ref.frame_metrics(f32, host[f], flags)[0])
        assert got == want, (f, got, want)
        assert got["n_win"] > 0 and 0 < got["psnr"] < 30 and got["n_px"] == int((host[f][..., 3] != 0).sum())
        p32, p8 = plain.download_slot(slot, want_rgba8=True)
        assert f32.tobytes() == p32.tobytes() and u8.tobytes() == p8.tobytes()        # the frames do not know they are scored
        frames.append(f32)
    assert (frames[0][..., 3] > 0).mean() > 0.1 and frames[0].tobytes() != frames[1].tobytes()
    assert r.metrics() == r.metrics(slots[-1])
    with pytest.raises(mnv.MnvError) as e:
        plain.metrics()
    assert e.value.code == mnv.MNV_E_INVALID


@pytest.mark.parametrize("kind", ["antialiased", "ortho", "equirect", "grid", "mesh", "frame_inputs", "one_slot"])
def test_renderer_scores_every_frame_kind(mnv, torch_gpu, tree, kind):
    flags = ref.SSIM | ref.QUANTISED
    host, dev = _targets(torch_gpu, 1, 43)
    pose = ORTHO if kind == "ortho" else PANORAMA if kind == "equirect" else POSE
    vert = np.zeros((3, 9), np.float32)
    vert[:, :3] = [(-0.8, -0.8, 0.2), (0.9, -0.6, 0.1), (0.0, 0.9, -0.2)]
    vert[:, 3:6] = (0.9, 0.4, 0.1)
    vert[:, 8] = 1.0
    mesh = mnv.Mesh(vert, np.arange(3, dtype=np.uint32), 3) if kind == "mesh" else None
    depth = torch_gpu.full((H, W), 4.6, dtype=torch_gpu.float32, device="cuda")        # a depth image that cuts the volume

    def make():
        x = _renderer(mnv, tree, pose=pose, in_flight=1 if kind == "one_slot" else None, show_grid=kind == "grid")
        if kind == "antialiased":
            x.set_antialiasing(4)
        if kind == "ortho":
            x.set_projection(mnv.PROJ_ORTHO)
        if kind == "equirect":
            x.set_projection(mnv.PROJ_EQUIRECT)
        if kind == "mesh":
            x.add_mesh(mesh)
        if kind == "frame_inputs":
            x.set_frame_inputs(depth, None)
        return x

    r, plain = make(), make()
    r.set_target(dev[0], flags)
    for f in range(2):
        for x in (r, plain):
            _move(x, pose, f)
            x.render()
        got = r.metrics()
        f32, u8 = r.download(want_rgba8=True)
        want = ref.finish(ref.frame_metrics(f32, host[0], flags)[0])
        assert got == want, (kind, f, got, want)
        p32, p8 = plain.download(want_rgba8=True)
        assert f32.tobytes() == p32.tobytes() and u8.tobytes() == p8.tobytes()
        assert (f32[..., 3] > 0).mean() > 0.1
    if kind == "grid":
        assert r.wireframe()


def test_renderer_scores_refinement_and_guided_frames_on_slot_0(mnv, torch_gpu):
    """frames that sample through the networks and grow the tree run one at a time on slot 0's stream: scored there, unchanged"""
    from test_aa_gpu import _model
    flags = ref.SSIM | ref.QUANTISED | ref.MASK_ALPHA
    host, dev = _targets(torch_gpu, 1, 53)

    def make():
        own = mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=77)          # (refinement frames edit their tree)
        x = mnv.Renderer()
        x.resize(W, H)
        x.set(own, own.capacity + 2000)
        x.set_model(*_model(mnv, own.host_view()))
        x.set_seed(3)
        for k, v in dict(use_splitting=True, use_guided_sampling=True, max_depth=6, split_batch_size=64, samples_per_corner=2, max_sample_count=24,
                         max_guided_samples=24, background_brightness=0.0).items():
            setattr(x.options, k, v)
        x.set_camera(POSE[0], POSE[1], fx=POSE[2])
        return x

    r, plain = make(), make()
    r.set_target(dev[0], flags)
    voted = 0
    for f in range(3):
        st = r.render()
        assert plain.render() == st and r.last_slot() == 0
        voted += st["split_candidates"] + st["sample_candidates"]
        got = r.metrics(0)
        f32, u8 = r.download(want_rgba8=True)
        want = ref.finish(ref.frame_metrics(f32, host[0], flags)[0])
        assert got == want, (f, got, want)
        p32, p8 = plain.download(want_rgba8=True)
        assert f32.tobytes() == p32.tobytes() and u8.tobytes() == p8.tobytes()
    assert voted > 0 and st["guided_samples"] > 0                              # the frames did refine and did sample through the networks


def test_renderer_target_off_and_refusals(mnv, torch_gpu, tree):
    host, dev = _targets(torch_gpu, 1, 47)
    r = _renderer(mnv, tree)
    r.set_target(dev[0], ref.SSIM)
    r.render()
    assert r.metrics()["n_win"] == 60 * 27
    r.set_target(None)
    with pytest.raises(mnv.MnvError) as e:
        r.metrics()
    assert e.value.code == mnv.MNV_E_INVALID
    r.render()
    with pytest.raises(mnv.MnvError) as e:
        r.metrics()
    assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        r.set_target(dev[0], 8)
    assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        r.set_target(dev[0][:10], 0)
    assert e.value.code == mnv.MNV_E_INVALID
    # a resize drops a target of the old size
    r.set_target(dev[0], 0)
    r.resize(W // 2, H // 2)
    r.render()
    with pytest.raises(mnv.MnvError):
        r.metrics()
    # several ranks: refused in either order, and the renderer works on once the obstacle is gone
    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)
    r = _renderer(mnv, tree)
    try:
        r.set_ranks(comm)
        with pytest.raises(mnv.MnvError) as e:
            r.set_target(dev[0], 0)
        assert e.value.code == mnv.MNV_E_INVALID and "set_ranks" in str(e.value)
        r.set_ranks(None)
        r.set_target(dev[0], 0)
        with pytest.raises(mnv.MnvError) as e:
            r.set_ranks(comm)
        assert e.value.code == mnv.MNV_E_INVALID and "set_target" in str(e.value)
        r.render()
        assert r.metrics()["n_px"] == W * H
    finally:
        r.set_ranks(None)
        comm.close()


# ------------------------------------------------------------------------------------------------ the command line

def _ppm(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read().split(b"\n", 3)[3], np.uint8).reshape(H, W, 3)


def test_cli_scores_frames_against_written_files(mnv, torch_gpu, tree, tmp_path):
    npz = str(tmp_path / "t.npz")
    tree.save_npz(npz)
    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    common = [EXE, npz, "-w", str(W), "-h", str(H), "--fx", "60", "--frames", "2", "--orbit", "10"]
    p = subprocess.run(common + ["--out", a], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    first = [_ppm(f"{a}_{f:04d}.ppm").copy() for f in range(2)]
    assert first[0].tobytes() != first[1].tobytes() and first[0].any()
    p = subprocess.run(common + ["--out", a, "--target", a, "--ssim"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for f in range(2):
        assert f"frame {f}: psnr inf ssim 1.000000\n" in p.stdout, p.stdout
        assert _ppm(f"{a}_{f:04d}.ppm").tobytes() == first[f].tobytes()
    assert "mean over 2 frame(s): psnr inf ssim 1.000000\n" in p.stdout
    # another background: the score of the two written files
    p = subprocess.run(common + ["--out", b, "--bg", "0.5", "--target", a, "--ssim"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    alpha = np.full((H, W, 1), 255, np.uint8)
    for f in range(2):
        written = np.concatenate([_ppm(f"{b}_{f:04d}.ppm").astype(np.float32) / np.float32(255), np.ones((H, W, 1), np.float32)], axis=2)
        want = ref.finish(ref.frame_metrics(written, np.concatenate([first[f], alpha], axis=2), ref.SSIM)[0])
        assert math.isfinite(want["psnr"]) and want["psnr"] < 40
        assert f"frame {f}: psnr {want['psnr']:.4f} ssim {want['ssim']:.6f}\n" in p.stdout, (p.stdout, want)
    # a mask file: the left half excluded; without --ssim only the PSNR is printed
    mask = np.zeros((H, W), np.uint8)
    mask[:, W // 2:] = 9
    for f in range(2):
        with open(f"{a}_{f:04d}.pgm", "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H) + mask.tobytes())
    p = subprocess.run(common + ["--bg", "0.5", "--target", a, "--target_mask", a], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for f in range(2):
        written = np.concatenate([_ppm(f"{b}_{f:04d}.ppm").astype(np.float32) / np.float32(255), np.ones((H, W, 1), np.float32)], axis=2)
        want = ref.finish(ref.frame_metrics(written, np.concatenate([first[f], mask[..., None]], axis=2), ref.MASK_ALPHA)[0])
        assert want["n_px"] == H * (W - W // 2)
        assert re.search(rf"^frame {f}: psnr {want['psnr']:.4f}$", p.stdout, re.M), (p.stdout, want)
    # refused, with a message, before anything is rendered
    for extra, word in ((["--target", a, "--gpus", "1"], "--gpus"), (["--ssim"], "--target"), (["--target_mask", a], "--target")):
        p = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and word in p.stderr, extra
    p = subprocess.run(common[:2] + ["-w", str(W + 1), "-h", str(H), "--target", a], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "expected" in p.stderr
