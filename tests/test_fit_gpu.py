"""Fitting on the device (csrc/mnv_fit.hip: mnv_rays_grad, mnv_rows_master_init, mnv_rows_sgd_step; N3Tree.fit / fit_to) against the numpy
restatement of the contract (tests/fit_ref.py): the forward of mnv_rays_grad is mnv_render_rays_accel's bit for bit; the accumulator words
and the sums equal the restatement word for word -- with a basis mask, rotated view directions, ray limits and excluded rays -- in any ray
order and image layout and under full contention; both row kernels are exact; fit_to reproduces the restatement's loss sequence and rows;
the loss falls at every step; refusals come before any launch.  The edge cases: SH16 / SH25 rows (the whole wavefront per sample, a second
trip over the columns), scales that differ per axis, skipped rays with the clamp and NaN terms, links that leave the tree, padded rows with
eight lanes per sample, more tiles than workgroups, ragged tiles.  The descent's limit of 23 levels is reached by no test: no ray list was
found for which the restatement reports a ray broken by it.  No tolerance anywhere."""
import numpy as np
import pytest

import cases
import fit_cases
import fit_ref
import rays_ref

pytestmark = pytest.mark.gpu
bits = cases.bits


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grad(mnv, torch, tree, opt, o, d, target, tmax=None, acc=None, want_rgba=True):
    """mnv_rays_grad on host arrays -> (rgba or None, acc int64 [capacity * 8, data_dim], sums dict); acc: a device tensor to add into"""
    v = tree if isinstance(tree, mnv.TreeView) else tree.device_view()
    n = int(np.prod(o.shape[:-1]))
    if acc is None:
        acc = torch.zeros((v.capacity * 8, v.data_dim), dtype=torch.int64, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    rgba = torch.full(o.shape[:-1] + (4,), float("nan"), dtype=torch.float32, device="cuda") if want_rgba else None
    mnv.rays_grad(v, _dev(torch, o), _dev(torch, d), _dev(torch, target), opt, acc, sums, rgba=rgba, tmax=_dev(torch, tmax))
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    assert not s[5:].any()
    return (None if rgba is None else rgba.cpu().numpy().reshape(n, 4)), acc.cpu().numpy(), dict(zip(fit_ref.FIT_SUMS, (int(x) for x in s[:5])))


@pytest.fixture(scope="module")
def truth(mnv):
    """per case: the tree on the device, options, rays and the restatement's answer -- computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            tree = cases.make_tree(mnv, fit_cases.tree_spec(name))
            T = fit_ref.tree_of(mnv, tree)
            opt = fit_cases.make_options(mnv, name)
            L = fit_cases.ray_list(mnv, name)
            rgba, acc, sums, fw = fit_ref.rays_grad(T, opt, L["o"], L["d"], L["target"], L["tmax"])
            tree.move_to_device()
            cache[name] = dict(tree=tree, T=T, opt=opt, L=L, rgba=rgba, acc=acc, sums=sums, fw=fw)
        return cache[name]

    return get


@pytest.mark.parametrize("name", fit_cases.NAMES)
def test_words_sums_and_pixels_equal_the_restatement(mnv, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    L = t["L"]
    rgba, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], L["o"], L["d"], L["target"], L["tmax"])
    # the forward is the ray march's, bit for bit, degenerate rays and misses included
    want = torch.full((L["o"].shape[0], 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_rays_accel(t["tree"].accel, _dev(torch, L["o"]), _dev(torch, L["d"]), t["opt"], rgba=want, tmax=_dev(torch, L["tmax"]))
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    assert not np.isnan(want).any()
    assert np.array_equal(bits(rgba), bits(want)), f"{int((bits(rgba) != bits(want)).any(axis=1).sum())} rays differ from mnv_render_rays_accel"
    assert np.array_equal(bits(rgba), bits(t["rgba"]))
    assert sums == t["sums"]
    assert t["sums"]["n_samples"] > 0 and np.count_nonzero(t["acc"]) > 0
    bad = acc != t["acc"]
    assert not bad.any(), f"{int(bad.sum())} of {int((t['acc'] != 0).sum())} non-zero words differ; first at {np.argwhere(bad)[:3].tolist()}"


@pytest.mark.parametrize("name", ["sh9_d4", "rgba_d1"])
def test_ray_order_and_layout_do_not_change_a_word(mnv, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    L = t["L"]
    perm = np.random.default_rng(5).permutation(L["o"].shape[0])
    _, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], L["o"][perm], L["d"][perm], L["target"][perm], L["tmax"][perm], want_rgba=False)
    assert np.array_equal(acc, t["acc"]) and sums == t["sums"]
    # the same rays as a 20 x 32 image: 8 x 8 ray tiles instead of 64 x 1
    rgba, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], L["o"].reshape(20, 32, 3), L["d"].reshape(20, 32, 3), L["target"].reshape(20, 32, 4),
                            L["tmax"].reshape(20, 32))
    assert np.array_equal(acc, t["acc"]) and sums == t["sums"] and np.array_equal(bits(rgba), bits(t["rgba"]))
    # two calls into one accumulator add up
    v = t["tree"].device_view()
    both = torch.zeros((v.capacity * 8, v.data_dim), dtype=torch.int64, device="cuda")
    h = 300
    _grad(mnv, torch, t["tree"], t["opt"], L["o"][:h], L["d"][:h], L["target"][:h], L["tmax"][:h], acc=both, want_rgba=False)
    _, acc, _ = _grad(mnv, torch, t["tree"], t["opt"], L["o"][h:], L["d"][h:], L["target"][h:], L["tmax"][h:], acc=both, want_rgba=False)
    assert np.array_equal(acc, t["acc"])


def test_full_contention_on_a_depth_one_tree(mnv, torch_gpu, truth):
    """4096 rays of a 64 x 64 frame into the eight voxels of the root chunk"""
    torch = torch_gpu
    t = truth("sh1_d1")
    o, d = rays_ref.pinhole_rays(fit_cases.frame_camera(mnv, 64, 1).c)
    target = np.random.default_rng(9).uniform(0, 1, size=(64, 64, 4)).astype(np.float32)
    target[..., 3] = 1.0
    _, want, want_sums, fw = fit_ref.rays_grad(t["T"], t["opt"], o, d, target)
    assert np.bincount(np.concatenate([b["vox"] for b in fw["batches"]])).max() >= 1000
    _, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], o, d, target, want_rgba=False)
    assert np.array_equal(acc, want) and sums == want_sums


# ---- the edge cases (fit_cases.EDGE_NAMES and the inputs built next to them): wide rows, scales that differ per axis, skipped rays, links
# that leave the tree, padded rows, more tiles than workgroups, ragged tiles.  tests/test_fit_ref.py says what each input contains.

@pytest.mark.parametrize("name", fit_cases.EDGE_NAMES)
def test_edge_cases_equal_the_restatement_word_for_word(mnv, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    L = t["L"]
    rgba, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], L["o"], L["d"], L["target"], L["tmax"])
    want = torch.full((L["o"].shape[0], 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_rays_accel(t["tree"].accel, _dev(torch, L["o"]), _dev(torch, L["d"]), t["opt"], rgba=want, tmax=_dev(torch, L["tmax"]))
    torch.cuda.synchronize()
    assert np.array_equal(bits(rgba), bits(want.cpu().numpy())) and np.array_equal(bits(rgba), bits(t["rgba"]))
    assert sums == t["sums"] and t["sums"]["n_samples"] >= 500
    bad = acc != t["acc"]
    assert not bad.any(), f"{int(bad.sum())} of {int((t['acc'] != 0).sum())} non-zero words differ; first at {np.argwhere(bad)[:3].tolist()}"
    # the same rays as a 20 x 32 image
    rgba, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], L["o"].reshape(20, 32, 3), L["d"].reshape(20, 32, 3), L["target"].reshape(20, 32, 4),
                            L["tmax"].reshape(20, 32))
    assert np.array_equal(acc, t["acc"]) and sums == t["sums"] and np.array_equal(bits(rgba), bits(t["rgba"]))


@pytest.mark.parametrize("name", ["sh4_d4_aniso", "sh25_d3"])
def test_skipped_rays_the_clamp_and_nan_terms(mnv, torch_gpu, truth, name):
    """targets far outside [0, 1], infinite and NaN (fit_cases.skip_targets): rays with a non-finite g are skipped and still get their
    pixel, terms beyond +-32 saturate, NaN terms read 0"""
    t = truth(name)
    L = t["L"]
    tg = fit_cases.skip_targets(L["target"])
    want, want_sums = fit_ref.backward(t["T"], t["opt"], t["fw"], tg)
    assert want_sums["n_skipped"] >= 10 and (np.abs(want) >= 2 ** 37).any()
    rgba, acc, sums = _grad(mnv, torch_gpu, t["tree"], t["opt"], L["o"], L["d"], tg, L["tmax"])
    assert sums == want_sums
    bad = acc != want
    assert not bad.any(), f"{int(bad.sum())} words differ; first at {np.argwhere(bad)[:3].tolist()}"
    assert np.array_equal(bits(rgba), bits(t["rgba"]))


def test_nan_terms_read_zero(mnv, torch_gpu, truth):
    """fit_cases.nan_terms: RGBA rows with colours up to 64 against targets of +-3e38: g is finite, products overflow to infinities of
    opposite sign, the density term is NaN and adds nothing (tests/test_fit_ref.py counts the NaN terms of this input)"""
    torch = torch_gpu
    t = truth("rgba_d4")
    L = t["L"]
    U, tg = fit_cases.nan_terms(t["T"], L["target"])
    want_rgba, want, want_sums, _ = fit_ref.rays_grad(U, t["opt"], L["o"], L["d"], tg, L["tmax"])
    assert want_sums["n_skipped"] == 0 and (np.abs(want) >= 2 ** 37).any()
    v, data_t, child_t = fit_cases.hand_view(mnv, torch, U)
    rgba, acc, sums = _grad(mnv, torch, v, t["opt"], L["o"], L["d"], tg, L["tmax"])
    assert sums == want_sums and np.array_equal(acc, want) and np.array_equal(bits(rgba), bits(want_rgba))


def test_links_that_leave_the_tree_skip_their_rays(mnv, torch_gpu, truth):
    """fit_cases.broken_links: links to chunk 0, to chunks at and above the view's capacity (all inside the allocated arrays): the rays
    that meet one are skipped, the others' words are the restatement's"""
    torch = torch_gpu
    t = truth(fit_cases.BROKEN["tree"])
    T, L = fit_cases.broken_links(t["T"], t["L"])
    want_rgba, want, want_sums, fw = fit_ref.rays_grad(T, t["opt"], L["o"], L["d"], L["target"], L["tmax"])
    assert want_sums["n_skipped"] >= 20 and want.shape[0] == fit_cases.BROKEN["capacity"] * 8
    v, data_t, child_t = fit_cases.hand_view(mnv, torch, T)
    assert v.capacity == fit_cases.BROKEN["capacity"] and child_t.numel() == t["T"]["capacity"] * 8 > v.capacity * 8
    acc = torch.zeros((child_t.numel(), T["data_dim"]), dtype=torch.int64, device="cuda")       # rows for every allocated chunk
    rgba, acc, sums = _grad(mnv, torch, v, t["opt"], L["o"], L["d"], L["target"], L["tmax"], acc=acc)
    assert sums == want_sums
    assert np.array_equal(acc[:want.shape[0]], want) and not acc[want.shape[0]:].any()
    assert np.array_equal(bits(rgba), bits(want_rgba))


def test_padded_rows_and_the_scatter_group_of_eight(mnv, torch_gpu, truth):
    """SH1 rows of data_dim 7 (fit_cases.padded_rows): eight lanes per sample, the padding columns 3 .. 5 get no word; then a step on them"""
    torch = torch_gpu
    t = truth("sh1_d4")
    L = t["L"]
    P = fit_cases.padded_rows(t["T"])
    want_rgba, want, want_sums, _ = fit_ref.rays_grad(P, t["opt"], L["o"], L["d"], L["target"], L["tmax"])
    v, data_t, child_t = fit_cases.hand_view(mnv, torch, P)
    acc_t = torch.zeros((P["capacity"] * 8, 7), dtype=torch.int64, device="cuda")
    rgba, acc, sums = _grad(mnv, torch, v, t["opt"], L["o"], L["d"], L["target"], L["tmax"], acc=acc_t)
    assert sums == want_sums and np.array_equal(acc, want) and np.array_equal(bits(rgba), bits(want_rgba))
    assert not acc[:, 3:6].any() and acc[:, :3].any() and acc[:, 6].any()
    master = mnv.rows_master_init(data_t)
    mnv.rows_sgd_step(data_t, master, acc_t, 7, 1.0, 20.0)
    torch.cuda.synchronize()
    want_d, want_m, want_a = P["data"].copy(), fit_ref.master_init(P["data"]), want.copy()
    fit_ref.sgd_step(want_d, want_m, want_a, 1.0, 20.0)
    got_d = data_t.cpu().numpy().view(np.uint16)
    assert np.array_equal(got_d, want_d) and np.array_equal(bits(master.cpu().numpy()), bits(want_m)) and not acc_t.cpu().numpy().any()
    # rows change only where acc had words: the rewrite of a touched row's other columns is binary16(master), the finite value it held
    changed = got_d != P["data"]
    assert changed.any() and not changed[want == 0].any() and not changed[:, 3:6].any()


@pytest.mark.parametrize("name", ["sh9_d4", "sh25_d3"])
def test_more_tiles_than_workgroups(mnv, torch_gpu, truth, name):
    """420 copies of the case's 640 rays and its first 37 again: 268,837 rays in 4201 flat tiles, more than the 4096 workgroups of the
    launch, so workgroups walk on to a second tile, the last of which has 37 rays; and the 268,800 as a 32 x 8400 image (4 x 1050 = 4200
    tiles of 8 x 8).  The words are integers: 420 x the restatement's words of the list plus those of its first 37 rays, whatever
    workgroup adds them.  Headroom: the busiest word takes fewer than 640 x 420 = 2.7e5 terms of at most 2^37 each, far below 2^62; the
    ray count is below the call's limit of 2^22."""
    torch = torch_gpu
    t = truth(name)
    L = t["L"]
    copies, tail = 420, 37
    many = {k: np.concatenate([np.tile(a, (copies,) + (1,) * (a.ndim - 1)), a[:tail]]) for k, a in L.items()}
    assert many["o"].shape[0] == 268837 and (268837 + 63) // 64 == 4201
    _, acc_tail, sums_tail, _ = fit_ref.rays_grad(t["T"], t["opt"], L["o"][:tail], L["d"][:tail], L["target"][:tail], L["tmax"][:tail])
    assert sums_tail["n_samples"] > 0 and sums_tail["n_rays"] < tail
    rgba, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], many["o"], many["d"], many["target"], many["tmax"])
    assert sums == {k: copies * t["sums"][k] + sums_tail[k] for k in sums}
    assert np.array_equal(acc, copies * t["acc"] + acc_tail)
    assert np.array_equal(bits(rgba), bits(np.concatenate([np.tile(t["rgba"], (copies, 1)), t["rgba"][:tail]])))
    n = copies * 640
    rgba, acc, sums = _grad(mnv, torch, t["tree"], t["opt"], many["o"][:n].reshape(8400, 32, 3), many["d"][:n].reshape(8400, 32, 3),
                            many["target"][:n].reshape(8400, 32, 4), many["tmax"][:n].reshape(8400, 32))
    assert sums == {k: copies * x for k, x in t["sums"].items()} and np.array_equal(acc, copies * t["acc"])
    assert np.array_equal(bits(rgba), bits(np.tile(t["rgba"], (copies, 1))))


@pytest.mark.parametrize("shape", [(13, 7), (7, 13), (65,)], ids=["7x13", "13x7", "flat65"])
def test_ragged_tiles_write_nothing_beside_their_rays(mnv, torch_gpu, truth, shape):
    """images narrower than a tile and of no multiple of 8 (7 wide x 13 high, 13 x 7), a flat list that ends one ray into its second tile:
    the restatement's words on top of what acc held, pixels for the listed rays and not one float behind them"""
    torch = torch_gpu
    t = truth("sh9_d4")
    n = int(np.prod(shape))
    L = {k: a[:n] for k, a in t["L"].items()}
    want_rgba, want, want_sums, _ = fit_ref.rays_grad(t["T"], t["opt"], L["o"], L["d"], L["target"], L["tmax"])
    assert want_sums["n_samples"] >= 20 and np.count_nonzero(want) >= 20
    v = t["tree"].device_view()
    before = np.random.default_rng(n).integers(-(1 << 40), 1 << 40, size=want.shape)
    acc = _dev(torch, before)
    guard = shape[-1]                                                                  # one more row of pixels
    rgba = torch.full((n + guard, 4), float("nan"), dtype=torch.float32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    o, d, tg = (_dev(torch, L[k].reshape(shape + (c,))) for k, c in (("o", 3), ("d", 3), ("target", 4)))
    mnv.rays_grad(v, o, d, tg, t["opt"], acc, sums, rgba=rgba, tmax=_dev(torch, L["tmax"].reshape(shape)))
    torch.cuda.synchronize()
    got, nan = rgba.cpu().numpy(), torch.full((guard, 4), float("nan"), dtype=torch.float32).numpy()
    assert np.array_equal(bits(got[:n]), bits(want_rgba)) and np.array_equal(bits(got[n:]), bits(nan))
    assert dict(zip(fit_ref.FIT_SUMS, sums.cpu().numpy()[:5].tolist())) == want_sums and not sums.cpu().numpy()[5:].any()
    got_acc = acc.cpu().numpy()
    assert np.array_equal(got_acc - before, want)
    assert np.array_equal(got_acc[~want.any(axis=1)], before[~want.any(axis=1)])        # rows of voxels no ray reached keep their words


def test_row_kernels_are_exact(mnv, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(11)
    n_rows, dd = 1500, 13
    data = rng.integers(0, 1 << 16, size=(n_rows, dd), dtype=np.uint16)           # every kind of bit pattern, NaN and inf among them
    data[:64] = np.arange(64 * dd, dtype=np.uint16).reshape(64, dd) * 77
    data[0, :6] = [0x7C00, 0xFC00, 0x7E00, 0x7BFF, 0xFBFF, 0x0001]
    d_dev = _dev(torch, data.view(np.int16))
    master = mnv.rows_master_init(d_dev)
    torch.cuda.synchronize()
    want_m = fit_ref.master_init(data)
    assert np.array_equal(bits(master.cpu().numpy()), bits(want_m))
    acc = np.zeros((n_rows, dd), np.int64)
    rows = rng.uniform(size=n_rows) < 0.4
    acc[rows] = (rng.normal(size=(int(rows.sum()), dd)) * 10.0 ** rng.uniform(-6, 3, size=(int(rows.sum()), dd)) * fit_ref.Q32).astype(np.int64)
    acc[rows & (rng.uniform(size=n_rows) < 0.5), ::2] = 0                          # rows with some zero words
    acc[0] = [-(1 << 62), 1 << 62, 1, -1, 1 << 55, 0, 0, 0, 0, 0, 0, 0, 1 << 40]     # saturation both ways; a density that would go negative
    a_dev = _dev(torch, acc)
    mnv.rows_sgd_step(d_dev, master, a_dev, dd, 0.75, 3.0)
    torch.cuda.synchronize()
    want_d = data.copy()
    want_a = acc.copy()
    fit_ref.sgd_step(want_d, want_m, want_a, 0.75, 3.0)
    got_d = d_dev.cpu().numpy().view(np.uint16)
    assert np.array_equal(got_d, want_d) and np.array_equal(bits(master.cpu().numpy()), bits(want_m))
    assert not a_dev.cpu().numpy().any()
    assert np.array_equal(got_d[~acc.any(axis=1)], data[~acc.any(axis=1)])          # untouched rows keep their bytes, non-finite ones too
    assert not ((got_d & 0x7C00) == 0x7C00)[acc.any(axis=1)].any()                  # no infinity or NaN is ever written
    assert (want_d != data).any()


@pytest.fixture(scope="module")
def fit_scene(mnv, torch_gpu):
    """the teacher on the device, its cut, the cameras, the teacher's frames (the accel march) and the options"""
    F = fit_cases.FIT
    teacher = cases.make_tree(mnv, fit_cases.TREES[F["tree"]])
    teacher.move_to_device()
    opt = mnv.RenderOptions.defaults()
    cams = fit_cases.fit_cameras(mnv)
    frames = []
    for c in cams:
        out = torch_gpu.full((c.height, c.width, 4), float("nan"), dtype=torch_gpu.float32, device="cuda")
        mnv.render_voxels_accel(teacher.accel, c, opt, rgba=out)
        frames.append(out)
    torch_gpu.cuda.synchronize()
    return dict(teacher=teacher, opt=opt, cams=cams, frames=frames)


def test_fit_to_reproduces_the_restatement(mnv, torch_gpu, fit_scene):
    F, s = fit_cases.FIT, fit_scene
    lod = s["teacher"].make_lod(F["cut"])
    T = fit_ref.tree_of(mnv, lod)
    before = T["data"].copy()
    rays = [tuple(a.reshape(-1, 3) for a in rays_ref.pinhole_rays(c.c)) for c in s["cams"]]
    targets = [f.cpu().numpy().reshape(-1, 4) for f in s["frames"]]
    want_se = fit_ref.fit(T, s["opt"], rays, targets, 2, F["lr_colour"], F["lr_sigma"])
    se = lod.fit_to(s["teacher"], s["cams"], s["opt"], 2, F["lr_colour"], F["lr_sigma"])
    assert se.tolist() == want_se and want_se[1] < want_se[0]
    got = np.array(lod.host_arrays()[0]).reshape(-1, T["data_dim"])                # the host copy was refreshed
    assert np.array_equal(got, T["data"]) and (got != before).any()
    # ... and so was the accel: the frame of the fitted tree through it is the frame of its rows
    c = s["cams"][0]
    out = torch_gpu.full((c.height, c.width, 4), float("nan"), dtype=torch_gpu.float32, device="cuda")
    mnv.render_voxels_accel(lod.accel, c, s["opt"], rgba=out)
    torch_gpu.cuda.synchronize()
    want = fit_ref.forward(T, s["opt"], *rays[0])["rgba"]
    assert np.array_equal(bits(out.cpu().numpy().reshape(-1, 4)), bits(want))
    # fit with the frames handed over is the same thing
    lod2 = s["teacher"].make_lod(F["cut"])
    se2 = lod2.fit(s["cams"], s["frames"], s["opt"], 2, F["lr_colour"], F["lr_sigma"])
    assert se2.tolist() == want_se and np.array_equal(np.array(lod2.host_arrays()[0]).reshape(-1, T["data_dim"]), T["data"])


def test_the_loss_falls_at_every_step(mnv, torch_gpu, fit_scene):
    F, s = fit_cases.FIT, fit_scene
    lod = s["teacher"].make_lod(F["cut"])
    se = lod.fit_to(s["teacher"], s["cams"], s["opt"], F["iterations"], F["lr_colour"], F["lr_sigma"]).tolist()
    assert len(se) == F["iterations"] and all(b < a for a, b in zip(se, se[1:])), se
    assert se[-1] < 0.9 * se[0]


def test_refusals_come_before_any_launch(mnv, torch_gpu, truth):
    torch = torch_gpu
    t = truth("sh4_d4")
    L = t["L"]
    v = t["tree"].device_view()
    o, d, tg = _dev(torch, L["o"]), _dev(torch, L["d"]), _dev(torch, L["target"])
    acc = torch.zeros((v.capacity * 8, v.data_dim), dtype=torch.int64, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    fn = mnv.lib().mnv_rays_grad
    n = L["o"].shape[0]
    import ctypes as C

    def call(view=v, opt=t["opt"], width=n, height=1, acc_p=acc.data_ptr(), tg_p=tg.data_ptr()):
        return fn(C.byref(view), o.data_ptr(), d.data_ptr(), tg_p, None, width, height, C.byref(opt), None, acc_p, sums.data_ptr(), None)

    def changed(obj, **kw):
        c = type(obj)()
        C.memmove(C.byref(c), C.byref(obj), C.sizeof(c))
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    assert call(opt=changed(t["opt"], render_depth=True)) == mnv.MNV_E_UNSUPPORTED
    assert call(view=changed(v, N=3)) == mnv.MNV_E_UNSUPPORTED
    assert call(view=changed(v, basis_dim=2)) == mnv.MNV_E_UNSUPPORTED
    assert call(view=changed(v, basis_dim=9)) == mnv.MNV_E_INVALID                 # data_dim 13 cannot hold SH9 rows
    for step in (0.0, -1e-4, float("nan"), float("inf")):
        assert call(opt=changed(t["opt"], step_size=step)) == mnv.MNV_E_INVALID, step
    assert b"step_size" in mnv.lib().mnv_last_error()
    assert call(width=(1 << 22) + 1) == mnv.MNV_E_INVALID and call(width=2049, height=2048) == mnv.MNV_E_INVALID
    assert call(width=0) == mnv.MNV_E_INVALID and call(acc_p=None) == mnv.MNV_E_INVALID and call(tg_p=tg.data_ptr() + 4) == mnv.MNV_E_INVALID
    assert call(view=changed(v, capacity=0)) == mnv.MNV_E_INVALID
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any() and not sums.cpu().numpy().any()             # nothing ran
    lib = mnv.lib()
    assert lib.mnv_rows_master_init(None, 4, None, None) == mnv.MNV_E_INVALID
    assert lib.mnv_rows_sgd_step(None, None, None, 4, 4, 1.0, 1.0, None) == mnv.MNV_E_INVALID
    assert lib.mnv_rows_sgd_step(acc.data_ptr(), acc.data_ptr(), acc.data_ptr(), 4, 4, float("nan"), 1.0, None) == mnv.MNV_E_INVALID
    lod = t["tree"]
    with pytest.raises(mnv.MnvError) as e:
        frame = torch.zeros((fit_cases.FRAME, fit_cases.FRAME, 4), dtype=torch.float32, device="cuda")
        cases.make_tree(mnv, fit_cases.TREES["sh1_d1"]).fit([fit_cases.frame_camera(mnv)], [frame], t["opt"], 1, 1.0, 1.0)   # not on the device
    assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        lod.fit_to(lod, [fit_cases.frame_camera(mnv)], t["opt"], 1, 1.0, 1.0)      # its own teacher
    assert e.value.code == mnv.MNV_E_INVALID


def test_mnv_render_lod_fit_and_save_lod(mnv, torch_gpu, tmp_path):
    """mnv_render --lod D --lod_fit N --save_lod: the written tree is the cut fitted by N3Tree.fit_to at the run's pose, it reloads, and the
    frame the run wrote is the frame of that tree (the renderer fitted its own cut: VolumeRenderer::set_lod_fit)"""
    import os
    import subprocess

    torch = torch_gpu
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mega-nerf-viewer_amd", "mnv_render")
    assert os.path.exists(exe), "mnv_render not built"
    F = fit_cases.FIT
    tree = cases.make_tree(mnv, fit_cases.TREES[F["tree"]])
    npz, saved, out = str(tmp_path / "scene.npz"), str(tmp_path / "fitted.npz"), str(tmp_path / "frame")
    tree.save_npz(npz)
    center, back, size = (-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48), 16
    common = [exe, npz, "-w", str(size), "-h", str(size), "--fx", "20", "--center", ",".join(map(str, center)), "--back", ",".join(map(str, back))]
    r = subprocess.run(common + ["--out", out, "--raw", "--frames", "1", "--lod", str(F["cut"]), "--lod_fit", "2", "--save_lod", saved],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lod_fit:" in r.stdout, r.stderr + r.stdout
    tree.move_to_device()
    cut = tree.make_lod(F["cut"])
    plain = np.array(cut.host_arrays()[0])
    cam = mnv.Camera(size, size, 20.0).set_pose(center, back)
    opt = mnv.RenderOptions.cli_defaults()
    se = cut.fit_to(tree, [cam], opt, 2, 1.0, 20.0)           # (the program's default learning rates)
    assert se[1] < se[0]
    back_in = mnv.N3Tree.open(saved)
    for x, y in zip(back_in.host_arrays(), cut.host_arrays()):
        assert np.array_equal(x, y)
    assert (np.array(back_in.host_arrays()[0]) != plain).any()
    back_in.move_to_device()
    want = torch.full((size, size, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(back_in.accel, cam, opt, rgba=want)
    torch.cuda.synchronize()
    got = np.fromfile(out + "_0000.f32", dtype=np.float32).reshape(size, size, 4)
    assert np.array_equal(bits(got), bits(want.cpu().numpy()))
    bad = subprocess.run(common + ["--lod_fit", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--lod_fit" in bad.stderr
    bad = subprocess.run(common + ["--lod", "3", "--fit_lr_sigma", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--lod_fit" in bad.stderr
