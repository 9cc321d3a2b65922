"""Fitting on a photo set on the device (csrc/mnv_fit_batch.hip: mnv_rows_adam_step, mnv_ray_batcher_*; N3Tree.fit_ex / fit_to_ex) against
the numpy restatement (tests/fit_adam_ref.py), bit for bit: the Adam row kernel on random bit patterns and special values for every row
width and tile boundary; the batcher's draws against mnv_generate_rays' own device output, with guard words, on several streams and
handles; mnv_rays_grad on a drawn batch; the batched Adam loop against the restated loop, rows, sums and the rebuilt accel; SGD with full
batch through the new loop against mnv_n3tree_fit; refusals before any launch.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import cases
import fit_adam_ref as far
import fit_cases
import fit_ref

pytestmark = pytest.mark.gpu
bits = cases.bits
F = np.float32
QNAN = np.uint32(0x7FC00000)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fbits(a):
    """binary32 bit patterns with every NaN read as one (the payload of a NaN that arithmetic made is not part of the contract)"""
    a = np.asarray(a, F)
    return np.where(np.isnan(a), QNAN, a.view(np.uint32))


# ---- the Adam row kernel ------------------------------------------------------------------------------------------------------------------
def _adam_inputs(rng, n_rows, dd):
    def finite_bits(shape):
        b = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        b[(b & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)            # no inf / NaN in the state: exponent 255 -> 127 .. 254
        return b

    data = rng.integers(0, 1 << 16, size=(n_rows, dd), dtype=np.uint16)
    master = finite_bits((n_rows, dd)).view(F)
    m1 = finite_bits((n_rows, dd)).view(F)
    m2 = (finite_bits((n_rows, dd)) & np.uint32(0x7FFFFFFF)).view(F)          # a second moment is never negative
    # half of the state in the range a fit produces
    usual = rng.uniform(size=(n_rows, dd)) < 0.5
    master[usual] = (rng.normal(size=int(usual.sum())) * 10.0 ** rng.uniform(-3, 2, size=int(usual.sum()))).astype(F)
    m1[usual] = (rng.normal(size=int(usual.sum())) * 10.0 ** rng.uniform(-6, 1, size=int(usual.sum()))).astype(F)
    m2[usual] = (rng.normal(size=int(usual.sum())) ** 2 * 10.0 ** rng.uniform(-12, 2, size=int(usual.sum()))).astype(F)
    acc = np.zeros((n_rows, dd), np.int64)
    rows = rng.uniform(size=n_rows) < 0.6                                      # untouched rows between touched ones
    k = int(rows.sum())
    acc[rows] = (rng.normal(size=(k, dd)) * 10.0 ** rng.uniform(-9, 3, size=(k, dd)) * far.Q32).astype(np.int64)
    acc[rows & (rng.uniform(size=n_rows) < 0.5), ::2] = 0                      # rows with some zero words
    # row 0: special values, repeated over the width
    sp_acc = [1, -1, 0, 0, 1 << 62, -(1 << 62), 1 << 32, 0]
    sp_m = [0.0, -0.0, 1e-40, 5.0, 65504.0, -65504.0, 1e5, -1e5]               # +-0, a subnormal, masters at +-65504 and beyond
    sp_m1 = [0.0, -0.0, 1e-42, 1e-3, -2.0, 1e-39, 0.0, 3.0]
    sp_m2 = [0.0, 1e-44, 0.0, 0.0, 3e38, 1e30, 1e-45, 0.0]                     # v = 0: den is eps alone; a large m2: v c2 overflows
    for c in range(dd):
        acc[0, c], master[0, c], m1[0, c], m2[0, c] = sp_acc[c % 8], sp_m[c % 8], sp_m1[c % 8], sp_m2[c % 8]
    acc[0, 0] = 1                                                              # (row 0 is touched whatever its width)
    return data, master, m1, m2, acc


@pytest.mark.parametrize("dd", [4, 13, 28, 49, 76])
def test_adam_row_kernel_is_exact(mnv, torch_gpu, dd):
    torch = torch_gpu
    rng = np.random.default_rng(300 + dd)
    moved = 0
    for n_rows in (1, 255, 256, 257, 1000):
        for step in (1, 2, 1000):
            data, master, m1, m2, acc = _adam_inputs(rng, n_rows, dd)
            d_dev, m_dev, m1_dev, m2_dev, a_dev = _dev(torch, data.view(np.int16)), _dev(torch, master), _dev(torch, m1), _dev(torch, m2), _dev(torch, acc)
            mnv.rows_adam_step(d_dev, m_dev, m1_dev, m2_dev, a_dev, dd, step, 0.03, 1.0)
            torch.cuda.synchronize()
            want = [data.copy(), master.copy(), m1.copy(), m2.copy(), acc.copy()]
            far.adam_step(*want, step, 0.03, 1.0)
            got_d = d_dev.cpu().numpy().view(np.uint16)
            where = (n_rows, step)
            assert np.array_equal(got_d, want[0]), where
            for got, w in zip((m_dev, m1_dev, m2_dev), want[1:4]):
                assert np.array_equal(_fbits(got.cpu().numpy()), _fbits(w)), where
            assert not a_dev.cpu().numpy().any(), where
            untouched = ~acc.any(axis=1)
            assert np.array_equal(got_d[untouched], data[untouched]) and np.array_equal(bits(m_dev.cpu().numpy()[untouched]), bits(master[untouched]))
            assert np.array_equal(bits(m1_dev.cpu().numpy()[untouched]), bits(m1[untouched]))
            assert not ((got_d & 0x7C00) == 0x7C00)[~untouched].any()                  # no infinity or NaN is ever written to the rows
            moved += int((want[0] != data).sum())
    assert moved > 1000


# ---- the batcher ----------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _draw_guarded(mnv, torch, batcher, epoch, first, count, stream=0, offset=0):
    """a draw into outputs with GUARD sentinel words behind them (offset: floats the ray outputs start behind a 16-byte boundary)
    -> (o, d, target) as numpy"""
    n = count * batcher.rays_per_unit
    o = torch.full((offset + n * 3 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    d = torch.full((offset + n * 3 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    t = torch.full((n * 4 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    batcher.draw(epoch, first, count, origins=o[offset:], dirs=d[offset:], target=t, stream=stream)
    torch.cuda.synchronize()
    o, d, t = o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()
    for a, lo, hi in ((o, offset, offset + n * 3), (d, offset, offset + n * 3), (t, 0, n * 4)):
        assert (a[hi:] == -7.0).all() and (a[:lo] == -7.0).all()                       # nothing beside the rays was written
    return o[offset:offset + n * 3].reshape(n, 3), d[offset:offset + n * 3].reshape(n, 3), t[:n * 4].reshape(n, 4)


@pytest.fixture(scope="module")
def batch_set(mnv, torch_gpu):
    """the three cameras of tests/test_fit_adam_ref.py, their target images on the device, and mnv_generate_rays' rays of each"""
    torch = torch_gpu
    cams = far.batch_cameras(mnv)
    host = far.batch_targets([c.c for c in cams])
    dev = [_dev(torch, t) for t in host]
    rays = [mnv.generate_rays(mnv.PROJ_PINHOLE, c) for c in cams]
    torch.cuda.synchronize()
    rays = [(o.cpu().numpy(), d.cpu().numpy()) for o, d in rays]
    return dict(cams=cams, structs=[c.c for c in cams], host=host, dev=dev, rays=rays)


@pytest.mark.parametrize("tile", [8, 1])
def test_draws_are_the_generated_rays_and_targets_of_the_permuted_units(mnv, torch_gpu, batch_set, tile):
    torch, s = torch_gpu, batch_set
    seed = 0x5EED0000BEEF
    b = mnv.RayBatcher(s["cams"], s["dev"], tile=tile, seed=seed)
    total = int(far.unit_table(s["structs"], tile)[-1])
    assert b.units == total and b.rays_per_unit == tile * tile
    for epoch in (0, 1, 2 ** 31 - 1):
        for first, count in ((0, total), (total - 1, 1), (5, 7)):
            o, d, t = _draw_guarded(mnv, torch, b, epoch, first, count)
            D = far.draw(s["structs"], s["host"], tile, seed, epoch, first, count)
            where = (epoch, first, count)
            for ci, c in enumerate(s["cams"]):
                inside = (D["cam"] == ci) & D["inside"]
                iy, ix = D["iy"][inside], D["ix"][inside]
                assert np.array_equal(bits(o[inside]), bits(s["rays"][ci][0][iy, ix])), where    # mnv_generate_rays' device output, gathered
                assert np.array_equal(bits(d[inside]), bits(s["rays"][ci][1][iy, ix])), where
                assert np.array_equal(bits(t[inside]), bits(s["host"][ci][iy, ix])), where
            # ... and every lane, the padded ones among them, is the restatement's
            assert np.array_equal(bits(o), bits(D["o"])) and np.array_equal(bits(d), bits(D["d"])) and np.array_equal(bits(t), bits(D["target"])), where
            pad = ~D["inside"]
            assert not d[pad].any() and not t[pad].any()
    # ray outputs that are only 4-byte aligned take the lanes' own stores: the same bytes
    o1, d1, t1 = _draw_guarded(mnv, torch, b, 1, 0, total, offset=1)
    o0, d0, t0 = _draw_guarded(mnv, torch, b, 1, 0, total)
    assert np.array_equal(bits(o1), bits(o0)) and np.array_equal(bits(d1), bits(d0)) and np.array_equal(bits(t1), bits(t0))


def test_a_draw_depends_on_the_seed_alone_not_on_handle_or_stream(mnv, torch_gpu, batch_set):
    torch, s = torch_gpu, batch_set
    a = mnv.RayBatcher(s["cams"], s["dev"], tile=8, seed=9)
    b = mnv.RayBatcher(s["cams"], s["dev"], tile=8, seed=9)
    c = mnv.RayBatcher(s["cams"], s["dev"], tile=8, seed=10)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = _draw_guarded(mnv, torch, a, 2, 0, a.units, stream=s1.cuda_stream)
    for other in (_draw_guarded(mnv, torch, a, 2, 0, a.units, stream=s2.cuda_stream), _draw_guarded(mnv, torch, b, 2, 0, b.units)):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(first, other))
    assert not np.array_equal(bits(first[2]), bits(_draw_guarded(mnv, torch, c, 2, 0, c.units)[2]))
    assert not np.array_equal(bits(first[2]), bits(_draw_guarded(mnv, torch, a, 3, 0, a.units)[2]))       # another epoch, another order
    for x in (a, b, c):
        x.close()


# ---- the gradient on a drawn batch and the loop ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_scene(mnv, torch_gpu):
    """tests/fit_cases.py's fit scene: the teacher on the device, the cameras, the teacher's frames (the accel march) and the options"""
    S = fit_cases.FIT
    teacher = cases.make_tree(mnv, fit_cases.TREES[S["tree"]])
    teacher.move_to_device()
    opt = mnv.RenderOptions.defaults()
    cams = fit_cases.fit_cameras(mnv)
    frames = []
    for c in cams:
        out = torch_gpu.full((c.height, c.width, 4), float("nan"), dtype=torch_gpu.float32, device="cuda")
        mnv.render_voxels_accel(teacher.accel, c, opt, rgba=out)
        frames.append(out)
    torch_gpu.cuda.synchronize()
    return dict(teacher=teacher, opt=opt, cams=cams, structs=[c.c for c in cams], frames=frames, targets=[f.cpu().numpy().reshape(-1, 4) for f in frames])


@pytest.mark.parametrize("tile", [8, 1])
def test_rays_grad_on_a_drawn_batch_equals_the_restatement(mnv, torch_gpu, fit_scene, tile):
    torch, s = torch_gpu, fit_scene
    lod = s["teacher"].make_lod(fit_cases.FIT["cut"])
    T = fit_ref.tree_of(mnv, lod)
    b = mnv.RayBatcher(s["cams"], s["frames"], tile=tile, seed=4)
    first, count = (3, 5) if tile == 8 else (100, 333)
    o, d, t = b.draw(1, first, count)
    v = lod.device_view()
    acc = torch.zeros((v.capacity * 8, v.data_dim), dtype=torch.int64, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    mnv.rays_grad(v, o, d, t, s["opt"], acc, sums)
    torch.cuda.synchronize()
    D = far.draw(s["structs"], s["targets"], tile, 4, 1, first, count)
    _, want_acc, want_sums, _ = fit_ref.rays_grad(T, s["opt"], D["o"], D["d"], D["target"])
    assert np.array_equal(acc.cpu().numpy(), want_acc) and want_acc.any()
    assert dict(zip(fit_ref.FIT_SUMS, (int(x) for x in sums.cpu().numpy()[:5]))) == want_sums and want_sums["n_rays"] > 0


@pytest.mark.parametrize("steps, units_per_batch", [(6, 4), (7, 5)])
def test_fit_to_ex_reproduces_the_restated_loop(mnv, torch_gpu, fit_scene, steps, units_per_batch):
    """Adam on tile-8 batches: 12 units, so 4 units per batch make three whole batches per epoch (six steps: two epochs) and 5 units leave a
    short third batch (seven steps: the short batch, then the next epoch's order)"""
    torch, s = torch_gpu, fit_scene
    lod = s["teacher"].make_lod(fit_cases.FIT["cut"])
    T = fit_ref.tree_of(mnv, lod)
    before = T["data"].copy()
    want_se, want_n = far.fit_ex(T, s["opt"], s["structs"], s["targets"], steps, "adam", batch_rays=units_per_batch * 64, tile=8, seed=77)
    se, n_rays = lod.fit_to(s["teacher"], s["cams"], s["opt"], steps, optimizer="adam", batch_rays=units_per_batch * 64, tile=8, seed=77, return_counts=True)
    assert se.tolist() == want_se and n_rays.tolist() == want_n and min(want_n) > 0
    got = np.array(lod.host_arrays()[0]).reshape(-1, T["data_dim"])                # the host copy was refreshed
    assert np.array_equal(got, T["data"]) and (got != before).any()
    # ... and so was the accel: the ray march through it gives the restatement's forward on those rows
    o, d = mnv.generate_rays(mnv.PROJ_PINHOLE, s["cams"][1])
    out = torch.full((s["cams"][1].height, s["cams"][1].width, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_rays_accel(lod.accel, o, d, s["opt"], rgba=out)
    torch.cuda.synchronize()
    want = fit_ref.forward(T, s["opt"], o.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1, 3))["rgba"]
    assert np.array_equal(bits(out.cpu().numpy().reshape(-1, 4)), bits(want))


def test_full_batch_adam_and_pixel_batches_reproduce_the_restated_loop(mnv, torch_gpu, fit_scene):
    s = fit_scene
    for kw in (dict(), dict(batch_rays=200, tile=1, seed=3)):
        lod = s["teacher"].make_lod(fit_cases.FIT["cut"])
        T = fit_ref.tree_of(mnv, lod)
        want_se, want_n = far.fit_ex(T, s["opt"], s["structs"], s["targets"], 3, "adam", 0.05, 0.5, 0.8, 0.99, 1e-6, **kw)
        se, n_rays = lod.fit(s["cams"], s["frames"], s["opt"], 3, 0.05, 0.5, optimizer="adam", betas=(0.8, 0.99), eps=1e-6, return_counts=True, **kw)
        assert se.tolist() == want_se and n_rays.tolist() == want_n, kw
        assert np.array_equal(np.array(lod.host_arrays()[0]).reshape(-1, T["data_dim"]), T["data"]), kw


def test_sgd_with_full_batch_is_mnv_n3tree_fit(mnv, torch_gpu, fit_scene):
    """N3Tree::fit is N3Tree::fit_ex with SGD and no batching, so this compares two entries into ONE host loop: it shows that the two C entry
    points and the binding's two paths agree, not that the loop still is what it was.  That pin is tests/test_fit_gpu.py's
    test_fit_to_reproduces_the_restatement, which holds the same loop against tests/fit_ref.py's restatement of mnv_n3tree_fit."""
    S, s = fit_cases.FIT, fit_scene
    old, new = s["teacher"].make_lod(S["cut"]), s["teacher"].make_lod(S["cut"])
    se_old = old.fit_to(s["teacher"], s["cams"], s["opt"], 3, S["lr_colour"], S["lr_sigma"])                 # mnv_n3tree_fit_to_tree
    se_new, n_rays = new.fit_to(s["teacher"], s["cams"], s["opt"], 3, S["lr_colour"], S["lr_sigma"], return_counts=True)   # ..._ex
    assert se_new.tolist() == se_old.tolist() and se_old[2] < se_old[0] and n_rays.min() > 0
    for x, y in zip(old.host_arrays(), new.host_arrays()):
        assert np.array_equal(x, y)
    third = s["teacher"].make_lod(S["cut"])
    se3 = third.fit(s["cams"], s["frames"], s["opt"], 3, S["lr_colour"], S["lr_sigma"], optimizer="sgd", return_counts=True)[0]
    assert se3.tolist() == se_old.tolist() and np.array_equal(third.host_arrays()[0], old.host_arrays()[0])


def test_batched_fit_takes_a_set_beyond_the_full_batch_bound(mnv, torch_gpu, fit_scene):
    """seventeen 1024 x 1024 target images pass 2^24 pixels: the full batch refuses them, a batched fit takes two steps on them"""
    torch, s = torch_gpu, fit_scene
    lod = s["teacher"].make_lod(fit_cases.FIT["cut"])
    cam = fit_cases.frame_camera(mnv, 1024, 0)
    frame = torch.zeros((1024, 1024, 4), dtype=torch.float32, device="cuda")
    frame[..., 3] = 1.0
    with pytest.raises(mnv.MnvError) as e:
        lod.fit([cam] * 17, [frame] * 17, s["opt"], 1, optimizer="adam")
    assert e.value.code == mnv.MNV_E_INVALID
    se, n_rays = lod.fit([cam] * 17, [frame] * 17, s["opt"], 2, optimizer="adam", batch_rays=4096, return_counts=True)
    assert n_rays.tolist() == [4096, 4096] and (se > 0).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(mnv, torch_gpu, batch_set, fit_scene):
    torch, s, lib = torch_gpu, batch_set, mnv.lib()
    E = mnv.MNV_E_INVALID
    # mnv_rows_adam_step
    n_rows, dd = 8, 4
    data = torch.full((n_rows, dd), 0x3C00, dtype=torch.int16, device="cuda")
    master, m1, m2 = (torch.full((n_rows, dd), x, dtype=torch.float32, device="cuda") for x in (1.0, 0.5, 0.25))
    acc = torch.full((n_rows, dd), 1 << 32, dtype=torch.int64, device="cuda")

    def adam(p=None, data_p=data.data_ptr(), m2_p=m2.data_ptr(), rows=n_rows, dim=dd, step=1, **kw):
        p = mnv.AdamParams(0.03, 1.0, 0.9, 0.999, 1e-8) if p is None else p
        for k, val in kw.items():
            setattr(p, k, val)
        return lib.mnv_rows_adam_step(data_p, master.data_ptr(), m1.data_ptr(), m2_p, acc.data_ptr(), rows, dim, C.byref(p), step, None)

    assert adam(data_p=None) == E and adam(m2_p=None) == E and adam(rows=-1) == E and adam(dim=0) == E and adam(step=0) == E and adam(step=-3) == E
    assert lib.mnv_rows_adam_step(data.data_ptr(), master.data_ptr(), m1.data_ptr(), m2.data_ptr(), acc.data_ptr(), n_rows, dd, None, 1, None) == E
    for bad in (dict(lr_colour=float("nan")), dict(lr_sigma=float("inf")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.5), dict(beta2=float("nan")),
                dict(eps=0.0), dict(eps=-1e-8), dict(eps=float("inf")), dict(eps=float("nan"))):
        assert adam(**bad) == E, bad
    assert adam(m2_p=m2.data_ptr() + 2) == E
    torch.cuda.synchronize()
    assert (data.cpu().numpy() == 0x3C00).all() and (master.cpu().numpy() == 1.0).all() and (m1.cpu().numpy() == 0.5).all()
    assert (m2.cpu().numpy() == 0.25).all() and (acc.cpu().numpy() == 1 << 32).all()
    assert adam(rows=0) == 0
    # mnv_ray_batcher_create
    n = len(s["cams"])
    arr = (mnv.CameraStruct * n)(*s["structs"])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in s["dev"]])
    h = C.c_void_p()
    create = lib.mnv_ray_batcher_create
    assert create(None, ptrs, n, 8, 0, C.byref(h)) == E and create(arr, None, n, 8, 0, C.byref(h)) == E and create(arr, ptrs, n, 8, 0, None) == E
    assert create(arr, ptrs, 0, 8, 0, C.byref(h)) == E and create(arr, ptrs, 4097, 8, 0, C.byref(h)) == E
    for tile in (0, 2, 4, 16, -8):
        assert create(arr, ptrs, n, tile, 0, C.byref(h)) == E, tile
    flat = mnv.CameraStruct.from_buffer_copy(s["structs"][0])
    flat.width = 0
    assert create((mnv.CameraStruct * 1)(flat), ptrs, 1, 8, 0, C.byref(h)) == E
    assert create(arr, (C.c_void_p * n)(ptrs[0], None, ptrs[2]), n, 8, 0, C.byref(h)) == E
    assert create(arr, (C.c_void_p * n)(ptrs[0], ptrs[1] + 4, ptrs[2]), n, 8, 0, C.byref(h)) == E      # a target image off its 16-byte boundary
    low = mnv.CameraStruct.from_buffer_copy(s["structs"][0])
    low.height = 0
    assert create((mnv.CameraStruct * 1)(low), ptrs, 1, 8, 0, C.byref(h)) == E
    low.height = -3
    assert create((mnv.CameraStruct * 1)(low), ptrs, 1, 1, 0, C.byref(h)) == E
    huge = mnv.CameraStruct.from_buffer_copy(s["structs"][0])
    huge.width, huge.height = 1 << 16, 1 << 15                                          # 2^31 pixels: U >= 2^31 with tile 1, fine with tile 8
    assert create((mnv.CameraStruct * 1)(huge), ptrs, 1, 1, 0, C.byref(h)) == E
    assert h.value is None
    # mnv_ray_batcher_draw
    b = mnv.RayBatcher(s["cams"], s["dev"], tile=8, seed=1)
    o = torch.full((b.units * 64 * 3 + 4,), -7.0, dtype=torch.float32, device="cuda")
    d, t = o.clone(), torch.full((b.units * 64 * 4 + 4,), -7.0, dtype=torch.float32, device="cuda")
    draw = lib.mnv_ray_batcher_draw

    def drawn(handle=b._h, epoch=0, first=0, count=b.units, o_p=o.data_ptr(), d_p=d.data_ptr(), t_p=t.data_ptr()):
        return draw(handle, epoch, first, count, o_p, d_p, t_p, None)

    assert drawn(handle=None) == E and drawn(o_p=None) == E and drawn(d_p=None) == E and drawn(t_p=None) == E
    assert drawn(epoch=-1) == E and drawn(first=-1) == E and drawn(count=0) == E and drawn(first=1) == E and drawn(first=b.units, count=1) == E
    assert drawn(count=1 << 62) == E and drawn(first=1 << 62, count=1 << 62) == E
    assert drawn(o_p=o.data_ptr() + 2) == E and drawn(t_p=t.data_ptr() + 4) == E and drawn(t_p=t.data_ptr() + 8) == E
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == -7.0).all() and (d.cpu().numpy() == -7.0).all() and (t.cpu().numpy() == -7.0).all()
    assert lib.mnv_ray_batcher_units(None, None, None) == E
    lib.mnv_ray_batcher_destroy(None)                                                   # (a null handle is nothing to destroy)
    # a draw of more than 2^22 rays: 2^16 + 1 tiles of one large image
    big_cam = mnv.CameraStruct.from_buffer_copy(s["structs"][0])
    big_cam.width, big_cam.height = 8 * 257, 8 * 256
    img = torch.zeros((big_cam.height, big_cam.width, 4), dtype=torch.float32, device="cuda")
    hb = C.c_void_p()
    assert create((mnv.CameraStruct * 1)(big_cam), (C.c_void_p * 1)(img.data_ptr()), 1, 8, 0, C.byref(hb)) == 0
    assert draw(hb, 0, 0, (1 << 16) + 1, o.data_ptr(), d.data_ptr(), t.data_ptr(), None) == E
    lib.mnv_ray_batcher_destroy(hb)
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == -7.0).all()
    # the loops
    f = fit_scene
    lod = f["teacher"].make_lod(fit_cases.FIT["cut"])
    rows = np.array(lod.host_arrays()[0]).copy()
    for kw in (dict(optimizer="adam", batch_rays=100), dict(optimizer="adam", batch_rays=(1 << 22) + 64), dict(optimizer="adam", batch_rays=-64),
               dict(optimizer="adam", tile=4), dict(optimizer="adam", betas=(1.0, 0.999)), dict(optimizer="adam", betas=(0.9, -0.5)),
               dict(optimizer="adam", eps=0.0), dict(optimizer="adam", lr_colour=float("nan")), dict(optimizer="adam", lr_sigma=-1.0)):
        with pytest.raises(mnv.MnvError) as e:
            lod.fit_to(f["teacher"], f["cams"], f["opt"], 1, **kw)
        assert e.value.code == E, kw
    with pytest.raises(mnv.MnvError) as e:                                              # more cameras than a batcher takes
        lod.fit([f["cams"][0]] * 4097, [f["frames"][0]] * 4097, f["opt"], 1, optimizer="adam", batch_rays=64)
    assert e.value.code == E
    px = mnv.FitParamsEx(1, 2, 0.03, 1.0, 0.9, 0.999, 1e-8, 0, 8, 0)                    # an optimizer that does not exist
    arr = (mnv.CameraStruct * len(f["cams"]))(*f["structs"])
    assert lib.mnv_n3tree_fit_to_tree_ex(lod._h, f["teacher"]._h, arr, len(f["cams"]), C.byref(f["opt"]), C.byref(px), None, None) == E
    assert lib.mnv_n3tree_fit_to_tree_ex(lod._h, f["teacher"]._h, arr, 0, C.byref(f["opt"]), C.byref(px), None, None) == E
    assert lib.mnv_n3tree_fit_ex(lod._h, arr, len(f["cams"]), None, C.byref(f["opt"]), C.byref(px), None, None) == E
    assert np.array_equal(np.array(lod.host_arrays()[0]), rows)


# ---- the command line -----------------------------------------------------------------------------------------------------------------------
def test_mnv_render_lod_fit_with_adam_on_batches(mnv, torch_gpu, tmp_path):
    """mnv_render --lod D --lod_fit N --fit_optimizer adam --fit_batch RAYS --save_lod: the written tree is the cut N3Tree.fit_to makes with
    the same keywords at the run's pose (Adam's default rates), and the frame the run wrote is the frame of that tree (the renderer fitted
    its own cut: VolumeRenderer::set_lod_fit with mnv_fit_params_ex); the new flags are refused without --lod_fit"""
    import os
    import subprocess

    torch = torch_gpu
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mega-nerf-viewer_amd", "mnv_render")
    assert os.path.exists(exe), "mnv_render not built"
    S = fit_cases.FIT
    tree = cases.make_tree(mnv, fit_cases.TREES[S["tree"]])
    npz, saved, out = str(tmp_path / "scene.npz"), str(tmp_path / "fitted.npz"), str(tmp_path / "frame")
    tree.save_npz(npz)
    center, back, size = (-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48), 32
    common = [exe, npz, "-w", str(size), "-h", str(size), "--fx", "40", "--center", ",".join(map(str, center)), "--back", ",".join(map(str, back))]
    r = subprocess.run(common + ["--out", out, "--raw", "--frames", "1", "--lod", str(S["cut"]), "--lod_fit", "5", "--fit_optimizer", "adam", "--fit_batch", "256",
                                 "--fit_seed", "6", "--save_lod", saved], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lod_fit:" in r.stdout, r.stderr + r.stdout
    tree.move_to_device()
    cut = tree.make_lod(S["cut"])
    plain = np.array(cut.host_arrays()[0])
    cam = mnv.Camera(size, size, 40.0).set_pose(center, back)
    opt = mnv.RenderOptions.cli_defaults()
    se, n_rays = cut.fit_to(tree, [cam], opt, 5, optimizer="adam", batch_rays=256, seed=6, return_counts=True)   # 16 tiles: four batches per epoch
    assert (n_rays > 0).all()
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
    for flags in (["--lod", "3", "--fit_optimizer", "adam"], ["--lod", "3", "--fit_batch", "256"], ["--fit_tile", "1"], ["--lod", "3", "--fit_seed", "1"]):
        bad = subprocess.run(common + flags, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--lod_fit" in bad.stderr, flags
    for flags in (["--fit_optimizer", "lbfgs"], ["--fit_tile", "4"], ["--fit_batch", "100"], ["--fit_batch", "-64"]):
        bad = subprocess.run(common + ["--lod", "3", "--lod_fit", "2"] + flags, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and flags[0] in bad.stderr, flags


def test_renderer_set_lod_fit_keywords(mnv, torch_gpu):
    """Renderer.set_lod_fit with Adam on pixel batches: the frame of the renderer's own fitted cut is the frame of the cut fit_to makes with
    the same keywords at the camera the renderer used"""
    torch = torch_gpu
    S = fit_cases.FIT
    tree, source = cases.make_tree(mnv, fit_cases.TREES[S["tree"]]), cases.make_tree(mnv, fit_cases.TREES[S["tree"]])
    size, kw = 24, dict(optimizer="adam", batch_rays=128, tile=1, seed=2)
    rend = mnv.Renderer()
    rend.resize(size, size)
    rend.set(tree, tree.capacity)
    opt = mnv.RenderOptions.cli_defaults()
    C.memmove(C.byref(rend.options), C.byref(opt), C.sizeof(opt))
    rend.set_camera((-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48), fx=30.0)
    rend.render()                                                    # (a plain frame: the camera the renderer marches with)
    plain = rend.download_slot(rend.last_slot())
    cam = mnv.Camera(size, size, 30.0)
    C.memmove(C.byref(cam.c), C.byref(rend.last_camera()), C.sizeof(cam.c))
    rend.set_lod(S["cut"])
    rend.set_lod_fit([cam], 4, None, None, **kw)
    rend.render()
    got = rend.download_slot(rend.last_slot())
    source.move_to_device()
    cut = source.make_lod(S["cut"])
    se = cut.fit_to(source, [cam], opt, 4, **kw)
    assert len(se) == 4 and (se > 0).all()
    want = torch.full((size, size, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(cut.accel, cam, opt, rgba=want)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(want.cpu().numpy())) and not np.array_equal(bits(got), bits(plain))
    rend.set_lod_fit()                                               # off again: the plain cut
    rend.render()
    unfitted = source.make_lod(S["cut"])
    mnv.render_voxels_accel(unfitted.accel, cam, opt, rgba=want)
    torch.cuda.synchronize()
    assert np.array_equal(bits(rend.download_slot(rend.last_slot())), bits(want.cpu().numpy()))


def test_mnv_render_fit_images_fits_the_marched_tree_to_written_frames(mnv, torch_gpu, tmp_path):
    """a run with --out, then --lod D --fit_images PREFIX --fit_steps 2 --save_lod: the written tree is the cut N3Tree.fit makes from the same
    bytes / 255 (alpha 1) at the fitted pose -- pose 1 of two is held out by --fit_holdout 2 --, the frames the run wrote are that tree's,
    and the PSNR lines are printed; with Adam on batches likewise; the refusals"""
    import os
    import subprocess

    torch = torch_gpu
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mega-nerf-viewer_amd", "mnv_render")
    assert os.path.exists(exe), "mnv_render not built"
    S = fit_cases.FIT
    tree = cases.make_tree(mnv, fit_cases.TREES[S["tree"]])
    npz, photos = str(tmp_path / "scene.npz"), str(tmp_path / "photo")
    tree.save_npz(npz)
    center, back, size = (-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48), 32
    common = [exe, npz, "-w", str(size), "-h", str(size), "--fx", "40", "--center", ",".join(map(str, center)), "--back", ",".join(map(str, back)), "--frames", "2"]
    r = subprocess.run(common + ["--out", photos], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(photos + "_0001.ppm"), r.stderr + r.stdout
    tree.move_to_device()
    cam = mnv.Camera(size, size, 40.0).set_pose(center, back)
    opt = mnv.RenderOptions.cli_defaults()
    photo = mnv.pnm_read(photos + "_0000.ppm", size, size)
    target = np.ones((size, size, 4), np.float32)
    target[..., :3] = photo.reshape(size, size, 3).astype(np.float32) / np.float32(255.0)
    target_dev = _dev(torch, target)
    for i, (flags, kw) in enumerate(((["--fit_lr_colour", "1", "--fit_lr_sigma", "20"], dict(lr_colour=1.0, lr_sigma=20.0)),
                                     (["--fit_optimizer", "adam", "--fit_batch", "256", "--fit_seed", "0xF000000000000001"],
                                      dict(optimizer="adam", batch_rays=256, seed=0xF000000000000001)))):
        saved, out = str(tmp_path / f"fitted{i}.npz"), str(tmp_path / f"frame{i}")
        r = subprocess.run(common + ["--lod", str(S["cut"]), "--fit_images", photos, "--fit_steps", "2", "--fit_holdout", "2", "--save_lod", saved, "--out", out,
                                     "--raw"] + (flags if i else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "fit_images: 1 pose(s) fitted, 1 held out" in r.stdout and "held-out poses" in r.stdout, r.stderr + r.stdout
        cut = tree.make_lod(S["cut"])
        plain = np.array(cut.host_arrays()[0])
        se = cut.fit([cam], [target_dev], opt, 2, **kw)
        assert len(se) == 2 and (se > 0).all()
        back_in = mnv.N3Tree.open(saved)
        for x, y in zip(back_in.host_arrays(), cut.host_arrays()):
            assert np.array_equal(x, y), i
        assert (np.array(back_in.host_arrays()[0]) != plain).any()
        want = torch.full((size, size, 4), float("nan"), dtype=torch.float32, device="cuda")
        mnv.render_voxels_accel(cut.accel, cam, opt, rgba=want)
        torch.cuda.synchronize()
        for f in (0, 1):                                                                   # the frames show the fitted tree
            got = np.fromfile(out + f"_000{f}.f32", dtype=np.float32).reshape(size, size, 4)
            assert np.array_equal(bits(got), bits(want.cpu().numpy())), (i, f)
    for flags, word in ((["--fit_images", photos], "--fit_steps"), (["--fit_steps", "2"], "--fit_images"), (["--fit_images", photos, "--fit_steps", "0"], "--fit_steps"),
                        (["--fit_images", photos, "--fit_steps", "2", "--fit_holdout", "1"], "--fit_holdout"),
                        (["--fit_images", photos, "--fit_steps", "2", "--lod", "3", "--lod_fit", "2"], "--lod_fit"),
                        (["--fit_images", photos, "--fit_steps", "2", "--cull", "0.01"], "--cull"),
                        (["--fit_images", photos, "--fit_steps", "2", "--gpus", "2"], "--gpus"),
                        (["--fit_images", photos, "--fit_steps", "2", "--use_splitting"], "--use_splitting"),
                        (["--fit_images", photos, "--fit_steps", "2", "--use_guided_sampling"], "--use_guided_sampling"),
                        (["--fit_images", str(tmp_path / "nothing"), "--fit_steps", "2"], "nothing"),
                        (["--fit_images", photos, "--fit_steps", "2", "--fit_seed", "-1"], "--fit_seed")):
        bad = subprocess.run(common + flags, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and word in bad.stderr, (flags, bad.stderr)
