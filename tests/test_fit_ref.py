"""The numpy restatement of the fitting contract (tests/fit_ref.py) held on the CPU: (a) its forward march equals the oracle bit for bit on
every test ray; (b) the contract's formulas, evaluated in binary64 on the recorded sample geometry, are the derivative of the binary64
loss (central differences, whole gradient vectors by relative L2 norm); (c) the binary32 contract words stay within a measured bound of
that binary64 gradient; (d) the cases contain what they are meant to: early stops, hits that do not stop, misses, degenerate rays, leaves
at several depths, a voxel fed by 64 rays and more.  tests/test_fit_gpu.py holds the device against the same restatement."""
import numpy as np
import pytest

import cases
import fit_cases
import fit_ref
import rays_ref

bits = cases.bits

# (b): central differences with h = 1e-6 (1 + |x|) on a loss of order 1 in binary64: truncation ~ h^2, rounding ~ 2^-53 / h ~ 1e-10 against
# gradient vectors of norm 1e-3 .. 1: a relative L2 error of 1e-6 leaves three orders of margin and would not pass a wrong term
FD_BOUND = 1e-6
# (c): measured here over the six cases: the largest relative L2 distance between the binary32 words and the binary64 gradient was
# 1.39e-7 (sh1_d4; the others 1.0e-8 .. 1.17e-7) -- binary32 rounding of a few dozen operations per term (2^-24 = 6e-8 each) plus the
# 2^-33 of the fixed-point rounding.  Rounding differs per scene, hence 4 x the maximum.
F32_BOUND = 4 * 1.39e-7


@pytest.fixture(scope="module")
def truth(mnv):
    """per case: the tree's arrays, the options, the rays and the restatement's answer -- computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            tree = cases.make_tree(mnv, fit_cases.TREES[name])
            T = fit_ref.tree_of(mnv, tree)
            opt = fit_cases.make_options(mnv, name)
            L = fit_cases.ray_list(mnv, name)
            rgba, acc, sums, fw = fit_ref.rays_grad(T, opt, L["o"], L["d"], L["target"], L["tmax"])
            cache[name] = dict(tree=tree, T=T, opt=opt, L=L, rgba=rgba, acc=acc, sums=sums, fw=fw)
        return cache[name]

    return get


@pytest.mark.parametrize("name", fit_cases.NAMES)
def test_forward_equals_the_oracle(mnv, orc, truth, name):
    t = truth(name)
    L = t["L"]
    n_frame = fit_cases.FRAME ** 2
    sel = np.r_[0:n_frame, n_frame + 4:L["o"].shape[0]]                      # (the oracle takes no degenerate ray: the four are below)
    want, _ = rays_ref.oracle_rays(orc, orc.tree_from_view(t["tree"].host_view()), L["o"][sel], L["d"][sel], t["opt"], L["tmax"][sel])
    assert not t["fw"]["broken"].any()
    diff = (bits(t["rgba"][sel]) != bits(want)).any(axis=1)
    assert not diff.any(), f"{name}: {int(diff.sum())} of {sel.size} rays differ from the oracle"
    # degenerate rays are misses: the background, alpha 0
    bg = np.float32(t["opt"].background_brightness)
    assert np.array_equal(bits(t["rgba"][n_frame:n_frame + 4]), bits(np.tile(np.float32([bg, bg, bg, 0.0]), (4, 1))))


def _fd_ray(t, i):
    """(analytic binary64 gradient, central differences) of ray i's loss by the rows of its samples"""
    T, opt, fw, tg = t["T"], t["opt"], t["fw"], t["L"]["target"][i]
    an, sm, rows = fit_ref.gradient64_ray(T, opt, fw, i, tg)
    m, dd = rows.shape
    h = 1e-6 * (1.0 + np.abs(rows))
    pert = np.broadcast_to(rows, (2, m, dd, m, dd)).copy()
    for s in range(m):
        for c in range(dd):
            pert[0, s, c, s, c] += h[s, c]
            pert[1, s, c, s, c] -= h[s, c]
    loss = fit_ref.loss64_ray(T, opt, fw, i, tg, pert)
    return an, (loss[0] - loss[1]) / (2.0 * h)


@pytest.mark.parametrize("name", fit_cases.NAMES)
def test_contract_formulas_are_the_derivative(truth, name):
    t = truth(name)
    fw = t["fw"]
    hit = np.nonzero((fw["n_dense"] > 0) & (t["L"]["target"][:, 3] != 0))[0]
    stopped, open_ = hit[fw["stopped"][hit]], hit[~fw["stopped"][hit]]
    pick = np.concatenate([stopped[:: max(1, stopped.size // 12)][:12], open_[:: max(1, open_.size // 12)][:12]])
    assert pick.size >= 8
    an, fd = zip(*[_fd_ray(t, int(i)) for i in pick])
    an, fd = np.concatenate([a.ravel() for a in an]), np.concatenate([f.ravel() for f in fd])
    err = np.linalg.norm(an - fd) / np.linalg.norm(fd)
    print(f"{name}: {pick.size} rays, {an.size} entries, |grad| = {np.linalg.norm(fd):.4g}, relative L2 error of the formulas = {err:.3g}")
    assert np.linalg.norm(fd) > 1e-4 and err < FD_BOUND


@pytest.mark.parametrize("name", fit_cases.NAMES)
def test_float32_words_against_the_float64_gradient(truth, name):
    t = truth(name)
    g64 = fit_ref.gradient64(t["T"], t["opt"], t["fw"], t["L"]["target"])
    g32 = t["acc"].astype(np.float64) / fit_ref.Q32
    err = np.linalg.norm(g32 - g64) / np.linalg.norm(g64)
    print(f"{name}: |grad| = {np.linalg.norm(g64):.4g}, relative L2 distance of the binary32 words = {err:.3g}")
    assert err < F32_BOUND


def test_cases_contain_what_they_are_meant_to(truth):
    depths_seen = set()
    for name in fit_cases.NAMES:
        t = truth(name)
        fw, L, s = t["fw"], t["L"], t["sums"]
        inc = L["target"][:, 3] != 0
        assert s["n_stopped"] >= 5, name                                              # early-stopped rays
        assert int((inc & ~fw["stopped"] & (fw["n_dense"] > 0)).sum()) >= 5, name       # hits that do not stop
        assert int((fw["in_bbox"] & (fw["n_dense"] == 0)).sum() + (~fw["in_bbox"]).sum()) >= 12, name   # misses
        assert not fw["in_bbox"][fit_cases.FRAME ** 2:fit_cases.FRAME ** 2 + 4].any()   # the degenerate rays
        assert s["n_skipped"] == 0 and s["n_rays"] == int(inc.sum()) and 0 < s["n_rays"] < inc.size
        vox = np.concatenate([b["vox"][inc[b["ray"]]] for b in fw["batches"]])
        assert np.bincount(vox).max() >= 64, name                                      # one voxel fed by 64 rays and more
        d = set(np.concatenate([b["depth"] for b in fw["batches"]]).tolist())
        depths_seen.add(len(d))
        if "_d4" in name:
            assert len(d) >= 2, name                                                   # leaves at two or more depths
        if name == "sh9_d4":                                                           # masked coefficients get no term
            B = 9
            cols = np.r_[[k * B + j for k in range(3) for j in (0, 6, 7, 8)]]
            assert not t["acc"][:, cols].any() and t["acc"][:, 1].any()
    assert max(depths_seen) >= 2


def test_row_kernels_restated():
    """master_init and sgd_step on special values: non-finite bits read +0; untouched rows keep their bytes; saturation; the clamp"""
    data = np.array([[0x3C00, 0x7C00, 0xFE00, 0xC000], [0x7BFF, 0x0001, 0x8000, 0xBC00], [0x7C00, 0x3C00, 0x3C00, 0x3C00]], np.uint16)
    m = fit_ref.master_init(data)
    assert np.array_equal(bits(m), bits(np.float32([[1, 0, 0, -2], [65504, 2.0 ** -24, -0.0, -1], [0, 1, 1, 1]])))
    acc = np.zeros((3, 4), np.int64)
    acc[1] = [-(1 << 40), 1 << 32, 0, 1 << 33]
    before = data.copy()
    fit_ref.sgd_step(data, m, acc, 1.0, 0.25)
    assert np.array_equal(data[[0, 2]], before[[0, 2]]) and not acc.any()             # the row of inf bits stays as it is: it was not touched
    assert data[1].tolist() == [0x7BFF, 0xBC00, 0x8000, 0x0000]                        # 65504 + 256 saturates; -1 - 0.5 clamps to 0
    assert m[1].tolist() == [65760.0, np.float32(2.0 ** -24 - 1.0), -0.0, 0.0]


def test_the_restatement_falls_at_every_step_with_the_chosen_rates(mnv, orc):
    """the learning rates and the iteration count of tests/test_fit_gpu.py's descent test (fit_cases.FIT), checked on the restatement: the
    teacher's frames from the oracle, the cut from tests/lod_ref.py"""
    import lod_ref

    F = fit_cases.FIT
    tree = cases.make_tree(mnv, fit_cases.TREES[F["tree"]])
    opt = mnv.RenderOptions.defaults()
    data, child, _ = tree.host_arrays()
    lod = lod_ref.make_lod(np.array(data), np.array(child), F["cut"])
    T = fit_ref.tree_of(mnv, tree)
    T.update(data=lod["data"].reshape(-1, T["data_dim"]).copy(), child=lod["child"].reshape(-1).copy(), capacity=lod["capacity"])
    cams = fit_cases.fit_cameras(mnv)
    targets = [orc.render(orc.tree_from_view(tree.host_view()), c.c, opt)["rgba"].reshape(-1, 4) for c in cams]
    rays = [tuple(a.reshape(-1, 3) for a in rays_ref.pinhole_rays(c.c)) for c in cams]
    se = fit_ref.fit(T, opt, rays, targets, F["iterations"], F["lr_colour"], F["lr_sigma"])
    print("se_q32 / 2^32 per iteration:", " ".join(f"{s / fit_ref.Q32:.4f}" for s in se))
    assert all(b < a for a, b in zip(se, se[1:])), se
    assert se[-1] < 0.9 * se[0]
