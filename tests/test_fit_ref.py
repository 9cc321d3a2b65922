"""The numpy restatement of the fitting contract (tests/fit_ref.py) held on the CPU: (a) its forward march equals the oracle bit for bit on
every test ray; (b) the contract's formulas, evaluated in binary64 on the recorded sample geometry, are the derivative of the binary64
loss (central differences, whole gradient vectors by relative L2 norm); (c) the binary32 contract words stay within a measured bound of
that binary64 gradient; (d) the cases contain what they are meant to: early stops, hits that do not stop, misses, degenerate rays, leaves
at several depths, a voxel fed by 64 rays and more; (e) the same four for the edge cases of tests/fit_cases.py -- SH16 / SH25 rows, scales
that differ per axis -- and what the inputs of the edge tests contain: skipped rays, saturated terms, broken links, padded rows.
tests/test_fit_gpu.py holds the device against the same restatement."""
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
# (c) for fit_cases.EDGE_NAMES, measured here with their own options: 1.86e-7 (sh16_d3_aniso), 1.63e-7 (sh25_d3), 3.07e-8 (sh4_d4_aniso).
# The wide rows sum 16 and 25 products per channel before the sigmoid, hence more rounding per term than the six above; the same margin
# for the same reason.
EDGE_F32_BOUND = 4 * 1.86e-7


@pytest.fixture(scope="module")
def truth(mnv):
    """per case: the tree's arrays, the options, the rays and the restatement's answer -- computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            tree = cases.make_tree(mnv, fit_cases.tree_spec(name))
            T = fit_ref.tree_of(mnv, tree)
            opt = fit_cases.make_options(mnv, name)
            L = fit_cases.ray_list(mnv, name)
            rgba, acc, sums, fw = fit_ref.rays_grad(T, opt, L["o"], L["d"], L["target"], L["tmax"])
            cache[name] = dict(tree=tree, T=T, opt=opt, L=L, rgba=rgba, acc=acc, sums=sums, fw=fw)
        return cache[name]

    return get


@pytest.mark.parametrize("name", fit_cases.NAMES + fit_cases.EDGE_NAMES)
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


@pytest.mark.parametrize("name", fit_cases.NAMES + fit_cases.EDGE_NAMES)
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


@pytest.mark.parametrize("name", fit_cases.EDGE_NAMES)
def test_float32_words_against_the_float64_gradient_on_the_edge_cases(truth, name):
    t = truth(name)
    g64 = fit_ref.gradient64(t["T"], t["opt"], t["fw"], t["L"]["target"])
    g32 = t["acc"].astype(np.float64) / fit_ref.Q32
    err = np.linalg.norm(g32 - g64) / np.linalg.norm(g64)
    print(f"{name}: |grad| = {np.linalg.norm(g64):.4g}, relative L2 distance of the binary32 words = {err:.3g}")
    assert err < EDGE_F32_BOUND


def test_edge_cases_contain_what_they_are_meant_to(truth):
    for name in fit_cases.EDGE_NAMES:
        t = truth(name)
        fw, L, s, T = t["fw"], t["L"], t["sums"], t["T"]
        inc = L["target"][:, 3] != 0
        assert s["n_stopped"] >= 5, name                                              # early-stopped rays
        assert int((inc & ~fw["stopped"] & (fw["n_dense"] > 0)).sum()) >= 5, name       # hits that do not stop
        assert s["n_skipped"] == 0 and s["n_rays"] == int(inc.sum()) and s["n_samples"] >= 500
        n_ds = np.unique(fw["R"]["delta_scale"][fw["in_bbox"]]).size
        print(f"{name}: sums {s}, {n_ds} distinct delta_scale, {np.count_nonzero(t['acc'])} non-zero words")
        if name.endswith("_aniso"):
            assert n_ds >= 300, name                                                   # delta_scale varies with the direction
        assert T["data_dim"] == {"sh16_d3_aniso": 49, "sh25_d3": 76, "sh4_d4_aniso": 13}[name]
        if name == "sh25_d3":                                                          # the second trip of the column loop has work to do
            assert np.count_nonzero(t["acc"][:, 64:75]) >= 500 and t["acc"][:, 75].any()
            assert all(t["acc"][:, c].any() for c in range(76))
        if name == "sh16_d3_aniso":                                                    # masked coefficients get no term, every other column does
            masked = np.r_[[k * 16 + j for k in range(3) for j in (0, 1, 12, 13, 14, 15)]]
            assert not t["acc"][:, masked].any()
            assert all(t["acc"][:, c].any() for c in range(49) if c not in masked)


def test_edge_inputs_contain_what_they_are_meant_to(mnv, truth, monkeypatch):
    """the skipped rays, the clamp and the NaN terms; links that leave the tree; padded rows: what the restatement says of the inputs that
    tests/test_fit_gpu.py and tests/test_visibility_gpu.py hold the device to"""
    import visibility_ref

    clamp32 = fit_ref.q32
    for name in ("sh4_d4_aniso", "sh25_d3"):
        t = truth(name)
        tg = fit_cases.skip_targets(t["L"]["target"])
        acc, s = fit_ref.backward(t["T"], t["opt"], t["fw"], tg)
        n_sat = int((np.abs(acc) >= 2 ** 37).sum())
        print(f"{name}: {s}, {n_sat} words at +-2^37")
        assert s["n_skipped"] >= 10 and n_sat >= 1 and s["n_rays"] > 500, name
        assert s["se_q32"] >= 10 * 2 ** 37                                            # the squared error saturates the same way
        # terms do meet the clamp: a wider clamp would give other words (a word of 2^37 could also be a sum of smaller terms)
        monkeypatch.setattr(fit_ref, "q32", lambda x: np.where(np.abs(x) > 32, np.sign(x) * 2 ** 38, clamp32(x)).astype(np.int64))
        wide, _ = fit_ref.backward(t["T"], t["opt"], t["fw"], tg)
        monkeypatch.undo()
        assert (wide != acc).any() and np.array_equal(fit_ref.backward(t["T"], t["opt"], t["fw"], tg)[0], acc)
    # NaN terms: none of the targets above makes one (SH colours stay in [0, 1]); fit_cases.nan_terms does, on RGBA rows with large
    # colours.  Counted where they reach q32; a q32 that read a NaN as anything but 0 would give other words.
    t = truth("rgba_d4")
    U, tg = fit_cases.nan_terms(t["T"], t["L"]["target"])
    fw = fit_ref.forward(U, t["opt"], t["L"]["o"], t["L"]["d"], t["L"]["tmax"])
    n_nan = []
    monkeypatch.setattr(fit_ref, "q32", lambda x: (n_nan.append(int(np.isnan(x).sum())), clamp32(x))[1])
    acc, s = fit_ref.backward(U, t["opt"], fw, tg)
    monkeypatch.setattr(fit_ref, "q32", lambda x: np.where(np.isnan(x), 1 << 32, clamp32(x)).astype(np.int64))
    other, _ = fit_ref.backward(U, t["opt"], fw, tg)
    monkeypatch.undo()
    print(f"nan_terms: {sum(n_nan)} NaN terms, {s}")
    assert sum(n_nan) >= 10 and s["n_skipped"] == 0 and (other != acc).any() and np.array_equal(other[:, :3], acc[:, :3])
    # links: rays break at the links to chunk 0, at the capacity and -- the inside rays -- at chunk 151 itself, the first one outside
    t = truth(fit_cases.BROKEN["tree"])
    T, L = fit_cases.broken_links(t["T"], t["L"])
    _, _, s, fw = fit_ref.rays_grad(T, t["opt"], L["o"], L["d"], L["target"], L["tmax"])
    n_in = fit_cases.BROKEN["inside"]
    print(f"links: {int(fw['broken'].sum())} rays broken, {s}")
    assert s["n_skipped"] >= 20 + n_in and fw["broken"][-n_in:].all() and 200 < s["n_rays"] and s["n_samples"] > 200
    one_more = fit_ref.forward(dict(T, capacity=T["capacity"] + 1), t["opt"], L["o"], L["d"], L["tmax"])
    assert int((fw["broken"] & ~one_more["broken"]).sum()) >= 20                       # (>= capacity, not > capacity, is what breaks those)
    _, vs, _ = visibility_ref.rays_visibility(T, t["opt"], L["o"], L["d"], L["tmax"])
    assert vs["n_skipped"] == int(fw["broken"].sum()) >= s["n_skipped"]
    # padded rows: the padding columns get no word, the others the words of the unpadded tree
    t = truth("sh1_d4")
    P = fit_cases.padded_rows(t["T"])
    rgba, acc, s, _ = fit_ref.rays_grad(P, t["opt"], t["L"]["o"], t["L"]["d"], t["L"]["target"], t["L"]["tmax"])
    assert s == t["sums"] and np.array_equal(bits(rgba), bits(t["rgba"]))
    assert not acc[:, 3:6].any() and np.array_equal(acc[:, [0, 1, 2, 6]], t["acc"]) and t["acc"].any()


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
