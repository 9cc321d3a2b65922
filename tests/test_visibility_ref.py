"""The numpy restatement of the culling contract (tests/visibility_ref.py) held on the CPU: (a) the weights it takes the maxima of are the
oracle's -- on a copy of every tree whose colours are all 1 the oracle's pixel is the sum of the weights, and the march does not depend
on colour; (b) the comparison with the threshold is strict; (c) the kept set is parent-closed; (d) at threshold 0 the culled rows, not
cut, give every listed ray the oracle's pixel of the source tree, bit for bit; (e) the scenes are mixed: dead chunks, live chunks, culled
and seen non-empty leaves, with the counts written down; (f) how far the frames of the CUT tree are from the source's, which
tests/test_visibility_gpu.py holds the device to."""
import numpy as np
import pytest

import cases
import fit_cases
import fit_ref
import lod_ref
import rays_ref
import visibility_cases as vc
import visibility_ref as ref

bits = cases.bits

# (e) what the restatement gives at weight_thresh = visibility_cases.MIXED_THRESH: (leaves seen, non-empty leaves culled, dead chunks, kept per depth)
MIXED = {
    "sh4_d4": (213, 345, 52, [1, 5, 23, 76]),
    "sh9_d4": (131, 128, 17, [1, 2, 10, 40]),
    "rgba_d4": (111, 180, 29, [1, 3, 15, 37]),
    "sh1_d4": (167, 64, 6, [1, 3, 10, 42]),
    "wall": (16, 116, 16, [1, 4]),
}
# (f) the largest channel difference between the oracle's pixels of the restated cut tree (weight_thresh 0) and of the source tree over the
# listed rays, measured here: the cut changes no sample's row, only the steps through collapsed regions, each of which adds step_size, so
# later sample lengths shift (include/mnv.h).  The quantity is deterministic; the device is held to 4 x it (slack for nothing but a
# reader's peace, as F32_BOUND in tests/test_fit_ref.py).
CUT_DIFF = {"wall": 0.0, "sh9_d4": 2.0 ** -24}       # (wall: 21 -> 5 chunks, every listed ray ends in the slab; sh9_d4: 70 -> 56 chunks, 5.96e-8)
CUT_BOUND = {k: 4 * v for k, v in CUT_DIFF.items()}


def scene(mnv, name):
    """(tree, options, ray list dict(o, d, tmax)) of a case"""
    if name == "wall":
        return vc.wall_tree(mnv), mnv.RenderOptions.defaults(), vc.wall_ray_list(mnv)
    return cases.make_tree(mnv, fit_cases.tree_spec(name)), fit_cases.make_options(mnv, name), fit_cases.ray_list(mnv, name)


@pytest.fixture(scope="module")
def truth(mnv):
    """per case: the tree, its arrays, options, rays, the restatement's words and the cull at threshold 0 -- computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            tree, opt, L = scene(mnv, name)
            T = fit_ref.tree_of(mnv, tree)
            wmax, sums, fw = ref.rays_visibility(T, opt, L["o"], L["d"], L["tmax"])
            data, child = T["data"].reshape(T["capacity"], 8, -1), T["child"].reshape(-1, 8)
            cache[name] = dict(tree=tree, T=T, opt=opt, L=L, wmax=wmax, sums=sums, fw=fw, data=data, child=child, cull0=ref.tree_cull(data, child, wmax, 0.0))
        return cache[name]

    return get


def _oracle(mnv, orc, t, data, child, sel=None):
    """the oracle's pixels of the listed rays on a tree with t's format and transform and the given arrays"""
    hv = t["tree"].host_view()
    host = mnv.N3Tree.from_arrays(np.ascontiguousarray(data), np.ascontiguousarray(child, np.int32), data_format=t["tree"].data_format, offset=tuple(hv.offset),
                                  scale=tuple(hv.scale))
    L = t["L"]
    sel = np.arange(L["o"].shape[0]) if sel is None else sel
    return rays_ref.oracle_rays(orc, orc.tree_from_view(host.host_view()), L["o"][sel], L["d"][sel], t["opt"], None if L["tmax"] is None else L["tmax"][sel])[0]


def _oracle_rays_of(name, n):
    """the rays the oracle takes (it takes no degenerate ray: fit_cases.hand_rays' first four)"""
    n_frame = fit_cases.FRAME ** 2
    return np.arange(n) if name == "wall" else np.r_[0:n_frame, n_frame + 4:n]


@pytest.mark.parametrize("name", vc.NAMES + ["wall"] + fit_cases.EDGE_NAMES)
def test_the_weights_are_the_oracles(mnv, orc, truth, name):
    t = truth(name)
    T, L = t["T"], t["L"]
    # the same topology and densities with RGBA rows whose colours are all 1: every term of a pixel is c * w = w
    ones = np.full((T["capacity"] * 8, 4), 0x3C00, np.uint16)
    ones[:, 3] = T["data"][:, T["data_dim"] - 1]
    U = dict(T, data=ones, data_dim=4, basis=-1)
    opt = fit_cases.make_options(mnv, name) if name != "wall" else mnv.RenderOptions.defaults()
    opt.background_brightness = 0.0
    fw1 = fit_ref.forward(U, opt, L["o"], L["d"], L["tmax"])
    assert len(fw1["batches"]) == len(t["fw"]["batches"]) > 0
    for a, b in zip(fw1["batches"], t["fw"]["batches"]):                  # the march does not depend on colour
        assert np.array_equal(a["ray"], b["ray"]) and np.array_equal(a["vox"], b["vox"]) and np.array_equal(bits(a["w"]), bits(b["w"]))
    S = np.zeros(L["o"].shape[0], np.float32)
    for b in t["fw"]["batches"]:
        S[b["ray"]] = S[b["ray"]] + b["w"]
    with np.errstate(all="ignore"):
        red = np.where(t["fw"]["stopped"], S * t["fw"]["scale"], S).astype(np.float32)
    assert np.array_equal(bits(red), bits(fw1["rgba"][:, 0]))             # ... whose red channel is the sum of the restatement's weights
    sel = _oracle_rays_of(name, L["o"].shape[0])
    host = mnv.N3Tree.from_arrays(ones.reshape(-1, 8, 4), T["child"].reshape(-1, 8), data_format="RGBA", offset=tuple(T["offset"]), scale=tuple(T["scale"]))
    want, _ = rays_ref.oracle_rays(orc, orc.tree_from_view(host.host_view()), L["o"][sel], L["d"][sel], opt, None if L["tmax"] is None else L["tmax"][sel])
    assert np.array_equal(bits(fw1["rgba"][sel]), bits(want))             # ... and the oracle's pixel
    assert t["sums"]["n_skipped"] == 0 and t["sums"]["n_rays"] == L["o"].shape[0] and t["sums"]["n_samples"] == sum(b["ray"].size for b in t["fw"]["batches"])


@pytest.mark.parametrize("name", fit_cases.EDGE_NAMES)
def test_the_forward_is_the_fitting_restatements_on_the_edge_cases(mnv, truth, name):
    """wide rows, scales that differ per axis: the march under the weights is fit_ref's own, which tests/test_fit_ref.py holds against the
    oracle on these cases, and the words are the maxima of its weights"""
    t = truth(name)
    L = t["L"]
    fw = fit_ref.forward(t["T"], t["opt"], L["o"], L["d"], L["tmax"])
    assert np.array_equal(bits(fw["rgba"]), bits(t["fw"]["rgba"])) and len(fw["batches"]) == len(t["fw"]["batches"])
    want = np.zeros(t["T"]["capacity"] * 8, np.float32)
    for b in fw["batches"]:
        np.maximum.at(want, b["vox"], b["w"])
    assert np.array_equal(t["wmax"], want.view(np.uint32)) and np.count_nonzero(want) >= 40
    assert t["sums"] == dict(n_rays=L["o"].shape[0], n_stopped=int(fw["stopped"].sum()), n_samples=int(fw["n_dense"].sum()), n_skipped=0)


def test_the_comparison_with_the_threshold_is_strict(truth):
    t = truth("sh9_d4")
    words = np.unique(t["wmax"][t["wmax"] != 0])
    tie = words[words.size // 2]
    v = int(np.nonzero(t["wmax"] == tie)[0][0])
    thresh = np.array([tie], np.uint32).view(np.float32)[0]
    at = ref.tree_cull(t["data"], t["child"], t["wmax"], thresh)
    below = ref.tree_cull(t["data"], t["child"], t["wmax"], np.nextafter(thresh, np.float32(0.0)))
    assert not at["data"].reshape(-1, t["T"]["data_dim"])[v].any()              # wmax == weight_thresh: not seen
    assert np.array_equal(below["data"].reshape(-1, t["T"]["data_dim"])[v], t["T"]["data"][v]) and t["T"]["data"][v].any()
    assert below["counts"]["leaves_seen"] == at["counts"]["leaves_seen"] + int((t["wmax"] == tie).sum())
    # NaN and negative patterns are not seen, +inf is
    w = np.array([0x7FC00000, 0xFFC00000, 0x80000001, 0xBF800000, 0x7F800000, 0x00000001, 0, 0], np.uint32)
    one = ref.tree_cull(np.full((1, 8, 4), 0x3C00, np.uint16), np.zeros((1, 8), np.int32), w, 0.0)
    assert (one["data"][0] != 0).all(axis=1).tolist() == [False, False, False, False, True, True, False, False] and one["keep"].tolist() == [1]
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="invalid"):
            ref.tree_cull(t["data"], t["child"], t["wmax"], bad)


@pytest.mark.parametrize("name", vc.NAMES + ["wall"])
def test_the_kept_set_is_parent_closed_and_the_rows_are_what_the_contract_says(truth, name):
    t = truth(name)
    depth, at_depth = lod_ref.chunk_depths(t["child"])
    for thresh in (0.0, 1e-3, vc.MIXED_THRESH, 1e-1, 10.0):
        c = ref.tree_cull(t["data"], t["child"], t["wmax"], thresh)
        assert ref.parent_closed(t["child"], c["keep"]) and c["keep"][0] == 1
        assert c["kept_at_depth"].sum() == c["keep"].sum() and c["counts"]["dead_chunks"] == t["T"]["capacity"] - c["keep"].sum()
        assert np.array_equal(c["kept_at_depth"], np.bincount(depth[c["keep"] != 0], minlength=24))
        zero = ~c["data"].any(axis=2)
        assert np.array_equal(c["data"][~zero], t["data"][~zero])               # a row is copied bit for bit or zero
        leaf = t["child"] == 0
        with np.errstate(invalid="ignore"):
            seen = t["wmax"].view(np.float32).reshape(-1, 8) > np.float32(thresh)
        assert zero[leaf & ~seen].all() and np.array_equal(zero[leaf & seen], ~t["data"][leaf & seen].any(axis=1))
        rows, cols = np.nonzero(t["child"])
        below = rows + t["child"][rows, cols]
        assert np.array_equal(zero[rows, cols] | ~t["data"][rows, cols].any(axis=1), (c["keep"][below] == 0) | ~t["data"][rows, cols].any(axis=1))
    assert c["keep"].sum() == 1 and not c["data"].any()                         # nothing weighs 10: the root alone, all rows zero


@pytest.mark.parametrize("name", vc.NAMES + ["wall"])
def test_threshold_zero_changes_no_listed_ray(mnv, orc, truth, name):
    t = truth(name)
    assert t["opt"].sigma_thresh >= 0 and t["opt"].stop_thresh >= 2.0 ** -24
    sel = _oracle_rays_of(name, t["L"]["o"].shape[0])
    source = _oracle(mnv, orc, t, t["data"], t["child"], sel)
    culled = _oracle(mnv, orc, t, t["cull0"]["data"], t["child"], sel)
    assert np.array_equal(bits(culled), bits(source))
    if "_d4" in name or name == "wall":
        assert (t["cull0"]["data"] != t["data"]).any()


@pytest.mark.parametrize("name", sorted(MIXED))
def test_the_scenes_are_mixed(truth, name):
    t = truth(name)
    c = ref.tree_cull(t["data"], t["child"], t["wmax"], vc.MIXED_THRESH)
    seen, culled, dead, kept = MIXED[name]
    assert (c["counts"]["leaves_seen"], c["counts"]["leaves_culled"], c["counts"]["dead_chunks"]) == (seen, culled, dead)
    assert c["kept_at_depth"][1:len(kept) + 1].tolist() == kept and c["kept_at_depth"].sum() == sum(kept)
    assert dead >= 1 and culled >= 1 and c["keep"].sum() > 1                    # dead chunks, culled non-empty leaves, live chunks
    full = lod_ref.half_value(t["data"][:, :, -1]) > 0
    assert (full & (t["child"] == 0) & c["data"].any(axis=2)).any()             # non-empty leaves that were seen
    if name == "wall":
        depth, _ = lod_ref.chunk_depths(t["child"])
        assert sorted(set(depth[c["keep"] == 0].tolist())) == [2, 3, 4]         # dead chunks at three depths
        assert t["fw"]["n_dense"].max() == 1 and t["sums"]["n_stopped"] == t["sums"]["n_samples"] > 1000     # one sample ends a ray


@pytest.mark.parametrize("name", sorted(CUT_DIFF))
def test_frames_of_the_cut_tree_are_close_to_the_sources(mnv, orc, truth, name):
    t = truth(name)
    sel = _oracle_rays_of(name, t["L"]["o"].shape[0])
    cut = ref.make_culled(t["T"], t["opt"], [(t["L"]["o"], t["L"]["d"], t["L"]["tmax"])], 0.0)["cut"]
    assert cut["capacity"] < t["T"]["capacity"]
    source = _oracle(mnv, orc, t, t["data"], t["child"], sel)
    after = _oracle(mnv, orc, t, cut["data"], cut["child"], sel)
    diff = float(np.abs(after.astype(np.float64) - source.astype(np.float64)).max())
    print(f"{name}: {t['T']['capacity']} -> {cut['capacity']} chunks, largest channel difference of the cut tree's pixels = {diff:.3g}")
    assert diff == CUT_DIFF[name]
