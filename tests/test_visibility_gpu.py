"""Culling on the device (csrc/mnv_visibility.hip: mnv_rays_visibility, mnv_tree_cull; N3Tree.make_culled) against tests/visibility_ref.py,
the numpy restatement of the contract in include/mnv.h: the words of wmax and the sums equal the restatement word for word in any ray
order, image layout, split over calls, under full contention and on top of earlier contents -- also on trees whose scale differs per axis,
with links that leave the tree, with more tiles than workgroups and with ragged tiles (the edge cases of tests/fit_cases.py);
mnv_tree_cull equals it byte for byte on hand-made words (NaN patterns, ties, renumbered trees, unreached chunks, chains); the cut tree's frames equal the oracle's three ways; at
threshold 0 the culled rows change no listed ray; refusals come before any launch.  No tolerance but the one measured bound on the cut
tree's frames (tests/test_visibility_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import cases
import fit_cases
import fit_ref
import rays_ref
import test_lod_gpu as L
import test_visibility_ref as R
import view_lod_ref
import visibility_cases as vc
import visibility_ref as ref

pytestmark = pytest.mark.gpu
bits = cases.bits
GUARD = 64          # elements behind every output that must keep their pattern


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _vis(mnv, torch, view, opt, o, d, tmax=None, wmax=None):
    """mnv_rays_visibility on host rays -> (wmax uint32 [capacity * 8], sums dict); wmax: a device tensor to take the maxima into"""
    if wmax is None:
        wmax = torch.zeros((view.capacity * 8,), dtype=torch.int32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    mnv.rays_visibility(view, _dev(torch, o), _dev(torch, d), opt, wmax, sums, tmax=_dev(torch, tmax))
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    assert not s[4:].any()
    return _u32(wmax), dict(zip(ref.VIS_SUMS, (int(x) for x in s[:4])))


@pytest.fixture(scope="module")
def truth(mnv):
    """per case: the tree on the device, its arrays, options, rays and the restatement's words -- computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            tree, opt, Lr = R.scene(mnv, name)
            T = fit_ref.tree_of(mnv, tree)
            wmax, sums, fw = ref.rays_visibility(T, opt, Lr["o"], Lr["d"], Lr["tmax"])
            tree.move_to_device(need_parent=True, need_sample_counts=True)
            cache[name] = dict(tree=tree, T=T, opt=opt, L=Lr, wmax=wmax, sums=sums, fw=fw, data=T["data"].reshape(T["capacity"], 8, -1),
                               child=T["child"].reshape(-1, 8))
        return cache[name]

    return get


# ---------------------------------------------------------------------------------------------------- mnv_rays_visibility

@pytest.mark.parametrize("name", vc.NAMES + ["wall"])
def test_words_and_sums_equal_the_restatement(mnv, torch_gpu, truth, name):
    t = truth(name)
    Lr = t["L"]
    wmax, sums = _vis(mnv, torch_gpu, t["tree"].device_view(), t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    assert sums == t["sums"] and t["sums"]["n_samples"] > 0 and np.count_nonzero(t["wmax"]) > 0
    bad = np.nonzero(wmax != t["wmax"])[0]
    assert bad.size == 0, f"{bad.size} of {int((t['wmax'] != 0).sum())} non-zero words differ; first at {bad[:4].tolist()}"
    assert np.array_equal(np.array(t["tree"].host_arrays()[0]).reshape(-1, t["T"]["data_dim"]), t["T"]["data"])


@pytest.mark.parametrize("name", ["sh9_d4", "rgba_d1"])
def test_layout_order_split_calls_and_earlier_contents(mnv, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    Lr, v = t["L"], t["tree"].device_view()
    perm = np.random.default_rng(5).permutation(Lr["o"].shape[0])
    wmax, sums = _vis(mnv, torch, v, t["opt"], Lr["o"][perm], Lr["d"][perm], Lr["tmax"][perm])
    assert np.array_equal(wmax, t["wmax"]) and sums == t["sums"]
    # the same rays as a 20 x 32 image: 8 x 8 ray tiles instead of 64 x 1
    wmax, sums = _vis(mnv, torch, v, t["opt"], Lr["o"].reshape(20, 32, 3), Lr["d"].reshape(20, 32, 3), Lr["tmax"].reshape(20, 32))
    assert np.array_equal(wmax, t["wmax"]) and sums == t["sums"]
    # two calls into one array
    both = torch.zeros((v.capacity * 8,), dtype=torch.int32, device="cuda")
    h = 300
    _, s1 = _vis(mnv, torch, v, t["opt"], Lr["o"][:h], Lr["d"][:h], Lr["tmax"][:h], wmax=both)
    wmax, s2 = _vis(mnv, torch, v, t["opt"], Lr["o"][h:], Lr["d"][h:], Lr["tmax"][h:], wmax=both)
    assert np.array_equal(wmax, t["wmax"]) and {k: s1[k] + s2[k] for k in s1} == t["sums"]
    # earlier contents: the maximum with them holds, as unsigned integers (words above every weight stay)
    rng = np.random.default_rng(6)
    before = rng.integers(0, 1 << 32, size=v.capacity * 8, dtype=np.uint64).astype(np.uint32)
    before[rng.uniform(size=before.size) < 0.5] = 0
    before[::3] >>= 3
    wmax, _ = _vis(mnv, torch, v, t["opt"], Lr["o"], Lr["d"], Lr["tmax"], wmax=_dev(torch, before.view(np.int32)))
    want = np.maximum(before, t["wmax"])
    assert np.array_equal(wmax, want) and (want != before).any() and (want != t["wmax"]).any()


def test_4096_copies_of_one_ray_onto_the_same_words(mnv, torch_gpu, truth):
    t = truth("sh4_d4")
    i = int(np.argmax(t["fw"]["n_dense"]))
    assert t["fw"]["n_dense"][i] >= 3
    o, d = np.tile(t["L"]["o"][i], (4096, 1)), np.tile(t["L"]["d"][i], (4096, 1))
    tmax = np.full(4096, t["L"]["tmax"][i], np.float32)
    want, want_sums, _ = ref.rays_visibility(t["T"], t["opt"], o[:1], d[:1], tmax[:1])
    wmax, sums = _vis(mnv, torch_gpu, t["tree"].device_view(), t["opt"], o, d, tmax)
    assert np.array_equal(wmax, want) and sums == {k: 4096 * x for k, x in want_sums.items()} and np.count_nonzero(want) >= 3


# ---- the edge cases of tests/fit_cases.py: scales that differ per axis, wide rows, links that leave the tree, more tiles than workgroups,
# ragged tiles.  tests/test_fit_ref.py and tests/test_visibility_ref.py say what each input contains.

@pytest.mark.parametrize("name", fit_cases.EDGE_NAMES)
def test_edge_cases_equal_the_restatement_word_for_word(mnv, torch_gpu, truth, name):
    t = truth(name)
    Lr, v = t["L"], t["tree"].device_view()
    wmax, sums = _vis(mnv, torch_gpu, v, t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    assert sums == t["sums"] and t["sums"]["n_samples"] >= 500 and np.count_nonzero(t["wmax"]) >= 40
    bad = np.nonzero(wmax != t["wmax"])[0]
    assert bad.size == 0, f"{bad.size} of {int((t['wmax'] != 0).sum())} non-zero words differ; first at {bad[:4].tolist()}"
    wmax, sums = _vis(mnv, torch_gpu, v, t["opt"], Lr["o"].reshape(20, 32, 3), Lr["d"].reshape(20, 32, 3), Lr["tmax"].reshape(20, 32))
    assert np.array_equal(wmax, t["wmax"]) and sums == t["sums"]


def test_links_that_leave_the_tree_skip_their_rays(mnv, torch_gpu, truth):
    """fit_cases.broken_links: links to chunk 0, to chunks at and above the view's capacity (all inside the allocated arrays) -- chunk 151,
    the first one outside, among them: a ray that meets one adds nothing, the others' words are the restatement's"""
    torch = torch_gpu
    t = truth(fit_cases.BROKEN["tree"])
    T, Lr = fit_cases.broken_links(t["T"], t["L"])
    want, want_sums, fw = ref.rays_visibility(T, t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    n_in = fit_cases.BROKEN["inside"]
    assert want_sums["n_skipped"] >= 20 + n_in and fw["broken"][-n_in:].all() and np.count_nonzero(want) >= 100
    v, data_t, child_t = fit_cases.hand_view(mnv, torch, T)
    assert v.capacity == fit_cases.BROKEN["capacity"] and child_t.numel() > v.capacity * 8
    words = torch.zeros((child_t.numel(),), dtype=torch.int32, device="cuda")          # a word for every allocated voxel
    wmax, sums = _vis(mnv, torch, v, t["opt"], Lr["o"], Lr["d"], Lr["tmax"], wmax=words)
    assert sums == want_sums
    assert np.array_equal(wmax[:want.size], want) and not wmax[want.size:].any()


@pytest.mark.parametrize("name", ["sh9_d4", "sh25_d3"])
def test_more_tiles_than_workgroups(mnv, torch_gpu, truth, name):
    """420 copies of the case's 640 rays and its first 37 again: 268,837 rays in 4201 flat tiles, more than the 4096 workgroups of the
    launch, so workgroups walk on to a second tile, the last of which has 37 rays; and the 268,800 as a 32 x 8400 image (4200 tiles of
    8 x 8).  The words are maxima: unchanged.  The sums multiply."""
    t = truth(name)
    Lr, v = t["L"], t["tree"].device_view()
    copies, tail = 420, 37
    o, d, tmax = (np.concatenate([np.tile(a, (copies,) + (1,) * (a.ndim - 1)), a[:tail]]) for a in (Lr["o"], Lr["d"], Lr["tmax"]))
    assert o.shape[0] == 268837
    _, sums_tail, _ = ref.rays_visibility(t["T"], t["opt"], Lr["o"][:tail], Lr["d"][:tail], Lr["tmax"][:tail])
    assert sums_tail["n_samples"] > 0
    wmax, sums = _vis(mnv, torch_gpu, v, t["opt"], o, d, tmax)
    assert np.array_equal(wmax, t["wmax"]) and sums == {k: copies * t["sums"][k] + sums_tail[k] for k in sums}
    n = copies * 640
    wmax, sums = _vis(mnv, torch_gpu, v, t["opt"], o[:n].reshape(8400, 32, 3), d[:n].reshape(8400, 32, 3), tmax[:n].reshape(8400, 32))
    assert np.array_equal(wmax, t["wmax"]) and sums == {k: copies * x for k, x in t["sums"].items()}


@pytest.mark.parametrize("shape", [(13, 7), (7, 13), (65,)], ids=["7x13", "13x7", "flat65"])
def test_ragged_tiles(mnv, torch_gpu, truth, shape):
    """images narrower than a tile and of no multiple of 8 (7 wide x 13 high, 13 x 7), a flat list that ends one ray into its second tile"""
    t = truth("sh9_d4")
    n = int(np.prod(shape))
    o, d, tmax = t["L"]["o"][:n], t["L"]["d"][:n], t["L"]["tmax"][:n]
    want, want_sums, _ = ref.rays_visibility(t["T"], t["opt"], o, d, tmax)
    assert want_sums["n_rays"] == n and want_sums["n_samples"] >= 20
    wmax, sums = _vis(mnv, torch_gpu, t["tree"].device_view(), t["opt"], o.reshape(shape + (3,)), d.reshape(shape + (3,)), tmax.reshape(shape))
    assert np.array_equal(wmax, want) and sums == want_sums


# ---------------------------------------------------------------------------------------------------- mnv_tree_cull

THRESH = np.float32(0.37)


def _words(rng, n, thresh=THRESH):
    """random words: weights in [0, 1), zeros, the exact tie, its neighbours, NaN patterns of both signs, negative values, +-inf"""
    w = rng.uniform(0, 1, size=n).astype(np.float32).view(np.uint32).copy()
    tie = np.array([thresh], np.float32).view(np.uint32)[0]
    special = np.array([0, 0, 0, tie, tie, tie + 1, tie - 1, 0x7FC00000, 0x7F800001, 0xFFC00000, 0xBF000000, 0x80000000, 0x7F800000, 0xFF800000, 1], np.uint32)
    hit = rng.uniform(size=n) < 0.45
    w[hit] = rng.choice(special, size=int(hit.sum()))
    return w


def _cull(mnv, torch, data, child, wmax, thresh):
    """(data_out, keep, kept_at_depth, counts) of mnv_tree_cull; the inputs must come back unchanged, nothing is written behind the outputs"""
    cap, _, dd = data.shape
    data_t, child_t, w_t = L._dev(torch, data), L._dev(torch, child), _dev(torch, wmax.view(np.int32))
    out_t = torch.full((cap + GUARD, 8, dd), 0x5555, dtype=torch.int16, device="cuda")
    keep_t = torch.full((cap + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    kept, counts = mnv.tree_cull(L._view(mnv, data_t, child_t, dd), w_t, float(thresh), out_t, keep_t)
    out, keep = L._host16(out_t), keep_t.cpu().numpy()
    assert (out[cap:] == 0x5555).all() and (keep[cap:] == 0x55).all()
    assert np.array_equal(L._host16(data_t), data) and np.array_equal(child_t.cpu().numpy(), child) and np.array_equal(_u32(w_t), wmax)
    return out[:cap], keep[:cap], kept, counts


def _check_cull(mnv, torch, data, child, wmax, thresh=THRESH):
    want = ref.tree_cull(data, child, wmax, thresh)
    out, keep, kept, counts = _cull(mnv, torch, data, child, wmax, thresh)
    assert counts == want["counts"], (counts, want["counts"])
    assert np.array_equal(kept, want["kept_at_depth"]), (kept, want["kept_at_depth"])
    assert np.array_equal(keep, want["keep"]), np.nonzero(keep != want["keep"])[0][:8]
    bad = np.argwhere(out != want["data"])
    assert bad.size == 0, (bad[:5], out[tuple(bad[0])], want["data"][tuple(bad[0])])
    return want


@pytest.mark.parametrize("dd", [4, 28, 76])
def test_cull_on_hand_made_words(mnv, torch_gpu, dd):
    data, child = L._random_tree(60 + dd, 6, dd, 0.45)
    cap = child.shape[0]
    assert 250 < cap < 1600
    rng = np.random.default_rng(dd)
    wmax = _words(rng, cap * 8)
    wmax[rng.uniform(size=cap * 8) < 0.5] = 0                                    # enough unseen leaves for whole chunks to die
    want = _check_cull(mnv, torch_gpu, data, child, wmax)
    c = want["counts"]
    assert c["dead_chunks"] >= 10 and c["leaves_seen"] >= 100 and c["leaves_culled"] >= 100 and 1 < want["keep"].sum() < cap
    assert ref.parent_closed(child, want["keep"])
    _check_cull(mnv, torch_gpu, data, child, wmax, 0.0)                           # threshold 0: every positive word counts, the smallest too


def test_cull_does_not_rely_on_chunk_order(mnv, torch_gpu):
    data, child = L._random_tree(21, 6, 13)
    rng = np.random.default_rng(21)
    wmax = _words(rng, child.shape[0] * 8)
    wmax[rng.uniform(size=wmax.size) < 0.5] = 0
    plain = _check_cull(mnv, torch_gpu, data, child, wmax)
    cap = child.shape[0]
    new = np.concatenate([[0], cap - np.arange(1, cap)]).astype(np.int64)
    data2, child2 = L._renumbered(data, child)
    assert (child2[1:][child2[1:] != 0] < 0).all()                               # every link below the root points backwards
    w2 = np.empty_like(wmax).reshape(cap, 8)
    w2[new] = wmax.reshape(cap, 8)
    moved = _check_cull(mnv, torch_gpu, data2, child2, w2.reshape(-1))
    assert np.array_equal(moved["keep"][new], plain["keep"]) and plain["counts"]["dead_chunks"] >= 5


def test_cull_copies_unreached_chunks_and_keeps_none_of_them(mnv, torch_gpu):
    data, child = L._with_unreached(*L._random_tree(22, 5, 28))
    rng = np.random.default_rng(22)
    wmax = _words(rng, child.shape[0] * 8)
    wmax[-24:] = np.float32(0.9).view(np.uint32)                                  # words of unreached chunks decide nothing
    want = _check_cull(mnv, torch_gpu, data, child, wmax)
    assert want["keep"][-3:].tolist() == [0, 0, 0] and np.array_equal(want["data"][-3:], data[-3:])


def test_cull_of_a_single_chunk_and_of_chains_fourteen_deep(mnv, torch_gpu):
    data, child = L._random_tree(0, 1, 28)
    want = _check_cull(mnv, torch_gpu, data, child, np.zeros(8, np.uint32))       # everything culled: the root stays, the rows are zero
    assert want["keep"].tolist() == [1] and not want["data"].any() and want["kept_at_depth"].tolist() == [0, 1] + [0] * 22
    data, child = L._chain()
    seen = np.float32(0.5).view(np.uint32)
    wmax = np.zeros(14 * 8, np.uint32)
    want = _check_cull(mnv, torch_gpu, data, child, wmax)                         # dies from the bottom up
    assert want["keep"].tolist() == [1] + [0] * 13 and not want["data"].any() and want["counts"]["dead_chunks"] == 13
    wmax[13 * 8 + 6] = seen                                                       # the deepest chunk's leaf 6 is seen: nothing dies
    want = _check_cull(mnv, torch_gpu, data, child, wmax)
    assert want["keep"].all() and want["kept_at_depth"][1:15].tolist() == [1] * 14 and want["counts"]["leaves_seen"] == 1
    for c in range(13):                                                           # the chain's interior rows stay bit for bit, every other leaf is zero
        assert np.array_equal(want["data"][c, c % 8], data[c, c % 8]) and not np.delete(want["data"][c], c % 8, axis=0).any()
    wmax[13 * 8 + 6] = 0
    wmax[5 * 8 + 7] = seen                                                        # a leaf half way: what is below dies, what is above lives
    want = _check_cull(mnv, torch_gpu, data, child, wmax)
    assert want["keep"].tolist() == [1] * 6 + [0] * 8


def test_cull_then_cut_equals_the_restatement(mnv, torch_gpu):
    torch = torch_gpu
    dd = 28
    data, child = L._random_tree(77, 6, dd, 0.45)
    cap = child.shape[0]
    rng = np.random.default_rng(77)
    wmax = _words(rng, cap * 8)
    wmax[rng.uniform(size=cap * 8) < 0.5] = 0
    sc = rng.integers(-100, 3000, size=(cap, 8)).astype(np.int16)
    cull = ref.tree_cull(data, child, wmax, THRESH)
    want = view_lod_ref.cut(cull["data"], child, cull["keep"], sc)
    n = want["capacity"]
    assert 8 < n < cap
    data_t, child_t, sc_t, w_t = L._dev(torch, data), L._dev(torch, child), L._dev(torch, sc), _dev(torch, wmax.view(np.int32))
    out_t = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    keep_t = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    kept, _ = mnv.tree_cull(L._view(mnv, data_t, child_t, dd, counts_t=sc_t), w_t, float(THRESH), out_t, keep_t)
    assert int(kept.sum()) == n
    o = dict(child=torch.full((n + GUARD, 8), 0x55555555, dtype=torch.int32, device="cuda"), data=torch.full((n + GUARD, 8, dd), 0x5555, dtype=torch.int16, device="cuda"),
             parent=torch.full((n + GUARD,), 0x55555555, dtype=torch.int32, device="cuda"), sample_counts=torch.full((n + GUARD, 8), 0x5555, dtype=torch.int16, device="cuda"))
    mnv.tree_cut(L._view(mnv, out_t, child_t, dd, counts_t=sc_t), keep_t, n, o["child"], o["data"], o["parent"], o["sample_counts"])
    torch.cuda.synchronize()
    for k, t in o.items():
        a = t.cpu().numpy()
        a = a.view(np.uint16) if k == "data" else a
        assert np.array_equal(a[:n], want[k]), k
        assert (a[n:] == (0x5555 if a.dtype.itemsize == 2 else 0x55555555)).all(), k
    # the voxel above a dead chunk became an empty leaf
    rows, cols = np.nonzero(child)
    dead_above = (cull["keep"][rows] != 0) & (cull["keep"][rows + child[rows, cols]] == 0)
    assert dead_above.any() and (want["child"] == 0).sum() > (child[cull["keep"] != 0] == 0).sum()


def test_refusals_come_before_any_launch(mnv, torch_gpu, truth):
    torch = torch_gpu
    lib = mnv.lib()
    t = truth("sh4_d4")
    Lr, v = t["L"], t["tree"].device_view()
    o, d = _dev(torch, Lr["o"]), _dev(torch, Lr["d"])
    wmax = torch.zeros((v.capacity * 8,), dtype=torch.int32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    n = Lr["o"].shape[0]

    def changed(obj, **kw):
        c = type(obj)()
        C.memmove(C.byref(c), C.byref(obj), C.sizeof(c))
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    def vis(view=v, opt=t["opt"], width=n, height=1, w_p=wmax.data_ptr(), s_p=sums.data_ptr(), o_p=o.data_ptr()):
        return lib.mnv_rays_visibility(C.byref(view), o_p, d.data_ptr(), None, width, height, C.byref(opt), w_p, s_p, None)

    assert vis(opt=changed(t["opt"], render_depth=True)) == mnv.MNV_E_UNSUPPORTED
    assert vis(view=changed(v, N=3)) == mnv.MNV_E_UNSUPPORTED
    assert vis(view=changed(v, basis_dim=2)) == mnv.MNV_E_UNSUPPORTED
    assert vis(view=changed(v, basis_dim=9)) == mnv.MNV_E_INVALID                  # data_dim 13 cannot hold SH9 rows
    for step in (0.0, -1e-4, float("nan"), float("inf")):
        assert vis(opt=changed(t["opt"], step_size=step)) == mnv.MNV_E_INVALID, step
    assert b"step_size" in lib.mnv_last_error()
    assert vis(width=(1 << 22) + 1) == mnv.MNV_E_INVALID and vis(width=2049, height=2048) == mnv.MNV_E_INVALID
    assert vis(width=0) == mnv.MNV_E_INVALID and vis(w_p=None) == mnv.MNV_E_INVALID and vis(s_p=None) == mnv.MNV_E_INVALID and vis(o_p=None) == mnv.MNV_E_INVALID
    assert vis(s_p=sums.data_ptr() + 4) == mnv.MNV_E_INVALID and vis(w_p=wmax.data_ptr() + 2) == mnv.MNV_E_INVALID
    assert vis(view=changed(v, capacity=0)) == mnv.MNV_E_INVALID
    torch.cuda.synchronize()
    assert not wmax.cpu().numpy().any() and not sums.cpu().numpy().any()            # nothing ran

    # mnv_tree_cull
    data, child = L._random_tree(41, 5, 4, 0.5)
    cap = child.shape[0]
    assert cap > 100
    data_t, child_t = L._dev(torch, data), L._dev(torch, child)
    w_t = torch.zeros((cap * 8,), dtype=torch.int32, device="cuda")
    out_t = torch.full((cap * 8 * 4 + 8,), 0x5555, dtype=torch.int16, device="cuda")
    keep_t = torch.full((cap,), 0x55, dtype=torch.uint8, device="cuda")
    kept, counts = (C.c_int64 * 24)(), mnv.CullCounts()
    tv = L._view(mnv, data_t, child_t, 4)

    host_w, host_keep = np.zeros(cap * 8, np.uint32), np.zeros(cap, np.uint8)

    def cull(view=tv, w=w_t.data_ptr(), thresh=0.0, rows=out_t.data_ptr(), keep=keep_t.data_ptr(), at=kept, cc=C.byref(counts)):
        return lib.mnv_tree_cull(C.byref(view) if view is not None else None, w, thresh, rows, keep, at, cc, None)

    for kw in (dict(view=None), dict(w=None), dict(rows=None), dict(keep=None), dict(at=None), dict(cc=None),
               dict(thresh=-1e-6), dict(thresh=float("nan")), dict(thresh=float("inf")),
               dict(rows=out_t.data_ptr() + 2), dict(w=w_t.data_ptr() + 2),                                 # misaligned
               dict(rows=data_t.data_ptr()), dict(rows=data_t.data_ptr() + 16), dict(keep=w_t.data_ptr()), dict(keep=child_t.data_ptr() + 5),   # overlapping
               dict(w=host_w.ctypes.data), dict(keep=host_keep.ctypes.data),                                  # host arrays
               dict(view=L._view(mnv, data_t, child_t, 1))):
        assert cull(**kw) == mnv.MNV_E_INVALID, kw
    host_child = np.ascontiguousarray(child)
    hv = L._view(mnv, data_t, child_t, 4)
    hv.child = host_child.ctypes.data
    assert cull(view=hv) == mnv.MNV_E_INVALID
    assert cull(view=changed(tv, N=3)) == mnv.MNV_E_UNSUPPORTED and cull(view=changed(tv, data_dim=1032)) == mnv.MNV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out_t.cpu().numpy() == 0x5555).all() and (keep_t.cpu().numpy() == 0x55).all()   # nothing ran
    # the links: chunk 0, capacity, a chunk that has a parent already
    leaf = np.argwhere(child[2:] == 0)[0]
    c, j = int(leaf[0]) + 2, int(leaf[1])
    for link in (-c, cap - c, 1 - c):
        bad = child.copy()
        bad[c, j] = link
        assert cull(view=L._view(mnv, data_t, L._dev(torch, bad), 4)) == mnv.MNV_E_INVALID, link
        with pytest.raises(ValueError, match="invalid"):
            ref.tree_cull(data, bad, np.zeros(cap * 8, np.uint32), 0.0)
    deep = L._chain(levels=24)[1]
    dv = L._view(mnv, torch.zeros((24, 8, 4), dtype=torch.int16, device="cuda"), L._dev(torch, deep), 4)
    assert cull(view=dv) == mnv.MNV_E_UNSUPPORTED                                   # more than 23 levels
    assert cull() == 0 and keep_t.cpu().numpy().tolist() == [1] + [0] * (cap - 1)   # no word set: the root alone
    host_only = cases.make_tree(mnv, fit_cases.TREES["sh1_d1"])
    with pytest.raises(mnv.MnvError) as e:
        host_only.make_culled([fit_cases.frame_camera(mnv)], t["opt"], 0.0)        # not on the device
    assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        t["tree"].make_culled([fit_cases.frame_camera(mnv)], t["opt"], -1.0)
    assert e.value.code == mnv.MNV_E_INVALID


# ---------------------------------------------------------------------------------------------------- frames

def _rays_frame(mnv, torch, tree, opt, o, d, tmax=None):
    """mnv_render_rays_accel of a device tree on host rays: float32 [n, 4]"""
    out = torch.full((o.shape[0], 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_rays_accel(tree.accel, _dev(torch, o), _dev(torch, d), opt, rgba=out, tmax=_dev(torch, tmax))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert not np.isnan(out).any()
    return out


def _on_device(mnv, t, data, child):
    """a tree with t's format and transform and the given arrays, on the device with its accel"""
    hv = t["tree"].host_view()
    tree = mnv.N3Tree.from_arrays(np.ascontiguousarray(data), np.ascontiguousarray(child, np.int32), data_format=t["tree"].data_format, offset=tuple(hv.offset),
                                  scale=tuple(hv.scale))
    tree.move_to_device()
    return tree


@pytest.mark.parametrize("name", vc.NAMES + ["wall"])
def test_threshold_zero_changes_no_listed_ray(mnv, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    Lr, v = t["L"], t["tree"].device_view()
    cap, dd = v.capacity, v.data_dim
    wmax = torch.zeros((cap * 8,), dtype=torch.int32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    mnv.rays_visibility(v, _dev(torch, Lr["o"]), _dev(torch, Lr["d"]), t["opt"], wmax, sums, tmax=_dev(torch, Lr["tmax"]))
    out_t = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    keep_t = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    mnv.tree_cull(v, wmax, 0.0, out_t, keep_t)
    culled = L._host16(out_t)
    want = ref.tree_cull(t["data"], t["child"], t["wmax"], 0.0)
    assert np.array_equal(culled, want["data"]) and np.array_equal(keep_t.cpu().numpy(), want["keep"])
    source = _rays_frame(mnv, torch, t["tree"], t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    after = _rays_frame(mnv, torch, _on_device(mnv, t, culled, t["child"]), t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    assert np.array_equal(bits(after), bits(source))
    if "_d4" in name or name == "wall":
        assert (culled != t["data"]).any()


CAMS = {"sh1_d4": (0, 1), "sh9_d4": (0, 2), "rgba_d4": (1, 2)}


@pytest.mark.parametrize("name", sorted(CAMS))
def test_make_culled_and_the_frames_of_the_cut_tree_three_ways(mnv, orc, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    cams = [fit_cases.frame_camera(mnv, fit_cases.FRAME, p) for p in CAMS[name]]
    want = ref.make_culled(t["T"], t["opt"], [vc.camera_rays(c) for c in cams], vc.MIXED_THRESH, np.full((t["T"]["capacity"], 8), 8, np.int16))
    cut, kept, counts = t["tree"].make_culled(cams, t["opt"], vc.MIXED_THRESH)
    assert counts == want["cull"]["counts"] and np.array_equal(kept, want["cull"]["kept_at_depth"])
    assert 1 < cut.capacity == want["cut"]["capacity"] < t["T"]["capacity"] and cut.data_format == t["tree"].data_format
    got_data, got_child, got_parent = cut.host_arrays()
    assert np.array_equal(got_child, want["cut"]["child"]) and np.array_equal(got_data, want["cut"]["data"]) and np.array_equal(got_parent, want["cut"]["parent"])
    assert np.array_equal(np.array(t["tree"].host_arrays()[0]), t["data"])          # the source tree is what it was
    # the chain by hand: the same arrays
    v = t["tree"].device_view()
    cap, dd = v.capacity, v.data_dim
    wmax = torch.zeros((cap * 8,), dtype=torch.int32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    for c in cams:
        o, d = mnv.generate_rays(mnv.PROJ_PINHOLE, c)
        mnv.rays_visibility(v, o, d, t["opt"], wmax, sums)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(wmax), want["wmax"])
    out_t = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    keep_t = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    kept2, _ = mnv.tree_cull(v, wmax, vc.MIXED_THRESH, out_t, keep_t)
    n = int(kept2.sum())
    o_child = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    o_data = torch.empty((n, 8, dd), dtype=torch.int16, device="cuda")
    cv = t["tree"].device_view()
    cv.data = out_t.data_ptr()
    mnv.tree_cut(cv, keep_t, n, o_child, o_data)
    torch.cuda.synchronize()
    assert np.array_equal(o_child.cpu().numpy(), got_child) and np.array_equal(L._host16(o_data), got_data)
    # frames of the cut tree against the oracle on the restated arrays, at a pose of the set and at one that is not in it
    hv = t["tree"].host_view()
    host = mnv.N3Tree.from_arrays(want["cut"]["data"], want["cut"]["child"], data_format=t["tree"].data_format, offset=tuple(hv.offset), scale=tuple(hv.scale))
    for pose in (CAMS[name][0], 3 - sum(CAMS[name])):
        cam = fit_cases.frame_camera(mnv, fit_cases.FRAME, pose)
        oracle = bits(orc.render(orc.tree_from_view(host.host_view()), cam.c, t["opt"])["rgba"]).reshape(-1, 4)
        for packed in (True, False):
            out = torch.full((fit_cases.FRAME, fit_cases.FRAME, 4), float("nan"), dtype=torch.float32, device="cuda")
            if packed:
                mnv.render_voxels_accel(cut.accel, cam, t["opt"], rgba=out)
            else:
                mnv.render_voxels(cut.device_view(), cam, t["opt"], rgba=out)
            torch.cuda.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()).reshape(-1, 4), oracle), (pose, packed)
        o, d = vc.camera_rays(cam)
        assert np.array_equal(bits(_rays_frame(mnv, torch, cut, t["opt"], o, d)), oracle), pose


@pytest.mark.parametrize("name", sorted(R.CUT_DIFF))
def test_frames_of_the_cut_tree_stay_within_the_measured_bound(mnv, torch_gpu, truth, name):
    torch = torch_gpu
    t = truth(name)
    Lr = t["L"]
    want = ref.make_culled(t["T"], t["opt"], [(Lr["o"], Lr["d"], Lr["tmax"])], 0.0)
    # the device's chain on the same list gives the restated cut
    v = t["tree"].device_view()
    cap, dd = v.capacity, v.data_dim
    wmax = torch.zeros((cap * 8,), dtype=torch.int32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    mnv.rays_visibility(v, _dev(torch, Lr["o"]), _dev(torch, Lr["d"]), t["opt"], wmax, sums, tmax=_dev(torch, Lr["tmax"]))
    out_t = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    keep_t = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    kept, _ = mnv.tree_cull(v, wmax, 0.0, out_t, keep_t)
    n = int(kept.sum())
    assert n == want["cut"]["capacity"] < cap
    o_child = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    o_data = torch.empty((n, 8, dd), dtype=torch.int16, device="cuda")
    v.data = out_t.data_ptr()
    mnv.tree_cut(v, keep_t, n, o_child, o_data)
    torch.cuda.synchronize()
    assert np.array_equal(o_child.cpu().numpy(), want["cut"]["child"]) and np.array_equal(L._host16(o_data), want["cut"]["data"])
    source = _rays_frame(mnv, torch, t["tree"], t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    after = _rays_frame(mnv, torch, _on_device(mnv, t, want["cut"]["data"], want["cut"]["child"]), t["opt"], Lr["o"], Lr["d"], Lr["tmax"])
    diff = float(np.abs(after.astype(np.float64) - source.astype(np.float64)).max())
    print(f"{name}: largest channel difference of the cut tree's device pixels = {diff:.3g} (bound {R.CUT_BOUND[name]:.3g})")
    assert diff <= R.CUT_BOUND[name]


# ---------------------------------------------------------------------------------------------------- Renderer.set_cull

W, H, EXE, POSES, FX = L.W, L.H, L.EXE, L.POSES, 224.0
CULL_THRESH = 1e-2


def _cull_cams(mnv, n=2):
    return [mnv.Camera(W, H, FX).set_pose(c, b) for c, b in POSES[:n]]


def test_renderer_with_a_cull_equals_a_renderer_of_the_culled_tree(mnv, torch_gpu):
    spec = cases.CASES["sh4_d6"]["tree"]
    tree, source = cases.make_tree(mnv, spec), cases.make_tree(mnv, spec)
    source.move_to_device()
    a = L._renderer(mnv, tree, tree.capacity)
    cams = _cull_cams(mnv)
    culled, _, counts = source.make_culled(cams, a.options, CULL_THRESH)
    assert 8 < culled.capacity < tree.capacity and counts["dead_chunks"] > 100
    b = L._renderer(mnv, culled, culled.capacity)
    before = L._walk(mnv, a, 3)
    a.set_cull(cams, CULL_THRESH)
    for in_flight in (3, 1):                                                    # in flight, the grid, anti-aliased, orthographic
        got, want = L._walk(mnv, a, in_flight), L._walk(mnv, b, in_flight)
        assert len(got) == len(want) == len(POSES) + 4
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (in_flight, i)
    assert not all(np.array_equal(x, y) for x, y in zip(got, before))          # three of the five poses were not listed
    # another threshold and other cameras: another tree
    fewer, _, _ = source.make_culled(cams[:1], a.options, 0.1)
    assert fewer.capacity < culled.capacity
    c = L._renderer(mnv, fewer, fewer.capacity)
    a.set_cull(cams[:1], 0.1)
    for i, (g, w) in enumerate(zip(L._walk(mnv, a, 3), L._walk(mnv, c, 3))):
        assert np.array_equal(g, w), i
    # other march options: the tree is built again under them
    a.options.stop_thresh = 0.2
    other, _, _ = source.make_culled(cams[:1], a.options, 0.1)
    assert other.capacity < fewer.capacity
    d = L._renderer(mnv, other, other.capacity)
    d.options.stop_thresh = 0.2
    for i, (g, w) in enumerate(zip(L._walk(mnv, a, 3), L._walk(mnv, d, 3))):
        assert np.array_equal(g, w), i
    a.options.stop_thresh = mnv.RenderOptions.cli_defaults().stop_thresh
    a.set_cull([])                                                              # off: byte for byte what it was
    for i, (x, y) in enumerate(zip(L._walk(mnv, a, 3), before)):
        assert np.array_equal(x, y), i
    # a new tree drops the culled one: the same cameras now cull the new tree
    other_tree = mnv.N3Tree.synth_random(depth=6, basis_dim=4, seed=77)
    other_source = mnv.N3Tree.synth_random(depth=6, basis_dim=4, seed=77)
    other_source.move_to_device()
    a.set_cull(cams, CULL_THRESH)
    a.set(other_tree, other_tree.capacity)
    other_culled, _, _ = other_source.make_culled(cams, a.options, CULL_THRESH)
    e = L._renderer(mnv, other_culled, other_culled.capacity)
    for r in (a, e):
        r.options.basis_minmax[0], r.options.basis_minmax[1] = 0, 3
        r.set_camera(*POSES[0], fx=FX)
        r.render()
    assert np.array_equal(bits(a.download_slot(a.last_slot())), bits(e.download_slot(e.last_slot())))


def test_renderer_refuses_a_cull_with_what_edits_the_tree_or_chooses_it_twice(mnv, torch_gpu):
    tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    r = L._renderer(mnv, tree, tree.capacity)
    r.set_camera(*POSES[0], fx=FX)
    cams = _cull_cams(mnv)
    r.set_cull(cams, CULL_THRESH)
    r.render()
    good = bits(r.download_slot(r.last_slot())).copy()

    def refused(word):
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == mnv.MNV_E_INVALID and word in str(e.value)

    r.options.use_splitting = True
    refused("set_cull")
    r.options.use_splitting = False
    r.options.use_guided_sampling = True
    refused("set_cull")
    r.options.use_guided_sampling = False
    r.set_lod(3)
    refused("set_cull")
    r.set_lod(0)
    r.set_view_lod([(POSES[0][0], FX)], 8.0)
    refused("set_cull")
    r.set_view_lod([])
    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)         # one rank through RCCL
    try:
        r.set_ranks(comm)
        refused("set_cull")
        r.set_ranks(None)
    finally:
        r.set_ranks(None)
        comm.close()
    for bad in (dict(weight_thresh=-1.0), dict(weight_thresh=float("nan")), dict(weight_thresh=float("inf")), dict(cams=[mnv.Camera(4096, 2048, FX)])):
        args = dict(cams=cams, weight_thresh=CULL_THRESH)
        args.update(bad)
        with pytest.raises(mnv.MnvError) as e:
            r.set_cull(**args)
        assert e.value.code == mnv.MNV_E_INVALID, bad
    r.render()                                               # the same call renders once the obstacle is gone; refused settings changed nothing
    assert np.array_equal(bits(r.download_slot(r.last_slot())), good)


# ---------------------------------------------------------------------------------------------------- mnv_render --cull

def test_mnv_render_cull_orbit_and_save_lod(mnv, torch_gpu, tmp_path):
    """One pose: the saved tree and the frame are make_culled's for that camera.  An orbit: the poses are the CLI's own, so the saved tree is
    checked through what it must do -- reload, and render the frames the run wrote, pose for pose -- and through the counts the run printed."""
    import os
    import subprocess

    import lod_ref

    torch = torch_gpu
    assert os.path.exists(EXE), "mnv_render not built"
    EYE, BACK = POSES[0]
    tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
    npz, saved, out = str(tmp_path / "scene.npz"), str(tmp_path / "culled.npz"), str(tmp_path / "frame")
    tree.save_npz(npz)
    pose = ["-w", str(W), "-h", str(H), "--fx", "224", "--center", ",".join(map(str, EYE)), "--back", ",".join(map(str, BACK))]
    common = [EXE, npz] + pose

    def run(cmd):
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120)

    r = run(common + ["--out", out, "--raw", "--frames", "1", "--cull", "0.01", "--save_lod", saved])
    assert r.returncode == 0, r.stderr + r.stdout
    tree.move_to_device()
    cam = mnv.Camera(W, H, FX).set_pose(EYE, BACK)
    opt = mnv.RenderOptions.cli_defaults()
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, 3
    culled, kept, counts = tree.make_culled([cam], opt, 0.01)
    assert 8 < culled.capacity < tree.capacity
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("cull:")]
    assert len(line) == 1 and "1 pose(s)" in line[0]
    _, at_depth = lod_ref.chunk_depths(tree.host_arrays()[1])
    assert line[0].split("chunks per depth before:")[1].split(",")[0].split() == [str(int(k)) for k in at_depth[1:] if k]
    assert line[0].split("kept per depth:")[1].split(";")[0].split() == [str(int(k)) for k in kept[1:] if k]
    assert f"leaves seen {counts['leaves_seen']}, non-empty leaves culled {counts['leaves_culled']}, dead chunks {counts['dead_chunks']}" in line[0]
    back_in = mnv.N3Tree.open(saved)
    for x, y in zip(back_in.host_arrays(), culled.host_arrays()):
        assert np.array_equal(x, y)
    assert back_in.data_format == culled.data_format and list(back_in.host_view().scale) == list(culled.host_view().scale)
    want = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(culled.accel, cam, opt, rgba=want)
    torch.cuda.synchronize()
    got = np.fromfile(out + "_0000.f32", dtype=np.float32).reshape(H, W, 4)
    assert np.array_equal(bits(got), bits(want.cpu().numpy()))

    orbit_saved, orbit_out, again = str(tmp_path / "orbit.npz"), str(tmp_path / "orbit"), str(tmp_path / "again")
    r = run(common + ["--out", orbit_out, "--raw", "--frames", "4", "--orbit", "60", "--cull", "0.01", "--save_lod", orbit_saved])
    assert r.returncode == 0, r.stderr + r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("cull:")]
    assert len(line) == 1 and "4 pose(s)" in line[0]
    kept_line = [int(x) for x in line[0].split("kept per depth:")[1].split(";")[0].split()]
    orbit_tree = mnv.N3Tree.open(orbit_saved)
    _, at_depth = lod_ref.chunk_depths(orbit_tree.host_arrays()[1])
    assert at_depth[1:len(kept_line) + 1].tolist() == kept_line and at_depth.sum() == orbit_tree.capacity == sum(kept_line)
    assert culled.capacity < orbit_tree.capacity < tree.capacity               # four poses see more than the first of them alone
    r = run([EXE, orbit_saved] + pose + ["--out", again, "--raw", "--frames", "4", "--orbit", "60"])
    assert r.returncode == 0, r.stderr + r.stdout
    for f in range(4):
        x, y = np.fromfile(f"{orbit_out}_{f:04d}.f32", dtype=np.uint32), np.fromfile(f"{again}_{f:04d}.f32", dtype=np.uint32)
        assert x.size == W * H * 4 and np.array_equal(x, y), f

    for extra in (["--lod", "4"], ["--lod_pixels", "8"], ["--gpus", "1"], ["--use_splitting"], ["--use_guided_sampling"]):
        bad = run(common + ["--cull", "0.01"] + extra)
        assert bad.returncode != 0 and "--cull" in bad.stderr, extra
    for extra in (["--cull", "-1"], ["--cull", "nan"], ["--save_lod", saved]):
        bad = run(common + extra)
        assert bad.returncode != 0 and "--cull" in bad.stderr, extra
