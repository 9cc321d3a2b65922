"""CPU checks of tests/primitives_ref.py (the references of tests/test_primitives_gpu.py must themselves be checked): each numpy
restatement against what already exists -- this container's libm, the oracle's C restatements, and small oracle frames."""
import ctypes as C
import ctypes.util
import hashlib
import os
import sys

import numpy as np
import pytest

import primitives_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _expf_inputs():
    rng = np.random.default_rng(0)
    return np.concatenate([
        R.structured_bits(1 << 16).view(np.float32),          # 65,536 patterns across all of binary32
        rng.uniform(-110, 90, 20000).astype(np.float32),
        R.expf_edge_inputs(),
    ])


def test_expf_restatement_matches_libm_and_the_oracle(orc):
    """>= 60,000 inputs, bit for bit (NaN against NaN): none may differ from orc_expf; libm gets the allowance that
    test_oracle_math.py documents for this container's FMA-contracted ifunc variant (at most 2 inputs, 1 ulp)."""
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype = C.c_float
    libm.expf.argtypes = [C.c_float]
    xs = _expf_inputs()
    assert xs.size >= 60000
    mine = R.expf(xs)
    o = np.array([orc.lib().orc_expf(float(x)) for x in xs], np.float32)
    m = np.array([libm.expf(float(x)) for x in xs], np.float32)
    bad = np.flatnonzero(R.canonical_bits(mine) != R.canonical_bits(o))
    assert bad.size == 0, [(float(xs[i]).hex(), hex(R.bits(mine)[i]), hex(R.bits(o)[i])) for i in bad[:5]]
    bad = np.flatnonzero(R.canonical_bits(mine) != R.canonical_bits(m))
    assert bad.size <= 2, [(float(xs[i]).hex(), hex(R.bits(mine)[i]), hex(R.bits(m)[i])) for i in bad[:5]]
    for i in bad:
        assert abs(int(mine[i:i + 1].view(np.int32)[0]) - int(m[i:i + 1].view(np.int32)[0])) <= 1


def test_expf_edges_by_value():
    """The special cases by what they must be, independent of any other implementation."""
    f = lambda v: R.expf(np.float32([v]))[0]  # noqa: E731
    assert f(0.0) == 1.0 and f(-0.0) == 1.0 and f(np.float32(1e-45)) == 1.0
    assert f(-np.inf) == 0.0 and not np.signbit(f(-np.inf)) and f(np.inf) == np.inf and np.isnan(f(np.nan))
    assert f(R.EXPF_OVERFLOW) < np.inf and f(np.nextafter(R.EXPF_OVERFLOW, np.float32(np.inf))) == np.inf
    assert R.bits(f(R.EXPF_UNDERFLOW)) == 1 and f(np.nextafter(R.EXPF_UNDERFLOW, np.float32(-np.inf))) == 0.0
    assert f(-1e30) == 0.0 and f(1e30) == np.inf
    x = np.linspace(-87, 88, 5001).astype(np.float32)
    assert np.allclose(R.expf(x).astype(np.float64), np.exp(x.astype(np.float64)), rtol=2.0 ** -23, atol=0)


def test_expf_digest_recipe_on_one_block():
    """The digest recipe restated the slow way on one block (patterns of [-2, -1.999...]: block 0xC00), and the committed golden's row."""
    got = R.expf_block_digests(0xC00, 1)[0]
    pats = np.arange(0xC00 << 20, (0xC00 << 20) + (1 << 20), dtype=np.uint64).astype(np.uint32)
    rb = [int(v) for v in R.canonical_bits(R.expf(pats.view(np.float32)))]
    assert int(got[0]) == sum(rb) % (1 << 64) and int(got[1]) == sum(v * (i + 1) for i, v in enumerate(rb)) % (1 << 64)
    golden = np.load(os.path.join(HERE, "golden", "expf_digests.npz"))["digests"]
    assert golden.shape == (4096, 2) and golden.dtype == np.uint64
    assert np.array_equal(golden[0xC00], got)
    # blocks of NaN inputs hold 2^20 canonical NaNs
    assert int(golden[0x7FF, 0]) == (R.QNAN << 20) and int(golden[0xFFF, 0]) == (R.QNAN << 20)


def test_make_expf_digests_writes_reproducible_bytes(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_expf_digests as mk
    finally:
        sys.path.pop(0)
    d = np.load(os.path.join(HERE, "golden", "expf_digests.npz"))["digests"]
    out = tmp_path / "again.npz"
    mk.write_npz(str(out), d)
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()  # noqa: E731
    assert sha(out) == sha(os.path.join(HERE, "golden", "expf_digests.npz"))


def test_half_decode_matches_the_oracle_on_all_patterns(orc):
    h = np.arange(65536, dtype=np.uint16)
    mine = R.half_bits_to_float(h)
    o = np.array([orc.lib().orc_half_to_float(int(v)) for v in h], np.float32)
    assert np.array_equal(R.canonical_bits(mine), R.canonical_bits(o))
    assert np.isnan(mine).sum() == 2 * 1023 and np.isinf(mine).sum() == 2


def test_sh_basis_matches_the_oracle_bit_for_bit(orc):
    rng = np.random.default_rng(4)
    d = rng.normal(size=(2000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:6] = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    d[6] = np.float32([-0.0, 0.0, 1.0])
    for nb in R.SH_BASES:
        mine = R.sh_basis(nb, d)
        out = (C.c_float * 25)()
        got = np.empty((d.shape[0], 25), np.float32)
        for i in range(d.shape[0]):
            orc.lib().orc_sh_basis(nb, (C.c_float * 3)(*d[i]), out)
            got[i] = out[:]
        assert np.array_equal(R.bits(mine), R.bits(got[:, :nb])), nb
        assert np.all(got[:, nb:] == 0)


def test_sh_channel_sum_is_the_grouped_sum():
    """The channel restatement against a scalar left-to-right evaluation of the reference's expression, one element at a time."""
    rng = np.random.default_rng(5)
    f = np.float32
    for nb in R.SH_BASES:
        b = rng.normal(size=(40, nb)).astype(f)
        k16 = rng.normal(0, 2, size=(40, 3 * nb)).astype(np.float16)
        got = R.sh_channels(nb, b, k16.view(np.uint16))
        k = k16.astype(f)
        for row in range(40):
            for c in range(3):
                mul = lambda t: f(b[row, t] * k[row, c * nb + t])  # noqa: E731
                tmp = mul(0)
                for lo, hi in ((16, 25), (9, 16), (4, 9), (1, 4)):
                    if nb >= hi:
                        g = mul(lo)
                        for t in range(lo + 1, hi):
                            g = f(g + mul(t))
                        tmp = f(tmp + g)
                assert R.bits(got[row, c]) == R.bits(tmp)


def test_sigmoid_restatements():
    t = np.float32([-np.inf, -200, -89, -88.8, -88.7, -20, -1, -0.0, 0.0, 1, 20, 88, 200, np.inf])
    for w in np.float32([0, 1, 2.0 ** -149, 0.37, 1 - 2.0 ** -24]):
        s = R.sigmoid_exact(np.full(t.shape, w), t)
        assert np.isfinite(s).all() and (s >= 0).all() and (s <= w).all()
        assert np.all(s[t < -88.73] == 0) and s[-1] == w and np.all(np.diff(s) >= 0)
        if w == 1:
            assert np.allclose(s, R.sigmoid_f64(t), rtol=3e-7, atol=1e-38)
    assert np.isnan(R.sigmoid_exact(np.float32([1]), np.float32([np.nan]))).all()
    assert R.sigmoid_hw_bound(1.0, np.linspace(-200, 200, 100001)).max() <= 2.9e-7


def test_pack_u8_edges():
    f = np.float32
    k = np.arange(256)
    v = (k / 255.0).astype(f)
    want = np.array([int(f(x) * f(255)) for x in v], np.uint8)   # float32 product, truncated
    assert np.array_equal(R.pack_u8(v), want)
    # float32(k / 255) * 255 rounds to k or above for every k, so k / 255 packs to k; one ulp below it the truncation lands on k - 1
    assert np.array_equal(R.pack_u8(v), k) and np.array_equal(R.pack_u8(np.nextafter(v, f(-1)))[1:], k[1:] - 1)
    assert list(R.pack_u8(f([np.nan, -np.inf, -1, -0.0, 0, 1e-45, 0.999999, 1, 1.5, np.inf]))) == [0, 0, 0, 0, 0, 0, 254, 255, 255, 255]


def _frame_of(cam, opt, offset, scale):
    return R.make_frame(cam.c.fx, cam.c.fy, cam.c.cx, cam.c.cy, list(cam.c.c2w), offset, scale, list(opt.render_bbox), tuple(opt.basis_minmax))


def _one_voxel_tree(mnv, sigma):
    """One chunk of eight leaves, SH1 rows (3 coefficients + sigma)."""
    data = np.zeros((1, 2, 2, 2, 4), np.float16)
    data[..., :3] = 0.5
    data[..., 3] = sigma
    child = np.zeros((1, 2, 2, 2), np.int32)
    return mnv.N3Tree.from_arrays(data, child, data_format="SH1"), (data, child)


@pytest.mark.parametrize("scene", ["empty_bbox", "inverted_bbox", "one_voxel_clear", "one_voxel_edge_on"])
def test_ray_setup_and_composite_against_small_oracle_frames(mnv, orc, scene):
    """5 x 3-pixel oracle frames: the restated in_bbox must count what the oracle's rays_in_bbox counter counts, and for every ray that
    misses -- the march adds nothing, out stays (0, 0, 0, 0) -- the restated composite must give the oracle's rgba / rgba8, over the
    background and over an image.  one_voxel_clear: a single chunk whose voxels are all below sigma_thresh, so every pixel composites
    zeros whether its ray hits or not."""
    tree, _keep = _one_voxel_tree(mnv, 0.0 if scene == "one_voxel_clear" else 50.0)
    opt = mnv.RenderOptions.defaults()
    opt.background_brightness = 0.3
    cam = mnv.Camera(5, 3, 2.5)
    if scene == "one_voxel_edge_on":        # the box fills the middle of the frame only: hits and misses in one frame
        cam.set_pose((0.0, -4.0, 0.0), (0.0, -1.0, 0.0))
    else:
        cam.set_pose((1.5, -2.0, 1.0), (0.55, -0.7, 0.45))
    if scene == "empty_bbox":
        for i, v in enumerate((0.5, 0.5, 0.5, 0.5, 0.5, 0.5)):
            opt.render_bbox[i] = v
    if scene == "inverted_bbox":
        for i, v in enumerate((0.9, 0.9, 0.9, 0.1, 0.1, 0.1)):
            opt.render_bbox[i] = v
    view = tree.host_view()
    ot = orc.tree_from_view(view)
    iy, ix = [a.ravel() for a in np.mgrid[0:3, 0:5]]
    fr = _frame_of(cam, opt, list(view.offset), list(view.scale))
    ref = R.setup_ray(fr, ix, iy, np.full(15, 1e9, np.float32), 1)
    image = np.random.default_rng(6).integers(0, 256, size=(3, 5, 4), dtype=np.uint8)
    for init in (None, image):
        r = orc.render(ot, cam.c, opt, want_rgba8=True, rgba8_init=init)
        assert r["counters"].rays_in_bbox == int(ref["in_bbox"].sum())
        if scene == "empty_bbox":
            assert not ref["in_bbox"].any()
        if scene == "inverted_bbox":      # min / max of t1, t2 do not care which corner is which: an inverted box is the box
            assert ref["in_bbox"].any() and not ref["in_bbox"].all()
        if scene == "one_voxel_edge_on":
            assert ref["in_bbox"].any() and not ref["in_bbox"].all()
        miss = ~ref["in_bbox"] if scene != "one_voxel_clear" else np.ones(15, bool)
        rgba, rgba8 = R.composite(np.zeros((15, 4), np.float32), None if init is None else init.reshape(15, 4), opt.background_brightness)
        assert np.array_equal(R.bits(rgba[miss]), R.bits(r["rgba"].reshape(15, 4)[miss]))
        assert np.array_equal(rgba8[miss], r["rgba8"].reshape(15, 4)[miss])
    # a depth image in front of the box turns its hits into misses: t_max feeds tmax through tmax_bg = t_max / delta_scale
    tm = np.full((3, 5), 1e-3, np.float32)
    tm[1, 2] = 1e9
    ref = R.setup_ray(fr, ix, iy, tm.ravel(), 1)
    assert orc.render(ot, cam.c, opt, tmax_px=tm)["counters"].rays_in_bbox == int(ref["in_bbox"].sum())
