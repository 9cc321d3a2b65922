"""The device math primitives of csrc/mnv_device.h, probed directly (csrc/mnv_probe.hip, test-hook build) against the numpy restatements of
tests/primitives_ref.py: both exponentials on all 2^32 inputs (digests in tests/golden/expf_digests.npz) and on the named edges, the
binary16 decode, both colour sigmoids, the SH basis and channel sums, ray set-up, the u8 pack and the composite.  Everything is bit for
bit (NaN against NaN) except the hardware exp2 / rcp sigmoid, which has a stated bound.

A replacement for either exponential or either sigmoid has to pass this file first (arithmetic specification)."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import primitives_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


class Probe:
    """numpy in, numpy out around the mnv_hook_probe_* entry points (arrays travel through torch tensors on the default stream)."""

    def __init__(self, mnv, torch):
        self.mnv, self.torch, self.h = mnv, torch, mnv.hooks_lib()

    def dev(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype in _SIGNED:
            a = a.view(_SIGNED[a.dtype])
        return self.torch.from_numpy(a).cuda()

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device="cuda")

    def host(self, t, dtype=None):
        self.torch.cuda.synchronize()
        a = t.cpu().numpy()
        return a.view(dtype) if dtype is not None else a

    def check(self, rc):
        self.mnv._check(rc, self.h)

    def expf(self, x, which):
        x = self.dev(R.f32(x))
        out = self.empty(x.shape, self.torch.float32)
        self.check(self.h.mnv_hook_probe_expf(x.data_ptr(), x.numel(), which, out.data_ptr(), None))
        return self.host(out)

    def expf_digest(self, first_block, n_blocks, which):
        out = self.empty((n_blocks, 2), self.torch.int64)
        self.check(self.h.mnv_hook_probe_expf_digest(first_block, n_blocks, which, out.data_ptr(), None))
        return self.host(out, np.uint64)

    def variants_differ(self, first_bits, n):
        count, first = self.empty((1,), self.torch.int64), self.empty((16,), self.torch.int32)
        self.check(self.h.mnv_hook_probe_expf_variants_differ(first_bits, n, count.data_ptr(), first.data_ptr(), None))
        return int(self.host(count)[0]), self.host(first, np.uint32)

    def half(self, h):
        h = self.dev(np.asarray(h, np.uint16))
        out = self.empty(h.shape, self.torch.float32)
        self.check(self.h.mnv_hook_probe_half(h.data_ptr(), h.numel(), out.data_ptr(), None))
        return self.host(out)

    def sigmoid(self, w, t, mode):
        w, t = self.dev(R.f32(w)), self.dev(R.f32(t))
        assert w.shape == t.shape
        out = self.empty(w.shape, self.torch.float32)
        self.check(self.h.mnv_hook_probe_sigmoid(w.data_ptr(), t.data_ptr(), w.numel(), mode, out.data_ptr(), None))
        return self.host(out)

    def sh(self, basis_dim, dirs, coef_bits):
        n = dirs.shape[0]
        d, k = self.dev(R.f32(dirs)), self.dev(np.asarray(coef_bits, np.uint16).reshape(n, 3 * basis_dim))
        basis, chan = self.empty((n, basis_dim), self.torch.float32), self.empty((n, 3), self.torch.float32)
        self.check(self.h.mnv_hook_probe_sh(basis_dim, d.data_ptr(), k.data_ptr(), n, basis.data_ptr(), chan.data_ptr(), None))
        return self.host(basis), self.host(chan)

    def setup_ray(self, fr, ix, iy, t_max, basis_dim):
        P = self.mnv.ProbeFrame()
        for name in ("fx", "fy", "cx", "cy"):
            setattr(P.cam, name, float(fr[name]))
        P.cam.c2w[:] = [float(v) for v in fr["c2w"]]
        P.cam.cen[:] = [float(v) for v in R.ray_origin(fr)]   # the host's fill_origin: offset + scale * c2w[9..11]
        P.offset[:] = [float(v) for v in fr["offset"]]
        P.scale[:] = [float(v) for v in fr["scale"]]
        P.render_bbox[:] = [float(v) for v in fr["render_bbox"]]
        P.basis_min, P.basis_max, P.rot_enabled = fr["basis_min"], fr["basis_max"], int(fr["rot_enabled"])
        P.rot_k[:] = [float(v) for v in fr["rot_k"]]
        P.rot_cos, P.rot_sin = float(fr["rot_cos"]), float(fr["rot_sin"])
        n = len(ix)
        x, y, t = self.dev(np.asarray(ix, np.int32)), self.dev(np.asarray(iy, np.int32)), self.dev(R.f32(t_max))
        out = self.empty((n, 41), self.torch.float32)
        self.check(self.h.mnv_hook_probe_setup_ray(C.byref(P), None, x.data_ptr(), y.data_ptr(), t.data_ptr(), n, basis_dim, out.data_ptr(), None))
        o = self.host(out)
        return dict(dir=o[:, 0:3], invdir=o[:, 3:6], delta_scale=o[:, 6], tmin=o[:, 7], tmax=o[:, 8], in_bbox=o[:, 9] != 0, basis=o[:, 10:35],
                    true_dir=o[:, 35:38], vdir=o[:, 38:41])

    def composite(self, o, init_px, background, want_rgba=True, want_rgba8=True):
        o = self.dev(R.f32(o).reshape(-1, 4))
        n = o.shape[0]
        px = self.dev(np.asarray(init_px, np.uint8).reshape(n, 4)) if init_px is not None else None
        rgba = self.empty((n, 4), self.torch.float32) if want_rgba else None
        rgba8 = self.empty((n, 4), self.torch.uint8) if want_rgba8 else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.check(self.h.mnv_hook_probe_composite(o.data_ptr(), ptr(px), float(background), n, ptr(rgba), ptr(rgba8), None))
        return (self.host(rgba) if want_rgba else None), (self.host(rgba8) if want_rgba8 else None)


@pytest.fixture(scope="module")
def probe(mnv, torch_gpu):
    return Probe(mnv, torch_gpu)


def same_bits(got, want):
    return np.array_equal(R.canonical_bits(got), R.canonical_bits(want))


def first_difference(x, got, want):
    """Words for an assertion message: how many elements differ and the first one, with its input row, in hex."""
    g, w = R.canonical_bits(got).reshape(len(got), -1), R.canonical_bits(want).reshape(len(got), -1)
    rows, cols = np.nonzero(g != w)
    if rows.size == 0:
        return "no difference"
    i, j = int(rows[0]), int(cols[0])
    xi = np.asarray(x).reshape(len(got), -1)[i]
    return (f"{rows.size} of {g.size} values differ; first at element {i}, column {j}: input {[float(v).hex() for v in xi.astype(np.float64)]} "
            f"device 0x{int(g[i, j]):08x} reference 0x{int(w[i, j]):08x}")


VARIANTS = {0: "exact_expf", 1: "exact_expf_select"}


# ---- expf ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=list(VARIANTS.values()))
def test_expf_all_inputs_by_digest(probe, which):
    """All 4,096 blocks of 2^20 consecutive bit patterns: sum(bits) and sum(bits * (i + 1)) of the canonical result bits equal the golden
    (tests/golden/make_expf_digests.py).  On a mismatch the first bad block is pulled and compared on the CPU to name the input."""
    golden = np.load(os.path.join(HERE, "golden", "expf_digests.npz"))["digests"]
    got = probe.expf_digest(0, 4096, which)
    bad = np.flatnonzero((got != golden).any(axis=1))
    if bad.size:
        blk = int(bad[0])
        x = (np.arange(1 << 20, dtype=np.uint64) + np.uint64(blk << 20)).astype(np.uint32).view(np.float32)
        dev, ref = probe.expf(x, which), R.expf(x)
        d = np.flatnonzero(R.canonical_bits(dev) != R.canonical_bits(ref))
        where = (f"first differing input 0x{int(R.bits(x)[d[0]]):08x} ({float(x[d[0]]).hex()}): device 0x{int(R.bits(dev)[d[0]]):08x}, "
                 f"reference 0x{int(R.bits(ref)[d[0]]):08x}") if d.size else "the block's results equal the reference element-wise: the digest kernel disagrees"
        pytest.fail(f"{VARIANTS[which]}: {bad.size} of 4096 blocks differ from the golden digests, first block 0x{blk:03x}; {where}")


def test_expf_variants_agree_on_all_inputs(probe):
    """exact_expf_select promises exact_expf's bits for every input (two NaNs count as equal)."""
    count, first = probe.variants_differ(0, 1 << 32)
    assert count == 0, f"{count} inputs differ, among them {[hex(int(v)) for v in first[:min(count, 16)]]}"


def test_expf_probe_kernels_agree_with_each_other(probe):
    """The digest of a block equals the digest recomputed from the element-wise probe's results (a wrong reduction cannot hide behind, or
    be blamed on, the exponential), on a block with denormal results and across the array's tail (n not a multiple of the workgroup)."""
    blk = 0xC2C   # inputs -88 .. -112: normal, denormal and zero results, the underflow threshold
    x = (np.arange(1 << 20, dtype=np.uint64) + np.uint64(blk << 20)).astype(np.uint32).view(np.float32)
    for which in (0, 1):
        rb = R.canonical_bits(probe.expf(x, which)).astype(np.uint64)
        want = np.array([rb.sum(dtype=np.uint64), (rb * np.arange(1, (1 << 20) + 1, dtype=np.uint64)).sum(dtype=np.uint64)], np.uint64)
        assert np.array_equal(probe.expf_digest(blk, 1, which)[0], want)
        assert same_bits(probe.expf(x[:1000 + which], which), R.expf(x[:1000 + which]))
    count, _ = probe.variants_differ(0xC2C00000, 12345)
    assert count == 0


@pytest.mark.parametrize("which", [0, 1], ids=list(VARIANTS.values()))
def test_expf_named_edges(probe, which):
    """+-0, denormals, the overflow / underflow thresholds, +-88 and +-128 (the select variant's clamp) with their neighbours, +-inf,
    quiet and signalling NaNs (NaN out, payload not compared), ln2 * i/32 for i in -4000 .. 4000 (r == 0, every table entry)."""
    x = R.expf_edge_inputs()
    got, want = probe.expf(x, which), R.expf(x)
    assert same_bits(got, want), VARIANTS[which] + ": " + first_difference(x, got, want)
    assert np.isnan(got[np.isnan(x)]).all()


def test_half_decode_all_patterns(probe):
    h = np.arange(65536, dtype=np.uint16)
    got, want = probe.half(h), R.half_bits_to_float(h)
    assert same_bits(got, want), first_difference(h.astype(np.float32), got, want)
    assert np.array_equal(np.isnan(got), np.isnan(want))


# ---- colour sigmoid ------------------------------------------------------------------------------------------------------------------
SIGMOID_W = np.float32([0.0, 1.0, 2.0 ** -149, 0.37, 1.0 - 2.0 ** -24])


@pytest.fixture(scope="module")
def sigmoid_inputs():
    """t: the structured sample of binary32 restricted to |t| <= 200, then +inf, -inf, NaN; crossed with SIGMOID_W (w-major)."""
    t = R.structured_bits().view(np.float32)
    t = t[np.abs(t) <= 200]
    t = np.concatenate([t, np.float32([np.inf, -np.inf, np.nan])])
    w = np.repeat(SIGMOID_W, t.size)
    return w, np.tile(t, SIGMOID_W.size)


def test_sigmoid_exact(probe, sigmoid_inputs):
    """w / (1 + exact_expf(-t)) bit for bit; for t < -88.73 the exponential is +inf and the term is exactly 0, never NaN."""
    w, t = sigmoid_inputs
    got, want = probe.sigmoid(w, t, 0), R.sigmoid_exact(w, t)
    assert same_bits(got, want), first_difference(np.stack([w, t], 1), got, want)
    over = t < -88.73
    assert over.sum() > 1000 and np.all(R.bits(got[over]) == 0)
    assert np.isnan(got[np.isnan(t)]).all() and not np.isnan(got[~np.isnan(t)]).any()


def test_sigmoid_hardware(probe, sigmoid_inputs, capsys):
    """The exp2 / rcp variant of mnv_accel_set_colour_math against the float64 sigmoid, point-wise: the accuracy of the two hardware
    instructions is documented nowhere here ("about 1 ulp each"), so the bound is twice what 1 ulp each and half-ulp float32 roundings give,
    2 * w * (s (1 - s) (|t| + 1) 2^-23 + s 2^-22).  That expression takes an ulp as a relative 2^-23, which holds down to 2^-126; where the
    exact term w * s is subnormal (only w = 2^-149 here) the half-ulp of the final rounding is the absolute 2^-150, which is added there --
    without it no float32 result could pass, a correctly rounded one included.  Exceeding the bound is a finding against
    mnv_accel_set_colour_math, not a reason to widen it.

    The expression scales its arguments so that neither instruction leaves its range (v_rcp_f32 returns 0 for a subnormal result, exp2
    overflows from 2^128): terms below 2^-126 (t < -87.3) are subnormal, not zero.  Measurements: LAB_NOTEBOOK.md, "Primitive probes"."""
    w, t = sigmoid_inputs
    got = probe.sigmoid(w, t, 1).astype(np.float64)
    fin = np.isfinite(t)
    w64 = w.astype(np.float64)
    exact = w64 * R.sigmoid_f64(t)
    bound = 2.0 * R.sigmoid_hw_bound(w64, t) + np.where(exact < 2.0 ** -126, 2.0 ** -150, 0.0)
    with np.errstate(all="ignore"):
        err = np.abs(got - exact)
        ratio = np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    normal = fin & (exact >= 2.0 ** -126)      # terms whose exact value is a normal float32
    i = int(np.argmax(np.where(normal, ratio, 0.0)))
    bad = np.flatnonzero(fin & (err > bound))
    with capsys.disabled():
        print(f"\nhardware sigmoid, {int(fin.sum())} finite inputs: over terms with a normal exact value max error / bound = {ratio[i]:.4f} at "
              f"t = {float(t[i])!r} ({float(t[i]).hex()}), w = {float(w[i])!r}; max abs error for w = 1: {err[fin & (w == 1)].max():.3e}")
        sub = fin & (exact < 2.0 ** -126) & (exact > 0)
        j = int(np.argmax(np.where(sub, ratio, 0.0)))
        print(f"hardware sigmoid: over the {int(sub.sum())} terms with a subnormal exact value max error / bound = {ratio[j]:.4f} at "
              f"t = {float(t[j])!r}, w = {float(w[j])!r}")
        if bad.size:
            print(f"hardware sigmoid: {bad.size} terms beyond the bound, t in [{float(t[bad].min())!r}, {float(t[bad].max())!r}], w in "
                  f"{sorted(set(float(v) for v in w[bad]))}; max abs error among them {err[bad].max():.3e}, max exact value {exact[bad].max():.3e}, "
                  f"results that are zero: {int((got[bad] == 0).sum())}")
    assert np.isfinite(got[fin]).all() and (got[fin] >= 0).all() and (got[fin] <= w64[fin]).all()
    assert np.array_equal(got[t == np.inf], w64[t == np.inf]) and np.all(got[t == -np.inf] == 0)
    assert bad.size == 0, (f"{bad.size} terms beyond the bound; worst ratio {ratio[fin].max():.3f}; first t = {float(t[bad[0]]).hex()}, "
                           f"w = {float(w[bad[0]])!r}: got {got[bad[0]]!r}, exact {exact[bad[0]]!r}")


# ---- spherical harmonics -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sh_inputs():
    rng = np.random.default_rng(11)
    d = rng.normal(size=(4096, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    grid = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    unit26 = (grid / np.linalg.norm(grid, axis=1, keepdims=True)).astype(np.float32)
    neg0 = np.float32([[-0.0, 0.0, 1.0], [0.0, -0.0, -1.0], [-0.0, -0.0, 1.0], [1.0, -0.0, -0.0], [-0.0, 1.0, 0.0], [-0.0, -0.0, -0.0]])
    odd = np.concatenate([d[:8] * np.float32(1e-3), d[8:16] * np.float32(1e3), np.float32([[1e-40, 0.6, -0.8], [0.6, -1e-45, 0.8]])])
    return np.concatenate([d, unit26, grid.astype(np.float32), neg0, odd])


def sh_coefficients(n, basis_dim):
    """binary16 rows from N(0, 2), then rows holding +-65504, +-denormal halfs and zeros."""
    rng = np.random.default_rng(12 + basis_dim)
    k = rng.normal(0, 2, size=(n, 3 * basis_dim)).astype(np.float16).view(np.uint16).copy()
    special = np.uint16([0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0000, 0x8000])
    for r, v in enumerate(special):
        k[r, :] = v
    k[8, :] = np.resize(special, 3 * basis_dim)
    k[9, ::2] = 0x7BFF
    k[10, 1::2] = 0xFBFF
    return k


@pytest.mark.parametrize("basis_dim", R.SH_BASES)
def test_sh_basis_and_channels(probe, orc, sh_inputs, basis_dim):
    """sh_basis<B> and sh_channel<B> (three channels of one coefficient row) bit for bit against the restatement, the basis also against
    orc_sh_basis: 4,096 unit directions, the 26 axis / diagonal ones (unit and integer), -0 components, lengths 1e-3 and 1e3, denormals."""
    d = sh_inputs
    k = sh_coefficients(d.shape[0], basis_dim)
    basis, chan = probe.sh(basis_dim, d, k)
    want_b = R.sh_basis(basis_dim, d)
    assert same_bits(basis, want_b), first_difference(d, basis, want_b)
    want_c = R.sh_channels(basis_dim, want_b, k)
    assert same_bits(chan, want_c), first_difference(d, chan, want_c)
    out = (C.c_float * 25)()
    o = np.empty((d.shape[0], 25), np.float32)
    for i in range(d.shape[0]):
        orc.lib().orc_sh_basis(basis_dim, (C.c_float * 3)(*d[i]), out)
        o[i] = out[:]
    assert same_bits(basis, o[:, :basis_dim]), first_difference(d, basis, o[:, :basis_dim])


# ---- ray set-up ----------------------------------------------------------------------------------------------------------------------
def _grid(w, h, nx, ny):
    xs = np.unique(np.linspace(0, w - 1, nx).astype(np.int32))
    ys = np.unique(np.linspace(0, h - 1, ny).astype(np.int32))
    iy, ix = np.meshgrid(ys, xs, indexing="ij")
    return ix.ravel(), iy.ravel()


def _axis_c2w(axis, sign, center):
    """A camera whose view direction (-back) is exactly sign * e_axis: rotation entries are 0 and +-1 only."""
    back = np.zeros(3)
    back[axis] = -sign
    right = np.zeros(3)
    right[(axis + 1) % 3] = 1.0
    up = np.cross(back, right)
    return np.concatenate([right, up, back, center]).astype(np.float32)


def _generic_c2w(mnv, center, back):
    cam = mnv.Camera(7, 5, 4.0).set_pose(center, back)
    return cam.c


def ray_families(mnv):
    """-> list of (name, frame, ix, iy, t_max, basis_dim)"""
    out = []
    far = lambda n: np.full(n, 1e9, np.float32)  # noqa: E731
    # the cameras of six tests/cases.py cases with their options and tree placement, 9 pixels each
    for name, bd in (("cfg1_sh1_d4", 1), ("sh4_d6", 4), ("sh9_d7_aniso", 9), ("camera_inside", 4), ("ray_miss", 1), ("terrain_d7_aniso", 9)):
        spec = cases.CASES[name]
        cam, opt = cases.make_camera(mnv, spec["camera"]), cases.make_options(mnv, spec["options"])
        fr = R.make_frame(cam.c.fx, cam.c.fy, cam.c.cx, cam.c.cy, list(cam.c.c2w), spec["tree"].get("offset", (0.5, 0.5, 0.5)),
                          spec["tree"].get("scale", (0.5, 0.5, 0.5)), list(opt.render_bbox), tuple(opt.basis_minmax))
        ix, iy = _grid(cam.width, cam.height, 3, 3)
        out.append((name, fr, ix, iy, far(ix.size), bd))
    # odd-width cameras looking exactly down the six axes: the centre pixel has ix + 0.5 == cx, iy + 0.5 == cy -> +0 / -0 components
    ix, iy = _grid(7, 5, 7, 5)
    for axis in range(3):
        for sign in (1.0, -1.0):
            center = np.zeros(3)
            center[axis] = -3.0 * sign
            for fx, fy in ((3.0, 3.0), (3.0, -3.0), (-3.0, 3.0), (-3.0, -3.0)):   # the sign of the focal lengths picks +0 or -0
                fr = R.make_frame(fx, fy, 3.5, 2.5, _axis_c2w(axis, sign, center), basis_minmax=(0, 24))
                out.append((f"axis{axis}{'+' if sign > 0 else '-'}fx{fx:+.0f}fy{fy:+.0f}", fr, ix, iy, far(ix.size), 25 if fy > 0 else 16))
    # the same cameras one ulp off the pixel centre with a long focal length: direction components of 1e-10 .. 1e-9, where the double
    # 1e-9 of the invdir line (not 1e-9f) decides the float32 result
    for axis in range(3):
        for sign in (1.0, -1.0):
            center = np.zeros(3)
            center[axis] = -3.0 * sign
            for j, (fx, towards) in enumerate(((250.0, 0.0), (1000.0, 9.0), (-500.0, 9.0), (2000.0, 0.0))):
                cx, cy = np.nextafter(np.float32(3.5), np.float32(towards)), np.nextafter(np.float32(2.5), np.float32(9.0 - towards))
                fr = R.make_frame(fx, 0.5 * fx, cx, cy, _axis_c2w(axis, sign, center))
                out.append((f"nearaxis{axis}{'+' if sign > 0 else '-'}_{j}", fr, ix, iy, far(ix.size), 4))
    g = _generic_c2w(mnv, (0.0, 0.0, 0.0), (0.48, -0.6, 0.64))

    def generic(center, **kw):
        c2w = np.float32(list(g.c2w))
        c2w[9:12] = center
        return R.make_frame(g.fx, g.fy, g.cx, g.cy, c2w, **kw)

    # camera inside the box, on a face, on an edge (world cube [-1, 1]^3 -> tree [0, 1]^3)
    for name, center in (("inside", (0.1, -0.2, 0.05)), ("on_face", (1.0, 0.2, 0.1)), ("on_edge", (1.0, -1.0, 0.3)), ("at_corner", (-1.0, -1.0, -1.0))):
        out.append((name, generic(center), ix, iy, far(ix.size), 9))
    # degenerate and inverted boxes, anisotropic scale
    out.append(("bbox_point", generic((2.0, 1.0, 0.5), render_bbox=(0.5, 0.5, 0.5, 0.5, 0.5, 0.5)), ix, iy, far(ix.size), 4))
    out.append(("bbox_inverted", generic((2.0, 1.0, 0.5), render_bbox=(0.9, 0.8, 0.7, 0.1, 0.2, 0.3)), ix, iy, far(ix.size), 4))
    out.append(("aniso", generic((2.0, 1.0, 0.5), scale=(1.0, 0.25, 3.0), offset=(0.5, 0.25, 0.1)), ix, iy, far(ix.size), 16))
    # per-pixel t_max of 0, 1e-3 and 1e9, camera outside and inside
    tm = np.resize(np.float32([0.0, 1e-3, 1e9]), ix.size)
    out.append(("tmax_outside", generic((2.0, 1.0, 0.5)), ix, iy, tm, 1))
    out.append(("tmax_inside", generic((0.1, -0.2, 0.05)), ix, iy, tm, 1))
    out.append(("tmax_aniso", generic((0.1, -0.2, 0.05), scale=(1.0, 0.25, 3.0)), ix, iy, tm, 4))
    # rotation of the view direction: cos of 1, -1, 0 and a generic angle, every basis
    k = np.float32([0.3, -0.2, 0.5])
    k = k / np.sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2])
    for cs, sn in ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (np.cos(0.6164414), np.sin(0.6164414))):
        for bd in R.SH_BASES:
            out.append((f"rot_cos{cs:.3f}_sh{bd}", generic((2.0, 1.0, 0.5), rot_k=k, rot_cos=cs, rot_sin=sn), ix, iy, far(ix.size), bd))
    # basis windows, every basis
    for mm in ((0, 24), (0, 0), (4, 8), (5, 3)):
        for bd in R.SH_BASES:
            out.append((f"minmax{mm}_sh{bd}", generic((2.0, 1.0, 0.5), basis_minmax=mm), ix, iy, far(ix.size), bd))
    return out


def test_ray_setup(probe, mnv):
    """setup_ray<B> and world_ray_dirs on about 2,000 rays: every output field bit for bit against the restatement, in_bbox included, and
    the 1 / (0 + 1e-9) inverse directions of the axis-parallel rays."""
    total, zero_components, negative_zeros, inside, outside = 0, 0, 0, 0, 0
    for name, fr, ix, iy, tm, bd in ray_families(mnv):
        got, want = probe.setup_ray(fr, ix, iy, tm, bd), R.setup_ray(fr, ix, iy, tm, bd)
        for field in ("true_dir", "vdir", "dir", "invdir", "delta_scale", "tmin", "tmax", "basis"):
            assert same_bits(got[field], want[field]), f"{name}.{field}: " + first_difference(np.stack([ix, iy], 1), got[field], want[field])
        assert np.array_equal(got["in_bbox"], want["in_bbox"]), (name, np.flatnonzero(got["in_bbox"] != want["in_bbox"])[:5])
        total += ix.size
        zero_components += int((want["dir"] == 0).sum())
        negative_zeros += int(((want["dir"] == 0) & np.signbit(want["dir"])).sum())
        inside += int(want["in_bbox"].sum())
        outside += int((~want["in_bbox"]).sum())
        if name.startswith("axis"):
            z = want["dir"] == 0
            assert np.all(np.abs(got["invdir"][z]) == np.float32(1e9)) and np.isfinite(got["invdir"]).all()
    # the families must have produced what they are there for
    assert total >= 1900 and zero_components >= 48 and 0 < negative_zeros < zero_components and inside > 300 and outside > 300


# ---- u8 pack and composite -----------------------------------------------------------------------------------------------------------
def test_pack_u8(probe):
    """pack_u8 through composite_and_write with alpha 1 (nothing is added to the colour): every 1024th binary32 pattern, every k / 255
    with its two neighbours (k / 255 packs to k, one ulp below it the truncation lands on k - 1), NaN, +-inf, negatives."""
    v = R.structured_bits(1 << 10).view(np.float32)
    k255 = (np.arange(256) / 255.0).astype(np.float32)
    extra = np.concatenate([k255, np.nextafter(k255, np.float32(-1)), np.nextafter(k255, np.float32(2)),
                            np.float32([np.nan, np.inf, -np.inf, -1.0, -1e-45, -0.0, 1.0, 256.0 / 255.0, 3.4e38, -3.4e38])])
    v = np.concatenate([v, extra])
    v = np.concatenate([v, np.zeros(-v.size % 3, np.float32)]).reshape(-1, 3)
    o = np.concatenate([v, np.ones((v.shape[0], 1), np.float32)], 1)
    for init in (None, np.full((o.shape[0], 4), 200, np.uint8)):
        _, got8 = probe.composite(o, init, 0.7, want_rgba=False)
        _, want8 = R.composite(o, init, 0.7)
        assert np.array_equal(got8, want8), first_difference(o, got8[:, :3].astype(np.float32), want8[:, :3].astype(np.float32))
        assert np.array_equal(got8[:, :3], R.pack_u8(v))   # alpha 1: the colour reaches the pack unchanged


def test_composite_both_branches(probe):
    """composite_and_write over background_brightness and over an image: alpha in {0, 0.5, 1, 1 + 2^-23, NaN}, colours from below 0 to
    beyond 1, every byte value as the pixel underneath; float and byte outputs together and each alone."""
    rng = np.random.default_rng(13)
    alphas = np.float32([0.0, 0.5, 1.0, 1.0 + 2.0 ** -23, np.nan])
    n = 256 * alphas.size * 4
    o = np.empty((n, 4), np.float32)
    o[:, :3] = rng.uniform(-0.25, 2.0, size=(n, 3)).astype(np.float32)
    o[::7, :3] = rng.uniform(0, 1, size=(o[::7].shape[0], 3)).astype(np.float32)
    o[:, 3] = np.repeat(alphas, n // alphas.size)
    px = np.empty((n, 4), np.uint8)
    for c in range(4):
        px[:, c] = (np.arange(n) * (1, 3, 5, 7)[c] + c * 64) % 256   # every byte value in every channel, alpha byte arbitrary
    for init, bg in ((None, 1.0), (None, 0.3), (px, 0.3)):
        want, want8 = R.composite(o, init, bg)
        got, got8 = probe.composite(o, init, bg)
        assert same_bits(got, want), first_difference(o, got, want)
        assert np.array_equal(got8, want8)
        only, none8 = probe.composite(o, init, bg, want_rgba8=False)
        none, only8 = probe.composite(o, init, bg, want_rgba=False)
        assert none8 is None and none is None and same_bits(only, want) and np.array_equal(only8, want8)
