"""numpy restatements of the device math primitives behind every bit-exact frame (csrc/mnv_device.h), written from DESIGN.md's arithmetic
specification and the reference's source lines, not from the device header: expf (glibc 2.35's table algorithm, non-FMA variant), the
binary16 decode, the colour sigmoid, the SH basis and channel sum (rt_core.cuh:12-68, 257-283), ray generation and march set-up
(renderer_kernel.cu:30-61, 272-283; rt_core.cuh:70-115, 182-209; common.cuh:11-55) and the composite with its u8 pack
(renderer_kernel.cu:215-241).

Everything is vectorised over elements; every float operation is one numpy operation on float32 or float64 arrays in the source's
evaluation order under the usual arithmetic conversions (a double literal promotes only the sub-expression it appears in).  numpy's
+ - * / sqrt are correctly rounded IEEE operations and never contracted, which is the specification.  tests/test_primitives_host.py
holds these restatements against libm and the oracle; tests/test_primitives_gpu.py holds the device functions against them."""
import struct
from decimal import Decimal, getcontext

import numpy as np

F = np.float32
QNAN = 0x7FC00000


def f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


def f64(a):
    return a.astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canonical_bits(a):
    """uint32 view with every NaN replaced by the one quiet NaN (payloads are not part of any contract here)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = QNAN
    return b


# ---- expf ----------------------------------------------------------------------------------------------------------------------------
def _exp2f_table():
    """tab[i] = asuint64(2^(i/32) correctly rounded to binary64) - (i << 47), from first principles."""
    getcontext().prec = 60
    out = []
    for i in range(32):
        d = float(Decimal(2) ** (Decimal(i) / Decimal(32)))
        out.append((struct.unpack("<Q", struct.pack("<d", d))[0] - (i << 47)) & 0xFFFFFFFFFFFFFFFF)
    return np.array(out, np.uint64)


EXP2F_TAB = _exp2f_table()
_N = 32.0
_INVLN2N = float.fromhex("0x1.71547652b82fep+0") * _N
_SHIFT = float.fromhex("0x1.8p+52")
_C0 = float.fromhex("0x1.c6af84b912394p-5") / _N / _N / _N
_C1 = float.fromhex("0x1.ebfce50fac4f3p-3") / _N / _N
_C2 = float.fromhex("0x1.62e42ff0c52d6p-1") / _N
EXPF_OVERFLOW = F(float.fromhex("0x1.62e42ep6"))     # x above this: +inf
EXPF_UNDERFLOW = F(float.fromhex("-0x1.9fe368p6"))   # x below this: 0


def expf(x):
    """glibc 2.35 expf (sysdeps/ieee754/flt-32/e_expf.c, TOINT_INTRINSICS == 0, no FMA): the binary64 main path
    2^(k/32) * (1 + C2 r + r^2 (C1 + C0 r)) with k = round(x * 32/ln2) taken from the low bits of z + 0x1.8p52, and the special cases for
    |x| >= 88 in the source's order: -inf -> 0, NaN / +inf -> x + x, x > 0x1.62e42ep6 -> inf, x < -0x1.9fe368p6 -> 0.  (Between the two
    underflow thresholds of the source, -0x1.9fe368p6 <= x < -0x1.9d1d9ep6, its errno path returns the same 2^-149 as the main path.)"""
    x = f32(x)
    ix = x.view(np.uint32)
    abstop = (ix >> np.uint32(20)) & np.uint32(0x7FF)
    big = abstop >= 0x42B
    is_ninf = ix == np.uint32(0xFF800000)
    nonfinite = big & (abstop >= 0x7F8) & ~is_ninf
    with np.errstate(all="ignore"):
        over = big & ~is_ninf & ~nonfinite & (x > EXPF_OVERFLOW)
        under = big & ~is_ninf & ~nonfinite & ~over & (x < EXPF_UNDERFLOW)
        special = is_ninf | nonfinite | over | under
        xd = np.where(special, 0.0, f64(x))
        z = _INVLN2N * xd
        kd = z + _SHIFT
        ki = kd.view(np.uint64)
        kd = kd - _SHIFT
        r = z - kd
        t = EXP2F_TAB[(ki & np.uint64(31)).astype(np.intp)] + (ki << np.uint64(47))
        s = t.view(np.float64)
        z = _C0 * r + _C1
        r2 = r * r
        y = _C2 * r + 1.0
        y = z * r2 + y
        y = y * s
        out = y.astype(np.float32)
        out[is_ninf] = 0.0
        out[nonfinite] = x[nonfinite] + x[nonfinite]
        out[over] = np.inf
        out[under] = 0.0
    return out


SAMPLE_STRIDE = 885


def structured_bits(stride=SAMPLE_STRIDE):
    """Every stride-th bit pattern of binary32 (4.85 M with the default stride): all exponents, both signs, NaNs and infinities' blocks."""
    return np.arange(0, 1 << 32, stride, dtype=np.uint64).astype(np.uint32)


def expf_edge_inputs():
    """The named edges: zeros, denormals, the overflow / underflow thresholds and +-88 / +-128 with their neighbours, infinities, quiet and
    signalling NaNs, and ln2 * i/32 for i in -4000 .. 4000 (r == 0 for every table entry)."""
    def around(v):
        b = int(F(v).view(np.uint32))
        return [b - 1, b, b + 1]

    pats = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x80400000, 0x00800000, 0x80800000,
            0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF]
    for v in (EXPF_OVERFLOW, EXPF_UNDERFLOW, 88.0, -88.0, 128.0, -128.0, float.fromhex("-0x1.9d1d9ep6"), float.fromhex("-0x1.5d589ep6")):
        pats += around(v)
    grid = (np.log(2.0) * np.arange(-4000, 4001) / 32.0).astype(np.float32)
    return np.concatenate([np.array(pats, np.uint32).view(np.float32), grid])


def expf_block_digests(first_block, n_blocks, fn=expf):
    """uint64 [n_blocks, 2]: per block of 2^20 consecutive bit patterns, sum(bits) and sum(bits * (i + 1)) mod 2^64 of the canonical result
    bits, i the index in the block."""
    idx1 = np.arange(1, (1 << 20) + 1, dtype=np.uint64)
    out = np.empty((n_blocks, 2), np.uint64)
    for b in range(n_blocks):
        base = (first_block + b) << 20
        pats = (np.arange(1 << 20, dtype=np.uint64) + np.uint64(base)).astype(np.uint32)
        rb = canonical_bits(fn(pats.view(np.float32))).astype(np.uint64)
        out[b, 0] = rb.sum(dtype=np.uint64)
        out[b, 1] = (rb * idx1).sum(dtype=np.uint64)
    return out


# ---- binary16, sigmoid ---------------------------------------------------------------------------------------------------------------
def half_bits_to_float(h):
    return np.ascontiguousarray(h, dtype=np.uint16).view(np.float16).astype(np.float32)


def sigmoid_exact(w, t):
    """weight / (1.f + expf(-tmp)) (rt_core.cuh:281) in binary32."""
    w, t = f32(w), f32(t)
    with np.errstate(all="ignore"):
        return w / (F(1.0) + expf(-t))


def sigmoid_f64(t):
    """1 / (1 + exp(-t)) in binary64: what the hardware exp2 / rcp variant is bounded against."""
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(t, np.float64)))


def sigmoid_hw_bound(w, t):
    """The error allowed to one term of the hardware variant, before the margin factor: with one ulp for each of exp2 and rcp and half an
    ulp for each float32 rounding (the product t * -log2(e), 1 + e, the product with w), w * (s (1 - s) (|t| + 1) 2^-23 + s 2^-22),
    s the float64 sigmoid."""
    w, t = np.asarray(w, np.float64), np.asarray(t, np.float64)
    s = sigmoid_f64(t)
    with np.errstate(all="ignore"):
        slope = np.where(np.isfinite(t), s * (1.0 - s) * (np.abs(t) + 1.0), 0.0)
    return w * (slope * 2.0 ** -23 + s * 2.0 ** -22)


# ---- spherical harmonics -------------------------------------------------------------------------------------------------------------
SH_BASES = (1, 4, 9, 16, 25)


def sh_basis(basis_dim, d):
    """maybe_precalc_basis (rt_core.cuh:12-68) for float32 directions d [n, 3] -> float32 [n, basis_dim].  A double literal times a float
    promotes the product chain to double; the parenthesised float sub-expressions stay float; an int literal times a float is float."""
    d = f32(d).reshape(-1, 3)
    n = d.shape[0]
    out = np.zeros((n, 25), np.float32)
    out[:, 0] = F(0.28209479177387814)
    if basis_dim >= 4:
        x, y, z = d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy()
        xx, yy, zz = x * x, y * y, z * z
        xy, yz, xz = x * y, y * z, x * z
        c2, c3, c4, c7, c30, c35, c1 = F(2), F(3), F(4), F(7), F(30), F(35), F(1)
        with np.errstate(all="ignore"):
            if basis_dim >= 25:
                out[:, 16] = 2.5033429417967046 * f64(xy) * f64(xx - yy)
                out[:, 17] = -1.7701307697799304 * f64(yz) * f64(c3 * xx - yy)
                out[:, 18] = 0.9461746957575601 * f64(xy) * f64(c7 * zz - c1)
                out[:, 19] = -0.6690465435572892 * f64(yz) * f64(c7 * zz - c3)
                out[:, 20] = 0.10578554691520431 * f64(zz * (c35 * zz - c30) + c3)
                out[:, 21] = -0.6690465435572892 * f64(xz) * f64(c7 * zz - c3)
                out[:, 22] = 0.47308734787878004 * f64(xx - yy) * f64(c7 * zz - c1)
                out[:, 23] = -1.7701307697799304 * f64(xz) * f64(xx - c3 * yy)
                out[:, 24] = 0.6258357354491761 * f64(xx * (xx - c3 * yy) - yy * (c3 * xx - yy))
            if basis_dim >= 16:
                out[:, 9] = -0.5900435899266435 * f64(y) * f64(c3 * xx - yy)
                out[:, 10] = 2.890611442640554 * f64(xy) * f64(z)
                out[:, 11] = -0.4570457994644658 * f64(y) * f64(c4 * zz - xx - yy)
                out[:, 12] = 0.3731763325901154 * f64(z) * f64(c2 * zz - c3 * xx - c3 * yy)
                out[:, 13] = -0.4570457994644658 * f64(x) * f64(c4 * zz - xx - yy)
                out[:, 14] = 1.445305721320277 * f64(z) * f64(xx - yy)
                out[:, 15] = -0.5900435899266435 * f64(x) * f64(xx - c3 * yy)
            if basis_dim >= 9:
                out[:, 4] = 1.0925484305920792 * f64(xy)
                out[:, 5] = -1.0925484305920792 * f64(yz)
                out[:, 6] = 0.31539156525252005 * (2.0 * f64(zz) - f64(xx) - f64(yy))
                out[:, 7] = -1.0925484305920792 * f64(xz)
                out[:, 8] = 0.5462742152960396 * f64(xx - yy)
            out[:, 1] = -0.4886025119029199 * f64(y)
            out[:, 2] = 0.4886025119029199 * f64(z)
            out[:, 3] = -0.4886025119029199 * f64(x)
    return np.ascontiguousarray(out[:, :basis_dim])


SH_GROUPS = ((16, 25), (9, 16), (4, 9), (1, 4))   # summed in this order after the DC term, each left to right (rt_core.cuh:262-279)


def sh_channels(basis_dim, b, coef_bits):
    """tmp of rt_core.cuh:262-279 for the three channels: b float32 [n, basis_dim], coef_bits uint16 [n, 3 * basis_dim] (channel c at
    c * basis_dim) -> float32 [n, 3]."""
    b = f32(b).reshape(-1, basis_dim)
    coef = half_bits_to_float(coef_bits).reshape(-1, 3, basis_dim)
    out = np.empty((b.shape[0], 3), np.float32)
    with np.errstate(all="ignore"):
        for c in range(3):
            k = coef[:, c, :]
            tmp = b[:, 0] * k[:, 0]
            for lo, hi in SH_GROUPS:
                if basis_dim >= hi:
                    g = b[:, lo] * k[:, lo]
                    for i in range(lo + 1, hi):
                        g = g + b[:, i] * k[:, i]
                    tmp = tmp + g
            out[:, c] = tmp
    return out


# ---- ray set-up ----------------------------------------------------------------------------------------------------------------------
def fmin32(a, b):
    """CUDA / IEEE minNum on float32: the other operand when one is NaN; -0 below +0."""
    r = np.fmin(a, b)
    both_zero = (a == 0) & (b == 0)
    return np.where(both_zero, np.where(np.signbit(a) | np.signbit(b), F(-0.0), F(0.0)), r).astype(np.float32)


def fmax32(a, b):
    r = np.fmax(a, b)
    both_zero = (a == 0) & (b == 0)
    return np.where(both_zero, np.where(np.signbit(a) & np.signbit(b), F(-0.0), F(0.0)), r).astype(np.float32)


def make_frame(fx, fy, cx, cy, c2w, offset=(0.5, 0.5, 0.5), scale=(0.5, 0.5, 0.5), render_bbox=(0, 0, 0, 1, 1, 1), basis_minmax=(0, 24),
               rot_k=None, rot_cos=1.0, rot_sin=0.0):
    """The per-frame constants of a launch as float32: rot_k None = rodrigues' early return (|rot_dirs| < 1e-6); otherwise its unit axis
    with the cosine and sine of the angle (renderer_kernel.cu:43-51: once per frame)."""
    return dict(fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), c2w=f32(c2w).reshape(12), offset=f32(offset), scale=f32(scale),
                render_bbox=f32(render_bbox), basis_min=int(basis_minmax[0]), basis_max=int(basis_minmax[1]), rot_enabled=rot_k is not None,
                rot_k=f32(rot_k if rot_k is not None else (0, 0, 0)), rot_cos=F(rot_cos), rot_sin=F(rot_sin))


def ray_origin(fr):
    """cen = offset + scale * c2w[9..11] (renderer_kernel.cu:272-275), float32 multiply then add."""
    prod = fr["scale"] * fr["c2w"][9:12]
    return (fr["offset"] + prod).astype(np.float32)


def _norm3(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def setup_ray(fr, ix, iy, t_max, basis_dim):
    """screen2worlddir, rodrigues, _get_delta_scale, the invdir line, _dda_world and the basis with its min / max mask for the pixels
    (ix, iy) with per-pixel t_max.  -> dict of float32 arrays: true_dir, vdir [n, 3] (world unit direction and its rotated copy), dir,
    invdir [n, 3] (tree space), delta_scale, tmin, tmax [n], in_bbox bool [n], basis [n, 25] (zero beyond basis_dim)."""
    ix, iy = np.asarray(ix, np.int32), np.asarray(iy, np.int32)
    t_max = f32(t_max)
    m = fr["c2w"]
    with np.errstate(all="ignore"):
        xyz0 = (ix.astype(np.float32) + F(0.5) - fr["cx"]) / fr["fx"]
        xyz1 = -(iy.astype(np.float32) + F(0.5) - fr["cy"]) / fr["fy"]
        xyz2 = np.full(xyz0.shape, -1.0, np.float32)
        d = [m[k] * xyz0 + m[3 + k] * xyz1 + m[6 + k] * xyz2 for k in range(3)]
        invnorm = F(1.0) / _norm3(d)
        d = [c * invnorm for c in d]
        true_dir = np.stack(d, 1)
        v = list(d)
        if fr["rot_enabled"]:
            k, cs, sn = fr["rot_k"], fr["rot_cos"], fr["rot_sin"]
            cross = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
            dot = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
            # dir[i] * cos + cross[i] * sin + k[i] * dot * (1.0 - cos): float + float, then + (float product promoted) * double
            v = [(f64(v[i] * cs + cross[i] * sn) + f64(k[i] * dot) * (1.0 - float(cs))).astype(np.float32) for i in range(3)]
        vdir = np.stack(v, 1)
        # _get_delta_scale
        d = [d[i] * fr["scale"][i] for i in range(3)]
        delta_scale = F(1.0) / _norm3(d)
        d = [c * delta_scale for c in d]
        tmax_bg = t_max / delta_scale
        cen = ray_origin(fr)
        tmin = np.zeros(xyz0.shape, np.float32)
        tmax = np.full(xyz0.shape, 1e4, np.float32)
        inv = []
        for i in range(3):
            inv.append((1.0 / (f64(d[i]) + 1e-9)).astype(np.float32))
        for i in range(3):
            t1 = ((float(fr["render_bbox"][i]) + 1e-6 - float(cen[i])) * f64(inv[i])).astype(np.float32)
            t2 = ((float(fr["render_bbox"][i + 3]) - 1e-6 - float(cen[i])) * f64(inv[i])).astype(np.float32)
            tmin = fmax32(tmin, fmin32(t1, t2))
            tmax = fmin32(tmax, fmax32(t1, t2))
        tmax = fmin32(tmax, tmax_bg)
        in_bbox = ~((tmax < 0) | (tmin > tmax))
    basis = np.zeros((xyz0.shape[0], 25), np.float32)
    basis[:, :basis_dim] = sh_basis(basis_dim, vdir)
    for i in range(25):
        if i < fr["basis_min"] or i > fr["basis_max"]:
            basis[:, i] = 0.0
    return dict(true_dir=true_dir, vdir=vdir, dir=np.stack(d, 1), invdir=np.stack(inv, 1), delta_scale=delta_scale.astype(np.float32),
                tmin=tmin, tmax=tmax, in_bbox=in_bbox, basis=basis)


# ---- composite -----------------------------------------------------------------------------------------------------------------------
def pack_u8(v):
    """uint8_t(v * 255) (renderer_kernel.cu:237) with the saturating float -> integer conversion of the reference's platform: NaN and
    everything not above 0 give 0, 255 and above give 255, the rest truncates."""
    with np.errstate(all="ignore"):
        s = f32(v) * F(255.0)
        out = np.zeros(s.shape, np.uint8)
        mid = (s > 0) & (s < F(255.0))
        out[mid] = np.floor(s[mid]).astype(np.uint8)
        out[s >= F(255.0)] = 255
    return out


def composite(o, init_px, background):
    """composite_and_write (renderer_kernel.cu:215-241): o float32 [n, 4]; init_px uint8 [n, 4] = the pixel already in the image
    (offscreen == false) or None = the background_brightness branch.  -> (rgba float32 [n, 4], rgba8 uint8 [n, 4], alpha byte 255)."""
    o = f32(o).reshape(-1, 4).copy()
    with np.errstate(all="ignore"):
        nalpha = F(1.0) - o[:, 3]
        if init_px is not None:
            px = np.ascontiguousarray(init_px, np.uint8).reshape(-1, 4)
            for c in range(3):
                o[:, c] = o[:, c] + px[:, c].astype(np.float32) / F(255.0) * nalpha
        else:
            remain = F(background) * nalpha
            for c in range(3):
                o[:, c] = o[:, c] + remain
    rgba8 = np.empty((o.shape[0], 4), np.uint8)
    for c in range(3):
        rgba8[:, c] = pack_u8(o[:, c])
    rgba8[:, 3] = 255
    return o, rgba8
