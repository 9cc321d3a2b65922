"""The march kernels' binary16 x binary32 product without a conversion instruction (csrc/mnv_device.h: half_mul, one v_fma_mix_f32 with an
addend of -0) and the channel sum built on it (sh_channel_mix), probed directly (csrc/mnv_probe.hip, test-hook build).

half_mul must be the binary32 product np.float32(h) * b bit for bit -- signed zeros, subnormal operands and results, overflow, infinities --
for every binary16 pattern in either half of a row word; sh_channel_mix must be tests/primitives_ref.py's sh_channels, term for term.  NaN
payloads are not compared (R.canonical_bits)."""
import numpy as np
import pytest

import primitives_ref as R

pytestmark = pytest.mark.gpu

F = np.float32


def _multipliers():
    """48 binary32 multipliers: the named values, then ones that push products of binary16 subnormals (2^-24 .. 2^-14) into the binary32
    subnormals and below them (ties at 2^-150), products of 65504 to FLT_MAX and over it, and ordinary values whose products round."""
    two = lambda e: np.ldexp(F(1.0), e)  # noqa: E731
    named = [0.0, -0.0, 1.0, -1.0, np.uint32(0x00000001).view(F), np.uint32(0x007FFFFF).view(F), two(-126), two(-103), two(100),
             np.finfo(F).max, np.inf, -np.inf, np.nan]
    small = [two(-110), -two(-118), two(-125), two(-126) * F(1.5), two(-127), -two(-127) * F(1.25), two(-135), two(-136) * F(3), -two(-149) * F(5),
             np.uint32(0x00000003).view(F), np.uint32(0x80400001).view(F), two(-112) * F(1.0000001), two(-140) * F(7)]
    large = [two(111), two(112), two(112) * F(1.0004884), -two(112) * F(1.0004885), two(113), -two(113), two(127), -np.finfo(F).max]
    ordinary = [1.0 / 3.0, -np.pi, 0.1, -1.7, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 0.28209479177387814, -0.4886025119029199, 1.0925484305920792,
                0.31539156525252005, 2.0 ** -24, -2.0 ** 24, 255.0, 1e-30]
    m = np.array([F(v) for v in named + small + large + ordinary], F)
    assert m.size == 48
    return m


def test_half_product_is_the_binary32_product_on_every_pattern_of_either_half(mnv, torch_gpu):
    """All 65,536 patterns in the low half, each beside a different pattern in the high half (p -> 40503 p + 12345 mod 2^16 is a bijection,
    so the high halves are all 65,536 patterns too), times 48 multipliers; every thread runs both forms, so every lane position does."""
    torch, h = torch_gpu, mnv.hooks_lib()
    lo = np.arange(65536, dtype=np.uint32)
    hi = (lo * np.uint32(40503) + np.uint32(12345)) & np.uint32(0xFFFF)
    assert np.unique(hi).size == 65536
    words = lo | (hi << np.uint32(16))
    mult = _multipliers()
    d_words, d_mult = torch.from_numpy(words.view(np.int32)).cuda(), torch.from_numpy(mult).cuda()
    out = torch.empty((2, mult.size, words.size), dtype=torch.float32, device="cuda")
    mnv._check(h.mnv_hook_probe_half_product(d_words.data_ptr(), words.size, d_mult.data_ptr(), mult.size, out.data_ptr(), None), h)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for which, halves in enumerate((lo, hi)):
        hf = R.half_bits_to_float(halves.astype(np.uint16))
        with np.errstate(all="ignore"):
            want = hf[None, :] * mult[:, None]
        g, w = R.canonical_bits(got[which]), R.canonical_bits(want)
        bad = np.argwhere(g != w)
        if bad.size:
            m, p = (int(v) for v in bad[0])
            pytest.fail(f"{'high' if which else 'low'} half: {bad.shape[0]} of {g.size} products differ; first: half 0x{int(halves[p]):04x} "
                        f"({float(hf[p]).hex()}) * 0x{int(R.bits(mult)[m]):08x} ({float(mult[m]).hex()}) = device 0x{int(g[m, p]):08x}, "
                        f"binary32 product 0x{int(w[m, p]):08x}")


SPECIAL_HALFS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x3C00, 0xBC00],
                         np.uint16)   # +-0, subnormals, smallest normal, +-65504, +-inf, NaNs, +-1


def _rows(basis_dim, rng):
    """256 rows of 3 * basis_dim raw binary16 words: 160 of ordinary coefficients, 64 of them with special values in a few places, 32 of
    arbitrary bit patterns."""
    n_half = 3 * basis_dim
    ordinary = rng.normal(0.0, 1.5, (160, n_half)).astype(np.float16).view(np.uint16)
    mixed = rng.normal(0.0, 1.5, (64, n_half)).astype(np.float16).view(np.uint16)
    for r in range(mixed.shape[0]):
        for _ in range(1 + r % 3):
            mixed[r, rng.integers(n_half)] = SPECIAL_HALFS[rng.integers(SPECIAL_HALFS.size)]
    mixed[:SPECIAL_HALFS.size, 0] = SPECIAL_HALFS              # each special value in the DC term of channel 0 ...
    mixed[:SPECIAL_HALFS.size, n_half - 1] = SPECIAL_HALFS[::-1]   # ... and in the row's last half (the high or low half of the last word)
    arbitrary = rng.integers(0, 65536, (32, n_half)).astype(np.uint16)
    return np.concatenate([ordinary, mixed, arbitrary])


@pytest.mark.parametrize("basis_dim", R.SH_BASES)
def test_channel_sum_on_raw_row_words_equals_sh_channel(mnv, torch_gpu, basis_dim):
    """256 rows x 200 view directions per basis: the three channel sums through sh_channel_mix (channel c at coefficient c * basis_dim of
    the row, as in a voxel row: odd word alignments for odd bases) against the numpy restatement of sh_channel."""
    torch, h = torch_gpu, mnv.hooks_lib()
    rng = np.random.default_rng(7000 + basis_dim)
    rows = _rows(basis_dim, rng)
    dirs = rng.normal(size=(200, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F)
    dirs[:3] = np.eye(3, dtype=F)   # axis directions: basis terms that are exactly +-0
    basis = R.sh_basis(basis_dim, dirs)
    b = np.ascontiguousarray(np.repeat(basis, rows.shape[0], axis=0))       # direction-major
    k = np.ascontiguousarray(np.tile(rows, (dirs.shape[0], 1)))
    n = b.shape[0]
    d_b, d_k = torch.from_numpy(b).cuda(), torch.from_numpy(k.view(np.int16)).cuda()
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    mnv._check(h.mnv_hook_probe_sh_mix(basis_dim, d_b.data_ptr(), d_k.data_ptr(), n, out.data_ptr(), None), h)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), R.sh_channels(basis_dim, b, k)
    g, w = R.canonical_bits(got), R.canonical_bits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{bad.shape[0]} of {g.size} channel sums differ; first: direction {int(bad[0][0]) // rows.shape[0]}, row "
                           f"{int(bad[0][0]) % rows.shape[0]}, channel {int(bad[0][1])}: device 0x{int(g[tuple(bad[0])]):08x}, reference 0x{int(w[tuple(bad[0])]):08x}")
    assert np.isfinite(want).mean() > 0.5   # the ordinary rows: most sums are finite numbers, not NaN against NaN
