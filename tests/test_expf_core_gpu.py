"""exact_expf_core (csrc/mnv_device.h) -- exact_expf's main path without its range test, which the march's per-lane colour block runs
behind ONE test per wavefront -- and that test (exact_expf_core_in_range), probed through csrc/mnv_probe.hip (test-hook build; variant 2
is the core, variant 3 the range test as 1.0 / 0.0).

All 2^32 inputs by the digest scheme of tests/test_primitives_gpu.py: a digest block is 2^20 consecutive bit patterns, that is ONE value of
exact_expf's `abstop` = (bits >> 20) & 0x7ff (the block number's low 11 bits), so the blocks with abstop < 0x42b hold exactly the inputs for
which the core is valid.  On those 2 x 1067 blocks the core's digests equal the golden digests of exact_expf
(tests/golden/expf_digests.npz, which the same file holds exact_expf against); on the others the core's result means nothing, but the
kernel runs them too (the table index is masked: nothing to fault on).  The range test's digests are those of a constant per block -- 1.0
exactly where abstop < 0x42b -- so no input sits on the wrong side.  Then the named edges of +-88, element-wise."""
import os

import numpy as np
import pytest

import primitives_ref as R
from test_primitives_gpu import Probe, first_difference, same_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CORE, RANGE = 2, 3
ABSTOP_LIMIT = 0x42B                       # exact_expf: `if (abstop >= 0x42b)` guards the special cases (|x| >= 88)
BLOCKS = np.arange(4096)
IN_RANGE = (BLOCKS & 0x7FF) < ABSTOP_LIMIT   # per digest block


@pytest.fixture(scope="module")
def probe(mnv, torch_gpu):
    return Probe(mnv, torch_gpu)


def constant_digest(value):
    """the two digest words of a block whose 2^20 results all have the bits of `value`"""
    b = np.uint64(np.float32(value).view(np.uint32))
    n = np.uint64(1 << 20)
    with np.errstate(over="ignore"):
        return np.array([b * n, b * (n * (n + np.uint64(1)) // np.uint64(2))], np.uint64)


def test_core_equals_exact_expf_wherever_it_is_valid(probe):
    assert IN_RANGE.sum() == 2 * ABSTOP_LIMIT
    golden = np.load(os.path.join(HERE, "golden", "expf_digests.npz"))["digests"]
    got = probe.expf_digest(0, 4096, CORE)
    bad = np.flatnonzero((got != golden).any(axis=1) & IN_RANGE)
    if bad.size:
        blk = int(bad[0])
        x = (np.arange(1 << 20, dtype=np.uint64) + np.uint64(blk << 20)).astype(np.uint32).view(np.float32)
        pytest.fail(f"exact_expf_core: {bad.size} of {int(IN_RANGE.sum())} in-range blocks differ from exact_expf's golden digests, first block "
                    f"0x{blk:03x}; {first_difference(x, probe.expf(x, CORE), R.expf(x))}")
    # the comparison is live: beyond the range the core is NOT exact_expf (it has no special cases), and the digests see it
    assert ((got != golden).any(axis=1) & ~IN_RANGE).sum() > 1000


def test_range_test_splits_all_inputs_where_exact_expf_does(probe):
    got = probe.expf_digest(0, 4096, RANGE)
    want = np.where(IN_RANGE[:, None], constant_digest(1.0)[None, :], constant_digest(0.0)[None, :])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} blocks hold an input on the wrong side of the range test, first block 0x{int(bad[0]):03x}"


def test_named_edges_of_88(probe):
    """0x42afffff (the last pattern below 88) and its negative are in range and the core gives exact_expf's bits; 0x42b00000 (88.0) and its
    negative are out of range, as are the thresholds beyond, +-inf and NaNs.  88.0 itself takes none of exact_expf's special returns, so the
    core would be right there too -- the range test is exact_expf's own `abstop` test, not the overflow threshold."""
    inside = np.array([0x42AFFFFF, 0xC2AFFFFF, 0x42AFFFFE, 0xC2AFFFFE, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000], np.uint32)
    outside = np.array([0x42B00000, 0xC2B00000, 0x42B00001, 0xC2B00001, 0x42B17218, 0xC2CFF1B5, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32)
    for bits, want in ((inside, 1.0), (outside, 0.0)):
        assert ((((bits >> 20) & 0x7FF) < ABSTOP_LIMIT) == bool(want)).all()        # the sides, by exact_expf's own expression
        got = probe.expf(bits.view(np.float32), RANGE)
        assert np.array_equal(got, np.full(bits.size, want, np.float32)), [hex(int(b)) for b in bits[got != want]]
    x = inside.view(np.float32)
    got, exact, ref = probe.expf(x, CORE), probe.expf(x, 0), R.expf(x)
    assert same_bits(got, exact) and same_bits(got, ref), first_difference(x, got, ref)
    # every input of the structured edge list that is in range, too (r == 0 for every table entry among them)
    e = R.expf_edge_inputs()
    e = e[(((R.bits(e) >> 20) & 0x7FF) < ABSTOP_LIMIT)]
    assert e.size > 1000
    got, ref = probe.expf(e, CORE), R.expf(e)
    assert same_bits(got, ref), first_difference(e, got, ref)
