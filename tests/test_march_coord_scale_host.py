"""The march's integer cell coordinates at the fixed scale 2^23 (csrc/mnv_march_accel_kernel.h) name the cells the tree's own scale names:
for every depth Lq in 1 .. 23 and every binary32 x in [0, 1 - 1e-6] (what the kernel's clamp leaves),

    uint32(x * 2^23) >> (23 - Lq) == uint32(x * 2^Lq)

with both products formed in binary32 as the kernel forms them (a multiplication by a power of two: exact) and truncated.  Numpy, no GPU."""
import numpy as np

HI = np.float32(1.0) - np.float32(1e-6)       # the kernel's upper clamp, 1.f - 1e-6f


def inputs():
    rng = np.random.default_rng(20230823)
    parts = [rng.uniform(0.0, float(HI), size=1 << 22).astype(np.float32)]
    parts.append(np.array([0.0, HI], np.float32))
    # every power of two inside the range (subnormals included) with its two neighbours
    p2 = np.float32(2.0) ** np.arange(-149, 0, dtype=np.float32)
    parts += [p2, np.nextafter(p2, np.float32(0.0)), np.nextafter(p2, np.float32(1.0))]
    # cell boundaries k / 2^d of every level d <= 12, one ulp either side: every k up to d = 8, a seeded sample of 512 above
    for d in range(0, 13):
        k = np.arange(0, (1 << d) + 1) if d <= 8 else np.unique(np.concatenate([[0, 1, (1 << d) - 1, 1 << d], rng.integers(0, (1 << d) + 1, size=512)]))
        v = (k.astype(np.float64) / float(1 << d)).astype(np.float32)     # exact: k < 2^24
        parts += [v, np.nextafter(v, np.float32(-1.0)), np.nextafter(v, np.float32(2.0))]
    x = np.concatenate(parts).astype(np.float32)
    x = x[(x >= 0) & (x <= HI)]
    return x


def test_cells_at_scale_2_23_are_the_cells_at_the_tree_scale():
    x = inputs()
    assert x.dtype == np.float32 and x.size > (1 << 22) and x.min() == 0 and x.max() == HI
    s23 = x * np.float32(2.0 ** 23)
    assert s23.dtype == np.float32 and np.array_equal(s23.astype(np.float64), x.astype(np.float64) * 2.0 ** 23)   # the product is exact ...
    q23 = s23.astype(np.uint32)
    assert int(q23.max()) == int(np.floor(float(HI) * 2.0 ** 23)) < (1 << 23)                                       # ... and below 2^23
    for Lq in range(1, 24):
        qL = (x * np.float32(2.0 ** Lq)).astype(np.uint32)
        assert np.array_equal(q23 >> np.uint32(23 - Lq), qL), f"Lq = {Lq}: {int((q23 >> np.uint32(23 - Lq) != qL).sum())} of {x.size} inputs differ"
