"""mnv_query_submodules against its definition BIT FOR BIT, through the public entry point, on networks where the order of the fp32
sums inside v_mfma_f32_16x16x32_f16 cannot matter (tests/mlp_exact.py; tests/test_mlp_exact_host.py asserts the exactness condition
max log2(S / q) < 24 for every configuration and seed used here, and that the comparison notices a rounding toward zero, a weight in the
wrong K slot and a dropped bias).  tests/test_mlp_gpu.py keeps the tolerance test on realistic weights.

  A  exact networks: both widths x 1, 2, 3, 4 and >= 5 first-layer K tiles (every template instance and the generic K-outer kernel), 1 - 6 and 16
     hidden layers at width 64, 1 - 4 at 128, out_dim 1, W and every residue mod 4, 1 / 3 / 8 clusters (one without rows, invalid ids),
     odd strides larger than the widths, a sentinel beyond out_dim, base pointers 4 bytes past a 16-byte boundary;
  B  a slice of the batch evaluated on its own gives the same bits;
  C  one-hot probes read out every encoded feature of rows on the triangle waves' breakpoints and their float32 neighbours, +-0, |p| in
     binary16's subnormal range and below it, the scenes' largest magnitudes, and embedding indices at and beyond both ends of the table;
  D  coordinates beyond binary16's range (|p| = 7e4, 1e6, 1e30) through exact networks and a probe: the same class per output (NaN, or the
     same infinity, or the same bits) -- a hidden layer's NaN accumulator is a zero activation on both sides (include/mnv.h).

Every comparison is np.array_equal on uint32 views against oracle/mnv_oracle.c:orc_mlp_forward; the numpy restatement is asserted equal to
the oracle first, so a disagreement names its side."""
import numpy as np
import pytest

import mlp_exact as mx

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def odd_above(k):
    return k + 3 - (k & 1)  # the next odd number past k + 1


def query(torch, mlp, desc, x, cluster):
    """mlp.query with row strides larger than the widths and odd, base pointers one float past the allocation (4-byte but not 16-byte
    aligned) and a sentinel in everything the call must not write -> float32 [n][out_dim]."""
    n, cols = x.shape
    sx, so = odd_above(cols), odd_above(desc.out_dim)
    flat_x = torch.full((n * sx + 1,), 0.5, dtype=torch.float32, device="cuda")
    flat_o = torch.full((n * so + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    d_x, d_o = flat_x[1:].view(n, sx), flat_o[1:].view(n, so)
    assert d_x.data_ptr() % 16 == 4 and d_o.data_ptr() % 16 == 4 and d_x.stride(0) == sx and d_o.stride(0) == so
    d_x[:, :cols] = torch.from_numpy(x).cuda()
    mlp.query(torch.from_numpy(np.ascontiguousarray(cluster, np.int16)).cuda(), d_x, d_o)
    torch.cuda.synchronize()
    got = d_o.cpu().numpy()
    assert float(flat_o[0]) == SENTINEL and np.all(got[:, desc.out_dim:] == SENTINEL), "written outside columns [0, out_dim)"
    return np.ascontiguousarray(got[:, :desc.out_dim])


def same_class(a, b):
    """Per element: both NaN, or the same bits (the same infinity, the same finite value)."""
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (bits(a) == bits(b)))


def describe(got, want, mask=None):
    """Where and how two results differ (for the assertion message)."""
    bad = ~same_class(got, want)
    if mask is not None:
        bad &= mask
    r, c = np.nonzero(bad)
    head = ", ".join(f"[{i},{j}] got {got[i, j]!r} want {want[i, j]!r}" for i, j in list(zip(r, c))[:8])
    w = np.abs(want[bad])
    return (f"{bad.sum()} of {bad.size} values in {np.unique(r).size} rows / columns {np.unique(c)[:16]} differ; wanted magnitudes "
            f"{w.min() if w.size else 0!r} .. {w.max() if w.size else 0!r}; {head}")


@pytest.mark.parametrize("name,seed", [(name, seed) for name in sorted(mx.EXACT_CONFIGS) for seed in mx.SEEDS])
def test_exact_networks_bit_for_bit(mnv, orc, torch_gpu, name, seed):
    desc, params, x, cluster = mx.exact_case(mnv, name, seed)
    want = orc.mlp_forward(desc, params, cluster, x)
    assert np.array_equal(bits(mx.forward(desc, params, cluster, x)), bits(want)), "the two CPU restatements disagree"
    mlp = mnv.Mlp(desc, params)
    got = query(torch_gpu, mlp, desc, x, cluster)
    assert np.array_equal(bits(got), bits(want)), describe(got, want)
    valid = (cluster >= 0) & (cluster < desc.n_clusters)
    assert np.all(bits(got[~valid]) == 0)
    # B: rows do not depend on the batch they come in
    n = x.shape[0]
    a, b = n // 3 + 1, n // 3 + n // 2
    part = query(torch_gpu, mlp, desc, x[a:b], cluster[a:b])
    assert np.array_equal(bits(part), bits(got[a:b]))


@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("layout_name", sorted(mx.PROBE_LAYOUTS))
def test_first_layer_features_bit_for_bit(mnv, orc, torch_gpu, layout_name, width):
    desc, params = mx.build_probe(mnv, hidden_width=width, **mx.PROBE_LAYOUTS[layout_name], **mx.PROBE_SCALE)
    if layout_name == "emb64_past_four_k_tiles":
        assert mx.layout(desc).nkk0 > 4
    rows = mx.probe_rows(desc)
    x, cluster = mx.probe_batch(desc, rows)
    want = mx.probe_expected(desc, params, rows)
    assert np.array_equal(bits(mx.forward(desc, params, cluster, x)), bits(want)), "numpy restatement: not the rounded features"
    assert np.array_equal(bits(orc.mlp_forward(desc, params, cluster, x)), bits(want)), "oracle: not the rounded features"
    got = query(torch_gpu, mnv.Mlp(desc, params), desc, x, cluster)
    subnormal = (want != 0) & (np.abs(want) < 2.0 ** -14)
    assert subnormal.sum() >= 3 * 8  # three axes x +-{2^-15, 2^-20, 2^-24, 1023 2^-24} at the least
    assert np.array_equal(bits(got), bits(want)), (describe(got, want) + f"; outside binary16's subnormal range: {describe(got, want, ~subnormal)}")


HUGE = (7e4, -7e4, 1e6, -1e6, 1e30, -1e30)


def with_huge_coordinates(desc, x, every):
    """Every `every`-th row gets |p| = 7e4, 1e6 or 1e30 on one axis -> (x, mask of those rows)."""
    x = x.copy()
    rows = np.arange(0, x.shape[0], every)
    axis = (rows // every) % 3
    p = np.asarray(HUGE, np.float32)[(rows // every) % len(HUGE)]
    x[rows, axis] = p / np.asarray(list(desc.inv_extent), np.float32)[axis] + np.asarray(list(desc.center), np.float32)[axis]
    mask = np.zeros(x.shape[0], bool)
    mask[rows] = True
    assert np.all(np.abs(mx.positions(desc, x)[rows, axis]) >= 65520) and np.isfinite(x).all()
    return x, mask


@pytest.mark.parametrize("name", ["w64_l1_k1_out1", "w64_l3_k2_c8", "w64_l6_k5_emb64_invalid_ids", "w128_l2_k2_out128", "w128_l4_k4_emb16"])
def test_exact_networks_beyond_binary16_range(mnv, orc, torch_gpu, name):
    """A coordinate that rounds to a binary16 infinity meets zero weights: 0 * inf, and inf - inf one layer on -- NaN accumulators.  The
    definition (include/mnv.h) sends a NaN accumulator of a hidden layer to 0 like a negative one and leaves the output layer's alone:
    one hidden layer gives NaN outputs, deeper networks finite ones.  Kernel and definition must agree on every output's class; rows
    without such a coordinate -- in the same tiles -- keep their bits, and the gap slots and a tile's padding rows add nothing to anybody."""
    desc, params, x0, cluster = mx.exact_case(mnv, name, mx.SEEDS[0])
    x, huge = with_huge_coordinates(desc, x0, 9)
    want = orc.mlp_forward(desc, params, cluster, x)
    ref = mx.forward(desc, params, cluster, x)
    assert same_class(ref, want).all(), "the two CPU restatements disagree: " + describe(ref, want)
    valid = (cluster >= 0) & (cluster < desc.n_clusters)
    moved = np.any(bits(want) != bits(orc.mlp_forward(desc, params, cluster, x0)), axis=1)
    assert moved[huge & valid].mean() > 0.9 and not moved[~huge].any() and np.isfinite(want[~huge]).all()
    assert np.isnan(want[huge & valid]).all() if desc.hidden_layers == 1 else np.isfinite(want[huge & valid]).any()
    got = query(torch_gpu, mnv.Mlp(desc, params), desc, x, cluster)
    assert np.array_equal(bits(got[~huge]), bits(want[~huge])), describe(got, want)
    assert same_class(got, want).all(), describe(got, want)


@pytest.mark.parametrize("width", [64, 128])
def test_features_beyond_binary16_range(mnv, orc, torch_gpu, width):
    """The same through the one-hot probe.  Every hidden unit of such a row but the coordinate's own pair holds a zero weight for the
    infinite feature: a NaN accumulator, a zero activation.  So the coordinate reads +-inf, the other outputs of its cluster NaN (the
    output layer's zero weights meet the infinite activation) and the row's outputs in every other cluster 0."""
    desc, params = mx.build_probe(mnv, hidden_width=width, **mx.PROBE_LAYOUTS["pos10_dir4_emb16"], **mx.PROBE_SCALE)
    rows, huge = with_huge_coordinates(desc, mx.probe_rows(desc)[:240], 5)
    x, cluster = mx.probe_batch(desc, rows)
    huge = np.tile(huge, desc.n_clusters)
    want = orc.mlp_forward(desc, params, cluster, x)
    ref = mx.forward(desc, params, cluster, x)
    assert same_class(ref, want).all(), "the two CPU restatements disagree: " + describe(ref, want)
    feats = mx.probe_expected(desc, params, rows)
    assert np.array_equal(bits(want[~huge]), bits(feats[~huge]))
    assert np.isnan(want[huge]).any() and np.isinf(want[huge]).any() and np.isfinite(want[huge]).any()
    assert np.all(bits(want[huge & (cluster > 0)]) == 0)  # (the coordinates live in cluster 0)
    got = query(torch_gpu, mnv.Mlp(desc, params), desc, x, cluster)
    assert np.array_equal(bits(got[~huge]), bits(want[~huge])), describe(got, want)
    assert same_class(got, want).all(), describe(got, want)
