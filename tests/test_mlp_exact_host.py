"""The exactly summable networks and one-hot probes of tests/mlp_exact.py, on the CPU: the oracle's restatement
(oracle/mnv_oracle.c:orc_mlp_forward) equals the independent numpy restatement in every bit; the exactness condition that makes the
summation order irrelevant holds; the comparison is not vacuous; and it would notice a kernel that rounds toward zero, reads a weight
from the wrong K slot or drops a bias.  tests/test_mlp_exact_gpu.py holds the kernel to the same bits.

Conditions (asserted, none of them a tolerance):
  - max log2(S / q) < 24 over every row, layer and neuron (mlp_exact.exactness): every partial sum is exact in fp32, in any order;
  - in every hidden layer at least 25 % of the activations are positive;
  - at least half of the valid rows are nonzero in EVERY output column (so every column is nonzero in at least half of them);
  - each mutant changes the output bits of at least 1 % of the valid rows (networks with one hidden layer are exempt from the rounding
    mutant: almost nothing rounds there)."""
import numpy as np
import pytest

import mlp_exact as mx

CASES = [(name, seed) for name in sorted(mx.EXACT_CONFIGS) for seed in mx.SEEDS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def exact(mnv, orc):
    """(desc, params, x, cluster, numpy restatement, its trace) of a configuration, computed once."""
    cache = {}

    def get(name, seed):
        if (name, seed) not in cache:
            desc, params, x, cluster = mx.exact_case(mnv, name, seed)
            trace = []
            want = mx.forward(desc, params, cluster, x, trace=trace)
            want.setflags(write=False)
            cache[name, seed] = (desc, params, x, cluster, want, trace)
        return cache[name, seed]
    return get


def test_the_configurations_cover_what_they_claim(mnv):
    descs = [mnv.mlp_desc(**cfg["desc"]) for cfg in mx.EXACT_CONFIGS.values()]
    for w, layers in ((64, {1, 2, 3, 4, 5, 6, 16}), (128, {1, 2, 3, 4})):
        mine = [d for d in descs if d.hidden_width == w]
        assert {min(mx.layout(d).nkk0, 5) for d in mine} == {1, 2, 3, 4, 5}
        assert {d.hidden_layers for d in mine} == layers
        assert {1, w} <= {d.out_dim for d in mine}
    assert {d.out_dim % 4 for d in descs} == {0, 1, 2, 3}
    assert {d.n_clusters for d in descs} == {1, 3, 8}
    assert any(not d.need_viewdir for d in descs) and any(d.need_viewdir and d.pos_octaves == 0 for d in descs)
    assert {33, 64} <= {d.embedding_dim for d in descs} and any(d.pos_octaves == 16 and d.dir_octaves == 16 for d in descs)
    assert any(0 in cfg.get("shares", ()) for cfg in mx.EXACT_CONFIGS.values()) and any(cfg.get("invalid") for cfg in mx.EXACT_CONFIGS.values())
    for d in descs:
        assert mx.param_count(d) == mnv.Mlp.param_count(d)


@pytest.mark.parametrize("name,seed", CASES)
def test_oracle_equals_numpy_on_exact_networks(orc, exact, name, seed):
    desc, params, x, cluster, want, trace = exact(name, seed)
    got = orc.mlp_forward(desc, params, cluster, x)
    assert np.array_equal(bits(got), bits(want))
    valid = (cluster >= 0) & (cluster < desc.n_clusters)
    assert np.all(bits(got[~valid]) == 0)


@pytest.mark.parametrize("name,seed", CASES)
def test_exact_networks_are_exact_and_not_vacuous(exact, name, seed):
    desc, params, x, cluster, want, trace = exact(name, seed)
    worst = mx.exactness(trace)
    pos = mx.positive_fractions(desc, trace)
    valid = (cluster >= 0) & (cluster < desc.n_clusters)
    nonzero = np.all(want[valid] != 0, axis=1).mean()
    print(f"{name} seed {seed}: max log2(S/q) {worst:.1f}; positive activations per layer {np.round(pos, 2)}; rows nonzero in every column {nonzero:.3f}")
    assert worst < 24
    assert np.isfinite(want).all()
    assert pos.min() >= 0.25
    assert nonzero >= 0.5


@pytest.mark.parametrize("name,seed", [(n, s) for n, s in CASES if mx.EXACT_CONFIGS[n]["desc"]["hidden_layers"] >= 2])
def test_mutants_are_noticed(mnv, exact, name, seed):
    desc, params, x, cluster, want, trace = exact(name, seed)
    valid = (cluster >= 0) & (cluster < desc.n_clusters)
    mutants = {
        "round toward zero": dict(rounding="rtz"),
        "two first-layer inputs swapped": dict(mutate=mx.mutant_swap_inputs(*mx.pick_swap_columns(desc, params))),
        "a bias of the last hidden layer dropped": dict(mutate=mx.mutant_drop_bias(desc.hidden_layers - 1, mx.pick_bias_units(desc, params))),
    }
    for what, kw in mutants.items():
        wrong = mx.forward(desc, params, cluster, x, **kw)
        changed = np.any(bits(wrong) != bits(want), axis=1)[valid].mean()
        print(f"{name} seed {seed}: {what}: {100 * changed:.1f} % of the rows change")
        assert changed >= 0.01, what


@pytest.fixture(scope="module")
def probe(mnv):
    cache = {}

    def get(layout_name, width):
        if (layout_name, width) not in cache:
            desc, params = mx.build_probe(mnv, hidden_width=width, **mx.PROBE_LAYOUTS[layout_name], **mx.PROBE_SCALE)
            rows = mx.probe_rows(desc)
            x, cluster = mx.probe_batch(desc, rows)
            cache[layout_name, width] = (desc, params, rows, x, cluster)
        return cache[layout_name, width]
    return get


@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("layout_name", sorted(mx.PROBE_LAYOUTS))
def test_oracle_reads_out_every_feature(orc, probe, layout_name, width):
    desc, params, rows, x, cluster = probe(layout_name, width)
    want = mx.probe_expected(desc, params, rows)
    assert np.isfinite(want).all() and np.count_nonzero(want) > rows.shape[0] * mx.layout(desc).in_dim // 4
    assert np.array_equal(bits(mx.forward(desc, params, cluster, x)), bits(want))
    assert np.array_equal(bits(orc.mlp_forward(desc, params, cluster, x)), bits(want))


def test_probe_rows_hit_the_breakpoints():
    """The rows do land where they claim to: on corners, zeros and wrap-arounds of both waves, and next to them."""
    v = mx.breakpoint_values(4)
    for k in range(4):
        t = v.astype(np.float64) * 2.0 ** k
        for target in (0.25, 0.5, 0.75, 1.5, -0.25, -0.5, -2.5):
            assert np.any(t == target)
            assert np.any(t == np.nextafter(np.float32(target / 2.0 ** k), np.float32(np.inf)).astype(np.float64) * 2.0 ** k)
    assert np.any(np.signbit(v) & (v == 0)) and np.any(~np.signbit(v) & (v == 0))
    for tiny in (2.0 ** -15, 2.0 ** -20, 2.0 ** -24, 2.0 ** -26):
        assert np.any(v == np.float32(tiny)) and np.any(v == -np.float32(tiny))
    assert np.abs(v).max() >= np.float32(3.2)


def test_restatement_rounding_and_index_corners(mnv):
    h = mx.to_half(np.float32([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -26, 65519.0, 65520.0]))
    assert np.array_equal(h.astype(np.float64), [1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 0.0, 2.0 ** -24, 65504.0, np.inf])
    z = mx.to_half(np.float32([1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 3 * 2.0 ** -26, 65520.0, 1e6]), "rtz")
    assert np.array_equal(z.astype(np.float64), [1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 0.0, 65504.0, 65504.0])
    desc = mnv.mlp_desc(n_embeddings=5, embedding_dim=4)
    assert list(mx.embedding_rows(desc, np.float32([-3, -0.5, 0.99, 4, 5, 5.5, 1e9, 1.99]))) == [0, 0, 0, 4, 4, 4, 4, 1]
