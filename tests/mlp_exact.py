"""Exactly summable sub-module networks, one-hot feature probes and an independent numpy restatement (no GPU).

The sub-module network (include/mnv.h: mnv_mlp_desc, mnv_query_submodules) differs from a sequential CPU sum only in the order in which the
matrix instruction adds its fp32 products.  On a network whose every partial sum is exactly representable that order does not matter, and
the kernel as shipped must equal the definition in every bit.  This module builds such networks and checks the condition:

  exact networks   a fixed number of nonzero weights per row from {+-0.5, +-1}, biases multiples of 2^-3, embeddings multiples of 2^-4,
                   coordinates on a 2^-7 grid.  `exactness` gives max log2(S / q) over every row, layer and neuron (S: sum of the magnitudes
                   of the neuron's terms w_k a_k and its bias; q: the largest power of two that divides all of them).  Every partial sum
                   is a multiple of q below S, so with S < 2^24 q it fits fp32's 24 bits: exact in any order.  A condition, not a tolerance.
  one-hot probes   one hidden layer; hidden units 2j / 2j+1 carry +1 / -1 at encoded feature f_j, output j = h[2j] - h[2j+1]: a single
                   nonzero product, the binary16-rounded feature itself.  Cluster c probes features [c W/2, (c+1) W/2).

`forward` is written from the definition in include/mnv.h (float32 encoding, binary16 activations, bias + sum in float64 rounded once to
float32), vectorised per cluster; it shares no code and no structure with oracle/mnv_oracle.c:orc_mlp_forward."""
from types import SimpleNamespace

import numpy as np


# ---------------------------------------------------------------- shapes and the parameter blob

def layout(desc):
    """Encoded widths and the first layer's K-slot layout (csrc/mnv_mlp.hip: fill_shape)."""
    n_pos = 3 + 6 * desc.pos_octaves
    n_dir = 3 + 6 * desc.dir_octaves if desc.need_viewdir else 0
    emb = desc.embedding_dim if desc.n_embeddings > 0 else 0
    dir_base = (n_pos + 15) // 16 * 16
    emb_base = dir_base + (n_dir + 15) // 16 * 16
    k_slots = emb_base + emb
    return SimpleNamespace(n_pos=n_pos, n_dir=n_dir, emb=emb, in_dim=n_pos + n_dir + emb, dir_base=dir_base, emb_base=emb_base,
                           k_slots=k_slots, nkk0=(k_slots + 31) // 32, cols=3 + (3 if desc.need_viewdir else 0) + (1 if emb else 0))


def layer_dims(desc):
    w = desc.hidden_width
    return [(w, layout(desc).in_dim)] + [(w, w)] * (desc.hidden_layers - 1) + [(desc.out_dim, w)]


def param_count(desc):
    return sum(o * i + o for o, i in layer_dims(desc)) + desc.n_embeddings * layout(desc).emb


def join_params(desc, nets):
    """nets: per cluster (layers [(W, b), ...], table or None) -> the binary16 blob of include/mnv.h (cluster-major)."""
    parts = []
    for layers, table in nets:
        for W, b in layers:
            parts += [np.asarray(W, np.float64).reshape(-1), np.asarray(b, np.float64)]
        if table is not None:
            parts.append(np.asarray(table, np.float64).reshape(-1))
    blob = np.concatenate(parts)
    half = blob.astype(np.float16)
    assert np.array_equal(half.astype(np.float64), blob), "parameters must be binary16 values"
    assert half.size == desc.n_clusters * param_count(desc)
    return half


def split_params(desc, params):
    """The inverse of join_params, in float64."""
    params = np.asarray(params).view(np.float16).reshape(-1).astype(np.float64)
    per, L = param_count(desc), layout(desc)
    assert params.size == per * desc.n_clusters
    nets = []
    for c in range(desc.n_clusters):
        P, off, layers = params[c * per:(c + 1) * per], 0, []
        for o, i in layer_dims(desc):
            layers.append((P[off:off + o * i].reshape(o, i), P[off + o * i:off + o * i + o]))
            off += o * i + o
        nets.append((layers, P[off:].reshape(desc.n_embeddings, L.emb) if L.emb else None))
    return nets


# ---------------------------------------------------------------- the definition

def tri(t):
    """4 |t - floor(t + 1/2)| - 1 in float32."""
    assert t.dtype == np.float32
    r = t - np.floor(t + np.float32(0.5))
    return np.float32(4) * np.abs(r) - np.float32(1)


def encode_block(v, octaves):
    """[v, tri(v 2^k), tri(v 2^k + 1/4)]_k, float32 [n][3 + 6 octaves]."""
    v = np.asarray(v, np.float32)
    out = [v]
    for k in range(octaves):
        t = v * np.float32(2.0 ** k)
        out += [tri(t), tri(t + np.float32(0.25))]
    return np.concatenate(out, axis=1)


def positions(desc, x):
    x = np.asarray(x, np.float32)
    return (x[:, :3] - np.asarray(list(desc.center), np.float32)) * np.asarray(list(desc.inv_extent), np.float32)


def embedding_rows(desc, column):
    """Index of the embedding: truncated toward zero, clamped to [0, n_embeddings)."""
    return np.clip(np.trunc(np.asarray(column, np.float64)), 0, desc.n_embeddings - 1).astype(np.int64)


def to_half(v, rounding="rne"):
    """float32 -> binary16: to nearest even, or toward zero (the mutant)."""
    assert rounding in ("rne", "rtz") and v.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16)
        if rounding == "rtz":
            away = np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))
            h = np.where(away, np.nextafter(h, np.float16(0)), h)
    return h


def features(desc, table, x, rounding="rne"):
    """Encoded inputs of the rows x for a cluster with embedding `table`: binary16 values as float64 [n][in_dim]."""
    x = np.asarray(x, np.float32)
    L = layout(desc)
    with np.errstate(invalid="ignore", over="ignore"):
        parts = [encode_block(positions(desc, x), desc.pos_octaves)]
        if desc.need_viewdir:
            parts.append(encode_block(x[:, 3:6], desc.dir_octaves))
    if L.emb:
        parts.append(np.asarray(table, np.float64)[embedding_rows(desc, x[:, L.cols - 1])].astype(np.float32))
    return to_half(np.concatenate(parts, axis=1), rounding).astype(np.float64)


def forward(desc, params, cluster, x, rounding="rne", mutate=None, trace=None):
    """The network on the rows x -> float32 [n][out_dim]; rows with a cluster id outside [0, n_clusters) are zeros.
    mutate(cluster, layer, W, b) -> (W, b): a deliberately wrong network (copies; layer hidden_layers is the output layer).
    trace: a list that receives, per cluster with rows and per layer, dict(cluster, layer, a, W, b, acc)."""
    x, cluster = np.asarray(x, np.float32), np.asarray(cluster)
    out = np.zeros((x.shape[0], desc.out_dim), np.float32)
    for c, (layers, table) in enumerate(split_params(desc, params)):
        rows = np.nonzero(cluster == c)[0]
        if rows.size == 0:
            continue
        h = features(desc, table, x[rows], rounding)
        for li, (W, b) in enumerate(layers):
            if mutate is not None:
                W, b = mutate(c, li, W, b)
            with np.errstate(invalid="ignore", over="ignore"):
                # bias + sum in float64 (no BLAS: 0 * inf must be NaN), ONE rounding to float32
                acc = (np.einsum("ri,oi->ro", h, W, optimize=False) + b).astype(np.float32)
            if trace is not None:
                trace.append(dict(cluster=c, layer=li, a=h, W=W, b=b, acc=acc))
            if li == desc.hidden_layers:
                out[rows] = acc
            else:  # ReLU: negative values, -0 and a NaN accumulator become +0 (include/mnv.h)
                with np.errstate(invalid="ignore"):
                    h = to_half(np.where(acc > 0, acc, np.float32(0)), rounding).astype(np.float64)
    return out


# ---------------------------------------------------------------- mutants (what a subtly wrong kernel would compute)

def mutant_swap_inputs(i, j):
    """Input columns i and j of the first layer swapped (a weight in the wrong K slot)."""
    def mutate(c, layer, W, b):
        if layer == 0:
            W = W.copy()
            W[:, [i, j]] = W[:, [j, i]]
        return W, b
    return mutate


def mutant_drop_bias(layer, units):
    """The bias of hidden unit units[cluster] of `layer` dropped."""
    def mutate(c, li, W, b):
        if li == layer:
            b = b.copy()
            b[units[c]] = 0.0
        return W, b
    return mutate


def pick_swap_columns(desc, params):
    """Two input columns of the first layer that every cluster uses, among the coordinates and the first octave (features that differ
    from each other on almost every row)."""
    used = np.min([np.count_nonzero(layers[0][0], axis=0) for layers, _ in split_params(desc, params)], axis=0)
    cand = np.argsort(-used[:min(9, layout(desc).n_pos)], kind="stable")[:2]
    assert used[cand].min() > 0, "the first layer does not use two of the leading input columns in every cluster"
    return int(cand[0]), int(cand[1])


def pick_bias_units(desc, params):
    """Per cluster: a unit of the last hidden layer that the output layer reads, with the largest bias (ties: the widest fan-out) -- deep
    networks' activations reach magnitudes whose binary16 spacing swallows a bias of 1/8."""
    units = []
    for layers, _ in split_params(desc, params):
        bias, fan = np.abs(layers[-2][1]), np.count_nonzero(layers[-1][0], axis=0)
        unit = int(np.argmax((fan > 0) * (bias * 1024 + fan)))
        assert bias[unit] > 0 and fan[unit] > 0
        units.append(unit)
    return units


# ---------------------------------------------------------------- the exactness condition and what the comparison sees

def exactness(trace):
    """max log2(S / q) over every row, layer and neuron of a traced forward pass of a SPARSE network (see the module docstring)."""
    worst = -np.inf
    for t in trace:
        W, a, b = t["W"], t["a"], t["b"]
        nz = int(np.count_nonzero(W, axis=1).max())
        idx = np.argsort(W == 0, axis=1, kind="stable")[:, :max(nz, 1)]      # a row's nonzero columns first
        terms = a[:, idx] * np.take_along_axis(W, idx, axis=1)[None]        # [rows][out][nz]
        terms = np.concatenate([terms, np.broadcast_to(b[None, :, None], terms.shape[:2] + (1,))], axis=2)
        assert np.isfinite(terms).all()
        scaled = terms * 2.0 ** 26                                           # products of binary16 values with +-0.5 / +-1: integers now
        ti = np.rint(scaled).astype(np.int64)
        assert np.array_equal(ti.astype(np.float64), scaled) and np.abs(scaled).max() < 2.0 ** 52
        S = np.abs(ti).sum(axis=2)
        q = np.where(ti != 0, ti & -ti, np.int64(1) << 62).min(axis=2)
        if (S > 0).any():
            worst = max(worst, float(np.log2(S[S > 0] / q[S > 0]).max()))
    return worst


def positive_fractions(desc, trace):
    """Per hidden layer: the fraction of activations that are positive, over all traced rows."""
    pos, cnt = np.zeros(desc.hidden_layers), np.zeros(desc.hidden_layers)
    for t in trace:
        if t["layer"] < desc.hidden_layers:
            pos[t["layer"]] += np.count_nonzero(t["acc"] > 0)
            cnt[t["layer"]] += t["acc"].size
    return pos / cnt


# ---------------------------------------------------------------- builders

def build_exact(desc, seed, nnz=8, values=(-1.0, -0.5, 0.5, 1.0)):
    """Parameters of an exactly summable network: `nnz` nonzeros per row from `values`, biases k / 8 in [-1, 1], embeddings k / 16 in [-2, 2]."""
    rng = np.random.default_rng(seed)
    L, nets = layout(desc), []
    for _ in range(desc.n_clusters):
        layers = []
        for o, i in layer_dims(desc):
            k = min(nnz, i)
            cols = rng.permuted(np.tile(np.arange(i), (o, 1)), axis=1)[:, :k]
            W = np.zeros((o, i))
            np.put_along_axis(W, cols, rng.choice(np.asarray(values), size=(o, k)), axis=1)
            layers.append((W, rng.integers(-8, 9, o) / 8.0))
        nets.append((layers, rng.integers(-32, 33, (desc.n_embeddings, L.emb)) / 16.0 if L.emb else None))
    return join_params(desc, nets)


def exact_samples(desc, n, seed, shares=None, invalid_frac=0.0):
    """Rows on the grid of the exact networks: coordinates k / 128 in [-1.5, 1.5], "directions" k / 64 in [-1, 1] (not normalised),
    integer embedding indices.  shares: relative number of rows per cluster (0: a cluster without rows)."""
    rng = np.random.default_rng(seed)
    L = layout(desc)
    x = np.zeros((n, L.cols), np.float32)
    x[:, :3] = rng.integers(-192, 193, (n, 3)) / 128.0
    if desc.need_viewdir:
        x[:, 3:6] = rng.integers(-64, 65, (n, 3)) / 64.0
    if L.emb:
        x[:, -1] = rng.integers(0, desc.n_embeddings, n)
    shares = np.ones(desc.n_clusters) if shares is None else np.asarray(shares, np.float64)
    assert shares.size == desc.n_clusters
    cluster = rng.choice(desc.n_clusters, size=n, p=shares / shares.sum()).astype(np.int16)
    bad = rng.random(n) < invalid_frac
    cluster[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, desc.n_clusters + 3)
    return x, cluster


def build_probe(mnv, seed=0, **kw):
    """The one-hot probe network of a layout (keywords of mnv.mlp_desc without n_clusters / hidden_layers / out_dim)
    -> (desc, params); the embedding table (shared by all clusters) holds random binary16 values and the format's corners."""
    W = kw.get("hidden_width", 64)
    per = W // 2
    L = layout(mnv.mlp_desc(**kw))
    desc = mnv.mlp_desc(n_clusters=(L.in_dim + per - 1) // per, hidden_layers=1, out_dim=per, **kw)
    table = None
    if L.emb:
        rng = np.random.default_rng(seed)
        table = (rng.standard_normal((desc.n_embeddings, L.emb)) * 0.5).astype(np.float16).astype(np.float64)
        corners = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -15, 65504.0, -65504.0, 2.0 ** -14])
        table.reshape(-1)[:corners.size] = corners
        table[-1, -1] = -1023 * 2.0 ** -24
    nets = []
    for c in range(desc.n_clusters):
        W0, Wo = np.zeros((W, L.in_dim)), np.zeros((per, W))
        for j in range(per):
            f = c * per + j
            if f < L.in_dim:
                W0[2 * j, f], W0[2 * j + 1, f] = 1.0, -1.0
                Wo[j, 2 * j], Wo[j, 2 * j + 1] = 1.0, -1.0
        nets.append(([(W0, np.zeros(W)), (Wo, np.zeros(per))], table))
    return desc, join_params(desc, nets)


def probe_batch(desc, x):
    """Every probe row once per cluster: one launch reads out every feature of every row."""
    return np.tile(np.asarray(x, np.float32), (desc.n_clusters, 1)), np.repeat(np.arange(desc.n_clusters, dtype=np.int16), x.shape[0])


def probe_expected(desc, params, x):
    """What the probe network must return on probe_batch(desc, x): the binary16-rounded features as float32 (a feature of -0 reads +0:
    h[2j] - h[2j+1] = 0 - 0), zeros in the columns past in_dim."""
    per, n = desc.out_dim, x.shape[0]
    f = features(desc, split_params(desc, params)[0][1], x)
    f = np.concatenate([f, np.zeros((n, desc.n_clusters * per - f.shape[1]))], axis=1)
    return (np.concatenate([f[:, c * per:(c + 1) * per] for c in range(desc.n_clusters)], axis=0) + 0.0).astype(np.float32)


def breakpoint_values(octaves, seed=0):
    """Coordinates at which the encoding can go wrong: +-0; every p with p 2^k in {n/4, n/2 +- 1/4, n + 1/2} (the zeros, corners and
    wrap-arounds of both triangle waves) and its float32 neighbours; the largest magnitudes the scenes reach (|p| about 3.2); magnitudes
    in binary16's subnormal range and below it; 200 random float32 values."""
    rng = np.random.default_rng(seed)
    vals = [0.0, 3.2, 3.1999, 2.999, 1.5, 2.0 ** -15, 2.0 ** -20, 2.0 ** -24, 2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14, 1023 * 2.0 ** -24]
    for k in range(max(octaves, 1)):
        for n in (0, 1, 2, 3, 6):
            vals += [t / 2.0 ** k for t in (n / 4, n / 2 + 0.25, n / 2 - 0.25, n + 0.5)]
    v = np.asarray(vals, np.float32)
    v = np.concatenate([v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))])
    v = np.concatenate([v, -v, np.float32([-0.0]), rng.uniform(-3.2, 3.2, 200).astype(np.float32)])
    _, first = np.unique(v.view(np.uint32), return_index=True)
    return v[np.sort(first)]


def probe_rows(desc, seed=0):
    """Probe rows of a layout: every axis of the position (and of the direction) takes every value of breakpoint_values, the other axes
    other values of the list; the embedding index walks over its corners (-3, -0.5, 0.99, n - 1, n, n + 0.5, 1e9) and the table's rows."""
    L = layout(desc)
    v = breakpoint_values(max(desc.pos_octaves, desc.dir_octaves if desc.need_viewdir else 0), seed)
    x = np.zeros((v.size, L.cols), np.float32)
    inv = np.asarray(list(desc.inv_extent), np.float32)
    for i in range(3):
        x[:, i] = np.roll(v, 7 * i) / inv[i] + np.float32(desc.center[i])
        if desc.need_viewdir:
            x[:, 3 + i] = np.roll(v, 3 + 5 * i)
    if L.emb:
        n = desc.n_embeddings
        corners = [-3.0, -0.5, 0.99, n - 1, n, n + 0.5, 1e9, -0.0, 0.5, 1.0, 1.99]
        x[:, -1] = np.resize(np.asarray(corners + list(range(n)), np.float32), v.size)
    return x


# ---------------------------------------------------------------- the committed configurations

PM1 = (-1.0, 1.0)
# name -> desc: keywords of mnv.mlp_desc; nkk0: K tiles of the first layer (asserted against layout()); nnz / values: build_exact;
# shares / invalid: exact_samples.  Between them: both widths x first-layer K tiles 1, 2, 3, 4 and >= 5 (every template instance and the
# generic K-outer kernel); 1 - 6 and 16 hidden layers at width 64, 1 - 4 at 128; out_dim 1, W and every residue mod 4; no direction block,
# a direction block right behind three position features, embeddings of 33 and 64, 16 octaves; 1, 3 and 8 clusters, one without rows,
# invalid ids.
EXACT_CONFIGS = {
    "w64_l1_k1_out1": dict(desc=dict(n_clusters=1, pos_octaves=2, hidden_width=64, hidden_layers=1, out_dim=1, center=(0.125, -0.25, 0.5), inv_extent=(2.0, 1.0, 0.5)), nkk0=1),
    "w64_l2_k1_dir_behind_xyz": dict(desc=dict(n_clusters=3, pos_octaves=0, dir_octaves=0, need_viewdir=True, hidden_width=64, hidden_layers=2, out_dim=4,
                                               center=(-0.125, 0.0, 0.25), inv_extent=(1.0, 2.0, 2.0)), nkk0=1, shares=(5, 1, 3)),
    "w64_l3_k2_c8": dict(desc=dict(n_clusters=8, pos_octaves=4, dir_octaves=2, need_viewdir=True, hidden_width=64, hidden_layers=3, out_dim=7,
                                   center=(0.25, 0.125, -0.375), inv_extent=(0.5, 1.0, 2.0)), nkk0=2, shares=(9, 1, 4, 2, 1, 6, 3, 2)),
    "w64_l4_k3_emb16": dict(desc=dict(n_clusters=3, pos_octaves=10, n_embeddings=12, embedding_dim=16, hidden_width=64, hidden_layers=4, out_dim=6,
                                      center=(0.0, 0.5, -0.5), inv_extent=(1.0, 1.0, 0.5)), nkk0=3, shares=(2, 7, 1)),
    "w64_l5_k4_empty_cluster": dict(desc=dict(n_clusters=3, pos_octaves=10, dir_octaves=4, need_viewdir=True, n_embeddings=12, embedding_dim=16, hidden_width=64,
                                              hidden_layers=5, out_dim=29, center=(0.125, 0.125, 0.125), inv_extent=(2.0, 2.0, 2.0)), nkk0=4, shares=(3, 0, 2)),
    "w64_l6_k5_emb64_invalid_ids": dict(desc=dict(n_clusters=8, pos_octaves=10, dir_octaves=4, need_viewdir=True, n_embeddings=7, embedding_dim=64, hidden_width=64,
                                                  hidden_layers=6, out_dim=64, center=(-0.25, 0.375, 0.0), inv_extent=(0.5, 0.5, 1.0)), nkk0=5, invalid=0.06),
    "w64_l16_k1": dict(desc=dict(n_clusters=1, pos_octaves=4, hidden_width=64, hidden_layers=16, out_dim=5, center=(0.0, 0.125, 0.0), inv_extent=(1.0, 1.0, 1.0)),
                       nkk0=1, nnz=4, values=PM1),
    "w64_l2_k7_oct16": dict(desc=dict(n_clusters=3, pos_octaves=16, dir_octaves=16, need_viewdir=True, hidden_width=64, hidden_layers=2, out_dim=3,
                                      center=(0.5, -0.5, 0.25), inv_extent=(1.0, 0.5, 2.0)), nkk0=7, shares=(1, 1, 6), nnz=16),
    "w128_l1_k1_out1": dict(desc=dict(n_clusters=1, pos_octaves=1, dir_octaves=1, need_viewdir=True, hidden_width=128, hidden_layers=1, out_dim=1,
                                      center=(0.25, 0.25, -0.125), inv_extent=(0.5, 2.0, 1.0)), nkk0=1),
    "w128_l2_k2_out128": dict(desc=dict(n_clusters=3, pos_octaves=5, dir_octaves=1, need_viewdir=True, hidden_width=128, hidden_layers=2, out_dim=128,
                                        center=(0.0, -0.125, 0.375), inv_extent=(2.0, 0.5, 1.0)), nkk0=2, shares=(1, 8, 2)),
    "w128_l3_k3_c8_invalid_ids": dict(desc=dict(n_clusters=8, pos_octaves=10, dir_octaves=4, need_viewdir=True, hidden_width=128, hidden_layers=3, out_dim=50,
                                                center=(-0.5, 0.0, 0.125), inv_extent=(1.0, 2.0, 0.5)), nkk0=3, shares=(1, 12, 1, 1, 2, 1, 1, 3), invalid=0.05),
    "w128_l4_k4_emb16": dict(desc=dict(n_clusters=3, pos_octaves=10, dir_octaves=4, need_viewdir=True, n_embeddings=9, embedding_dim=16, hidden_width=128,
                                       hidden_layers=4, out_dim=29, center=(0.125, -0.375, 0.25), inv_extent=(0.5, 1.0, 1.0)), nkk0=4, shares=(4, 0, 5)),
    "w128_l2_k6_oct16_emb33": dict(desc=dict(n_clusters=3, pos_octaves=16, dir_octaves=3, need_viewdir=True, n_embeddings=5, embedding_dim=33, hidden_width=128,
                                             hidden_layers=2, out_dim=9, center=(0.0, 0.25, -0.25), inv_extent=(2.0, 1.0, 2.0)), nkk0=6),
}
SEEDS = (1, 2)


def exact_case(mnv, name, seed):
    """(desc, params, x, cluster) of a committed configuration: about three tiles' worth of rows (a tile: 256 rows of a 64-wide network, 512 of
    a 128-wide one), spread unevenly over the clusters so that tiles are partial."""
    cfg = EXACT_CONFIGS[name]
    desc = mnv.mlp_desc(**cfg["desc"])
    assert layout(desc).nkk0 == cfg["nkk0"] if cfg["nkk0"] < 5 else layout(desc).nkk0 >= 5
    params = build_exact(desc, seed, nnz=cfg.get("nnz", 8), values=cfg.get("values", (-1.0, -0.5, 0.5, 1.0)))
    x, cluster = exact_samples(desc, 700 if desc.hidden_width == 64 else 1400, seed + 1000, shares=cfg.get("shares"), invalid_frac=cfg.get("invalid", 0.0))
    return desc, params, x, cluster


# layouts of the one-hot probes (keywords of mnv.mlp_desc), for both widths
PROBE_LAYOUTS = {
    "pos10_dir4_emb16": dict(pos_octaves=10, dir_octaves=4, need_viewdir=True, n_embeddings=6, embedding_dim=16),
    "pos16_dir16": dict(pos_octaves=16, dir_octaves=16, need_viewdir=True),
    "coords_only": dict(pos_octaves=0, dir_octaves=0),
    "emb64_past_four_k_tiles": dict(pos_octaves=10, dir_octaves=4, need_viewdir=True, n_embeddings=5, embedding_dim=64),
}
PROBE_SCALE = dict(center=(0.0, 0.0, 0.0), inv_extent=(2.0, 1.0, 0.5))  # powers of two: the listed p are reached exactly
