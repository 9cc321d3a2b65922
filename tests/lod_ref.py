"""A numpy restatement of the two level-of-detail contracts of include/mnv.h (mnv_tree_mip_rows, mnv_tree_truncate).  Every float operation
is float32 in the order the contract states (numpy's float32 multiply, add and divide are correctly rounded and never contracted),
astype(np.float16) is the single round-to-nearest-even to binary16 (subnormals kept), depths come from walking `child` from the root."""
import numpy as np

MAX_DEPTH = 23


def chunk_depths(child):
    """child int32 [cap, 8] -> (chunk_depth int32 [cap] with 0 = not reached, chunks_at_depth int64 [24]).  The root chunk's voxels have
    depth 1; chunk c + child[c][j] has depth(c) + 1.  ValueError("invalid"): a link outside [1, cap) or a chunk reached twice;
    ValueError("unsupported"): more than 23 levels."""
    child = np.asarray(child, np.int64).reshape(-1, 8)
    cap = child.shape[0]
    depth = np.zeros(cap, np.int32)
    counts = np.zeros(24, np.int64)
    depth[0] = 1
    counts[1] = 1
    front = np.array([0], np.int64)
    d = 1
    while True:
        links = child[front]
        rows, cols = np.nonzero(links)
        target = front[rows] + links[rows, cols]
        if target.size == 0:
            break
        if (target < 1).any() or (target >= cap).any():
            raise ValueError("invalid: a child link leaves the tree")
        if np.unique(target).size != target.size or (depth[target] != 0).any():
            raise ValueError("invalid: a chunk is reached twice")
        if d + 1 > MAX_DEPTH:
            raise ValueError("unsupported: more than 23 levels")
        d += 1
        depth[target] = d
        counts[d] = target.size
        front = np.sort(target)
    return depth, counts


def half_value(bits):
    """h(bits): the binary16 value as float32; bits that are not finite read as +0."""
    v = np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)
    return np.where(np.isfinite(v), v, np.float32(0.0)).astype(np.float32)


def mip_parent_rows(rows):
    """rows uint16 [n, 8, dd]: the eight rows of n child chunks -> uint16 [n, dd], the row of the voxel above each."""
    rows = np.asarray(rows, np.uint16)
    n, _, dd = rows.shape
    v = half_value(rows)
    sigma = v[:, :, dd - 1]
    w = np.where(sigma > 0, sigma, np.float32(0.0)).astype(np.float32)
    W = w[:, 0]
    for i in range(1, 8):
        W = (W + w[:, i]).astype(np.float32)
    t = (w[:, :, None] * v).astype(np.float32)
    S = t[:, 0]
    for i in range(1, 8):
        S = (S + t[:, i]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = (S / W[:, None]).astype(np.float32).astype(np.float16).view(np.uint16)
        out[:, dd - 1] = (W * np.float32(0.125)).astype(np.float32).astype(np.float16).view(np.uint16)
    out[W == 0] = 0
    return out


def mip_rows(data, child):
    """data uint16 [cap, 8, dd], child int32 [cap, 8] -> (data_out, chunk_depth, chunks_at_depth): leaf rows and the rows of chunks that
    were not reached are copied, interior rows are derived from the (already mipped) rows of the voxel's child chunk, deepest first."""
    data = np.asarray(data, np.uint16)
    child = np.asarray(child, np.int32).reshape(-1, 8)
    depth, counts = chunk_depths(child)
    out = data.copy()
    levels = int(np.nonzero(counts)[0].max())
    for d in range(levels - 1, 0, -1):
        chunks = np.nonzero(depth == d)[0]
        rows, cols = np.nonzero(child[chunks])
        c = chunks[rows]
        k = c + child[c, cols]
        out[c, cols] = mip_parent_rows(out[k])
    return out, depth, counts


def truncate(data, child, chunk_depth, max_depth, sample_counts=None):
    """The chunks with 1 <= chunk_depth <= max_depth in ascending order -> dict(child, data, parent, sample_counts, capacity).  `data`
    holds the rows to carry (normally mip_rows')."""
    if max_depth < 1:
        raise ValueError("invalid: max_depth < 1")
    data = np.asarray(data, np.uint16)
    child = np.asarray(child, np.int32).reshape(-1, 8)
    chunk_depth = np.asarray(chunk_depth, np.int32)
    keep = (chunk_depth >= 1) & (chunk_depth <= max_depth)
    rank = (np.cumsum(keep) - keep).astype(np.int64)
    old = np.nonzero(keep)[0]
    n = old.size
    new_child = np.zeros((n, 8), np.int32)
    parent = np.full(n, -1, np.int32)
    links = child[old].astype(np.int64)
    has = (links != 0) & (chunk_depth[old] < max_depth)[:, None]
    rows, cols = np.nonzero(has)
    target = old[rows] + links[rows, cols]
    new_child[rows, cols] = (rank[target] - rank[old[rows]]).astype(np.int32)
    parent[rank[target]] = (rank[old[rows]] * 8 + cols).astype(np.int32)
    return dict(child=new_child, data=data[old].copy(), parent=parent,
                sample_counts=None if sample_counts is None else np.asarray(sample_counts, np.int16).reshape(-1, 8)[old].copy(), capacity=n)


def make_lod(data, child, max_depth, sample_counts=None):
    """mip_rows, then truncate at max_depth: what N3Tree.make_lod builds."""
    mipped, depth, _ = mip_rows(data, child)
    return truncate(mipped, child, depth, max_depth, sample_counts)
