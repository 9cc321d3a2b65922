"""A numpy restatement of the two view-dependent level-of-detail contracts of include/mnv.h (mnv_tree_select_cut, mnv_tree_cut).  Every
float operation is one float32 operation in the order the contract states (numpy's float32 add, subtract, multiply, divide and maximum are
correctly rounded, never contracted, and keep subnormals); integers times a power of two are exact.  Depths and the mip are lod_ref's."""
import numpy as np

import lod_ref

MAX_DEPTH = lod_ref.MAX_DEPTH
MAX_VIEWS = 4096
f32 = np.float32


def view_tables(offset, scale, views, pixels):
    """views: sequence of (eye[3], focal_px) -> (q float32 [n, 3], R2 float32 [n, 24]): the host half of mnv_tree_select_cut.
    q = offset + scale * eye (a product, then a sum); R2[v][d] = r * r with e_d = max_k(2^-d / scale[k]), r = (focal_px * e_d) / pixels;
    pixels == 0 makes every R2 +inf.  ValueError("invalid") as the entry point refuses."""
    offset, scale = np.asarray(offset, f32).reshape(3), np.asarray(scale, f32).reshape(3)
    if not (np.isfinite(scale).all() and (scale > 0).all() and np.isfinite(offset).all()):
        raise ValueError("invalid: offset / scale")
    pixels = f32(pixels)
    if not np.isfinite(pixels) or pixels < 0:
        raise ValueError("invalid: pixels")
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError("invalid: n_views")
    q = np.zeros((len(views), 3), f32)
    R2 = np.full((len(views), 24), np.inf, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for v, (eye, focal) in enumerate(views):
            eye, focal = np.asarray(eye, f32).reshape(3), f32(focal)
            if not (np.isfinite(eye).all() and np.isfinite(focal) and focal > 0):
                raise ValueError("invalid: eye / focal_px")
            q[v] = offset + (scale * eye).astype(f32)
            if not np.isfinite(q[v]).all():
                raise ValueError("invalid: the eye leaves binary32 in tree space")
            if pixels == 0:
                continue
            for d in range(24):
                e = (f32(2.0 ** -d) / scale).astype(f32).max()
                r = f32(f32(focal * e) / pixels)
                R2[v, d] = f32(r * r)
    return q, R2


def refines(ix, d, q, R2, scale):
    """ix int64 [n, 3]: integer corners of voxels of depth d -> bool [n]: D2 <= R2[v][d] for some view v."""
    scale = np.asarray(scale, f32).reshape(3)
    inv = f32(2.0 ** -d)
    lo = (ix.astype(f32) * inv).astype(f32)
    hi = ((ix + 1).astype(f32) * inv).astype(f32)
    out = np.zeros(ix.shape[0], bool)
    with np.errstate(over="ignore", under="ignore"):
        for v in range(q.shape[0]):
            g = np.maximum(np.maximum((lo - q[v]).astype(f32), (q[v] - hi).astype(f32)), f32(0.0)).astype(f32)
            w = (g / scale).astype(f32)
            D2 = (((w[:, 0] * w[:, 0]).astype(f32) + (w[:, 1] * w[:, 1]).astype(f32)).astype(f32) + (w[:, 2] * w[:, 2]).astype(f32)).astype(f32)
            out |= D2 <= R2[v, d]
    return out


def select_cut(child, offset, scale, views, pixels, min_depth, max_depth):
    """child int32 [cap, 8] -> (keep uint8 [cap], kept_at_depth int64 [24]).  The root chunk is kept; the child chunk of voxel j of a kept
    chunk of depth d is kept iff d < max_depth and (d < min_depth or refines).  Only links that are followed are checked:
    ValueError("invalid") for one outside [1, cap) or a chunk reached twice, ValueError("unsupported") beyond 23 levels."""
    if min_depth < 1 or max_depth < min_depth:
        raise ValueError("invalid: min_depth / max_depth")
    child = np.asarray(child, np.int64).reshape(-1, 8)
    cap = child.shape[0]
    q, R2 = view_tables(offset, scale, views, pixels)
    keep = np.zeros(cap, np.uint8)
    counts = np.zeros(24, np.int64)
    keep[0] = 1
    counts[1] = 1
    front, corner, d = np.array([0], np.int64), np.zeros((1, 3), np.int64), 1      # corner: of the voxel above the chunk, at depth d - 1
    while d < max_depth:
        rows, cols = np.nonzero(child[front])
        ix = corner[rows] * 2 + np.stack([cols >> 2, (cols >> 1) & 1, cols & 1], axis=1)
        take = np.ones(rows.size, bool) if d < min_depth else refines(ix, d, q, R2, scale)
        rows, cols, ix = rows[take], cols[take], ix[take]
        target = front[rows] + child[front[rows], cols]
        if target.size == 0:
            break
        if (target < 1).any() or (target >= cap).any():
            raise ValueError("invalid: a child link leaves the tree")
        if np.unique(target).size != target.size or (keep[target] != 0).any():
            raise ValueError("invalid: a chunk is reached twice")
        if d + 1 > MAX_DEPTH:
            raise ValueError("unsupported: more than 23 levels")
        d += 1
        keep[target] = 1
        counts[d] = target.size
        order = np.argsort(target)
        front, corner = target[order], ix[order]
    return keep, counts


def cut(data, child, keep, sample_counts=None):
    """The chunks with keep != 0 in ascending order -> dict(child, data, parent, sample_counts, capacity); lod_ref.truncate with another
    survivor predicate.  A link is carried iff it leads to a kept chunk inside the tree; `keep` is the caller's to make parent-closed."""
    data = np.asarray(data, np.uint16)
    child = np.asarray(child, np.int64).reshape(-1, 8)
    keep = np.asarray(keep) != 0
    cap = child.shape[0]
    if not keep[0]:
        raise ValueError("invalid: the root chunk is not kept")
    rank = (np.cumsum(keep) - keep).astype(np.int64)
    old = np.nonzero(keep)[0]
    n = old.size
    target = old[:, None] + child[old]
    inside = (child[old] != 0) & (target >= 1) & (target < cap)
    has = inside & keep[np.where(inside, target, 0)]
    rows, cols = np.nonzero(has)
    new_child = np.zeros((n, 8), np.int32)
    parent = np.full(n, -1, np.int32)
    new_child[rows, cols] = (rank[target[rows, cols]] - rank[old[rows]]).astype(np.int32)
    parent[rank[target[rows, cols]]] = (rank[old[rows]] * 8 + cols).astype(np.int32)
    return dict(child=new_child, data=data[old].copy(), parent=parent,
                sample_counts=None if sample_counts is None else np.asarray(sample_counts, np.int16).reshape(-1, 8)[old].copy(), capacity=n)


def make_view_lod(data, child, offset, scale, views, pixels, min_depth=1, max_depth=MAX_DEPTH, sample_counts=None):
    """mip_rows, select_cut, then cut: what N3Tree.make_view_lod builds."""
    mipped, _, _ = lod_ref.mip_rows(data, child)
    keep, counts = select_cut(child, offset, scale, views, pixels, min_depth, max_depth)
    out = cut(mipped, child, keep, sample_counts)
    out["keep"], out["kept_at_depth"] = keep, counts
    return out
