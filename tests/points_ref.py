"""numpy restatement of the points contract of include/mnv.h ("a tree from a coloured point cloud": mnv_point_tree_*): voxel codes, drops,
records, occupancy, breadth-first numbering, child, parent, rows, counts, stats.  Everything after the voxel of a point is integer arithmetic."""
import numpy as np

F = np.float32
U = np.uint64
C0 = 0.28209479177387814


def data_dim(fmt):
    return 4 if fmt == "RGBA" else 3 * int(fmt[2:]) + 1


def colour_table(fmt):
    """uint16 [256]: the half bits of an 8-bit mean in a row of `fmt`."""
    v = np.arange(256)
    if fmt == "RGBA":
        return np.float16(F(v) / F(255)).view(np.uint16)
    x = np.clip(v.astype(np.float64) / 255.0, 1.0 / 512.0, 511.0 / 512.0)
    return np.float16(F(np.log(x / (1.0 - x)) / C0)).view(np.uint16)


def voxel_codes(xyz, offset, scale, depth):
    """(code uint64 [n], accepted bool [n]): q = offset + scale * p, product then sum in binary32; dropped unless p and q are finite and
    0 <= q < 1; i = floor(q * 2^D); the code interleaves the bits of (i_x, i_y, i_z), x first."""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        m = F(scale)[None, :] * p
        q = F(offset)[None, :] + m
        ok = (np.isfinite(p) & np.isfinite(q) & (q >= F(0)) & (q < F(1))).all(axis=1)
        cell = np.floor(np.where(ok[:, None], q, F(0)) * F(2.0 ** depth)).astype(np.int64)
    code = np.zeros(p.shape[0], U)
    for level in range(depth):                  # bit `level` of each axis, from the least significant
        for k in range(3):
            bit = ((cell[:, k] >> level) & 1).astype(U)
            code |= bit << U(3 * level + (2 - k))
    return code, ok


def records(xyz, rgb, offset, scale, depth):
    """(codes uint64 [r] ascending, n int64 [r], sums int64 [r, 3], dropped)."""
    code, ok = voxel_codes(xyz, offset, scale, depth)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)[ok].astype(np.int64)
    code = code[ok]
    order = np.argsort(code, kind="stable")
    code, rgb = code[order], rgb[order]
    if code.size == 0:
        return code, np.zeros(0, np.int64), np.zeros((0, 3), np.int64), int((~ok).sum())
    head = np.concatenate([[True], code[1:] != code[:-1]])
    starts = np.nonzero(head)[0]
    n = np.diff(np.concatenate([starts, [code.size]]))
    sums = np.add.reduceat(rgb, starts, axis=0)
    return code[starts], n.astype(np.int64), sums, int((~ok).sum())


def build(xyz, rgb, offset, scale, depth, fmt="RGBA", min_points=1, sigma=100.0, table=None):
    """mnv_point_tree_create / add / finish / write: dict(child int32 [cap, 8], data uint16 [cap, 8, dd], parent int32 [cap], sample_counts
    int16 [cap, 8], counts uint32 [cap, 8], stats dict, capacity, occupied uint64 codes)."""
    dd = data_dim(fmt)
    stride = 1 if fmt == "RGBA" else int(fmt[2:])
    table = colour_table(fmt) if table is None else table
    codes, n, sums, dropped = records(xyz, rgb, offset, scale, depth)
    occ = n >= min_points
    level = {depth + 1: codes[occ]}             # level[d], d = 2 .. D: the code of the voxel above every chunk of depth d
    for d in range(depth, 1, -1):
        level[d] = np.unique(level[d + 1] >> U(3))
    level[1] = np.zeros(1, U)                    # the root always exists
    at_depth = [0] * 24
    first = {}
    cap = 0
    for d in range(1, depth + 1):
        at_depth[d] = int(level[d].size)
        first[d] = cap
        cap += at_depth[d]
    child = np.zeros((cap, 8), np.int32)
    parent = np.full(cap, -1, np.int32)
    data = np.zeros((cap, 8, dd), np.uint16)
    counts = np.zeros((cap, 8), np.uint32)
    for d in range(2, depth + 1):               # every chunk of depth d hangs under voxel j of the chunk of its code >> 3
        v = level[d]
        if v.size == 0:
            continue
        up = np.searchsorted(level[d - 1], v >> U(3)) if d > 2 else np.zeros(v.size, np.int64)
        assert d == 2 or np.array_equal(level[d - 1][up], v >> U(3))
        j = (v & U(7)).astype(np.int64)
        me = first[d] + np.arange(v.size)
        above = first[d - 1] + up
        child[above, j] = (me - above).astype(np.int32)
        parent[me] = (above * 8 + j).astype(np.int32)
    # depth-D voxels of the chunks that exist
    if codes.size:
        if depth == 1:
            k, there = np.zeros(codes.size, np.int64), np.ones(codes.size, bool)
        elif level[depth].size == 0:
            k, there = np.zeros(codes.size, np.int64), np.zeros(codes.size, bool)
        else:
            top, pre = level[depth], codes >> U(3)
            k = np.minimum(np.searchsorted(top, pre), top.size - 1)
            there = top[k] == pre
            k = np.where(there, k, 0)
        c = first[depth] + k
        j = (codes & U(7)).astype(np.int64)
        counts[c[there], j[there]] = n[there].astype(np.uint32)
        sel = there & occ
        mean = (2 * sums[sel] + n[sel, None]) // (2 * n[sel, None])
        assert ((mean >= 0) & (mean <= 255)).all()
        half_sigma = np.float16(F(sigma)).view(np.uint16)
        for ch in range(3):
            data[c[sel], j[sel], ch * stride] = table[mean[:, ch]]
        data[c[sel], j[sel], dd - 1] = half_sigma
    stats = dict(accepted=int(n.sum()), dropped=dropped, distinct_voxels=int(codes.size), occupied_voxels=int(occ.sum()), chunks_at_depth=at_depth)
    return dict(child=child, data=data, parent=parent, sample_counts=np.full((cap, 8), 8, np.int16), counts=counts, stats=stats, capacity=cap,
                occupied=codes[occ])


def brute_force_voxels(xyz, offset, scale, depth):
    """{(i_x, i_y, i_z): count} with Python floats rounded step by step -- no code, no sort."""
    out = {}
    for p in np.ascontiguousarray(xyz, F).reshape(-1, 3):
        cell = []
        for k in range(3):
            with np.errstate(all="ignore"):
                q = F(F(offset[k]) + F(F(scale[k]) * p[k]))
            if not (np.isfinite(p[k]) and np.isfinite(q) and F(0) <= q < F(1)):
                cell = None
                break
            cell.append(int(np.floor(float(q) * 2.0 ** depth)))
        if cell is not None:
            out[tuple(cell)] = out.get(tuple(cell), 0) + 1
    return out


def code_of_cell(cell, depth):
    code = 0
    for level in range(depth):
        for k in range(3):
            code |= ((cell[k] >> level) & 1) << (3 * level + (2 - k))
    return code
