"""numpy restatement of the merge contract of include/mnv.h ("merging two trees": mnv_tree_merge_plan / write, mnv_tree_voxel_cube): a
recursive dual walk over the two trees decides the structure and the sources of every merged voxel, the chunks are then numbered by
(depth, Morton code of the voxel above), and the rows follow from the sources in float32 numpy with the contract's operation order (numpy's
float32 multiply, add and divide are correctly rounded and never contracted; astype(np.float16) is the single round to nearest even)."""
import numpy as np

from lod_ref import half_value

F = np.float32
MAX_DEPTH = 23
OVER, ADD = 0, 1


def voxel_cube(offset, scale, level, corner):
    """mnv_tree_voxel_cube: (offset_out, scale_out) of the depth-`level` voxel with integer corner `corner` of the cube (offset, scale):
    scale_out = scale * 2^level (exact), offset_out = offset * 2^level - corner (the product, then the difference)."""
    two = F(2.0 ** level)
    p = (F(np.asarray(offset, F)) * two).astype(F)
    return (p - np.asarray(corner, np.int64).astype(F)).astype(F), (np.asarray(scale, F) * two).astype(F)


def empty_tree(dd):
    """The one-chunk tree whose eight voxels are empty leaves."""
    return dict(data=np.zeros((1, 8, dd), np.uint16), child=np.zeros((1, 8), np.int32))


def pos(bits):
    """pos(bits) = h(bits) > 0"""
    return half_value(bits) > 0


def sat_half(v):
    """float32 -> binary16 bits, to nearest even, once; a result that would be infinite becomes +-65504."""
    with np.errstate(over="ignore"):
        h = np.asarray(v, F).astype(np.float16)
    bits = h.view(np.uint16).copy()
    inf = (bits & 0x7FFF) == 0x7C00
    bits[inf] = (bits[inf] & 0x8000) | 0x7BFF
    return bits


def walk(a_child, b_child, level=0, corner=(0, 0, 0)):
    """The structure: dict(child int32 [cap, 8], parent int32 [cap], a_vox int32 [cap, 8], b_vox int32 [cap, 8] (-1: none), a_exact /
    b_exact bool [cap, 8] (the source has the voxel exactly), chunks_at_depth int64 [24], capacity, codes: the (depth, Morton code of the
    voxel above) of every chunk in order).  ValueError("invalid ..."): a corner outside 2^level, a followed link outside [1, capacity), more
    merged chunks than the two inputs and the path can give (a chunk reached twice); ValueError("unsupported ..."): a merged depth beyond
    23."""
    a_child = np.asarray(a_child, np.int64).reshape(-1, 8)
    b_child = np.asarray(b_child, np.int64).reshape(-1, 8)
    cap_a, cap_b = a_child.shape[0], b_child.shape[0]
    if not 0 <= level <= 22:
        raise ValueError("invalid: level outside 0 .. 22")
    if any(not 0 <= int(c) < (1 << level) for c in corner):
        raise ValueError("invalid: corner outside 2^level")
    x, y, z = (int(c) for c in corner)
    budget = cap_a + cap_b + level
    chunks = {}

    def digit(l):
        s = level - l
        return 4 * ((x >> s) & 1) + 2 * ((y >> s) & 1) + ((z >> s) & 1)

    def step(ref, links, cap, j):
        """(voxel id, exact, interior, the reference of the chunk below) for a source that is ("chunk", c) or ("leaf", voxel)"""
        if ref[0] == "leaf":
            return ref[1], False, False, ref
        c = ref[1]
        vox, link = c * 8 + j, int(links[c, j])
        if link == 0:
            return vox, True, False, ("leaf", vox)
        if not 1 <= c + link < cap:
            raise ValueError("invalid: a child link leaves the tree")
        return vox, True, True, ("chunk", c + link)

    def visit(d, code, a, b):
        if d > MAX_DEPTH:
            raise ValueError("unsupported: merged depth beyond 23")
        if len(chunks) >= budget:
            raise ValueError("invalid: more merged chunks than the inputs hold (a chunk is reached twice)")
        rec = dict(a_vox=[0] * 8, b_vox=[-1] * 8, a_exact=[False] * 8, b_exact=[False] * 8, interior=[False] * 8)
        chunks[(d, code)] = rec
        below = []
        for j in range(8):
            av, a_exact, a_int, na = step(a, a_child, cap_a, j)
            bv, b_exact, b_int, nb, on_path = -1, False, False, ("none",), False
            if b[0] == "path":
                if j == digit(d):
                    on_path = True
                    nb = ("chunk", 0) if d == level else ("path",)
            elif b[0] != "none":
                bv, b_exact, b_int, nb = step(b, b_child, cap_b, j)
            rec["a_vox"][j], rec["b_vox"][j], rec["a_exact"][j], rec["b_exact"][j] = av, bv, a_exact, b_exact
            if a_int or b_int or on_path:
                rec["interior"][j] = True
                below.append((j, na, nb))
        for j, na, nb in below:
            visit(d + 1, code * 8 + j, na, nb)

    visit(1, 0, ("chunk", 0), ("chunk", 0) if level == 0 else ("path",))
    order = sorted(chunks)
    index = {key: i for i, key in enumerate(order)}
    cap = len(order)
    out = dict(child=np.zeros((cap, 8), np.int32), parent=np.full(cap, -1, np.int32), a_vox=np.zeros((cap, 8), np.int32),
               b_vox=np.full((cap, 8), -1, np.int32), a_exact=np.zeros((cap, 8), bool), b_exact=np.zeros((cap, 8), bool),
               chunks_at_depth=np.zeros(24, np.int64), capacity=cap, codes=order)
    for (d, code), i in index.items():
        rec = chunks[(d, code)]
        out["chunks_at_depth"][d] += 1
        for k in ("a_vox", "b_vox", "a_exact", "b_exact"):
            out[k][i] = rec[k]
        for j in range(8):
            if rec["interior"][j]:
                k = index[(d + 1, code * 8 + j)]
                out["child"][i, j] = k - i
                out["parent"][k] = i * 8 + j
    return out


def rows(a_data, b_data, a_vox, b_vox, mode, a_counts=None, b_counts=None):
    """(data uint16 [n, dd], sample_counts int16 [n], kind uint8 [n]: 0 A's row, 1 B's row, 2 blended) of n merged voxels."""
    a_data, b_data = np.asarray(a_data, np.uint16), np.asarray(b_data, np.uint16)
    dd = a_data.shape[-1]
    a_rows, b_rows = a_data.reshape(-1, dd), b_data.reshape(-1, dd)
    a_vox, b_vox = np.asarray(a_vox, np.int64).reshape(-1), np.asarray(b_vox, np.int64).reshape(-1)
    ra, rb = a_rows[a_vox], b_rows[np.maximum(b_vox, 0)]
    ca = np.full(a_vox.size, 8, np.int64) if a_counts is None else np.asarray(a_counts, np.int16).reshape(-1)[a_vox].astype(np.int64)
    cb = np.full(a_vox.size, 8, np.int64) if b_counts is None else np.asarray(b_counts, np.int16).reshape(-1)[np.maximum(b_vox, 0)].astype(np.int64)
    take_b = (b_vox >= 0) & pos(rb[:, dd - 1])
    blend = take_b & pos(ra[:, dd - 1]) if mode == ADD else np.zeros_like(take_b)
    kind = np.where(blend, 2, np.where(take_b, 1, 0)).astype(np.uint8)
    data = np.where((kind == 1)[:, None], rb, ra)
    counts = np.where(kind == 1, cb, ca)
    if blend.any():
        va, vb = half_value(ra[blend]), half_value(rb[blend])
        wa, wb = va[:, dd - 1], vb[:, dd - 1]
        W = (wa + wb).astype(F)
        ta, tb = (wa[:, None] * va).astype(F), (wb[:, None] * vb).astype(F)
        mixed = sat_half(((ta + tb).astype(F) / W[:, None]).astype(F))
        mixed[:, dd - 1] = sat_half(W)
        data[blend] = mixed
        counts[blend] = np.clip(ca[blend] + cb[blend], -32768, 32767)
    return data, counts.astype(np.int16), kind


def merge(a, b, level=0, corner=(0, 0, 0), mode=OVER):
    """mnv_tree_merge_plan + write.  a, b: dict(data uint16 [cap, 8, dd], child int32 [cap, 8], sample_counts int16 [cap, 8] or absent).
    -> dict(child, data, parent, sample_counts, src_a, src_b, stats, capacity)."""
    if a["data"].shape[-1] != b["data"].shape[-1]:
        raise ValueError("invalid: mismatched row formats")
    s = walk(a["child"], b["child"], level, corner)
    cap, dd = s["capacity"], a["data"].shape[-1]
    data, counts, kind = rows(a["data"], b["data"], s["a_vox"], s["b_vox"], mode, a.get("sample_counts"), b.get("sample_counts"))
    stats = dict(chunks_at_depth=[int(v) for v in s["chunks_at_depth"]], capacity=cap, rows_from_a=int((kind == 0).sum()), rows_from_b=int((kind == 1).sum()),
                 rows_blended=int((kind == 2).sum()), pushed_a=int((~s["a_exact"]).sum()), pushed_b=int(((s["b_vox"] >= 0) & ~s["b_exact"]).sum()))
    return dict(child=s["child"], data=data.reshape(cap, 8, dd), parent=s["parent"], sample_counts=counts.reshape(cap, 8), src_a=s["a_vox"], src_b=s["b_vox"],
                stats=stats, capacity=cap)


def structure(child):
    """The set of (depth, Morton code of the voxel above) of every chunk reached from the root: what two isomorphic trees share."""
    child = np.asarray(child, np.int64).reshape(-1, 8)
    out, front = set(), [(0, 1, 0)]
    while front:
        c, d, code = front.pop()
        out.add((d, code))
        for j in range(8):
            if child[c, j]:
                front.append((c + int(child[c, j]), d + 1, code * 8 + j))
    return out
