"""numpy restatement of the culling contract of include/mnv.h ("culling a tree to a pose set": mnv_rays_visibility, mnv_tree_cull,
mnv_n3tree_make_culled).  The march is fit_ref.forward -- mnv_rays_grad's forward, which tests/test_fit_ref.py holds against the oracle --
whose batches carry the leaf voxel and the weight of every dense sample; the visibility words are np.maximum.at on their uint32 view.
tree_cull is a plain recursive walk; the cut is view_lod_ref.cut."""
import numpy as np

import fit_ref
import lod_ref
import view_lod_ref

VIS_SUMS = ("n_rays", "n_stopped", "n_samples", "n_skipped")


def rays_visibility(T, opt, origins, dirs, tmax=None, wmax=None):
    """mnv_rays_visibility restated: -> (wmax uint32 [capacity * 8] -- the given array, updated, or a new one --, sums dict, the forward
    march).  A skipped (broken) ray adds nothing; a sample whose weight is not > 0 (NaN included) writes nothing."""
    fw = fit_ref.forward(T, opt, origins, dirs, tmax)
    if wmax is None:
        wmax = np.zeros(T["capacity"] * 8, np.uint32)
    ok = ~fw["broken"]
    with np.errstate(invalid="ignore"):
        for b in fw["batches"]:
            take = ok[b["ray"]] & (b["w"] > 0)
            np.maximum.at(wmax, b["vox"][take], np.ascontiguousarray(b["w"][take], np.float32).view(np.uint32))
    sums = dict(n_rays=int(ok.sum()), n_stopped=int((ok & fw["stopped"]).sum()), n_samples=int(fw["n_dense"][ok].sum()), n_skipped=int((~ok).sum()))
    return wmax, sums, fw


def tree_cull(data, child, wmax, weight_thresh):
    """mnv_tree_cull restated.  data uint16 [cap, 8, dd], child int32 [cap, 8], wmax uint32 [cap * 8] -> dict(data, keep uint8 [cap],
    kept_at_depth int64 [24], counts dict(leaves_seen, leaves_culled, dead_chunks)).  ValueError("invalid" / "unsupported") as the entry
    point refuses (the links: lod_ref.chunk_depths)."""
    thresh = np.float32(weight_thresh)
    if not np.isfinite(thresh) or thresh < 0:
        raise ValueError("invalid: weight_thresh")
    data = np.asarray(data, np.uint16)
    child = np.asarray(child, np.int64).reshape(-1, 8)
    cap = child.shape[0]
    lod_ref.chunk_depths(child)                                        # refuses what the walk refuses
    with np.errstate(invalid="ignore"):
        seen = np.ascontiguousarray(wmax, np.uint32).reshape(cap, 8).view(np.float32) > thresh      # strict; a NaN pattern is not seen
    full = lod_ref.half_value(data[:, :, -1]) > 0
    out = data.copy()
    keep = np.zeros(cap, np.uint8)
    kept = np.zeros(24, np.int64)
    counts = dict(leaves_seen=0, leaves_culled=0, dead_chunks=0)

    def visit(k, d):
        live = False
        for j in range(8):
            if child[k, j] == 0:
                if seen[k, j]:
                    live = True
                    counts["leaves_seen"] += 1
                else:
                    counts["leaves_culled"] += int(full[k, j])
                    out[k, j] = 0
            elif visit(k + child[k, j], d + 1):
                live = True
            else:
                out[k, j] = 0                                           # the voxel above a dead chunk
        keep[k] = 1 if (live or k == 0) else 0                          # the root chunk always stays
        if keep[k]:
            kept[d] += 1
        else:
            counts["dead_chunks"] += 1
        return live

    visit(0, 1)
    return dict(data=out, keep=keep, kept_at_depth=kept, counts=counts)


def parent_closed(child, keep):
    """every kept chunk but the root hangs under a kept chunk"""
    child = np.asarray(child, np.int64).reshape(-1, 8)
    rows, cols = np.nonzero(child)
    target = rows + child[rows, cols]
    has_kept_parent = np.zeros(child.shape[0], bool)
    has_kept_parent[target[keep[rows] != 0]] = True
    return bool(keep[0]) and bool(has_kept_parent[np.nonzero(keep)[0][1:]].all())


def make_culled(T, opt, ray_lists, weight_thresh, sample_counts=None):
    """mnv_n3tree_make_culled restated on a fit_ref.tree_of dict: ray_lists: sequence of (origins, dirs[, tmax]).  -> dict(wmax, cull (tree_cull's
    dict), cut (view_lod_ref.cut's dict: child, data, parent, sample_counts, capacity))"""
    wmax = np.zeros(T["capacity"] * 8, np.uint32)
    for rays in ray_lists:
        rays_visibility(T, opt, *rays, wmax=wmax)
    data = T["data"].reshape(T["capacity"], 8, T["data_dim"])
    child = T["child"].reshape(T["capacity"], 8)
    cull = tree_cull(data, child, wmax, weight_thresh)
    return dict(wmax=wmax, cull=cull, cut=view_lod_ref.cut(cull["data"], child, cull["keep"], sample_counts))


def as_tree(T, data, child):
    """a fit_ref tree dict with other arrays (the culled rows, the cut tree)"""
    out = dict(T)
    child = np.asarray(child, np.int32)
    out.update(data=np.ascontiguousarray(data, np.uint16).reshape(-1, T["data_dim"]), child=child.reshape(-1), capacity=int(child.reshape(-1, 8).shape[0]))
    return out
