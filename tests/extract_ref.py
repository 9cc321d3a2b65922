"""numpy restatement of the geometry contract of include/mnv.h: the point query of mnv_accel_sample_points and the surface of
mnv_extract_surface.  Every float operation is float32 in the order the contract states (numpy's float32 division and square root are
correctly rounded; numpy never contracts a multiply and an add).  Inputs are the host arrays of N3Tree.host_arrays()."""
import numpy as np

import primitives_ref as pr

F = np.float32
CLAMP_HI = F(1.0) - F(1e-6)


def descend(child, u):
    """query_single_from_root (rt_core.cuh:125-150) for tree-space points u float32 [n, 3] (copied): (chunk, child index, depth) int64 [n]."""
    u = np.array(u, F).reshape(-1, 3)
    u = np.maximum(np.minimum(u, CLAMP_HI), F(0.0))
    n = u.shape[0]
    chunk = np.zeros(n, np.int64)
    leaf = np.zeros(n, np.int64)
    depth = np.ones(n, np.int64)
    live = np.arange(n)
    for _ in range(64):
        if live.size == 0:
            break
        x = u[live] * F(2.0)
        f = np.floor(x)
        u[live] = x - f
        c = (f[:, 0].astype(np.int64) * 2 + f[:, 1].astype(np.int64)) * 2 + f[:, 2].astype(np.int64)
        skip = child[chunk[live], c].astype(np.int64)
        stop = skip == 0
        leaf[live[stop]] = c[stop]
        go = ~stop
        chunk[live[go]] += skip[go]
        depth[live[go]] += 1
        live = live[go]
    assert live.size == 0, "the tree is deeper than 64 levels (or has a cycle)"
    return chunk, leaf, depth


def sample_points(data, child, offset, scale, points):
    """mnv_accel_sample_points: (voxel int32 [n], depth int32 [n], sigma float32 [n]) for world-space points float32 [n, 3]."""
    p = np.array(points, F).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1)
    with np.errstate(all="ignore"):
        u = np.asarray(offset, F)[None, :] + np.where(ok[:, None], p, F(0.0)) * np.asarray(scale, F)[None, :]
    chunk, leaf, depth = descend(child, u)
    sigma = pr.half_bits_to_float(data[chunk, leaf, -1])
    voxel = (chunk * 8 + leaf).astype(np.int32)
    voxel[~ok] = -1
    depth = depth.astype(np.int32)
    depth[~ok] = 0
    sigma[~ok] = F(0.0)
    return voxel, depth, sigma


def lattice(data, child, level):
    """S float32 [n, n, n] and the voxel int64 [n, n, n] behind each sample of the level's lattice (tree-space points ((i + 0.5) / n, ..))."""
    n = 1 << level
    c = (np.arange(n, dtype=F) + F(0.5)) / F(n)          # exact in binary32
    u = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    chunk, leaf, _ = descend(child, u)
    bits = data[chunk, leaf, -1]
    s = pr.half_bits_to_float(bits)
    s[(bits & 0x7C00) == 0x7C00] = F(0.0)                  # sigma bits that are not finite read as 0
    return s.reshape(n, n, n), (chunk * 8 + leaf).reshape(n, n, n)


def colours(data, basis_dim, voxel, normal):
    """The march's colour of a sample of `voxel` seen along d = -normal: basis_dim -1 = RGBA rows, else SH rows of that many coefficients."""
    rows = data.reshape(-1, data.shape[-1])[voxel]
    if basis_dim < 0:
        return pr.half_bits_to_float(rows[:, :3])
    b = pr.sh_basis(basis_dim, -np.asarray(normal, F))
    tmp = pr.sh_channels(basis_dim, b, np.ascontiguousarray(rows[:, :3 * basis_dim]))
    return pr.sigmoid_exact(np.ones_like(tmp), tmp)


def extract(data, child, offset, scale, level, iso, colour=True, basis_dim=None):
    """mnv_extract_surface: (vert float32 [V, 9], faces uint32 [T, 3], info).  basis_dim: -1 for RGBA rows, the SH basis size otherwise
    (needed with colour).  info: cells int64 [V, 3] (the active cells in vertex order), local float32 [V, 3], samples, inside."""
    offset, scale, iso = np.asarray(offset, F), np.asarray(scale, F), F(iso)
    n = 1 << level
    m = n - 1                                               # cells per axis
    S, VOX = lattice(data, child, level)
    inside = S > iso
    corner = [((k >> 2) & 1, (k >> 1) & 1, k & 1) for k in range(8)]

    def at(a, k):                                           # corner k of every cell
        dx, dy, dz = corner[k]
        return a[dx:dx + m, dy:dy + m, dz:dz + m]

    n_in = sum(at(inside, k).astype(np.int32) for k in range(8))
    active = (n_in > 0) & (n_in < 8)
    cells = np.argwhere(active).astype(np.int64)
    nb = n // 8
    key = (((cells[:, 0] >> 3) * nb + (cells[:, 1] >> 3)) * nb + (cells[:, 2] >> 3)) * 512 + ((cells[:, 0] & 7) * 8 + (cells[:, 1] & 7)) * 8 + (cells[:, 2] & 7)
    cells = cells[np.argsort(key, kind="stable")]
    V = cells.shape[0]
    cx, cy, cz = cells[:, 0], cells[:, 1], cells[:, 2]
    Sc = np.stack([S[cx + d[0], cy + d[1], cz + d[2]] for d in corner], axis=1).astype(F) if V else np.zeros((0, 8), F)
    ins = Sc > iso
    total = np.zeros((V, 3), F)
    count = np.zeros(V, np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            bit = 4 >> a
            for k0 in range(8):
                if k0 & bit:
                    continue
                k1 = k0 | bit
                cross = ins[:, k0] != ins[:, k1]
                t = (iso - Sc[:, k0]) / (Sc[:, k1] - Sc[:, k0])
                p = np.empty((V, 3), F)
                p[:] = np.array(corner[k0], F)
                p[:, a] = t
                total = np.where(cross[:, None], total + p, total)
                count += cross
        local = total / count.astype(F)[:, None]
        u = ((cells.astype(F) + local) + F(0.5)) * F(2.0 ** -level)
        pos = (u - offset[None, :]) / scale[None, :]
        g = np.empty((V, 3), F)
        for a in range(3):
            bit = 4 >> a
            hi = [k for k in range(8) if k & bit]
            lo = [k for k in range(8) if not k & bit]
            g[:, a] = (((Sc[:, hi[0]] + Sc[:, hi[1]]) + Sc[:, hi[2]]) + Sc[:, hi[3]]) - (((Sc[:, lo[0]] + Sc[:, lo[1]]) + Sc[:, lo[2]]) + Sc[:, lo[3]])
        w = -(g * scale[None, :])
        ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        normal = w / ln[:, None]
    bad = (ln == 0) | ~np.isfinite(ln)
    normal[bad] = (0.0, 0.0, 1.0)
    vert = np.empty((V, 9), F)
    vert[:, 0:3] = pos
    vert[:, 6:9] = normal
    if colour and V:
        best = np.argmax(Sc, axis=1)                        # the first of equal maxima
        d = np.array(corner, np.int64)[best]
        vert[:, 3:6] = colours(data, basis_dim, VOX[cx + d[:, 0], cy + d[:, 1], cz + d[:, 2]], normal)
    else:
        vert[:, 3:6] = F(1.0)
    # faces
    rank = np.full((m, m, m), -1, np.int64)
    rank[cx, cy, cz] = np.arange(V)
    quads, keys = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        e = np.zeros(3, np.int64)
        e[a] = 1
        owner = np.zeros((m, m, m), bool)
        owner[:] = inside[:m, :m, :m] != inside[e[0]:e[0] + m, e[1]:e[1] + m, e[2]:e[2] + m]
        p = np.argwhere(owner).astype(np.int64)
        p = p[(p[:, b] >= 1) & (p[:, c] >= 1)]
        if p.shape[0] == 0:
            continue
        eb, ec = np.zeros(3, np.int64), np.zeros(3, np.int64)
        eb[b], ec[c] = 1, 1

        def ids(q):
            r = rank[q[:, 0], q[:, 1], q[:, 2]]
            assert (r >= 0).all(), "a quad names a cell that is not active"
            return r

        i0, i1, i2, i3 = ids(p - eb - ec), ids(p - ec), ids(p), ids(p - eb)
        in0 = inside[p[:, 0], p[:, 1], p[:, 2]]
        ia, ic = np.where(in0, i1, i3), np.where(in0, i3, i1)
        quads.append(np.stack([i0, ia, i2, i0, i2, ic], axis=1))
        keys.append(i2 * 3 + a)
    if quads:
        quads = np.concatenate(quads)[np.argsort(np.concatenate(keys), kind="stable")]
        faces = quads.reshape(-1, 3).astype(np.uint32)
    else:
        faces = np.zeros((0, 3), np.uint32)
    return vert, faces, dict(cells=cells, local=local, samples=S, inside=inside)


def reindex_like_load_obj(vert, faces):
    """What Mesh::load_obj makes of an OBJ file that names vertex i as `i//i`: vertices in order of first use by a face (a vertex no face
    names is gone), faces renumbered."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order, first = [], {}
    for v in flat:
        if int(v) not in first:
            first[int(v)] = len(order)
            order.append(int(v))
    new_faces = np.array([first[int(v)] for v in flat], np.uint32).reshape(-1, 3)
    return np.asarray(vert, F).reshape(-1, 9)[order], new_faces
