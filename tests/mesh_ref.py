"""numpy restatement of the raster contract of mnv_render_meshes (include/mnv.h, steps A-G) and of mnv_model_matrix.  Every float
operation is float32 in the order the contract states (numpy's float32 division and square root are correctly rounded)."""
import numpy as np

F = np.float32
NEAR = F(1e-3)
EMPTY = np.iinfo(np.uint64).max
L1 = np.array([0.4402254521846771, 0.17609018087387085, 0.8804509043693542], F)
L2 = np.array([-0.40824830532073975, -0.8164966106414795, -0.40824830532073975], F)


class RefMesh:
    def __init__(self, vert, faces=None, face_size=3, unlit=False, matrix=None, visible=True):
        self.vert = np.ascontiguousarray(vert, F).reshape(-1, 9)
        self.faces = None if faces is None else np.ascontiguousarray(faces, np.int64).reshape(-1, face_size)
        self.face_size, self.unlit, self.visible = face_size, unlit, visible
        self.matrix = np.eye(3, 4, dtype=F) if matrix is None else np.asarray(matrix, F).reshape(3, 4)

    def prims(self):
        return self.faces if self.faces is not None else np.arange(self.vert.shape[0], dtype=np.int64).reshape(-1, self.face_size)


def model_matrix(rotation, translation, scale):
    """Double-precision Rodrigues formula (an independent statement of Mesh::draw's matrix): R = I + sin(t) K + (1 - cos(t)) K^2."""
    r = np.asarray(rotation, F).astype(np.float64)
    t = np.linalg.norm(r)
    R = np.eye(3)
    if not t < 1e-3:
        k = r / t
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    M = np.empty((3, 4))
    M[:, :3] = R * float(F(scale))
    M[:, 3] = np.asarray(translation, F)
    return M


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _to_cam(m, w):
    d0, d1, d2 = w[..., 0] - m[9], w[..., 1] - m[10], w[..., 2] - m[11]
    X = (m[0] * d0 + m[1] * d1) + m[2] * d2
    Y = (m[3] * d0 + m[4] * d1) + m[5] * d2
    Z = -((m[6] * d0 + m[7] * d1) + m[8] * d2)
    return np.stack([X, Y, Z], axis=-1).astype(F)


def _world(M, p):
    return np.stack([((M[c, 0] * p[..., 0] + M[c, 1] * p[..., 1]) + M[c, 2] * p[..., 2]) + M[c, 3] for c in range(3)], axis=-1).astype(F)


def _normals(M, a):
    t = np.stack([(M[c, 0] * a[..., 0] + M[c, 1] * a[..., 1]) + M[c, 2] * a[..., 2] for c in range(3)], axis=-1).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])
        return (t / ln[..., None]).astype(F)


def _key(Z, dist):
    return (Z.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | dist.astype(F).view(np.uint32).astype(np.uint64)


def _expand(cnt):
    """index of the owner and running index inside it for `cnt[i]` items each"""
    own = np.repeat(np.arange(cnt.size), cnt)
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    return own, np.arange(own.size) - first


def _line_fragments(A, B, view):
    """steps 2-5 of the wireframe contract on camera-space endpoints [n, 3]: (prim, px, py, w [k, 3], XYZ [k, 3], dist)"""
    x0, y0, w, h, fx, fy, cx, cy = view
    idx = np.arange(A.shape[0])
    Xa, Ya, za, Xb, Yb, zb = (A[:, 0].copy(), A[:, 1].copy(), A[:, 2].copy(), B[:, 0].copy(), B[:, 1].copy(), B[:, 2].copy())
    keep = ~((za < NEAR) & (zb < NEAR))
    idx, Xa, Ya, za, Xb, Yb, zb = (a[keep] for a in (idx, Xa, Ya, za, Xb, Yb, zb))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ca = za < NEAR
        t = (NEAR - za[ca]) / (zb[ca] - za[ca])
        Xa[ca] = Xa[ca] + t * (Xb[ca] - Xa[ca])
        Ya[ca] = Ya[ca] + t * (Yb[ca] - Ya[ca])
        za[ca] = NEAR
        cb = (zb < NEAR) & ~ca
        t = (NEAR - zb[cb]) / (za[cb] - zb[cb])
        Xb[cb] = Xb[cb] + t * (Xa[cb] - Xb[cb])
        Yb[cb] = Yb[cb] + t * (Ya[cb] - Yb[cb])
        zb[cb] = NEAR
        pxa, pya = cx + fx * (Xa / za), cy - fy * (Ya / za)
        pxb, pyb = cx + fx * (Xb / zb), cy - fy * (Yb / zb)
        dx, dy = pxb - pxa, pyb - pya
        dd = dx * dx + dy * dy
    ok = (dd > 0) & np.isfinite(dd)
    idx, Xa, Ya, za, Xb, Yb, zb, pxa, pya, pxb, pyb, dx, dy, dd = (a[ok] for a in (idx, Xa, Ya, za, Xb, Yb, zb, pxa, pya, pxb, pyb, dx, dy, dd))
    xm = np.abs(dx) >= np.abs(dy)
    ua, ub, va, du, dv = np.where(xm, pxa, pya), np.where(xm, pxb, pyb), np.where(xm, pya, pxa), np.where(xm, dx, dy), np.where(xm, dy, dx)
    a0 = np.where(xm, x0, y0)
    a1 = a0 + np.where(xm, w, h)
    b0 = np.where(xm, y0, x0)
    b1 = b0 + np.where(xm, h, w)
    lo = np.minimum(np.maximum(np.minimum(ua, ub), (a0 - 1).astype(F)), (a1 + 1).astype(F))
    hi = np.minimum(np.maximum(np.maximum(ua, ub), (a0 - 1).astype(F)), (a1 + 1).astype(F))
    s0 = np.maximum(np.ceil(lo - F(0.5)).astype(np.int64), a0)
    s1 = np.minimum(np.ceil(hi - F(0.5)).astype(np.int64), a1)
    seg, k = _expand(np.maximum(s1 - s0, 0))
    u = s0[seg] + k
    uc = u.astype(F) + F(0.5)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = va[seg] + ((uc - ua[seg]) / du[seg]) * dv[seg]
    vf = np.floor(v)
    inb = (vf >= b0[seg].astype(F)) & (vf < b1[seg].astype(F))
    seg, u, uc, vf = seg[inb], u[inb], uc[inb], vf[inb]
    vi = vf.astype(np.int64)
    vc = vf + F(0.5)
    xmf = xm[seg]
    px, py = np.where(xmf, u, vi), np.where(xmf, vi, u)
    xc, yc = np.where(xmf, uc, vc), np.where(xmf, vc, uc)
    t = ((xc - pxa[seg]) * dx[seg] + (yc - pya[seg]) * dy[seg]) / dd[seg]
    t = np.minimum(np.maximum(t, F(0)), F(1))
    qa, qb = (F(1) - t) / za[seg], t / zb[seg]
    sq = qa + qb
    X = (qa * Xa[seg] + qb * Xb[seg]) / sq
    Y = (qa * Ya[seg] + qb * Yb[seg]) / sq
    Z = (qa * za[seg] + qb * zb[seg]) / sq
    dist = np.sqrt((X * X + Y * Y) + Z * Z)
    wts = np.stack([qa / sq, qb / sq, np.zeros_like(qa)], axis=1).astype(F)
    return idx[seg], px, py, wts, np.stack([X, Y, Z], axis=1).astype(F), dist.astype(F)


def _point_fragments(P, view):
    x0, y0, w, h, fx, fy, cx, cy = view
    idx = np.arange(P.shape[0])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        px = np.floor(cx + fx * (P[:, 0] / P[:, 2]))
        py = np.floor(cy - fy * (P[:, 1] / P[:, 2]))
        ok = ~(P[:, 2] < NEAR) & (px >= F(x0)) & (px < F(x0 + w)) & (py >= F(y0)) & (py < F(y0 + h))
    idx, px, py, P = idx[ok], px[ok].astype(np.int64), py[ok].astype(np.int64), P[ok]
    dist = np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])
    wts = np.zeros((idx.size, 3), F)
    wts[:, 0] = 1
    return idx, px, py, wts, P.astype(F), dist.astype(F)


def _edge_normal(A, B):
    """A x B with the pair in canonical order (smaller X, then Y, then Z first), negated when the triangle names it the other way"""
    swap = np.where(A[:, 0] != B[:, 0], B[:, 0] < A[:, 0], np.where(A[:, 1] != B[:, 1], B[:, 1] < A[:, 1], B[:, 2] < A[:, 2]))
    a = np.where(swap[:, None], B, A)
    b = np.where(swap[:, None], A, B)
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)
    return np.where(swap[:, None], -n, n).astype(F)


def _tri_fragments(V, view):
    """V [n, 3, 3] camera-space triangles"""
    x0, y0, w, h, fx, fy, cx, cy = view
    idx = np.arange(V.shape[0])
    behind = V[:, :, 2] < NEAR
    keep = ~behind.all(axis=1)
    idx, V, behind = idx[keep], V[keep], behind[keep]
    n0, n1, n2 = _edge_normal(V[:, 1], V[:, 2]), _edge_normal(V[:, 2], V[:, 0]), _edge_normal(V[:, 0], V[:, 1])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        px = cx + fx * (V[:, :, 0] / V[:, :, 2])
        py = cy - fy * (V[:, :, 1] / V[:, :, 2])
    whole = behind.any(axis=1) | ~np.isfinite(px).all(axis=1) | ~np.isfinite(py).all(axis=1)
    with np.errstate(invalid="ignore"):
        def span(p, a0, n):
            lo = np.floor(np.clip(np.where(whole, 0, p.min(axis=1)), a0 - 2, a0 + n + 2)).astype(np.int64) - 1
            hi = np.floor(np.clip(np.where(whole, 0, p.max(axis=1)), a0 - 2, a0 + n + 2)).astype(np.int64) + 2
            lo, hi = np.maximum(lo, a0), np.minimum(hi, a0 + n)
            return np.where(whole, a0, lo), np.where(whole, a0 + n, hi)
        bx0, bx1 = span(px, x0, w)
        by0, by1 = span(py, y0, h)
    bw, bh = np.maximum(bx1 - bx0, 0), np.maximum(by1 - by0, 0)
    tri, k = _expand(bw * bh)
    x = bx0[tri] + k % np.maximum(bw[tri], 1)
    y = by0[tri] + k // np.maximum(bw[tri], 1)
    xc, yc = x.astype(F) + F(0.5), y.astype(F) + F(0.5)
    u, v = (xc - cx) / fx, (cy - yc) / fy
    e0 = (n0[tri, 0] * u + n0[tri, 1] * v) + n0[tri, 2]
    e1 = (n1[tri, 0] * u + n1[tri, 1] * v) + n1[tri, 2]
    e2 = (n2[tri, 0] * u + n2[tri, 1] * v) + n2[tri, 2]
    s = (e0 + e1) + e2
    cov = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (s > 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0) & (s < 0))
    tri, x, y, e0, e1, e2, s = (a[cov] for a in (tri, x, y, e0, e1, e2, s))
    w0, w1, w2 = e0 / s, e1 / s, e2 / s
    T = V[tri]
    P = np.stack([(w0 * T[:, 0, c] + w1 * T[:, 1, c]) + w2 * T[:, 2, c] for c in range(3)], axis=1).astype(F)
    ok = P[:, 2] >= NEAR
    tri, x, y, w0, w1, w2, P = (a[ok] for a in (tri, x, y, w0, w1, w2, P))
    dist = np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])
    return idx[tri], x, y, np.stack([w0, w1, w2], axis=1).astype(F), P, dist.astype(F)


def _pack(c):
    return np.floor(np.minimum(np.maximum(c, F(0)), F(1)) * F(255) + F(0.5)).astype(np.uint8)


def _shade(mesh, ids, wts, P, cam_pos):
    """step F for fragments of one mesh: ids [k, face_size] vertex indices, wts [k, 3], P [k, 3] -> uint8 [k, 4]"""
    nv = mesh.face_size
    col = np.zeros((ids.shape[0], 3), F)
    nrm = np.zeros((ids.shape[0], 3), F)
    vn = None if mesh.unlit else _normals(mesh.matrix, mesh.vert[:, 6:9])
    for i in range(nv):
        term = wts[:, i:i + 1] * mesh.vert[ids[:, i], 3:6]
        col = term if i == 0 else col + term
        if vn is not None:
            tn = wts[:, i:i + 1] * vn[ids[:, i]]
            nrm = tn if i == 0 else nrm + tn
    out = np.empty((ids.shape[0], 4), np.uint8)
    out[:, 3] = 255
    if mesh.unlit:
        out[:, :3] = _pack(col)
        return out
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        max0 = lambda t: np.where(t > 0, t, F(0)).astype(F)
        n0, n1, n2 = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        diffuse = F(0.7) * max0(_dot3(L1[0], L1[1], L1[2], n0, n1, n2))
        diffuse2 = F(0.2) * max0(_dot3(L2[0], L2[1], L2[2], n0, n1, n2))
        v0, v1, v2 = cam_pos[0] - P[:, 0], cam_pos[1] - P[:, 1], cam_pos[2] + P[:, 2]
        vl = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
        d0, d1, d2 = v0 / vl, v1 / vl, v2 / vl
        i0, i1, i2 = -L1[0], -L1[1], -L1[2]
        dn = (n0 * i0 + n1 * i1) + n2 * i2
        t = F(2) * dn
        r0, r1, r2 = i0 - t * n0, i1 - t * n1, i2 - t * n2
        sp = max0(_dot3(d0, d1, d2, r0, r1, r2))
        for _ in range(5):
            sp = sp * sp
        k = ((F(0.3) + diffuse) + diffuse2) + F(0.6) * sp
        out[:, :3] = _pack((k[:, None] * col).astype(F))
    return out


def render(meshes, cam, tile, background_brightness, under=None):
    """The contract of mnv_render_meshes: (tmax float32 [h, w], rgba8 uint8 [h, w, 4]) of `tile`.  cam: the mnv_camera struct;
    under: None or (tmax [h, w] or None, rgba8 [h, w, 4] or None)."""
    x0, y0, w, h = tile
    m = np.array(cam.c2w[:], F)
    view = (x0, y0, w, h, F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy))
    cam_pos = m[9:12]
    frags = []  # per visible mesh: (ordinal, pix, key, dist, rgba8)
    first = 0
    for mesh in meshes:
        prims = mesh.prims()
        if not mesh.visible or prims.shape[0] == 0:
            continue
        V = _to_cam(m, _world(mesh.matrix, mesh.vert[prims, 0:3]))   # [n, face_size, 3]
        if mesh.face_size == 3:
            p, x, y, wts, P, dist = _tri_fragments(V, view)
        elif mesh.face_size == 2:
            p, x, y, wts, P, dist = _line_fragments(V[:, 0], V[:, 1], view)
        else:
            p, x, y, wts, P, dist = _point_fragments(V[:, 0], view)
        rgba = _shade(mesh, prims[p], wts, P, cam_pos)
        frags.append((first + p, (y - y0) * w + (x - x0), _key(P[:, 2], dist), dist, rgba))
        first += prims.shape[0]
    bbv = min(max(F(background_brightness), F(0)), F(1))
    c = int(np.floor(F(bbv) * F(255) + F(0.5)))
    tmax = np.full(w * h, F(1e9), F)
    rgba8 = np.empty((w * h, 4), np.uint8)
    rgba8[:] = (c, c, c, 255)
    if under is not None:
        if under[0] is not None:
            tmax = np.array(under[0], F).reshape(-1).copy()
        if under[1] is not None:
            rgba8 = np.array(under[1], np.uint8).reshape(-1, 4).copy()
    if frags:
        ordinal, pix, key, dist, rgba = (np.concatenate([f[i] for f in frags]) for i in range(5))
        best = np.full(w * h, EMPTY, np.uint64)
        np.minimum.at(best, pix, key)
        win = key == best[pix]
        ordinal, pix, dist, rgba = ordinal[win], pix[win], dist[win], rgba[win]
        owner = np.full(w * h, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(owner, pix, ordinal)
        win = ordinal == owner[pix]
        pix, dist, rgba = pix[win], dist[win], rgba[win]
        if under is not None:
            win = dist < tmax[pix]
            pix, dist, rgba = pix[win], dist[win], rgba[win]
        tmax[pix] = dist
        rgba8[pix] = rgba
    return tmax.reshape(h, w), rgba8.reshape(h, w, 4)
