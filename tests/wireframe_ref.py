"""numpy restatements for the grid overlay tests: N3Tree::gen_wireframe (reference n3tree.cpp:249-329) and the raster contract of
mnv_render_wireframe (include/mnv.h).  Every float operation is float32 in the order the contract states."""
import numpy as np

F = np.float32

# _push_wireframe_bb's vertex order: for i, for j: (0,i,j) (1,i,j) (i,0,j) (i,1,j) (i,j,0) (i,j,1); a vertex (a,b,c) is (bb[a*3], bb[b*3+1], bb[c*3+2])
_VERTS = []
for _i in range(2):
    for _j in range(2):
        _VERTS += [(0, _i, _j), (1, _i, _j), (_i, 0, _j), (_i, 1, _j), (_i, _j, 0), (_i, _j, 1)]
_VERTS = np.array(_VERTS)                                    # [24, 3] selectors
_VIDX = np.stack([_VERTS[:, 0] * 3, _VERTS[:, 1] * 3 + 1, _VERTS[:, 2] * 3 + 2], axis=1)  # [24, 3] indices into bb


def wireframe_cubes(child, max_depth):
    """(level, i, j, k) of every cube gen_wireframe pushes, in its depth-first order.  child: int32 [capacity, 8] (N == 2)."""
    child = np.asarray(child).reshape(-1, 8)
    nodes, corner, paths = np.zeros(1, np.int64), np.zeros((1, 3), np.int64), np.zeros(1, np.int64)
    levels, corners, keys = [], [], []
    depth = 0
    c = np.arange(8)
    off = np.stack([c >> 2, (c >> 1) & 1, c & 1], axis=1)  # cnt -> (i, j, k), k fastest
    while nodes.size:
        assert depth <= 20
        ch = child[nodes][:, :8]                                          # [n, 8]
        g = (corner[:, None, :] * 2 + off[None, :, :])                    # [n, 8, 3]
        p = paths[:, None] * 8 + c[None, :]                               # path of child indices, base 8
        leaf = (ch == 0) | (depth >= max_depth)
        levels.append(np.full(int(leaf.sum()), depth))
        corners.append(g[leaf])
        keys.append(p[leaf] * (8 ** (20 - depth)))                        # padded: no cube's path is a prefix of another's
        nodes = (nodes[:, None] + ch)[~leaf]
        corner, paths = g[~leaf], p[~leaf]
        depth += 1
    level, corner, key = np.concatenate(levels), np.concatenate(corners), np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    return level[order], corner[order]


def cube_boxes(level, corner, offset, scale):
    """bb [n, 6] = x0 y0 z0 x1 y1 z1: ((float)i / gridsz - offset[a]) / scale[a], gridsz = 2^(level+1)."""
    g = (2.0 ** (level + 1)).astype(F)[:, None]
    off, sc = np.asarray(offset, F), np.asarray(scale, F)
    lo = (corner.astype(F) / g - off) / sc
    hi = ((corner + 1).astype(F) / g - off) / sc
    return np.concatenate([lo, hi], axis=1).astype(F)


def gen_wireframe(child, offset, scale, max_depth):
    """float32 [n_vertices, 9] exactly as N3Tree::gen_wireframe."""
    level, corner = wireframe_cubes(child, max_depth)
    bb = cube_boxes(level, corner, offset, scale)
    v = np.zeros((level.size, 24, 9), F)
    v[:, :, 0:3] = bb[:, _VIDX]
    v[:, :, 8] = 1.0
    return v.reshape(-1, 9)


def segments_from_vertices(verts):
    """[n, 6] world endpoints from a gen_wireframe vertex list (GL_LINES: vertex pairs)."""
    return np.ascontiguousarray(verts[:, :3].reshape(-1, 6))


def raster(segments, cam, tile, background_brightness):
    """The raster contract of mnv_render_wireframe: (tmax float32 [h, w], rgba8 uint8 [h, w, 4]) of `tile`.
    cam: the mnv_camera struct (c2w column-major [r | u | b | C], fx, fy, cx, cy)."""
    x0, y0, w, h = tile
    m = np.array(cam.c2w[:], F)
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    s = np.asarray(segments, F).reshape(-1, 6)

    def to_cam(p):
        d0, d1, d2 = p[:, 0] - m[9], p[:, 1] - m[10], p[:, 2] - m[11]
        X = (m[0] * d0 + m[1] * d1) + m[2] * d2
        Y = (m[3] * d0 + m[4] * d1) + m[5] * d2
        z = -((m[6] * d0 + m[7] * d1) + m[8] * d2)
        return X, Y, z

    Xa, Ya, za = to_cam(s[:, 0:3])
    Xb, Yb, zb = to_cam(s[:, 3:6])
    near = F(1e-3)
    keep = ~((za < near) & (zb < near))
    Xa, Ya, za, Xb, Yb, zb = (a[keep] for a in (Xa, Ya, za, Xb, Yb, zb))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ca = za < near
        t = (near - za[ca]) / (zb[ca] - za[ca])
        Xa[ca] = Xa[ca] + t * (Xb[ca] - Xa[ca])
        Ya[ca] = Ya[ca] + t * (Yb[ca] - Ya[ca])
        za[ca] = near
        cb = (zb < near) & ~ca
        t = (near - zb[cb]) / (za[cb] - zb[cb])
        Xb[cb] = Xb[cb] + t * (Xa[cb] - Xb[cb])
        Yb[cb] = Yb[cb] + t * (Ya[cb] - Yb[cb])
        zb[cb] = near
        pxa, pya = cx + fx * (Xa / za), cy - fy * (Ya / za)
        pxb, pyb = cx + fx * (Xb / zb), cy - fy * (Yb / zb)
        dx, dy = pxb - pxa, pyb - pya
        dd = dx * dx + dy * dy
    ok = (dd > 0) & np.isfinite(dd)
    Xa, Ya, za, Xb, Yb, zb, pxa, pya, pxb, pyb, dx, dy, dd = (a[ok] for a in (Xa, Ya, za, Xb, Yb, zb, pxa, pya, pxb, pyb, dx, dy, dd))
    xm = np.abs(dx) >= np.abs(dy)
    # along the major axis u (x for x-major) and the other axis v
    ua, ub, va, du, dv = np.where(xm, pxa, pya), np.where(xm, pxb, pyb), np.where(xm, pya, pxa), np.where(xm, dx, dy), np.where(xm, dy, dx)
    a0 = np.where(xm, x0, y0)
    a1 = a0 + np.where(xm, w, h)
    b0 = np.where(xm, y0, x0)
    b1 = b0 + np.where(xm, h, w)
    lo = np.minimum(np.maximum(np.minimum(ua, ub), (a0 - 1).astype(F)), (a1 + 1).astype(F))
    hi = np.minimum(np.maximum(np.maximum(ua, ub), (a0 - 1).astype(F)), (a1 + 1).astype(F))
    s0 = np.maximum(np.ceil(lo - F(0.5)).astype(np.int64), a0)
    s1 = np.minimum(np.ceil(hi - F(0.5)).astype(np.int64), a1)
    cnt = np.maximum(s1 - s0, 0)
    seg = np.repeat(np.arange(cnt.size), cnt)
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    u = s0[seg] + (np.arange(seg.size) - first)
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
    key = (Z.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | dist.astype(F).view(np.uint32).astype(np.uint64)
    pix = (py - y0) * w + (px - x0)
    keys = np.full(w * h, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(keys, pix, key)
    hit = keys != np.iinfo(np.uint64).max
    tmax = np.full(w * h, F(1e9), F)
    tmax[hit] = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(F)
    bbv = min(max(F(background_brightness), F(0)), F(1))
    c = int(np.floor(F(bbv) * F(255) + F(0.5)))
    rgba8 = np.empty((w * h, 4), np.uint8)
    rgba8[:] = (c, c, c, 255)
    rgba8[hit] = (0, 0, 0, 255)
    return tmax.reshape(h, w), rgba8.reshape(h, w, 4)
