"""numpy restatement of the fitting contract of include/mnv.h ("fitting a tree's rows": mnv_rays_grad, mnv_rows_master_init,
mnv_rows_sgd_step, mnv_n3tree_fit), written from the header and from the reference's march (rt_core.cuh:117-331), on top of
tests/primitives_ref.py.  Three parts:

* the per-step march of a ray list -- ray set-up (primitives_ref.setup_ray through the one-pixel camera of tests/rays_ref.py), descent,
  _dda_unit, delta_t -- in binary32, all rays in lock step, emitting every step's dense samples (`forward`);
* the backward contract to int64 words (`backward`), and the same formulas in binary64 on the recorded sample geometry (`gradient64`,
  `loss64_ray`: what tests/test_fit_ref.py holds against central differences);
* the two row kernels (`master_init`, `sgd_step`) and the fit loop (`fit`).

Every float operation is one numpy operation on float32 arrays in the contract's order; numpy never contracts."""
import ctypes as C

import numpy as np

import primitives_ref as pr

F = np.float32
MAX_DESCENT = 23
Q32 = 4294967296.0
FIT_SUMS = ("n_rays", "n_stopped", "n_samples", "n_skipped", "se_q32")


# ---- the tree and the frame constants ------------------------------------------------------------------------------------------------
def tree_of(mnv, tree):
    """dict of a binding N3Tree's host arrays (copies): data uint16 [capacity * 8, data_dim], child int32 [capacity * 8], offset, scale,
    data_dim, basis (-1: RGBA rows), capacity."""
    v = tree.host_view()
    data, child, _ = tree.host_arrays()
    basis = v.basis_dim if (v.format == mnv.FORMAT_SH and v.basis_dim >= 0) else -1
    return dict(data=np.array(data, np.uint16).reshape(-1, v.data_dim), child=np.array(child, np.int32).reshape(-1), offset=pr.f32(list(v.offset)),
                scale=pr.f32(list(v.scale)), data_dim=int(v.data_dim), basis=int(basis), capacity=int(v.capacity))


_libm = None


def _cosf_sinf(x):
    """the host's cosf / sinf: what the library calls for the rot_dirs constants (renderer_kernel.cu:43-51)"""
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        for fn in (_libm.cosf, _libm.sinf):
            fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return F(_libm.cosf(float(x))), F(_libm.sinf(float(x)))


def _frame(T, opt, o, d):
    """primitives_ref's frame of the one-pixel camera of ray (o, d): c2w = [1,0,0 | 0,1,0 | -d | o], fx = fy = 1, cx = cy = 0.5"""
    aa = pr.f32(list(opt.rot_dirs))
    angle = np.sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2])
    rot = {}
    if not float(angle) < 1e-6:
        cs, sn = _cosf_sinf(angle)
        rot = dict(rot_k=aa / angle, rot_cos=cs, rot_sin=sn)
    m = np.zeros(12, np.float32)
    m[0] = m[4] = 1.0
    m[6:9] = -d
    m[9:12] = o
    return pr.make_frame(1.0, 1.0, 0.5, 0.5, m, offset=T["offset"], scale=T["scale"], render_bbox=list(opt.render_bbox),
                         basis_minmax=(opt.basis_minmax[0], opt.basis_minmax[1]), **rot)


def setup_rays(T, opt, origins, dirs, tmax=None):
    """ray set-up of the ray march for float32 rays [n, 3]: dict of per-ray arrays (cen, dir, invdir [n, 3]; delta_scale, tmin, tmax [n];
    in_bbox [n]; basis [n, 25], masked) -- a degenerate ray (direction of zero or non-finite squared length, non-finite origin) is a miss."""
    o, d = pr.f32(origins).reshape(-1, 3), pr.f32(dirs).reshape(-1, 3)
    n = o.shape[0]
    t_max = np.full(n, 1e9, np.float32) if tmax is None else pr.f32(tmax).reshape(n)
    out = dict(cen=np.zeros((n, 3), F), dir=np.zeros((n, 3), F), invdir=np.ones((n, 3), F), delta_scale=np.ones(n, F), tmin=np.zeros(n, F),
               tmax=np.zeros(n, F), in_bbox=np.zeros(n, bool), basis=np.zeros((n, 25), F))
    nb = max(T["basis"], 1)
    with np.errstate(all="ignore"):
        len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        valid = (len2 > 0) & (len2 < np.inf) & np.isfinite(o).all(axis=1)
    for i in np.nonzero(valid)[0]:
        fr = _frame(T, opt, o[i], d[i])
        s = pr.setup_ray(fr, [0], [0], t_max[i:i + 1], nb if T["basis"] > 0 else 1)
        out["cen"][i] = pr.ray_origin(fr)
        for k in ("dir", "invdir", "basis"):
            out[k][i] = s[k][0]
        for k in ("delta_scale", "tmin", "tmax", "in_bbox"):
            out[k][i] = s[k][0]
    return out


# ---- the march -----------------------------------------------------------------------------------------------------------------------
def _step(T, R, idx, t, step_size):
    """one march step (rt_core.cuh:220-231) of the rays idx at their t: -> (vox, depth, delta_t, sigma, ok); ok False: the descent left the
    tree (a link outside [1, capacity), or no leaf within 23 levels)"""
    n = idx.size
    with np.errstate(all="ignore"):
        pos = R["cen"][idx] + t[:, None] * R["dir"][idx]
        pos = np.fmax(np.fmin(pos, F(1.0) - F(1e-6)), F(0.0)).astype(F)
        chunk = np.zeros(n, np.int64)
        vox = np.full(n, -1, np.int64)
        depth = np.zeros(n, np.int32)
        walking = np.ones(n, bool)
        for level in range(1, MAX_DESCENT + 1):
            pos2 = pos * F(2.0)
            f = np.floor(pos2)
            frac = pos2 - f
            pos = np.where(walking[:, None], frac, pos).astype(F)
            cidx = (f[:, 0].astype(np.int64) * 2 + f[:, 1].astype(np.int64)) * 2 + f[:, 2].astype(np.int64)
            cell = chunk * 8 + cidx
            skip = np.where(walking, T["child"][np.where(walking, cell, 0)], 1).astype(np.int64)
            leaf = walking & (skip == 0)
            vox[leaf] = cell[leaf]
            depth[leaf] = level
            nxt = chunk + skip
            bad = walking & ~leaf & ((nxt < 1) | (nxt >= T["capacity"]))
            walking = walking & ~leaf & ~bad
            chunk = np.where(walking, nxt, chunk)
            if not walking.any():
                break
        ok = vox >= 0
        inv = R["invdir"][idx]
        tu = np.full(n, 1e4, F)
        for i in range(3):
            t1 = -pos[:, i] * inv[:, i]
            t2 = t1 + inv[:, i]
            tu = np.fmin(tu, np.fmax(t1, t2))
        cube = np.ldexp(F(1.0), depth).astype(F)
        delta_t = (tu / cube + F(step_size)).astype(F)
        sigma = pr.half_bits_to_float(T["data"][np.where(ok, vox, 0), T["data_dim"] - 1])
    return vox, depth, delta_t, sigma, ok


def _colours(T, R, idx, vox, weight):
    """the forward's three terms of a dense sample and c_sk: (term [m, 3], c [m, 3]) float32"""
    B = T["basis"]
    rows = T["data"][vox]
    with np.errstate(all="ignore"):
        if B > 0:
            tmp = pr.sh_channels(B, R["basis"][idx][:, :B], rows[:, :3 * B])
            den = (F(1.0) + pr.expf(-tmp.reshape(-1)).reshape(-1, 3)).astype(F)
            return (weight[:, None] / den).astype(F), (F(1.0) / den).astype(F)
        c = pr.half_bits_to_float(rows[:, :3])
        return (c * weight[:, None]).astype(F), c


def forward(T, opt, origins, dirs, tmax=None, max_steps=1 << 20):
    """the forward march of a ray list: dict(rgba float32 [n, 4], S [n, 3] (the sums before the early-stop rescale), T_end, scale [n],
    stopped, broken, in_bbox [n], n_dense [n], R (the set-up), batches: per march step that had a dense sample a dict of arrays over those
    samples -- ray, vox, depth, d (= delta_t * delta_scale), att, w, Tn, c [m, 3], term [m, 3])."""
    R = setup_rays(T, opt, origins, dirs, tmax)
    n = R["tmin"].size
    S = np.zeros((n, 3), F)
    Tl = np.ones(n, F)
    t = R["tmin"].copy()
    stopped, broken = np.zeros(n, bool), np.zeros(n, bool)
    n_dense = np.zeros(n, np.int64)
    steps = np.zeros(n, np.int64)
    batches = []
    sigma_thresh, stop_thresh = F(opt.sigma_thresh), F(opt.stop_thresh)
    with np.errstate(all="ignore"):
        alive = R["in_bbox"] & (t < R["tmax"])
        while alive.any():
            idx = np.nonzero(alive)[0]
            steps[idx] += 1
            vox, depth, delta_t, sigma, ok = _step(T, R, idx, t[idx], opt.step_size)
            ok &= steps[idx] <= max_steps
            broken[idx[~ok]] = True
            alive[idx[~ok]] = False
            dense = ok & (sigma > sigma_thresh)
            if dense.any():
                di = idx[dense]
                ds = R["delta_scale"][di]
                att = pr.expf((-delta_t[dense] * ds) * sigma[dense])
                w = (Tl[di] * (F(1.0) - att)).astype(F)
                term, c = _colours(T, R, di, vox[dense], w)
                S[di] = S[di] + term
                n_dense[di] += 1
                Tn = (Tl[di] * att).astype(F)
                Tl[di] = Tn
                batches.append(dict(ray=di, vox=vox[dense], depth=depth[dense], d=(delta_t[dense] * ds).astype(F), att=att, w=w, Tn=Tn, c=c, term=term))
                stop = Tn < stop_thresh
                stopped[di[stop]] = True
                alive[di[stop]] = False
            go = idx[ok & alive[idx]]
            dt = delta_t[ok & alive[idx]]
            tn = (t[go] + dt).astype(F)
            stuck = ~(tn > t[go])
            broken[go[stuck]] = True
            t[go] = tn
            alive[go] = ~stuck & (tn < R["tmax"][go])
        scale = np.where(stopped, F(1.0) / (F(1.0) - Tl), F(1.0)).astype(F)
        Cc = np.where(stopped[:, None], S * scale[:, None], S).astype(F)
        o3 = np.where(stopped, F(1.0), np.where(R["in_bbox"], F(1.0) - Tl, F(0.0))).astype(F)
        remain = (F(opt.background_brightness) * (F(1.0) - o3)).astype(F)
        rgba = np.concatenate([(Cc + remain[:, None]).astype(F), o3[:, None]], axis=1)
    return dict(rgba=rgba, S=S, T_end=Tl, scale=scale, stopped=stopped, broken=broken, in_bbox=R["in_bbox"], n_dense=n_dense, R=R, batches=batches)


# ---- the backward contract -----------------------------------------------------------------------------------------------------------
def q32(x):
    """llrint((double)sat(x) * 2^32), sat: clamp to [-32, 32], NaN -> 0"""
    x = pr.f32(x)
    with np.errstate(all="ignore"):
        s = np.where(np.isnan(x), F(0.0), np.fmin(np.fmax(x, F(-32.0)), F(32.0)))
        return np.rint(s.astype(np.float64) * Q32).astype(np.int64)


def backward(T, opt, fw, target, acc=None):
    """the backward contract on a forward march: adds into acc (int64 [capacity * 8, data_dim], made when None) and returns (acc, sums dict)."""
    B, dd = T["basis"], T["data_dim"]
    n = fw["rgba"].shape[0]
    tg = pr.f32(target).reshape(n, 4)
    if acc is None:
        acc = np.zeros((T["capacity"] * 8, dd), np.int64)
    with np.errstate(all="ignore"):
        included = tg[:, 3] != 0
        Cc = fw["rgba"][:, :3]
        g = (Cc - tg[:, :3]).astype(F)
        skipped = included & (fw["broken"] | ~np.isfinite(Cc).all(axis=1) | ~np.isfinite(g).all(axis=1))
        counts = included & ~skipped
        se = ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
        sums = dict(n_rays=int(counts.sum()), n_stopped=int((counts & fw["stopped"]).sum()), n_samples=int(fw["n_dense"][counts].sum()),
                    n_skipped=int(skipped.sum()), se_q32=int(q32(se[counts]).sum()))
        gs = (g * fw["scale"][:, None]).astype(F)
        Bk = np.where(fw["stopped"][:, None], Cc, F(opt.background_brightness)).astype(F)
        bt = (Bk * fw["T_end"][:, None]).astype(F)
        P = np.zeros((n, 3), F)
        bmin, bmax = int(opt.basis_minmax[0]), int(opt.basis_minmax[1])
        for b in fw["batches"]:
            keep = counts[b["ray"]]
            r, vox = b["ray"][keep], b["vox"][keep]
            if r.size == 0:
                continue
            term, c, w, Tn, d = b["term"][keep], b["c"][keep], b["w"][keep], b["Tn"][keep], b["d"][keep]
            P[r] = P[r] + term
            Q = (fw["S"][r] - P[r]).astype(F)
            gc = (gs[r] * w[:, None]).astype(F)
            e = ((Tn[:, None] * c).astype(F) - Q).astype(F) - bt[r]
            dsc = (d * fw["scale"][r]).astype(F)
            gr = g[r]
            dot = ((gr[:, 0] * e[:, 0]).astype(F) + (gr[:, 1] * e[:, 1]).astype(F)).astype(F) + (gr[:, 2] * e[:, 2]).astype(F)
            np.add.at(acc[:, dd - 1], vox, q32(dsc * dot))
            if B > 0:
                gt = (gc * (c * (F(1.0) - c)).astype(F)).astype(F)
                basis = fw["R"]["basis"][r]
                for k in range(3):
                    for j in range(max(bmin, 0), min(bmax, B - 1) + 1):
                        np.add.at(acc[:, k * B + j], vox, q32(gt[:, k] * basis[:, j]))
            else:
                for k in range(3):
                    np.add.at(acc[:, k], vox, q32(gc[:, k]))
    return acc, sums


def rays_grad(T, opt, origins, dirs, target, tmax=None, acc=None):
    """mnv_rays_grad restated: -> (rgba float32 [n, 4], acc int64 [capacity * 8, data_dim], sums dict, the forward march)"""
    fw = forward(T, opt, origins, dirs, tmax)
    acc, sums = backward(T, opt, fw, target, acc)
    return fw["rgba"], acc, sums, fw


# ---- the same formulas in binary64 on the recorded geometry ---------------------------------------------------------------------------
def ray_samples(fw, i):
    """the sample list of ray i in march order: dict(vox [m], d [m] float64)"""
    vox, d = [], []
    for b in fw["batches"]:
        hit = np.nonzero(b["ray"] == i)[0]
        if hit.size:
            vox.append(int(b["vox"][hit[0]]))
            d.append(float(b["d"][hit[0]]))
    return dict(vox=np.array(vox, np.int64), d=np.array(d, np.float64))


def _pixel64(B, rows, d, basis, stopped, bg):
    """rows float64 [..., m, data_dim] of the ray's samples (leading axes: perturbations) -> pixel [..., 3], with everything the
    derivative needs"""
    m = rows.shape[-2]
    T = np.ones(rows.shape[:-2])
    S = np.zeros(rows.shape[:-2] + (3,))
    w, c, Tn = [], [], []
    for s in range(m):
        att = np.exp(-d[s] * rows[..., s, -1])
        ws = T * (1.0 - att)
        if B > 0:
            tmp = (rows[..., s, :3 * B].reshape(rows.shape[:-2] + (3, B)) * basis[:B]).sum(axis=-1)
            cs = 1.0 / (1.0 + np.exp(-tmp))
        else:
            cs = rows[..., s, :3]
        S = S + ws[..., None] * cs
        T = T * att
        w.append(ws), c.append(cs), Tn.append(T)
    Cc = S / (1.0 - T)[..., None] if stopped else S + bg * T[..., None]
    return Cc, S, T, w, c, Tn


def loss64_ray(T, opt, fw, i, target, rows):
    """1/2 |C - target|^2 of ray i in binary64 with its sample geometry (voxels, d_s, basis, the stop decision) held fixed; rows float64
    [..., m, data_dim]: the rows of its samples"""
    sm = ray_samples(fw, i)
    Cc = _pixel64(T["basis"], rows, sm["d"], fw["R"]["basis"][i].astype(np.float64), bool(fw["stopped"][i]), float(F(opt.background_brightness)))[0]
    return 0.5 * ((Cc - np.asarray(target, np.float64)[:3]) ** 2).sum(axis=-1)


def gradient64_ray(T, opt, fw, i, target):
    """the contract's formulas in binary64 for ray i: float64 [m, data_dim], the derivative of loss64_ray by the row of every sample"""
    B, dd = T["basis"], T["data_dim"]
    sm = ray_samples(fw, i)
    m = sm["vox"].size
    rows = pr.half_bits_to_float(T["data"][sm["vox"]]).astype(np.float64).reshape(m, dd)
    basis = fw["R"]["basis"][i].astype(np.float64)
    stopped, bg = bool(fw["stopped"][i]), float(F(opt.background_brightness))
    Cc, S, T_end, w, c, Tn = _pixel64(B, rows, sm["d"], basis, stopped, bg)
    g = Cc - np.asarray(target, np.float64)[:3]
    scale = 1.0 / (1.0 - T_end) if stopped else 1.0
    Bk = Cc if stopped else np.full(3, bg)
    out = np.zeros((m, dd))
    P = np.zeros(3)
    bmin, bmax = int(opt.basis_minmax[0]), int(opt.basis_minmax[1])
    for s in range(m):
        P = P + w[s] * c[s]
        Q = S - P
        gc = (g * scale) * w[s]
        if B > 0:
            gt = gc * (c[s] * (1.0 - c[s]))
            for k in range(3):
                for j in range(max(bmin, 0), min(bmax, B - 1) + 1):
                    out[s, k * B + j] = gt[k] * basis[j]
        else:
            out[s, :3] = gc
        e = (Tn[s] * c[s] - Q) - Bk * T_end
        out[s, dd - 1] = (sm["d"][s] * scale) * ((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2])
    return out, sm, rows


def gradient64(T, opt, fw, target):
    """the binary64 gradient of the whole ray list, summed per row like acc: float64 [capacity * 8, data_dim]"""
    tg = pr.f32(target).reshape(-1, 4)
    out = np.zeros((T["capacity"] * 8, T["data_dim"]))
    with np.errstate(all="ignore"):
        Cc = fw["rgba"][:, :3]
        counts = (tg[:, 3] != 0) & ~fw["broken"] & np.isfinite(Cc).all(axis=1) & np.isfinite(Cc - tg[:, :3]).all(axis=1)
    for i in np.nonzero(counts & (fw["n_dense"] > 0))[0]:
        gr, sm, _ = gradient64_ray(T, opt, fw, i, tg[i])
        np.add.at(out, sm["vox"], gr)
    return out


# ---- the row kernels and the loop -----------------------------------------------------------------------------------------------------
def master_init(data):
    """mnv_rows_master_init: float32 of binary16 bits, non-finite patterns read +0"""
    bits = np.ascontiguousarray(data, np.uint16)
    out = pr.half_bits_to_float(bits).reshape(bits.shape)
    out[(bits & 0x7C00) == 0x7C00] = 0.0
    return out


def half_sat(m):
    """binary16(m), round to nearest even, saturating at +-65504; NaN -> +0: uint16 bits"""
    m = pr.f32(m)
    with np.errstate(all="ignore"):
        s = np.where(np.isnan(m), F(0.0), np.fmin(np.fmax(m, F(-65504.0)), F(65504.0))).astype(F)
        return s.astype(np.float16).view(np.uint16)


def sgd_step(data, master, acc, lr_colour, lr_sigma):
    """mnv_rows_sgd_step in place on data uint16 / master float32 / acc int64, all [rows, data_dim]"""
    dd = data.shape[1]
    touched = np.nonzero((acc != 0).any(axis=1))[0]
    with np.errstate(all="ignore"):
        g = (acc[touched].astype(np.float64) * (1.0 / Q32)).astype(F)
        lr = np.full(dd, lr_colour, F)
        lr[dd - 1] = F(lr_sigma)
        m = (master[touched] - (lr[None, :] * g).astype(F)).astype(F)
        last = m[:, dd - 1]
        m[:, dd - 1] = np.where(last < 0, F(0.0), last)
    master[touched] = m
    data[touched] = half_sat(m)
    acc[touched] = 0


def fit(T, opt, rays, targets, iterations, lr_colour, lr_sigma):
    """mnv_n3tree_fit restated on T (its data changes in place): rays: list of (origins, dirs) per camera, targets: list of float32 [n, 4].
    -> list of se_q32 per iteration"""
    master = master_init(T["data"])
    acc = np.zeros(T["data"].shape, np.int64)
    out = []
    for _ in range(iterations):
        se = 0
        for (o, d), tg in zip(rays, targets):
            _, acc, sums, _ = rays_grad(T, opt, o, d, tg, acc=acc)
            se += sums["se_q32"]
        sgd_step(T["data"], master, acc, lr_colour, lr_sigma)
        out.append(se)
    return out
