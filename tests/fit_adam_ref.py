"""numpy restatement of include/mnv.h's "fitting on a photo set" on top of tests/fit_ref.py: mnv_rows_adam_step (`adam_step`, and `adam_step64`,
the same update in binary64), the batcher's permutation, units and rays (`perm`, `unit_table`, `draw`) and the loop mnv_n3tree_fit_ex
(`fit_ex`).  Every float operation is one numpy operation on float32 arrays in the contract's order; the permutation is integer arithmetic.

Adam's default rates (lr_colour 0.03, lr_sigma 1, beta 0.9 / 0.999, eps 1e-8) were chosen with `sweep` below -- `python tests/fit_adam_ref.py`
prints it -- on the fit scene of tests/fit_cases.py (FIT), twelve full-batch steps, se_q32 / 2^32 of the fitted rays before each step:
    lr_colour  lr_sigma   step 0   step 4   step 8   step 11
    0.01       0.3        4.585    3.870    3.382    3.064    falls at every step
    0.01       1.5        4.585    3.178    2.776    2.640    falls at every step
    0.03       0.3        4.585    3.481    2.907    2.590    falls at every step
    0.03       1.0        4.585    2.993    2.463    2.254    falls at every step      <- the defaults
    0.03       1.5        4.585    2.896    2.420    2.251    falls at every step
    0.05       0.3        4.585    3.263    2.691    2.398    falls at every step
    0.05       1.5        4.585    2.752    2.269    2.102    falls at every step
    0.03       3.0        4.585    3.020    2.684    2.491    falls at every step here (also over 30 steps: 1.941 at step 29), but
                                                              unevenly -- 4.585 4.543 3.270 3.023 3.020 -- and more slowly than lr_sigma 1 .. 1.5
    0.1        3.0        4.585    2.931    2.395    2.247    rises at one step
    0.3        10.0       4.585    18.30    16.62    16.49    diverges
Every pair in lr_colour 0.01 .. 0.05 x lr_sigma 0.3 .. 1.5 falls at each step; (0.03, 1) sits inside that range with a factor of 1.5 and more
to the nearest pair that misbehaves.  SGD at fit_cases.FIT's rates (1, 20) reaches 3.609 at step 8.
"""
import math

import numpy as np

import fit_ref
import primitives_ref as pr

F = np.float32
Q32 = fit_ref.Q32
ADAM = dict(lr_colour=0.03, lr_sigma=1.0, beta1=0.9, beta2=0.999, eps=1e-8)
M32 = np.uint64(0xFFFFFFFF)


# ---- the row step -------------------------------------------------------------------------------------------------------------------------
def adam_consts(beta1, beta2, step):
    """the four constants the host computes: omb1, omb2 in binary32; c1, c2 in binary64 (libm pow), rounded once"""
    b1, b2 = F(beta1), F(beta2)
    c1 = F(1.0 / (1.0 - math.pow(float(b1), float(step))))
    c2 = F(1.0 / (1.0 - math.pow(float(b2), float(step))))
    return F(1.0) - b1, F(1.0) - b2, c1, c2


def adam_step(data, master, m1, m2, acc, step, lr_colour=ADAM["lr_colour"], lr_sigma=ADAM["lr_sigma"], beta1=ADAM["beta1"], beta2=ADAM["beta2"],
              eps=ADAM["eps"]):
    """mnv_rows_adam_step in place on data uint16 / master, m1, m2 float32 / acc int64, all [rows, data_dim]"""
    dd = data.shape[1]
    touched = np.nonzero((acc != 0).any(axis=1))[0]
    b1, b2, e = F(beta1), F(beta2), F(eps)
    omb1, omb2, c1, c2 = adam_consts(beta1, beta2, step)
    with np.errstate(all="ignore"):
        g = (acc[touched].astype(np.float64) * (1.0 / Q32)).astype(F)
        a = ((m1[touched] * b1).astype(F) + (g * omb1).astype(F)).astype(F)
        v = ((m2[touched] * b2).astype(F) + ((g * g).astype(F) * omb2).astype(F)).astype(F)
        den = (np.sqrt((v * c2).astype(F)).astype(F) + e).astype(F)
        lr = np.full(dd, lr_colour, F)
        lr[dd - 1] = F(lr_sigma)
        upd = ((lr[None, :] * (a * c1).astype(F)).astype(F) / den).astype(F)
        m = (master[touched] - upd).astype(F)
        last = m[:, dd - 1]
        m[:, dd - 1] = np.where(last < 0, F(0.0), last)
    m1[touched] = a
    m2[touched] = v
    master[touched] = m
    data[touched] = fit_ref.half_sat(m)
    acc[touched] = 0


def adam_step64(master, m1, m2, acc, step, lr_colour, lr_sigma, beta1, beta2, eps):
    """the same update in binary64 on float64 copies of binary32 state (no rounding to binary32 anywhere): -> (master, m1, m2) float64"""
    dd = master.shape[1]
    g = acc.astype(np.float64) / Q32
    b1, b2 = float(F(beta1)), float(F(beta2))
    a = m1.astype(np.float64) * b1 + g * (1.0 - b1)
    v = m2.astype(np.float64) * b2 + g * g * (1.0 - b2)
    lr = np.full(dd, float(F(lr_colour)))
    lr[dd - 1] = float(F(lr_sigma))
    upd = lr[None, :] * (a / (1.0 - b1 ** step)) / (np.sqrt(v / (1.0 - b2 ** step)) + float(F(eps)))
    m = master.astype(np.float64) - upd
    m[:, dd - 1] = np.maximum(m[:, dd - 1], 0.0)
    touched = (acc != 0).any(axis=1)
    keep = ~touched[:, None]
    return np.where(keep, master, m), np.where(keep, m1, a), np.where(keep, m2, v)


# ---- the permutation ----------------------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def perm_params(units, seed, epoch):
    """-> (k, mask, the four round keys) of the Feistel network for `units` units"""
    k = max(1, (int(units - 1).bit_length() + 1) // 2)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    base = mix32(lo ^ mix32(hi ^ np.uint64(epoch & 0xFFFFFFFF)))
    keys = [mix32((base + np.uint64(r)) & M32) for r in range(4)]
    return k, np.uint64((1 << k) - 1), keys


def perm(units, seed, epoch, places):
    """perm(epoch, i) for every i of `places` (all below units): int64 array"""
    k, mask, keys = perm_params(units, seed, epoch)
    x = np.array(places, np.uint64).reshape(-1)
    assert x.size == 0 or int(x.max()) < units
    walking = np.ones(x.size, bool)
    sk = np.uint64(k)
    while walking.any():
        cur = x[walking]
        L, R = cur >> sk, cur & mask
        for r in range(4):
            L, R = R, L ^ (mix32(R ^ keys[r]) & mask)
        cur = (L << sk) | R
        x[walking] = cur
        walking[walking] = cur >= np.uint64(units)
    return x.astype(np.int64)


# ---- units and rays -----------------------------------------------------------------------------------------------------------------------
def unit_table(cams, tile):
    """int64 [n_cams + 1]: the first unit of every camera (CameraStruct), then U"""
    n = [((c.width + 7) // 8) * ((c.height + 7) // 8) if tile == 8 else c.width * c.height for c in cams]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def unit_pixels(cams, tile, units):
    """the pixels of a list of units, tile * tile per unit in lane order: -> (cam, ix, iy int64 [n], inside bool [n])"""
    prefix = unit_table(cams, tile)
    units = np.asarray(units, np.int64)
    cam = np.searchsorted(prefix, units, side="right") - 1
    local = units - prefix[cam]
    w = np.array([c.width for c in cams], np.int64)[cam]
    h = np.array([c.height for c in cams], np.int64)[cam]
    if tile == 1:
        return cam, local % w, local // w, np.ones(units.size, bool)
    tiles_x = (w + 7) // 8
    lane = np.arange(64, dtype=np.int64)
    ix = ((local % tiles_x) * 8)[:, None] + (lane & 7)[None, :]
    iy = ((local // tiles_x) * 8)[:, None] + (lane >> 3)[None, :]
    inside = (ix < w[:, None]) & (iy < h[:, None])
    return np.repeat(cam, 64), ix.reshape(-1), iy.reshape(-1), inside.reshape(-1)


def pixel_rays(cams, cam, ix, iy, inside):
    """mnv_generate_rays(MNV_PROJ_PINHOLE) per pixel, in its operation order; outside lanes: the camera's centre, direction zero"""
    n = cam.size
    o, d = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for ci, c in enumerate(cams):
        s = cam == ci
        if not s.any():
            continue
        m = np.array(list(c.c2w), F)
        u = ((ix[s].astype(np.int32).astype(F) + F(0.5)).astype(F) - F(c.cx)).astype(F) / F(c.fx)
        v = (-((iy[s].astype(np.int32).astype(F) + F(0.5)).astype(F) - F(c.cy)).astype(F)) / F(c.fy)
        for k in range(3):
            o[s, k] = m[9 + k]
            dk = (((m[k] * u).astype(F) + (m[3 + k] * v).astype(F)).astype(F) + (m[6 + k] * F(-1.0))).astype(F)
            d[s, k] = np.where(inside[s], dk, F(0.0))
    return o, d


def draw(cams, targets, tile, seed, epoch, first, count):
    """mnv_ray_batcher_draw restated: targets: float32 [h, w, 4] (or [h * w, 4]) per camera.  -> dict(o, d float32 [n, 3], target float32
    [n, 4], unit int64 [count], cam, ix, iy int64 [n], inside bool [n]), n = count * tile * tile"""
    total = int(unit_table(cams, tile)[-1])
    assert 0 <= first and count >= 1 and first + count <= total
    units = perm(total, seed, epoch, np.arange(first, first + count))
    cam, ix, iy, inside = unit_pixels(cams, tile, units)
    o, d = pixel_rays(cams, cam, ix, iy, inside)
    tg = np.zeros((cam.size, 4), F)
    for ci, c in enumerate(cams):
        s = (cam == ci) & inside
        tg[s] = np.asarray(targets[ci], F).reshape(c.height, c.width, 4)[iy[s], ix[s]]
    return dict(o=o, d=d, target=tg, unit=units, cam=cam, ix=ix, iy=iy, inside=inside)


# ---- the cameras and images of the batcher tests ----------------------------------------------------------------------------------------
SIZES = ((32, 20), (9, 17), (8, 8))


def batch_cameras(mnv):
    """the batcher tests' cameras: three of different sizes (a whole number of tiles, ragged both ways, exactly one tile) at fit_cases' poses"""
    centers = [(-2.4, 1.1, 1.6), (1.9, 2.2, -1.2), (0.7, -2.6, 1.5)]
    out = []
    for (w, h), c in zip(SIZES, centers):
        back = np.array(c) / np.linalg.norm(c)
        out.append(mnv.Camera(w, h, 1.25 * w).set_pose(tuple(float(x) for x in c), tuple(float(x) for x in back.astype(np.float32))))
    return out


def batch_targets(cams, seed=5):
    """a random float32 [h, w, 4] image per camera, a few alphas 0"""
    rng = np.random.default_rng(seed)
    out = []
    for c in cams:
        t = rng.uniform(0.0, 1.0, size=(c.height, c.width, 4)).astype(F)
        t[..., 3] = np.where(rng.uniform(size=(c.height, c.width)) < 0.1, 0.0, 1.0)
        out.append(t)
    return out


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
def fit_ex(T, opt, cams, targets, steps, optimizer="adam", lr_colour=None, lr_sigma=None, beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"],
           batch_rays=0, tile=8, seed=0, rays=None):
    """mnv_n3tree_fit_ex restated on T (its data changes in place).  cams: CameraStruct per camera, targets: float32 [h * w, 4] per camera;
    rays: the cameras' (origins, dirs) when the caller has them (full batch).  -> (se_q32 per step, n_rays per step)"""
    import rays_ref

    lr_colour = ADAM["lr_colour"] if lr_colour is None else lr_colour
    lr_sigma = ADAM["lr_sigma"] if lr_sigma is None else lr_sigma
    master = fit_ref.master_init(T["data"])
    m1, m2 = np.zeros_like(master), np.zeros_like(master)
    acc = np.zeros(T["data"].shape, np.int64)
    if batch_rays:
        total = int(unit_table(cams, tile)[-1])
        B = batch_rays // (tile * tile)
        nb = -(-total // B)
    elif rays is None:
        rays = [tuple(a.reshape(-1, 3) for a in rays_ref.pinhole_rays(c)) for c in cams]
    se, n_rays = [], []
    for s in range(steps):
        if batch_rays:
            b = s % nb
            D = draw(cams, targets, tile, seed, s // nb, b * B, min(B, total - b * B))
            _, acc, sums, _ = fit_ref.rays_grad(T, opt, D["o"], D["d"], D["target"], acc=acc)
            se.append(sums["se_q32"]), n_rays.append(sums["n_rays"])
        else:
            tot = dict(se_q32=0, n_rays=0)
            for (o, d), tg in zip(rays, targets):
                _, acc, sums, _ = fit_ref.rays_grad(T, opt, o, d, tg, acc=acc)
                tot = {k: tot[k] + sums[k] for k in tot}
            se.append(tot["se_q32"]), n_rays.append(tot["n_rays"])
        if optimizer == "adam":
            adam_step(T["data"], master, m1, m2, acc, s + 1, lr_colour, lr_sigma, beta1, beta2, eps)
        else:
            fit_ref.sgd_step(T["data"], master, acc, lr_colour, lr_sigma)
    return se, n_rays


def full_loss(T, opt, cams, targets, rays=None):
    """se_q32 of all the cameras' rays on T's rows as they are"""
    import rays_ref

    if rays is None:
        rays = [tuple(a.reshape(-1, 3) for a in rays_ref.pinhole_rays(c)) for c in cams]
    return sum(fit_ref.backward(T, opt, fit_ref.forward(T, opt, o, d), tg)[1]["se_q32"] for (o, d), tg in zip(rays, targets))


def fit_scene(mnv, orc):
    """the fit scene of tests/fit_cases.py on the host: -> dict(T: the cut's tree dict, opt, cams: CameraStructs, targets: the oracle's frames
    of the full tree, rays)"""
    import cases
    import fit_cases
    import lod_ref
    import rays_ref

    S = fit_cases.FIT
    tree = cases.make_tree(mnv, fit_cases.TREES[S["tree"]])
    opt = mnv.RenderOptions.defaults()
    data, child, _ = tree.host_arrays()
    lod = lod_ref.make_lod(np.array(data), np.array(child), S["cut"])
    T = fit_ref.tree_of(mnv, tree)
    T.update(data=lod["data"].reshape(-1, T["data_dim"]).copy(), child=lod["child"].reshape(-1).copy(), capacity=lod["capacity"])
    cams = [c.c for c in fit_cases.fit_cameras(mnv)]
    targets = [orc.render(orc.tree_from_view(tree.host_view()), c, opt)["rgba"].reshape(-1, 4) for c in cams]
    rays = [tuple(a.reshape(-1, 3) for a in rays_ref.pinhole_rays(c)) for c in cams]
    return dict(T=T, opt=opt, cams=cams, targets=targets, rays=rays)


def sweep(mnv, orc, steps=12, pairs=((0.01, 0.3), (0.01, 1.5), (0.03, 0.3), (0.03, 1.0), (0.03, 1.5), (0.05, 0.3), (0.05, 1.5), (0.03, 3.0), (0.1, 3.0),
                                     (0.3, 10.0))):
    """twelve full-batch Adam steps on the fit scene for every rate pair: -> {(lr_colour, lr_sigma): [se / 2^32 per step]}"""
    S = fit_scene(mnv, orc)
    out = {}
    for lc, ls in pairs:
        T = dict(S["T"], data=S["T"]["data"].copy())
        se, _ = fit_ex(T, S["opt"], S["cams"], S["targets"], steps, "adam", lc, ls, rays=S["rays"])
        out[(lc, ls)] = [x / Q32 for x in se]
    return out


if __name__ == "__main__":
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import mega_nerf_viewer_amd as _mnv
    import mnv_oracle as _orc

    for (lc, ls), se in sweep(_mnv, _orc).items():
        falls = all(b < a for a, b in zip(se, se[1:]))
        print(f"lr_colour {lc:<5} lr_sigma {ls:<5} {'falls at every step' if falls else 'does NOT fall at every step'}: "
              + " ".join(f"{x:.3f}" for x in se[::4] + se[-1:]))
