"""The cases of the fitting tests (tests/test_fit_ref.py on the CPU, tests/test_fit_gpu.py on the device): synth_random trees at depth 1
and 4 with SH1 / SH4 / SH9 and RGBA rows, and per case a ray list -- the 24 x 24 pinhole frame of a camera that sees the whole volume
plus 64 hand-made rays (degenerate ones, misses, axis-parallel rays, rays from inside) -- with ray limits, targets and excluded rays."""
import numpy as np

import rays_ref

F = np.float32

TREES = {
    "sh1_d1": dict(kind="random", depth=1, basis_dim=1, refine_prob=0.6, empty_prob=0.25, sigma_max=30.0, coef_sd=1.5, seed=21),
    "rgba_d1": dict(kind="random", depth=1, basis_dim=-1, fmt=0, refine_prob=0.6, empty_prob=0.25, sigma_max=8.0, seed=22),
    "sh4_d4": dict(kind="random", depth=4, basis_dim=4, refine_prob=0.6, empty_prob=0.5, sigma_max=30.0, coef_sd=1.0, seed=23),
    "sh9_d4": dict(kind="random", depth=4, basis_dim=9, refine_prob=0.6, empty_prob=0.5, sigma_max=30.0, coef_sd=1.0, seed=24),
    "rgba_d4": dict(kind="random", depth=4, basis_dim=-1, fmt=0, refine_prob=0.6, empty_prob=0.5, sigma_max=25.0, seed=25),
    "sh1_d4": dict(kind="random", depth=4, basis_dim=1, refine_prob=0.6, empty_prob=0.5, sigma_max=12.0, coef_sd=1.5, seed=26),
}
# options on top of the struct defaults: the mask and the rotation of the view direction meet the SH9 rows
OPTIONS = {
    "sh9_d4": dict(basis_minmax=(1, 5), rot_dirs=(0.3, -0.2, 0.5)),
    "sh4_d4": dict(rot_dirs=(-0.1, 0.4, 0.2), background_brightness=0.5),
    "rgba_d4": dict(step_size=1e-3, stop_thresh=0.05),
}
NAMES = list(TREES)
FRAME = 24


def frame_camera(mnv, size=FRAME, pose=0):
    """the whole volume (world [-1, 1]^3) in a size x size frame, a pose without a zero in its matrix"""
    centers = [(-2.4, 1.1, 1.6), (1.9, 2.2, -1.2), (0.7, -2.6, 1.5)]
    c = np.array(centers[pose % 3], np.float64)
    back = (c / np.linalg.norm(c)).astype(np.float32)
    return mnv.Camera(size, size, 1.25 * size).set_pose(tuple(float(x) for x in c), tuple(float(x) for x in back))


def hand_rays(seed):
    """64 rays around the world box [-1, 1]^3: -> origins, dirs float32 [64, 3]"""
    rng = np.random.default_rng(seed)
    o = np.zeros((64, 3), np.float64)
    d = np.zeros((64, 3), np.float64)
    # 0 .. 3 degenerate: no direction, a NaN origin, an infinite direction, a direction whose squared length underflows
    o[0], d[0] = (-3.0, 0.1, 0.2), (0.0, 0.0, 0.0)
    o[1], d[1] = (np.nan, 0.0, 0.0), (1.0, 0.0, 0.0)
    o[2], d[2] = (-3.0, 0.1, 0.2), (np.inf, 0.0, 0.0)
    o[3], d[3] = (-3.0, 0.1, 0.2), (1e-30, 0.0, 0.0)
    # 4 .. 15 parallel to an axis, through the volume, lengths 1e-3 .. 1e3
    for i in range(4, 16):
        ax, sign = (i - 4) % 3, 1.0 if (i - 4) % 2 == 0 else -1.0
        o[i] = rng.uniform(-0.9, 0.9, 3)
        o[i, ax] = -sign * rng.uniform(1.5, 3.0)
        d[i, ax] = sign * 10.0 ** rng.uniform(-3, 3)
    # 16 .. 23 misses: from outside, away from the volume
    for i in range(16, 24):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o[i], d[i] = 2.5 * u, u + 0.2 * rng.normal(size=3)
    # 24 .. 35 from inside
    for i in range(24, 36):
        o[i], d[i] = rng.uniform(-0.9, 0.9, 3), rng.normal(size=3)
    # 36 .. 63 from outside at a point of the volume
    for i in range(36, 64):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o[i] = u * rng.uniform(2.0, 4.0)
        d[i] = (rng.uniform(-0.8, 0.8, 3) - o[i]) * 10.0 ** rng.uniform(-1, 1)
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    d32[d32 == 0] = 0.0   # (+0.0: the one-pixel camera of the oracle turns -0 into +0)
    return o32, d32


def make_options(mnv, name):
    import cases

    return cases.make_options(mnv, OPTIONS.get(name, {}))


def ray_list(mnv, name):
    """-> dict(o, d float32 [640, 3]; tmax float32 [640]; target float32 [640, 4]): the frame's rays first (row-major), then the 64"""
    seed = 1000 + NAMES.index(name)
    rng = np.random.default_rng(seed)
    fo, fd = rays_ref.pinhole_rays(frame_camera(mnv).c)
    ho, hd = hand_rays(seed)
    o = np.concatenate([fo.reshape(-1, 3), ho]).astype(np.float32)
    d = np.concatenate([fd.reshape(-1, 3), hd]).astype(np.float32)
    n = o.shape[0]
    tmax = np.full(n, 1e9, np.float32)
    pick = rng.uniform(size=n)
    lim = pick < 0.25                                   # a quarter of the rays end inside the volume, some before it
    tmax[lim] = (np.linalg.norm(o[lim].astype(np.float64), axis=1) * rng.uniform(0.5, 1.3, size=int(lim.sum()))).astype(np.float32)
    tmax[~np.isfinite(tmax)] = 1e9
    target = rng.uniform(0.0, 1.0, size=(n, 4)).astype(np.float32)
    target[:, 3] = 1.0
    target[rng.uniform(size=n) < 0.12, 3] = 0.0         # excluded rays
    target[5, 3] = np.nan                                # (any alpha but 0 includes the ray)
    return dict(o=o, d=d, tmax=tmax, target=target)


# The fit scene of both test files: the sh4_d4 tree cut one level down, three 16 x 16 cameras, struct-default options.  The learning rates
# were chosen with the restatement on this scene (tests/test_fit_ref.py repeats the check): lr_colour 2 and above lets the loss rise again
# after five or six steps (a coarse voxel under many rays), lr_colour 1 falls at every one of twelve steps for lr_sigma 5 .. 80; 20 is in
# the middle of that range.
FIT = dict(tree="sh4_d4", cut=3, size=16, cameras=3, lr_colour=1.0, lr_sigma=20.0, iterations=8)


def fit_cameras(mnv):
    return [frame_camera(mnv, FIT["size"], p) for p in range(FIT["cameras"])]
