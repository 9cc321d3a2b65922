"""The cases of the fitting tests (tests/test_fit_ref.py on the CPU, tests/test_fit_gpu.py on the device): synth_random trees at depth 1
and 4 with SH1 / SH4 / SH9 and RGBA rows, and per case a ray list -- the 24 x 24 pinhole frame of a camera that sees the whole volume
plus 64 hand-made rays (degenerate ones, misses, axis-parallel rays, rays from inside) -- with ray limits, targets and excluded rays.
Apart from those six, the edge cases (EDGE_TREES: SH16 / SH25 rows, scales that differ per axis) and the inputs of the edge tests: targets
that skip rays and saturate terms, links that leave the tree, padded rows, a tree view filled by hand."""
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

# The edge cases, kept apart from the six above (tables elsewhere are keyed on NAMES): the two widest SH rows -- data_dim 49 and 76, where
# one sample's row takes the whole wavefront and, for SH25, a second trip over columns 64 .. 75 -- and trees whose scale differs per
# axis, so that delta_scale varies with the ray's direction.
EDGE_TREES = {
    "sh16_d3_aniso": dict(kind="random", depth=3, basis_dim=16, refine_prob=0.6, empty_prob=0.4, sigma_max=30.0, coef_sd=0.7, seed=41,
                          scale=(0.5, 0.25, 0.125)),
    "sh25_d3": dict(kind="random", depth=3, basis_dim=25, refine_prob=0.6, empty_prob=0.4, sigma_max=30.0, coef_sd=0.5, seed=42),
    "sh4_d4_aniso": dict(kind="random", depth=4, basis_dim=4, refine_prob=0.6, empty_prob=0.5, sigma_max=30.0, coef_sd=1.0, seed=43,
                         offset=(0.4, 0.55, 0.5), scale=(0.3, 0.5, 0.2)),
}
EDGE_OPTIONS = {
    "sh16_d3_aniso": dict(basis_minmax=(2, 11), rot_dirs=(0.3, -0.2, 0.5)),
    "sh4_d4_aniso": dict(sigma_thresh=2.0, stop_thresh=0.05, background_brightness=0.5),
}
EDGE_NAMES = list(EDGE_TREES)
EDGE_SEEDS = {name: 1000 + len(NAMES) + i for i, name in enumerate(EDGE_NAMES)}     # the ray lists' seeds go on where NAMES' end


def tree_spec(name):
    return TREES[name] if name in TREES else EDGE_TREES[name]


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

    return cases.make_options(mnv, OPTIONS.get(name, EDGE_OPTIONS.get(name, {})))


def ray_list(mnv, name, seed=None):
    """-> dict(o, d float32 [640, 3]; tmax float32 [640]; target float32 [640, 4]): the frame's rays first (row-major), then the 64.
    seed: the six NAMES have their own; an edge name's is EDGE_SEEDS' unless given"""
    if seed is None:
        seed = 1000 + NAMES.index(name) if name in NAMES else EDGE_SEEDS[name]
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


# ---- inputs of the edge tests: what tests/test_fit_ref.py checks on the restatement, tests/test_fit_gpu.py and tests/test_visibility_gpu.py run
def skip_targets(target):
    """a list's targets with colours that leave [0, 1]: rows 10 .. 39 a finite red whose terms pass the +-32 clamp, rows 40 .. 49 an
    infinite green and rows 50 .. 59 a NaN blue (g is not finite: the ray is skipped), rows 60 .. 69 a red whose g is finite while its
    square is not (an infinite squared error and infinite terms saturate; for NaN terms see nan_terms).  Alpha stays as drawn."""
    tg = np.array(target, np.float32)
    tg[10:40, 0] = 1e6
    tg[40:50, 1] = np.inf
    tg[50:60, 2] = np.nan
    tg[60:70, 0] = 3e38
    return tg


# Links that leave the tree, on sh4_d4's arrays (157 chunks): the view's capacity is 151 while all 157 chunks stay allocated, and four
# links (flat index k: chunk k // 8) point back at chunk 0 -- so every bad link points inside the arrays.  Link 240 is the one whose
# target is chunk 151 itself, the first chunk outside: `inside` rays that start in its voxel meet it at their first step.
BROKEN = dict(tree="sh4_d4", capacity=151, to_root=(9, 20, 28, 41), edge_link=240, inside=64)


def cell_of(child, k):
    """(low corner [3], edge length) in tree space [0, 1]^3 of voxel k (flat index) of a child array"""
    child = np.asarray(child, np.int64).reshape(-1)
    path = [k % 8]
    chunk = k // 8
    while chunk != 0:
        above = np.nonzero((np.arange(child.size) // 8 + child == chunk) & (child != 0))[0]
        assert above.size == 1
        path.append(int(above[0]) % 8)
        chunk = int(above[0]) // 8
    lo, size = np.zeros(3), 1.0
    for j in reversed(path):
        size *= 0.5
        lo += size * np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1])
    return lo, size


def broken_links(T, L):
    """-> (the tree dict with the links of BROKEN and its capacity, the ray list with BROKEN's inside rays appended)"""
    child = T["child"].copy()
    for k in BROKEN["to_root"]:
        assert child[k] != 0 and k // 8 > 0
        child[k] = -(k // 8)
    k = BROKEN["edge_link"]
    assert k // 8 + child[k] == BROKEN["capacity"] < T["capacity"]
    lo, size = cell_of(T["child"], k)
    rng = np.random.default_rng(77)
    n = BROKEN["inside"]
    tree_pos = lo + size * rng.uniform(0.1, 0.9, size=(n, 3))
    o = ((tree_pos - T["offset"].astype(np.float64)) / T["scale"].astype(np.float64)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    target = rng.uniform(0.0, 1.0, size=(n, 4)).astype(np.float32)
    target[:, 3] = 1.0
    L2 = dict(o=np.concatenate([L["o"], o]), d=np.concatenate([L["d"], d]), tmax=np.concatenate([L["tmax"], np.full(n, 1e9, np.float32)]),
              target=np.concatenate([L["target"], target]))
    return dict(T, child=child, capacity=BROKEN["capacity"]), L2


def padded_rows(T):
    """an SH1 tree dict (data_dim 4) with its rows re-packed to data_dim 7: the coefficients in columns 0 .. 2, arbitrary finite binary16
    values in the padding columns 3 .. 5, sigma in column 6"""
    assert T["basis"] == 1 and T["data_dim"] == 4
    rng = np.random.default_rng(78)
    data = np.zeros((T["data"].shape[0], 7), np.uint16)
    data[:, :3] = T["data"][:, :3]
    shape = (data.shape[0], 3)
    pad = rng.normal(size=shape) * 10.0 ** rng.uniform(-4, 4, size=shape)
    data[:, 3:6] = pad.astype(np.float32).clip(-6e4, 6e4).astype(np.float16).view(np.uint16)
    data[:, 6] = T["data"][:, 3]
    return dict(T, data=data, data_dim=7)


def nan_terms(T, target):
    """an RGBA tree dict with its colours times 64, and a list's targets with rows 70 .. 399 at red = 3e38, green = -3e38: g stays finite,
    |e_k| passes 1.13 where the colours do, so g_0 * e_0 and g_1 * e_1 overflow to infinities of opposite sign and the density term is
    NaN: it reads 0.  (The SH cases cannot get there: their colours stay inside [0, 1], and no product of a finite g overflows.)"""
    assert T["basis"] == -1
    data = T["data"].copy()
    colours = data[:, :3].view(np.float16).astype(np.float32) * np.float32(64.0)
    data[:, :3] = colours.astype(np.float16).view(np.uint16)
    tg = np.array(target, np.float32)
    tg[70:400, 0] = 3e38
    tg[70:400, 1] = -3e38
    return dict(T, data=data), tg


def hand_view(mnv, torch, T):
    """a TreeView filled by hand over plain device tensors of a tree dict's arrays (all of them, whatever T["capacity"] says; no N3Tree,
    no accel) -> (view, data tensor int16 [rows, data_dim], child tensor): the tensors own the memory"""
    data_t = torch.from_numpy(np.ascontiguousarray(T["data"]).view(np.int16)).cuda()
    child_t = torch.from_numpy(np.ascontiguousarray(T["child"], np.int32)).cuda()
    v = mnv.TreeView()
    v.data, v.child = data_t.data_ptr(), child_t.data_ptr()
    for i in range(3):
        v.offset[i], v.scale[i] = float(T["offset"][i]), float(T["scale"][i])
    v.N, v.data_dim, v.capacity = 2, T["data_dim"], T["capacity"]
    v.format, v.basis_dim = (mnv.FORMAT_SH, T["basis"]) if T["basis"] > 0 else (mnv.FORMAT_RGBA, -1)
    return v, data_t, child_t


# The fit scene of both test files: the sh4_d4 tree cut one level down, three 16 x 16 cameras, struct-default options.  The learning rates
# were chosen with the restatement on this scene (tests/test_fit_ref.py repeats the check): lr_colour 2 and above lets the loss rise again
# after five or six steps (a coarse voxel under many rays), lr_colour 1 falls at every one of twelve steps for lr_sigma 5 .. 80; 20 is in
# the middle of that range.
FIT = dict(tree="sh4_d4", cut=3, size=16, cameras=3, lr_colour=1.0, lr_sigma=20.0, iterations=8)


def fit_cameras(mnv):
    return [frame_camera(mnv, FIT["size"], p) for p in range(FIT["cameras"])]
