"""The table behind tests/test_march_matrix_gpu.py: trees, cameras, options, the oracle's answers with the conditions under which they
say anything, the launcher's rule restated (which march_accel_kernel<BASIS, 256, MODE, BRICK, RAYS> a request should get), and the calls
of the packed-layout entry points in every launch shape.  Everything above `class Scene` runs without a GPU."""
import os

import numpy as np

import cases
import hooks
import rays_ref

W, H = 76, 52                 # ragged 8 x 8 tiles on both axes, 70 tiles (> 8 ray queues), more than one refill per wavefront
N_RAYS = 4097                 # as tests/test_rays_gpu.py: not a multiple of the block, of the tile or of the wavefront
TILE = (13, 9, 51, 35)        # a sub-rectangle whose origin and size are no multiples of 8
PART = (3, 16, 8)             # world, macro tile: 5 x 7 macro tiles, ragged on both axes
MAX_G = 8                     # max_guided_samples
THRESH_NEG = -0.25
FORMATS = (-1, 1, 4, 9, 16, 25)
DEPTHS = (6, 8, 10)
FAST_BOUND = 2e-6             # include/mnv.h: colours of the fast colour math against the exact ones

# random trees: leaves at every depth (record codes 0, 1, 2 on P3); shells: every leaf near the surface at the deepest level (inline words /
# record code 3).  sigma of the deep shells is raised until rays stop early in a 76 x 52 frame (see shares()).
RANDOM = {6: dict(empty_prob=0.6, sigma_max=60.0), 8: dict(empty_prob=0.85, sigma_max=200.0), 10: dict(empty_prob=0.93, sigma_max=400.0)}
# (refine_prob, seed number) per (format, depth): the first of a search over refine_prob 0.40 .. 0.55 and seeds 900 + depth + basis + 100 k whose
# three poses all meet Truth.check_conditions on the oracle's frames (many seeds look at one big leaf, or at no background at all).
# search_random_pick() below repeats the search without a GPU (python tests/march_matrix.py)
RANDOM_PICK = {(-1, 6): (0.42, 24), (-1, 8): (0.42, 0), (-1, 10): (0.42, 0), (1, 6): (0.46, 175), (1, 8): (0.42, 0), (1, 10): (0.42, 5),
               (4, 6): (0.46, 6), (4, 8): (0.42, 1), (4, 10): (0.42, 0), (9, 6): (0.4, 9), (9, 8): (0.46, 2), (9, 10): (0.42, 1),
               (16, 6): (0.42, 6), (16, 8): (0.46, 0), (16, 10): (0.42, 15), (25, 6): (0.46, 14), (25, 8): (0.42, 0), (25, 10): (0.42, 0)}
SHELL = {8: dict(radius=0.3, sigma_lo=5.0, sigma_hi=60.0), 10: dict(radius=0.08, sigma_lo=50.0, sigma_hi=400.0),
         12: dict(radius=0.03, sigma_lo=200.0, sigma_hi=1600.0)}
RANDOM_POSES = [((-2.5, 1.4, 1.8), (-0.74, 0.4, 0.54)), ((2.2, -1.9, 1.1), (0.7, -0.6, 0.39)), ((1.3, 2.4, -1.5), (0.42, 0.77, -0.48))]

# Every instantiation of march_accel_kernel outside the diagnostics MODE 1 (tests/test_march_diag_gpu.py runs that one), read off the three units that instantiate it
# (csrc/mnv_accel_march.hip, mnv_accel_march_brick.hip, mnv_accel_march_rays.hip times the MODEs of csrc/mnv_march_launch.h):
# (BASIS, MODE, BRICK, RAYS).  MODE 3 (samples) and 5 (depth image) exist for BASIS 9 only, MODE 4 (fast colour) for SH rows of frames only.
VARIANTS = sorted(
    [(b, m, 0, 0) for b in (-1, 1, 4, 16, 25) for m in ((0, 2) if b < 0 else (0, 2, 4))] + [(9, m, 0, 0) for m in (0, 2, 3, 4, 5)]
    + [(b, m, 1, 0) for b in (-1, 1, 4) for m in ((0, 2) if b < 0 else (0, 2, 4))] + [(9, m, 1, 0) for m in (0, 2, 3, 4, 5)]
    + [(b, 0, 0, 1) for b in (-1, 1, 4, 9, 16, 25)] + [(9, 5, 0, 1)] + [(b, 0, 1, 1) for b in (-1, 1, 4, 9)] + [(9, 5, 1, 1)])
assert len(VARIANTS) == 44 and len(set(VARIANTS)) == 44

RECORDING = os.path.abspath(os.environ.get("MNV_LIB_PATH", "")) == os.path.abspath(hooks.HOOKS_LIB)   # the child run on the test-hook build
recorded = set()     # variants the recorder reported (child run)
predicted = set()    # variants the table predicts for the cells that ran


def predict(b, bricks, *, rays=False, tracked=False, samples=False, depth=False, fast=False, thresh=0.01):
    """The launcher's rule (csrc/mnv_accel_capi.hip launch_accel, csrc/mnv_march_launch.h launch_march_mode) restated."""
    colourless = samples or (depth and not tracked)
    brick = bricks and not thresh < 0 and (b < 16 or colourless)
    basis = 9 if colourless else b
    if not rays and samples:
        mode = 3
    elif not rays and tracked:
        mode = 2
    elif basis == 9 and depth:
        mode = 5
    elif not rays and basis >= 1 and fast:
        mode = 4
    else:
        mode = 0
    return (basis, mode, int(bool(brick)), int(rays))


# the requests run_whole_frame_cells issues on every tree, as predict() takes them: kinds (a) .. (h), (i) = (c) .. (h) in fast mode, (j)
WHOLE_FRAME_REQUESTS = (
    [dict(), dict(fast=True), dict(depth=True), dict(tracked=True), dict(tracked=True, depth=True), dict(samples=True), dict(rays=True),
     dict(rays=True, depth=True)]
    + [dict(fast=True, **kw) for kw in (dict(depth=True), dict(tracked=True), dict(tracked=True, depth=True), dict(samples=True), dict(rays=True),
                                        dict(rays=True, depth=True))]
    + [dict(thresh=THRESH_NEG, **kw) for kw in (dict(), dict(tracked=True), dict(samples=True), dict(rays=True))])


def planned_variants():
    """what the table predicts for the whole-frame cells of every (format, lookup path)"""
    return {predict(b, bricks, **kw) for b in FORMATS for bricks in (False, True) for kw in WHOLE_FRAME_REQUESTS}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.ascontiguousarray(a)


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def make_grid(mnv):
    g = mnv.ClusterGrid()
    g.grid_dim[0], g.grid_dim[1] = 3, 2
    for i, (lo, rng) in enumerate([(-1.0, 2.0), (-1.1, 2.2), (-0.9, 1.8)]):
        g.min_position[i], g.range[i] = lo, rng
    return g


def chunk_depths(parent):
    cap = len(parent)
    depth = np.zeros(cap, np.int32)
    depth[0] = 1
    pc = parent >> 3
    for _ in range(64):
        todo = (depth == 0) & (depth[pc] > 0)
        todo[0] = False
        if not todo.any():
            break
        depth[todo] = depth[pc[todo]] + 1
    assert (depth > 0).all()
    return depth


def make_tree(mnv, b, depth, kind):
    """-> (N3Tree, whatever must stay alive with it)"""
    if kind == "random":
        fmt = dict(fmt=0) if b == -1 else {}
        refine, seed = RANDOM_PICK[(b, depth)]
        return mnv.N3Tree.synth_random(depth=depth, basis_dim=b, refine_prob=refine, seed=900 + depth + b + 100 * seed, **RANDOM[depth], **fmt), None
    p = SHELL[depth]
    if b != -1:
        return mnv.N3Tree.synth_shell(depth=depth, basis_dim=b, half_thickness=1.5 / 2 ** depth, seed=b, **p), None
    # the shell generator writes SH rows; an SH1 row has the four halves of an RGBA row: the same arrays read as RGBA
    sh1 = mnv.N3Tree.synth_shell(depth=depth, basis_dim=1, half_thickness=1.5 / 2 ** depth, seed=b, **p)
    data, child, parent = (np.array(a) for a in sh1.host_arrays())
    keep = (data, child, parent)
    return mnv.N3Tree.from_arrays(data, child, data_format=mnv.data_format_to_string(mnv.FORMAT_RGBA, -1), parent=parent), keep


def cameras(mnv, depth, kind):
    """three poses of one image size: pose 0 is the cell's frame, all three are the batch"""
    if kind == "random":
        return [mnv.Camera(W, H, 190.0).set_pose(c, bk) for c, bk in RANDOM_POSES]
    # the camera orbits at 3.5 shell diameters (world radius 2 r: the unit cube is world [-1, 1]); the shell spans 0.8 of the width
    r = 2.0 * SHELL[depth]["radius"]
    dist = 7.0 * r
    fx = 0.8 * W / (2.0 * r / np.sqrt(dist * dist - r * r))
    return [mnv.orbit_camera(W, H, float(fx), dist, 22.5 * k + 10.0, 20.0 + 7.0 * k) for k in range(3)]


def options(mnv, depth_image=False, thresh=None, viewdir=False, embedding=-1):
    opt = mnv.RenderOptions.cli_defaults()
    opt.max_depth, opt.max_sample_count, opt.max_guided_samples = 16, 9, MAX_G   # max_depth above every tree's depth
    opt.render_depth = bool(depth_image)
    opt.need_viewdir, opt.appearance_embedding = int(viewdir), embedding
    if thresh is not None:
        opt.sigma_thresh = thresh
    return opt


def ray_inputs(seed, shape, dist):
    """The two on-screen inputs of a ray list, after cases.onscreen_inputs (which builds images: frames use it as it is): limits scattered
    around the camera's distance to the scene centre, 15 % "no mesh", 5 % "mesh in front of the camera"; blocks + noise under the volume."""
    rng = np.random.default_rng(seed)
    tmax = (dist * rng.uniform(0.55, 1.35, size=shape)).astype(np.float32)
    u = rng.uniform(size=shape)
    tmax[u < 0.15] = np.float32(1e9)
    tmax[u > 0.95] = np.float32(0.0)
    image = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    block = ((idx // 16) % 2).astype(bool)
    image[block, :3] = image[block, :3] // 4 + np.uint8(180)
    image[idx % 37 == 0, :3] = (0, 255, 1)
    return tmax, np.ascontiguousarray(image)


def shares(rgba):
    """(background only, 0 < alpha < 1, stopped early) shares of a colour frame's pixels or of a ray list: alpha is the volume's own, 0 for a
    ray without a dense sample and exactly 1 for one that stopped early (rt_core.cuh:295-307 rescales by 1 / (1 - T) and sets it)"""
    a = rgba[..., 3].ravel()
    return float((a == 0).mean()), float(((a > 0) & (a < 1)).mean()), float((a >= 1).mean())


class Truth:
    """Host side of one (format, depth, tree kind): the tree, the oracle's tree with sample counts, and the oracle's answers, cached."""

    def __init__(self, mnv, orc, b, depth, kind):
        self.mnv, self.orc, self.b, self.depth, self.kind = mnv, orc, b, depth, kind
        self.name = f"{'RGBA' if b < 0 else 'SH%d' % b}/d{depth}/{kind}"
        self.tree, self._keep = make_tree(mnv, b, depth, kind)
        self.view = self.tree.host_view()
        self.cap = self.view.capacity
        # 0..13 against max_sample_count = 9.  Four in five are saturated, and every voxel of the four coarsest levels is: a ray that crosses
        # coarse leaves only finds no candidate (its row stays -1), the others fall back to the walk over saturated leaves
        self.chunk_depth = chunk_depths(np.array(self.tree.host_arrays()[2]))
        self.counts = np.random.default_rng(1000 + depth + b).choice(14, size=(self.cap, 8), p=[0.2 / 9] * 9 + [0.8 / 5] * 5).astype(np.int16)
        self.counts[self.chunk_depth <= 4] = 12
        self.otree = orc.tree_from_view(self.view, sample_counts=self.counts)
        self.cams = cameras(mnv, depth, kind)
        self.grid = make_grid(mnv)
        idx = FORMATS.index(b) + DEPTHS.index(min(depth, 10)) + (kind == "shell")
        self.viewdir, self.embedding = bool(idx % 2), (5 if idx % 4 >= 2 else -1)     # extras of the sample rows on half of the cells each
        self.dim = 4 + 3 * self.viewdir + (self.embedding != -1)
        self.dist = float(np.linalg.norm(np.array(list(self.cams[0].c.c2w), np.float64)[9:12]))
        self.cache = {}
        self._rays = None

    def opt(self, depth_image=False, thresh=None):
        return options(self.mnv, depth_image, thresh, self.viewdir, self.embedding)

    def inputs(self, tile=None):
        tmax, image = cases.onscreen_inputs("onscreen_both", self.cams[0])    # (tmax_px and rgba8_init, as the viewer's render loop passes them)
        if tile is not None:
            x0, y0, w, h = tile
            tmax, image = np.ascontiguousarray(tmax[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(image[y0:y0 + h, x0:x0 + w])
        return tmax, image

    def frame(self, pose=0, depth_image=False, tracked=False, thresh=None, tile=None, onscr=False):
        key = ("frame", pose, depth_image, tracked, thresh, tile, onscr)
        if key not in self.cache:
            tmax, image = self.inputs(tile) if onscr else (None, None)
            visited = np.zeros(self.cap, np.int32) if tracked else None
            r = self.orc.render(self.otree, self.cams[pose].c, self.opt(depth_image, thresh), tile, want_rgba8=True, want_trackers=tracked,
                                visited=visited, track_visit=tracked, tmax_px=tmax, rgba8_init=image)
            r["visited"] = visited
            r["hits"] = int(r["counters"].hits)
            self.cache[key] = r
        return self.cache[key]

    def samples(self, thresh=None, onscr=False):
        key = ("samples", thresh, onscr)
        if key not in self.cache:
            visited = np.zeros(self.cap, np.int32)
            r = self.orc.get_samples(self.otree, self.cams[0].c, self.opt(False, thresh), self.grid, self.dim, visited=visited, track_visit=True,
                                     tmax_px=self.inputs()[0] if onscr else None)
            r["visited"] = visited
            self.cache[key] = r
        return self.cache[key]

    def ray_list(self):
        """N_RAYS rays: the pixels' rays of pose 0 and the first of pose 1, directions of lengths 1e-3 .. 1e3; a limit and a pixel under each"""
        if self._rays is None:
            o0, d0 = rays_ref.pinhole_rays(self.cams[0].c)
            o1, d1 = rays_ref.pinhole_rays(self.cams[1].c)
            o = np.concatenate([o0.reshape(-1, 3), o1.reshape(-1, 3)])[:N_RAYS]
            d = np.concatenate([d0.reshape(-1, 3), d1.reshape(-1, 3)])[:N_RAYS]
            rng = np.random.default_rng(31 + self.depth + self.b)
            d = (d * (10.0 ** rng.uniform(-3, 3, size=(N_RAYS, 1))).astype(np.float32)).astype(np.float32)
            d[d == 0] = 0.0
            tmax, image = ray_inputs(78 + self.depth + self.b, (N_RAYS,), self.dist)
            self._rays = (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d), tmax, image)
        return self._rays

    def rays(self, depth_image=False, thresh=None, onscr=False):
        key = ("rays", depth_image, thresh, onscr)
        if key not in self.cache:
            o, d, tmax, image = self.ray_list()
            rgba, rgba8 = rays_ref.oracle_rays(self.orc, self.otree, o, d, self.opt(depth_image, thresh), tmax if onscr else None, image if onscr else None)
            self.cache[key] = dict(rgba=rgba, rgba8=rgba8)
        return self.cache[key]

    # ---- the conditions under which a cell says anything, on the oracle's output alone

    def check_conditions(self, info):
        """info: mnv.accel_info of the tree's accel (the lookup path).  Returns the measured figures."""
        fig = {}
        ref = self.frame()
        s = shares(ref["rgba"])
        fig["shares"] = s
        assert min(s) >= 0.05, f"{self.name}: shares (background, partial, stopped early) {s}"
        sr = shares(self.rays()["rgba"])
        fig["ray_shares"] = sr
        assert min(sr) >= 0.05, f"{self.name}: ray-list shares {sr}"
        trk = self.frame(tracked=True)
        named = trk["sample"][..., 1] >= 0
        assert named.any() and (~named).any(), f"{self.name}: sample tracker rows that name a voxel {int(named.sum())} of {named.size}"
        fig["sample_rows"] = (int(named.sum()), int((~named).sum()))
        split = trk["split"].reshape(-1, 3)
        has = split[:, 1] >= 0
        # depth of the leaf a split row names: of its chunk (the root chunk's voxels are depth 1), as the row's first column says
        cd = self.chunk_depth
        leaf_depth = cd[split[has, 1].astype(np.int64)]
        assert np.array_equal(leaf_depth, split[has, 0].astype(np.int32) + 1) or np.array_equal(leaf_depth, split[has, 0].astype(np.int32)), self.name
        if self.kind == "shell" and info["brick_levels"] > 0:
            deepest = float((leaf_depth == cd.max()).sum()) / split.shape[0]
            fig["deepest"] = deepest
            assert cd.max() == self.depth and deepest >= 0.5, f"{self.name}: {deepest:.3f} of the pixels' split rows name a leaf of depth {cd.max()}"
        if self.kind == "random" and info["brick_levels"] == 2:
            L2 = info["grid2_level"]
            n = (int((leaf_depth == L2 + 1).sum()), int((leaf_depth == L2 + 2).sum()), int((leaf_depth <= L2).sum()))
            fig["record_depths"] = n
            assert min(n) >= 5, f"{self.name}: split rows at depth {L2 + 1}, {L2 + 2}, <= {L2}: {n}"
        neg = self.frame(thresh=THRESH_NEG)
        fig["hits_ratio"] = neg["hits"] / max(1, ref["hits"])
        assert neg["hits"] >= 3 * ref["hits"], f"{self.name}: hits {ref['hits']} -> {neg['hits']} with sigma_thresh {THRESH_NEG}"
        # the sample march takes the steps of the frame's march: its visit marks are the tracked frame's (used for the sub-rectangle of
        # sample emission, which the oracle renders as a whole frame only)
        assert np.array_equal(self.samples()["visited"], trk["visited"]), self.name
        return fig


PATHS = {6: (0, 0), 8: (7, 1), 10: (8, 2), 12: (8, 2)}   # tree depth -> (grid2_level, brick_levels): P0, P2 (inline cell words), P3 (records)


class Scene:
    """Device side of a Truth: the tree on the device, its accel, and one method per frame kind that issues the request in a launch shape
    and returns numpy arrays laid out like the oracle's.  Every launch is held against predict() in the recording run."""

    def __init__(self, truth, torch):
        self.t, self.torch, self.mnv = truth, torch, truth.mnv
        mnv = self.mnv
        truth.tree.move_to_device(need_parent=True)
        self.accel = truth.tree.accel
        self.dv = truth.tree.device_view()
        self.parent = self.dv.parent
        assert self.parent
        self.counts = torch.from_numpy(truth.counts).cuda()
        self.dv.sample_counts = self.counts.data_ptr()       # (the reference-layout kernel reads the counts from the view)
        self.info = mnv.accel_info(self.accel)
        assert (self.info["grid2_level"], self.info["brick_levels"]) == PATHS[truth.depth], (truth.name, self.info)
        self.bricks = self.info["brick_levels"] > 0
        self.fast = False
        self.max_fast_diff = 0.0
        self.fast_bytes_off = self.fast_bytes = 0     # RGBA8 colour bytes of MODE 4 frames that differ from the oracle's, of how many

    # ---- plumbing

    def set_fast(self, on):
        self.mnv.accel_set_colour_math(self.accel, 1 if on else 0)
        self.fast = bool(on)

    def note(self, **kw):
        want = predict(self.t.b, self.bricks, fast=self.fast, **kw)
        predicted.add(want)
        if RECORDING:
            got = self.mnv.last_march_variant()
            assert got == want, f"{self.t.name} {kw} fast={self.fast}: launched {got}, the table predicts {want}"
            recorded.add(got)

    def f32(self, *shape, fill=float("nan")):
        return self.torch.full(shape, fill, dtype=self.torch.float32, device="cuda")

    def u8(self, *shape):
        return self.torch.full(shape, 7, dtype=self.torch.uint8, device="cuda")

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def host(self, **tensors):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in tensors.items() if v is not None}

    def assemble(self, per_rank, root_period, channels):
        """per_rank[r]: [local tiles][th][tw][channels] of rank r -> the frame, as rank 0 puts the gathered tiles back"""
        from mega_nerf_viewer_amd.multigpu import TilePartition
        world, tw, th = PART
        part = TilePartition(W, H, world, tw, th, root_period)
        mx, my = -(-W // tw), -(-H // th)
        out = np.zeros((my * th, mx * tw, channels), per_rank[0].dtype)
        for rank in range(world):
            tiles = part.tiles_of(rank)
            assert len(tiles) == self.mnv.partition_local_tiles((0, 0, W, H), rank, world, tw, th, root_period) <= per_rank[rank].shape[0]
            for j, m in enumerate(tiles):
                out[(m // mx) * th:(m // mx + 1) * th, (m % mx) * tw:(m % mx + 1) * tw] = per_rank[rank][j]
        return out[:H, :W]

    def local_tiles(self, rank, root_period):
        world, tw, th = PART
        return max(1, self.mnv.partition_local_tiles((0, 0, W, H), rank, world, tw, th, root_period))

    # ---- frame kinds

    def frame(self, pose=0, depth_image=False, thresh=None, tile=None, part=None, onscr=False, want8=True):
        """kinds (a), (b), (c): mnv_render_voxels_accel[_ex|_part].  part: the root_period of the PART partition (every rank, put back together)"""
        mnv, cam, opt = self.mnv, self.t.cams[pose], self.t.opt(depth_image, thresh)
        kw = dict(depth=depth_image, thresh=opt.sigma_thresh)
        if part is None:
            w, h = (tile[2], tile[3]) if tile else (W, H)
            rgba, rgba8 = self.f32(h, w, 4), (self.u8(h, w, 4) if want8 else None)
            tmax, image = (self.dev(a) for a in self.t.inputs(tile)) if onscr else (None, None)
            mnv.render_voxels_accel(self.accel, cam, opt, tile=tile, rgba=rgba, rgba8=rgba8, tmax_px=tmax, rgba8_init=image)
            self.note(**kw)
            return self.host(rgba=rgba, rgba8=rgba8)
        world, tw, th = PART
        bufs, bufs8 = [], []
        for rank in range(world):
            n = self.local_tiles(rank, part)
            rgba, rgba8 = self.f32(n, th, tw, 4), self.u8(n, th, tw, 4)
            mnv.render_voxels_accel_part(self.accel, cam, opt, rank, world, tw, th, rgba=rgba, rgba8=rgba8, root_period=part)
            self.note(**kw)
            got = self.host(rgba=rgba, rgba8=rgba8)
            bufs.append(got["rgba"])
            bufs8.append(got["rgba8"])
        return dict(rgba=self.assemble(bufs, part, 4), rgba8=self.assemble(bufs8, part, 4))

    def batch(self, depth_image=False):
        """three cameras in one launch (mnv_render_voxels_accel_batch)"""
        opt = self.t.opt(depth_image)
        rgba, rgba8 = self.f32(3, H, W, 4), self.u8(3, H, W, 4)
        self.mnv.render_voxels_accel_batch(self.accel, self.t.cams, opt, rgba=rgba, rgba8=rgba8)
        self.note(depth=depth_image)
        return self.host(rgba=rgba, rgba8=rgba8)

    def tracked(self, depth_image=False, thresh=None, tile=None, part=None, onscr=False):
        """kinds (d), (e): mnv_render_voxels_accel_visit_ex / _visit_part with both trackers, the counts, visit marks and their closure"""
        mnv, torch, cam, opt = self.mnv, self.torch, self.t.cams[0], self.t.opt(depth_image, thresh)
        kw = dict(tracked=True, depth=depth_image, thresh=opt.sigma_thresh)
        visited = torch.zeros(self.t.cap, dtype=torch.int32, device="cuda")
        if part is None:
            w, h = (tile[2], tile[3]) if tile else (W, H)
            rgba, rgba8, split, sample = self.f32(h, w, 4), self.u8(h, w, 4), self.f32(h, w, 3, fill=-1.0), self.f32(h, w, 3, fill=-1.0)
            tmax, image = (self.dev(a) for a in self.t.inputs(tile)) if onscr else (None, None)
            mnv.render_voxels_accel_visit(self.accel, cam, opt, visited, self.parent, tile=tile, rgba=rgba, rgba8=rgba8, split_track=split,
                                          sample_track=sample, sample_counts=self.counts, tmax_px=tmax, rgba8_init=image)
            self.note(**kw)
            return self.host(rgba=rgba, rgba8=rgba8, split=split, sample=sample, visited=visited)
        world, tw, th = PART
        bufs = {k: [] for k in ("rgba", "rgba8", "split", "sample")}
        for rank in range(world):
            n = self.local_tiles(rank, part)
            t = dict(rgba=self.f32(n, th, tw, 4), rgba8=self.u8(n, th, tw, 4), split=self.f32(n, th, tw, 3, fill=-1.0), sample=self.f32(n, th, tw, 3, fill=-1.0))
            mnv.render_voxels_accel_visit(self.accel, cam, opt, visited, self.parent, rgba=t["rgba"], rgba8=t["rgba8"], split_track=t["split"],
                                          sample_track=t["sample"], sample_counts=self.counts, part=(rank, world, tw, th, part))
            self.note(**kw)
            for k, v in self.host(**t).items():
                bufs[k].append(v)
        out = {k: self.assemble(v, part, v[0].shape[-1]) for k, v in bufs.items()}
        out.update(self.host(visited=visited))     # the ranks' marks in one array: the whole frame's
        return out

    def samples(self, thresh=None, tile=None, onscr=False):
        """kind (f): mnv_get_samples_from_voxels_accel_visit_ex"""
        mnv, torch, opt = self.mnv, self.torch, self.t.opt(False, thresh)
        w, h = (tile[2], tile[3]) if tile else (W, H)
        n = w * h
        num = torch.zeros(n, dtype=torch.int16, device="cuda")
        smp = self.f32(n, MAX_G, self.t.dim, fill=-1.0)
        cl = torch.full((n, MAX_G), -1, dtype=torch.int16, device="cuda")
        split, sample = self.f32(n, 3, fill=-1.0), self.f32(n, 3, fill=-1.0)
        visited = torch.zeros(self.t.cap, dtype=torch.int32, device="cuda")
        tmax = self.dev(self.t.inputs(tile)[0]) if onscr else None
        mnv.get_samples_from_voxels_accel_visit(self.accel, self.t.cams[0], opt, visited, self.parent, num, smp, cl, self.t.grid, split_track=split,
                                                sample_track=sample, sample_counts=self.counts, tile=tile, tmax_px=tmax)
        self.note(samples=True, thresh=opt.sigma_thresh)
        return self.host(num_samples=num, samples=smp, cluster_indices=cl, split=split, sample=sample, visited=visited)

    def rays(self, depth_image=False, thresh=None, onscr=False):
        """kinds (g), (h): mnv_render_rays_accel on the flat list"""
        opt = self.t.opt(depth_image, thresh)
        o, d, tmax, image = self.t.ray_list()
        rgba, rgba8 = self.f32(N_RAYS, 4), self.u8(N_RAYS, 4)
        self.mnv.render_rays_accel(self.accel, self.dev(o), self.dev(d), opt, rgba=rgba, rgba8=rgba8, tmax=self.dev(tmax) if onscr else None,
                                   rgba8_init=self.dev(image) if onscr else None)
        self.note(rays=True, depth=depth_image, thresh=opt.sigma_thresh)
        return self.host(rgba=rgba, rgba8=rgba8)

    def ref_layout(self, depth_image=False, tracked=False):
        """march_ref_layout_kernel on the same arrays (mnv_render_voxels)"""
        torch, opt = self.torch, self.t.opt(depth_image)
        rgba, rgba8 = self.f32(H, W, 4), self.u8(H, W, 4)
        split = sample = visited = None
        if tracked:
            split, sample = self.f32(H, W, 3, fill=-1.0), self.f32(H, W, 3, fill=-1.0)
            visited = torch.zeros(self.t.cap, dtype=torch.int32, device="cuda")
        self.mnv.render_voxels(self.dv, self.t.cams[0], opt, rgba=rgba, rgba8=rgba8, split_track=split, sample_track=sample, visited=visited,
                               track_visit=tracked)
        return self.host(rgba=rgba, rgba8=rgba8, split=split, sample=sample, visited=visited)

    # ---- comparisons with the oracle

    def frame_check(self, depth_image):
        """how a frame of kinds (a) / (b) / (c) is held against the oracle: bit for bit, but for the frames that MODE 4 renders"""
        if predict(self.t.b, self.bricks, depth=depth_image, fast=self.fast)[1] == 4:
            return lambda got, want, what: self.fast_close(got, want, what)
        return lambda got, want, what: self.equal(got, want, what, FRAME_KEYS)

    def equal(self, got, want, what, keys):
        for k in keys:
            assert same(got[k], want[k].reshape(got[k].shape)), f"{self.t.name} {what}: {k} differs from the oracle " \
                f"({int((bits(got[k]) != bits(want[k].reshape(got[k].shape))).sum())} of {got[k].size} words)"

    def fast_close(self, got, want, what):
        """a MODE 4 frame: alpha bit-identical to the oracle, colours within FAST_BOUND of it.  Its RGBA8 pixels get no tolerance of their own:
        they are the frame's OWN float colours packed as the reference packs them (renderer_kernel.cu:237, uint8_t(v * 255): truncation,
        saturating), alpha byte 255 -- so a byte differs from the oracle's only where the float colour crossed a multiple of 1 / 255."""
        g, w = got["rgba"], want["rgba"].reshape(got["rgba"].shape)
        assert same(g[..., 3], w[..., 3]), f"{self.t.name} {what}: alpha of the fast colour math differs from the oracle"
        d = float(np.abs(g[..., :3] - w[..., :3]).max())
        self.max_fast_diff = max(self.max_fast_diff, d)
        assert d <= FAST_BOUND, f"{self.t.name} {what}: colours of the fast colour math are {d:.3g} from the oracle (bound {FAST_BOUND})"
        scaled = g[..., :3] * np.float32(255.0)
        packed = np.where(scaled > 0, np.minimum(scaled, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)    # (truncates)
        g8, w8 = got["rgba8"], want["rgba8"].reshape(got["rgba8"].shape)
        assert np.array_equal(g8[..., 3], w8[..., 3]), f"{self.t.name} {what}: RGBA8 alpha byte"
        assert np.array_equal(g8[..., :3], packed), f"{self.t.name} {what}: {int((g8[..., :3] != packed).sum())} RGBA8 colour bytes are not the frame's float colours packed"
        self.fast_bytes_off += int((g8[..., :3] != w8[..., :3]).sum())
        self.fast_bytes += packed.size
        return d


FRAME_KEYS = ("rgba", "rgba8")
TRACK_KEYS = ("rgba", "rgba8", "split", "sample", "visited")
SAMPLE_KEYS = ("num_samples", "samples", "cluster_indices", "split", "sample", "visited")


def run_whole_frame_cells(sc):
    """Kinds (a) .. (j) and the reference-layout kernel, whole frame, one camera (ray lists: the whole list).  -> figures of the cell"""
    t = sc.t
    fig = t.check_conditions(sc.info)
    exact = sc.frame()
    sc.equal(exact, t.frame(), "(a) plain", FRAME_KEYS)
    sc.equal(sc.frame(depth_image=True), t.frame(depth_image=True), "(c) depth image", FRAME_KEYS)
    for e, name in ((False, "(d) trackers"), (True, "(e) trackers + render_depth")):
        sc.equal(sc.tracked(depth_image=e), t.frame(depth_image=e, tracked=True), name, TRACK_KEYS)
    sc.equal(sc.samples(), t.samples(), "(f) sample emission", SAMPLE_KEYS)
    sc.equal(sc.rays(), t.rays(), "(g) ray list", FRAME_KEYS)
    sc.equal(sc.rays(depth_image=True), t.rays(depth_image=True), "(h) ray list, depth", FRAME_KEYS)
    # (j) a negative threshold: empty leaves are dense samples, the inline words / records cannot answer, the launch walks the node words
    sc.equal(sc.frame(thresh=THRESH_NEG), t.frame(thresh=THRESH_NEG), "(j) plain, sigma_thresh < 0", FRAME_KEYS)
    sc.equal(sc.tracked(thresh=THRESH_NEG), t.frame(tracked=True, thresh=THRESH_NEG), "(j) trackers, sigma_thresh < 0", TRACK_KEYS)
    sc.equal(sc.samples(thresh=THRESH_NEG), t.samples(thresh=THRESH_NEG), "(j) sample emission, sigma_thresh < 0", SAMPLE_KEYS)
    sc.equal(sc.rays(thresh=THRESH_NEG), t.rays(thresh=THRESH_NEG), "(j) ray list, sigma_thresh < 0", FRAME_KEYS)
    # the reference-layout kernel on the same arrays
    sc.equal(sc.ref_layout(depth_image=True), t.frame(depth_image=True), "(c) reference layout", FRAME_KEYS)
    for e in (False, True):
        sc.equal(sc.ref_layout(depth_image=e, tracked=True), t.frame(depth_image=e, tracked=True), f"(d/e) reference layout, render_depth={e}", TRACK_KEYS)
    # (b) and (i): the accel in fast mode
    sc.set_fast(True)
    try:
        fast = sc.frame()
        sc.frame_check(False)(fast, t.frame(), "(b) fast colour math")     # (RGBA rows have no MODE 4: bit for bit)
        fig["fast_diff"] = sc.max_fast_diff
        if t.b >= 1:   # the condition under which (b) says anything: SH rows go through the sigmoid, and the hardware's differs somewhere
            assert not same(fast["rgba"], exact["rgba"]), f"{t.name}: the fast frame equals the exact one bit for bit"
        else:
            assert same(fast["rgba"], exact["rgba"]) and same(fast["rgba8"], exact["rgba8"]), f"{t.name}: RGBA rows have no sigmoid"
        sc.equal(sc.frame(depth_image=True), t.frame(depth_image=True), "(i) depth image, fast mode", FRAME_KEYS)
        for e in (False, True):
            sc.equal(sc.tracked(depth_image=e), t.frame(depth_image=e, tracked=True), f"(i) trackers, render_depth={e}, fast mode", TRACK_KEYS)
        sc.equal(sc.samples(), t.samples(), "(i) sample emission, fast mode", SAMPLE_KEYS)
        sc.equal(sc.rays(), t.rays(), "(i) ray list, fast mode", FRAME_KEYS)
        sc.equal(sc.rays(depth_image=True), t.rays(depth_image=True), "(i) ray list, depth, fast mode", FRAME_KEYS)
    finally:
        sc.set_fast(False)
    return fig


def run_shape_cells(sc):
    """Every launch shape of every kind on one tree, in exact and in fast mode; whole frames are run_whole_frame_cells'.  Kind (j) --
    sigma_thresh = -0.25: the node words, below the second grid on the P2 / P3 trees -- takes every shape of (a), (d), (f), (g) again."""
    t = sc.t
    for pose in (1, 2):   # the batch's other frames meet the frame condition too
        s = shares(t.frame(pose)["rgba"])
        assert min(s) >= 0.05, f"{t.name} pose {pose}: shares {s}"
    x0, y0, w, h = TILE
    for fast in (False, True):
        sc.set_fast(fast)
        try:
            for thresh in (None, THRESH_NEG):
                neg = thresh is not None
                # kinds (a) / (b) and (c); (j): the colour frame
                for depth_image in ((False,) if neg else (False, True)):
                    check = sc.frame_check(depth_image)      # only the frames MODE 4 renders (SH rows, fast mode, colour) may differ from the oracle
                    kw = dict(depth_image=depth_image, thresh=thresh)
                    tag = f"depth={depth_image} fast={fast} sigma_thresh={thresh}"
                    check(sc.frame(tile=TILE, **kw), t.frame(tile=TILE, **kw), "sub-rectangle " + tag)
                    for period in (0, 2):
                        check(sc.frame(part=period, **kw), t.frame(**kw), f"partition, root_period {period}, " + tag)
                    if not neg:
                        want3 = {k: np.stack([t.frame(p, **kw)[k] for p in range(3)]) for k in FRAME_KEYS}
                        check(sc.batch(depth_image), want3, "batch of three " + tag)
                    check(sc.frame(onscr=True, **kw), t.frame(onscr=True, **kw), "on-screen inputs " + tag)
                    both = sc.frame(**kw)
                    check(both, t.frame(**kw), "float + RGBA8 " + tag)
                    only_float = sc.frame(want8=False, **kw)
                    assert set(only_float) == {"rgba"} and same(only_float["rgba"], both["rgba"]), f"{t.name}: float output alone " + tag
                # kinds (d), (e): exact in either mode; (j): (d)
                for e in ((False,) if neg else (False, True)):
                    kw = dict(depth_image=e, thresh=thresh)
                    tag = f"trackers render_depth={e} fast={fast} sigma_thresh={thresh}"
                    sc.equal(sc.tracked(tile=TILE, **kw), t.frame(tracked=True, tile=TILE, **kw), "sub-rectangle " + tag, TRACK_KEYS)
                    for period in (0, 2):
                        sc.equal(sc.tracked(part=period, **kw), t.frame(tracked=True, **kw), f"partition, root_period {period}, " + tag, TRACK_KEYS)
                    sc.equal(sc.tracked(onscr=True, **kw), t.frame(tracked=True, onscr=True, **kw), "on-screen inputs " + tag, TRACK_KEYS)
                # kind (f): a sub-rectangle and the depth attachment.  The oracle emits whole frames only: the rectangle's rows are cut out of
                # its frame, and the expected visit marks are those of the oracle's TRACKED frame of the rectangle -- the sample march takes
                # the steps of the frame's march, which check_conditions asserts on the whole frame (marks of the two oracle marches equal)
                whole = t.samples(thresh)
                crop = {k: whole[k].reshape((H, W) + whole[k].shape[1:])[y0:y0 + h, x0:x0 + w].reshape((w * h,) + whole[k].shape[1:]) for k in SAMPLE_KEYS[:-1]}
                crop["visited"] = t.frame(tracked=True, thresh=thresh, tile=TILE)["visited"]
                tag = f"fast={fast} sigma_thresh={thresh}"
                sc.equal(sc.samples(thresh, tile=TILE), crop, "sample emission, sub-rectangle " + tag, SAMPLE_KEYS)
                sc.equal(sc.samples(thresh, onscr=True), t.samples(thresh, onscr=True), "sample emission, depth attachment " + tag, SAMPLE_KEYS)
                # kinds (g), (h); (j): (g)
                for depth_image in ((False,) if neg else (False, True)):
                    sc.equal(sc.rays(depth_image, thresh, onscr=True), t.rays(depth_image, thresh, onscr=True),
                             f"ray list, limits and pixels under the volume, depth={depth_image} " + tag, FRAME_KEYS)
        finally:
            sc.set_fast(False)


def search_random_pick(mnv, orc, cells=None, seeds=200, refines=(0.42, 0.46, 0.5, 0.55, 0.4), max_chunks=116000):
    """How RANDOM_PICK was found, for whoever changes the generator: per (format, depth) the first (refine_prob, seed number) whose tree
    stays under max_chunks and whose three poses meet the conditions on the oracle's frames.  CPU only (the lookup path is taken from
    PATHS): python tests/march_matrix.py prints the table."""
    found = {}
    for key in (cells or sorted(RANDOM_PICK)):
        b, depth = key
        kept, found[key] = RANDOM_PICK.get(key), None
        for seed in range(seeds):
            for refine in refines:
                RANDOM_PICK[key] = (refine, seed)
                try:
                    t = Truth(mnv, orc, b, depth, "random")
                    assert t.cap <= max_chunks
                    for pose in (1, 2):
                        assert min(shares(t.frame(pose)["rgba"])) >= 0.05
                    t.check_conditions(dict(grid2_level=PATHS[depth][0], brick_levels=PATHS[depth][1]))
                    found[key] = (refine, seed)
                    break
                except AssertionError:
                    pass
            if found[key]:
                break
        RANDOM_PICK[key] = kept
        print(key, found[key], flush=True)
    return found


if __name__ == "__main__":
    import sys

    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]
    import mega_nerf_viewer_amd
    import mnv_oracle

    print("RANDOM_PICK =", search_random_pick(mega_nerf_viewer_amd, mnv_oracle))
