"""The two exponential paths of the march's per-lane SH colour block (csrc/mnv_march_accel_kernel.h, BRICK kernels, SH1 / SH4 / SH9):
behind one range test per wavefront the sample's four exponentials -- opacity and three channel sigmoids -- run either as one block of
exact_expf_core (every argument of every dense lane below 88 in magnitude) or through exact_expf.  Both must give the oracle's frame bit
for bit, on arguments inside the range, outside it, and with both kinds in one wavefront.

Scene: 128 x 96 camera at fx 300 (and a second pose for the batch), `synth_random` trees with refine_prob 0.6, empty_prob 0.3, sigma_max 30,
coef_sd 0.5, seed 11.  Four kinds per format:
  p0     the tree as generated.  Every argument is in range: a channel sum is at most max|coefficient| x sum_k max|basis_k| (asserted on the
         host, BASIS_BOUND below), the opacity argument at most sigma x delta_t x delta_scale <= 30 x (sqrt(3) / 2 + step) x 2 = 52;
  p64    the DC coefficient of all three channels overwritten with +-60000 (a finite binary16) in 1 / 64 of the leaves: at some 27 dense lanes
         per iteration about a third of the dense iterations hold an out-of-range lane, so both paths run in one launch;
  p1     ... in every leaf: no dense iteration takes the uniform path;
  sigma  sigma_max 65000, step_size 5e-2, stop_thresh 0: only the opacity argument leaves the range (att == 0 exactly, T == 0 from there on).
No NaN or infinite coefficient (those rows are another matter); the twelve reference frames are finite, checked on the oracle.

Depths.  6 is the issue's tree (4081 chunks).  A depth-6 tree has no second lookup grid (mnv_accel_build: the grid sits above depth
max_depth - 1 and below the level-5 top grid), so it renders on the node-word kernels, whose colour block is unchanged: those cases hold
the surrounding code.  7 (19542 chunks) is the smallest depth that gets a second grid with inline cell words, i.e. the BRICK kernels and the
new block under default knobs: asserted through accel_info.  Per tree: plain frame, batch of two, tracker frame (RGBA, RGBA8, both tracker
rows, visit marks), each equal to the oracle bit for bit.

Child processes on the test-hook build (this file run as a script):
  * `shape`: the depth-10 random SH9 tree of march_matrix with p = 1 / 64 under MNV_GRID2_LEVEL=9, so that fixed lookup shape 1 runs the
    block (as tests/test_march_shape_gpu.py does it): plain frame and batch equal the oracle, the recorder says shape 1;
  * `count <kind>`: the depth-7 SH9 tree under MNV_STATS=1, so the diagnostics instantiation (MODE 1) renders the plain frame -- equal to
    the oracle -- and reports how many dense iterations took each path ("[mnv exp paths]" of csrc/mnv_accel_diag.hip):
    p0: general == 0 and uniform > 0; p1: uniform == 0 (and general > 0); p64: both > 0."""
import gc
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hooks
import march_matrix as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FX = 128, 96, 300.0
SEED = 11
CHUNKS = {6: 4081, 7: 19542}
BASES = (1, 4, 9)
KINDS = ("p0", "p64", "p1", "sigma")
SHARE = {"p0": 0.0, "p64": 1.0 / 64.0, "p1": 1.0, "sigma": 0.0}
BIG = 60000.0                  # finite in binary16 (max 65504); 0.282 x 60000 is far beyond 88
# sum over the basis functions of the largest magnitude each takes on the unit sphere, rounded up (csrc/mnv_device.h sh_basis:
# 0.2821; 0.4886 |y|, |z|, |x|; 1.0925 |xy|, |yz|, |xz| <= 1.0925, 0.3154 |2zz - xx - yy| <= 0.6308, 0.5463 |xx - yy| <= 0.5463)
BASIS_BOUND = {1: 0.2821, 4: 0.2821 + 3 * 0.4886, 9: 0.2821 + 3 * 0.4886 + 3 * 1.0925 + 0.6308 + 0.5463}
EXP_PATHS = re.compile(r"^\[mnv exp paths\] uniform wave-level (\d+) lane-level (\d+), general wave-level (\d+) lane-level (\d+)$", re.M)


def make_tree(mnv, b, depth, kind):
    """-> the tree, with its DC coefficients overwritten (through host_arrays, before anything reads them)"""
    sigma_max = 65000.0 if kind == "sigma" else 30.0
    tree = mnv.N3Tree.synth_random(depth=depth, basis_dim=b, refine_prob=0.6, empty_prob=0.3, sigma_max=sigma_max, coef_sd=0.5, seed=SEED)
    return overwrite_dc(tree, b, SHARE[kind], seed=100 * depth + b)


def overwrite_dc(tree, b, share, seed):
    data, child, _parent = tree.host_arrays()
    assert data.shape[2] == 3 * b + 1
    if share > 0.0:
        rng = np.random.default_rng(seed)
        leaf = child == 0
        pick = leaf & (rng.random(child.shape) < share) if share < 1.0 else leaf
        sign = np.where(rng.random(child.shape) < 0.5, -BIG, BIG).astype(np.float16).view(np.uint16)
        assert pick.sum() > 0 and (share == 1.0 or pick.sum() < leaf.sum())
        for c in range(3):
            data[..., c * b][pick] = sign[pick]
    coef = data.view(np.float16).astype(np.float32)
    assert np.isfinite(coef).all()
    return tree


def cameras(mnv):
    return [mnv.Camera(W, H, FX), mnv.Camera(W, H, FX).set_pose(*mm.RANDOM_POSES[0])]


def options(mnv, kind):
    opt = mm.options(mnv)
    if kind == "sigma":
        opt.step_size, opt.stop_thresh = 5e-2, 0.0
    return opt


class Case:
    """One tree: the oracle's answers (computed once, on the host), then the tree on the device."""

    def __init__(self, mnv, orc, b, depth, kind):
        self.mnv, self.b, self.depth, self.kind = mnv, b, depth, kind
        self.name = f"SH{b}/d{depth}/{kind}"
        self.tree = make_tree(mnv, b, depth, kind)
        self.view = self.tree.host_view()
        self.cap = int(self.view.capacity)
        self.cams, self.opt = cameras(mnv), options(mnv, kind)
        self.counts = np.random.default_rng(7 + depth + b).integers(0, 14, size=(self.cap, 8)).astype(np.int16)
        otree = orc.tree_from_view(self.view, sample_counts=self.counts)
        self.frames = [orc.render(otree, c.c, self.opt, None, want_rgba8=True) for c in self.cams]
        visited = np.zeros(self.cap, np.int32)
        self.tracked = orc.render(otree, self.cams[0].c, self.opt, None, want_rgba8=True, want_trackers=True, visited=visited, track_visit=True)
        self.tracked["visited"] = visited

    def host_checks(self):
        data = self.tree.host_arrays()[0].view(np.float16).astype(np.float32)
        if self.kind == "p0":
            largest = float(np.abs(data[..., :-1]).max()) * BASIS_BOUND[self.b]
            assert largest < 88.0, f"{self.name}: a channel sum may reach {largest}"
            assert float(data[..., -1].max()) * (np.sqrt(3.0) / 2 + self.opt.step_size) * 2.0 < 88.0
        for i, f in enumerate(self.frames + [self.tracked]):
            assert np.isfinite(f["rgba"]).all(), f"{self.name}: the oracle's frame {i} is not finite"
        for i, f in enumerate(self.frames):   # the frames say something: background, partly covered and saturated pixels
            assert (f["rgba"][..., 3] > 0).mean() > 0.2 and int(f["counters"].hits) > 1000, (self.name, i, mm.shares(f["rgba"]))

    def to_device(self, torch):
        self.torch = torch
        self.tree.move_to_device(need_parent=True)
        self.accel = self.tree.accel
        self.info = self.mnv.accel_info(self.accel)
        return self

    def f32(self, *shape, fill=float("nan")):
        return self.torch.full(shape, fill, dtype=self.torch.float32, device="cuda")

    def u8(self, *shape):
        return self.torch.full(shape, 7, dtype=self.torch.uint8, device="cuda")

    def host(self, **tensors):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in tensors.items()}

    def equal(self, got, want, what, keys):
        for k in keys:
            w = want[k].reshape(got[k].shape)
            assert mm.same(got[k], w), f"{self.name} {what}: {k} differs from the oracle ({int((mm.bits(got[k]) != mm.bits(w)).sum())} of {got[k].size} words)"

    def plain(self):
        rgba, rgba8 = self.f32(H, W, 4), self.u8(H, W, 4)
        self.mnv.render_voxels_accel(self.accel, self.cams[0], self.opt, rgba=rgba, rgba8=rgba8)
        self.equal(self.host(rgba=rgba, rgba8=rgba8), self.frames[0], "plain frame", mm.FRAME_KEYS)

    def batch(self):
        rgba, rgba8 = self.f32(2, H, W, 4), self.u8(2, H, W, 4)
        self.mnv.render_voxels_accel_batch(self.accel, self.cams, self.opt, rgba=rgba, rgba8=rgba8)
        want = {k: np.stack([f[k].reshape(H, W, 4) for f in self.frames]) for k in mm.FRAME_KEYS}
        self.equal(self.host(rgba=rgba, rgba8=rgba8), want, "batch of two", mm.FRAME_KEYS)

    def tracker(self):
        torch = self.torch
        rgba, rgba8, split, sample = self.f32(H, W, 4), self.u8(H, W, 4), self.f32(H, W, 3, fill=-1.0), self.f32(H, W, 3, fill=-1.0)
        visited = torch.zeros(self.cap, dtype=torch.int32, device="cuda")
        counts = torch.from_numpy(self.counts).cuda()
        self.mnv.render_voxels_accel_visit(self.accel, self.cams[0], self.opt, visited, self.tree.device_view().parent, rgba=rgba, rgba8=rgba8,
                                           split_track=split, sample_track=sample, sample_counts=counts)
        self.equal(self.host(rgba=rgba, rgba8=rgba8, split=split, sample=sample, visited=visited), self.tracked, "tracker frame", mm.TRACK_KEYS)


# ---- in this process, on the shipped library


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", BASES, ids=[f"SH{b}" for b in BASES])
@pytest.mark.parametrize("depth", sorted(CHUNKS), ids=[f"d{d}" for d in sorted(CHUNKS)])
def test_frames_equal_the_oracle(mnv, orc, torch_gpu, depth, b, kind):
    case = Case(mnv, orc, b, depth, kind)
    assert case.cap == CHUNKS[depth]
    case.host_checks()
    case.to_device(torch_gpu)
    # depth 7: second grid at level 6 with inline cell words -> the BRICK kernels (the colour block with the range test); depth 6: node words
    assert (case.info["grid2_level"], case.info["brick_levels"]) == ((6, 1) if depth == 7 else (0, 0)), (case.name, case.info)
    case.plain()
    case.batch()
    case.tracker()
    del case
    gc.collect()


# ---- the children (test-hook build)


def child_shape():
    import torch

    import mega_nerf_viewer_amd as mnv
    import mnv_oracle as orc

    tree, _keep = mm.make_tree(mnv, 9, 10, "random")
    overwrite_dc(tree, 9, SHARE["p64"], seed=1009)

    class Deep(Case):
        def __init__(self):
            self.mnv, self.b, self.depth, self.kind, self.name = mnv, 9, 10, "p64", "SH9/d10/random/p64"
            self.tree, self.view, self.cap = tree, tree.host_view(), int(tree.host_view().capacity)
            self.cams, self.opt = cameras(mnv), mm.options(mnv)
            otree = orc.tree_from_view(self.view)
            self.frames = [orc.render(otree, c.c, self.opt, None, want_rgba8=True) for c in self.cams]

    case = Deep()
    for f in case.frames:
        assert np.isfinite(f["rgba"]).all() and int(f["counters"].hits) > 1000
    case.to_device(torch)
    assert (case.info["grid2_level"], case.info["brick_levels"]) == (9, 1), case.info
    case.plain()
    shapes = [mnv.last_march_shape()]
    case.batch()
    shapes.append(mnv.last_march_shape())
    assert mnv.last_march_variant() == (9, 0, 1, 0), mnv.last_march_variant()
    print("expf-paths child ok: " + json.dumps(dict(shapes=shapes, hits=[int(f["counters"].hits) for f in case.frames])), flush=True)


def child_count(kind):
    import torch

    import mega_nerf_viewer_amd as mnv
    import mnv_oracle as orc

    case = Case(mnv, orc, 9, 7, kind).to_device(torch)
    assert case.info["brick_levels"] == 1, case.info
    case.plain()
    variant = mnv.last_march_variant()
    assert variant == (9, 1, 1, 0), f"MNV_STATS=1 should launch the diagnostics instantiation on inline cell words, got {variant}"
    hits = int(case.frames[0]["counters"].hits)
    del case       # mnv_accel_destroy: the report on stderr
    gc.collect()
    print("expf-paths child ok: " + json.dumps(dict(kind=kind, hits=hits)), flush=True)


def start_child(*args, **knobs):
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    env = hooks.hooks_env()
    for k in ("MNV_GRID2_LEVEL", "MNV_MARCH_SHAPE", "MNV_LDS_LEVEL", "MNV_BRICK_LEVELS", "MNV_STATS"):
        env.pop(k, None)
    env.update(knobs)
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), *args], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def finish_child(p):
    stdout, stderr = p.communicate(timeout=300)
    assert p.returncode == 0 and "expf-paths child ok: " in stdout, (stdout[-3000:], stderr[-3000:])
    return json.loads(stdout.split("expf-paths child ok: ")[1].splitlines()[0]), stderr


def test_fixed_lookup_shape_runs_both_paths(torch_gpu):
    res, _ = finish_child(start_child("shape", MNV_GRID2_LEVEL="9"))
    assert res["shapes"] == [1, 1], res


@pytest.fixture(scope="module")
def path_counts(torch_gpu):
    """kind -> (uniform wave-level, uniform lane-level, general wave-level, general lane-level, the oracle's hits); the three children together"""
    procs = {kind: start_child("count", kind, MNV_STATS="1") for kind in ("p0", "p64", "p1")}
    out = {}
    for kind, p in procs.items():
        res, stderr = finish_child(p)
        m = EXP_PATHS.search(stderr)
        assert m, stderr[-2000:]
        out[kind] = tuple(int(x) for x in m.groups()) + (res["hits"],)
        print(f"\n{kind}: uniform {out[kind][0]} iterations / {out[kind][1]} lanes, general {out[kind][2]} / {out[kind][3]}, oracle hits {res['hits']}", flush=True)
    return out


def test_counters_every_argument_in_range(path_counts):
    u_w, u_l, g_w, g_l, hits = path_counts["p0"]
    assert (g_w, g_l) == (0, 0) and u_w > 0
    assert u_l == hits          # every dense sample of the frame, once (this tree has no candidate leaves: no brick records at depth 7)


def test_counters_every_leaf_out_of_range(path_counts):
    u_w, u_l, g_w, g_l, hits = path_counts["p1"]
    assert (u_w, u_l) == (0, 0) and g_w > 0 and g_l == hits


def test_counters_both_paths_in_one_launch(path_counts):
    u_w, u_l, g_w, g_l, hits = path_counts["p64"]
    assert u_w > 0 and g_w > 0 and u_l + g_l == hits


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    if sys.argv[1] == "shape":
        child_shape()
    else:
        child_count(sys.argv[2])
