"""The inner march loop of the plain colour kernels on inline cell words (csrc/mnv_march_accel_kernel.h, INNER: BRICK, frames, MODE 0 / 4):
the step and the colour block repeat in a loop of their own while some lane is alive and too few are idle for a refill, and the outer loop
keeps refill, flush and the end-of-tile bookkeeping.  Every frame below equals the C oracle's bit for bit; the cases are the transitions
between the two loops.

Trees.  Depth 7, `synth_random` with refine_prob 0.6, empty_prob 0.3, coef_sd 0.5, seed 11 (19542 chunks: the smallest depth that gets a
second grid with inline cell words, i.e. the BRICK kernels -- asserted through accel_info), SH1 / SH4 / SH9, sigma_max 30 and, for (b),
sigma_max 3000.  128 x 96 camera at fx 200.
  (a) far     the camera 10 world units away: the bounding box covers the middle of the image and a share of the 8 x 8 tiles misses it
              entirely (held on the host: every ray of such a tile passes the box centre farther than sqrt(3) away).  A refill of such a
              tile leaves no lane alive: the inner loop is not entered, the background pixels are written;
  (b) inside  the camera inside the bounding box of the sigma_max 3000 tree: nearly every ray stops at its first dense sample, whole tiles
              in the same iteration (held on the oracle's frame: alpha == 1 on more than 0.9 of the pixels);
  (c) rect    the sub-rectangle (13, 9, 51, 35) of (a)'s near pose: tiles with lanes that never hold a ray;
  (d) tiny    the sub-rectangle (56, 44, 16, 8): two tiles, so nearly every resident wavefront finds every queue empty at once
              (`drained` with nothing alive);
  (e) batch   three frames of different poses in one launch: refills change the camera;
  (g) fast    MODE 4 on (a)'s frame: alpha bit for bit the exact frame's, colours within 1e-6 of it.
Children on the test-hook build (this file run as a script), all at once:
  (f) `refill 16` (with MNV_QUEUES=1) and `refill 56`: MNV_REFILL_MIN = 16 / 56, the single-frame launches (a) .. (d) on the SH9 tree --
      partial refills, so the inner loop is left with lanes still alive;
  `shape`: the depth-10 random SH9 tree of march_matrix under MNV_GRID2_LEVEL=9, so that fixed lookup shape 1 (the headline instantiation)
      runs: whole frame, sub-rectangle, a two-tile rectangle, a far pose, the batch of three, and the whole frame in fast mode; the recorder
      says shape 1 after every launch.
The diagnostics instantiation (MODE 1) keeps the one-loop form, so there is no work comparison to make."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hooks
import march_matrix as mm
import rays_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FX = 128, 96, 200.0
SEED, CHUNKS = 11, 19542
BASES = (1, 4, 9)
RECT, TINY = (13, 9, 51, 35), (56, 44, 16, 8)
NEAR = mm.RANDOM_POSES[0]                                     # 3.4 world units from the centre
FAR = ((-7.4, 4.0, 5.4), (-0.74, 0.4, 0.54))                  # 10 world units, the same direction
OTHER = [mm.RANDOM_POSES[1], mm.RANDOM_POSES[2]]
INSIDE = ((0.3, -0.2, 0.25), (0.6, -0.4, 0.693))
FAST_BOUND = 1e-6


def tiles_that_miss(cam):
    """share of the 8 x 8 tiles all of whose rays pass the centre of the world cube [-1, 1]^3 farther away than its corners"""
    o, d = rays_ref.pinhole_rays(cam.c)
    o, d = o.astype(np.float64), d.astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    closest = np.linalg.norm(np.cross(o, d), axis=-1)          # distance of the ray's line from the origin
    miss = (closest > np.sqrt(3.0) + 1e-3).reshape(H // 8, 8, W // 8, 8).all(axis=(1, 3))
    return float(miss.mean())


class Case:
    """One tree: the oracle's frames (computed once), then the tree on the device."""

    def __init__(self, mnv, orc, b, sigma_max):
        self.mnv, self.b, self.name = mnv, b, f"SH{b}/d7/sigma_max {sigma_max:g}"
        self.tree = mnv.N3Tree.synth_random(depth=7, basis_dim=b, refine_prob=0.6, empty_prob=0.3, sigma_max=sigma_max, coef_sd=0.5, seed=SEED)
        self.view = self.tree.host_view()
        assert int(self.view.capacity) == CHUNKS
        self.otree = orc.tree_from_view(self.view)
        self.orc, self.opt, self.want = orc, mm.options(mnv), {}
        self.cams = {k: mnv.Camera(W, H, FX).set_pose(*p) for k, p in dict(near=NEAR, far=FAR, inside=INSIDE, other0=OTHER[0], other1=OTHER[1]).items()}

    def oracle(self, pose, tile=None):
        key = (pose, tile)
        if key not in self.want:
            self.want[key] = self.orc.render(self.otree, self.cams[pose].c, self.opt, tile, want_rgba8=True)
            assert np.isfinite(self.want[key]["rgba"]).all()
        return self.want[key]

    def to_device(self, torch):
        self.torch = torch
        self.tree.move_to_device()
        self.accel = self.tree.accel
        info = self.mnv.accel_info(self.accel)
        # second grid at level 6 with inline cell words: the BRICK kernels
        assert (info["grid2_level"], info["brick_levels"]) == (6, 1), (self.name, info)
        return self

    def render(self, poses, tile=None):
        """one launch: a frame (poses: a name) or a batch (a list of names) -> rgba, rgba8 on the host"""
        torch, batch = self.torch, not isinstance(poses, str)
        w, h = (tile[2], tile[3]) if tile else (W, H)
        shape = ((len(poses),) if batch else ()) + (h, w, 4)
        rgba = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        rgba8 = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
        if batch:
            self.mnv.render_voxels_accel_batch(self.accel, [self.cams[p] for p in poses], self.opt, rgba=rgba, rgba8=rgba8)
        else:
            self.mnv.render_voxels_accel(self.accel, self.cams[poses], self.opt, tile=tile, rgba=rgba, rgba8=rgba8)
        torch.cuda.synchronize()
        return dict(rgba=rgba.cpu().numpy(), rgba8=rgba8.cpu().numpy())

    def equal(self, got, want, what):
        for k in mm.FRAME_KEYS:
            w = want[k].reshape(got[k].shape)
            assert mm.same(got[k], w), f"{self.name} {what}: {k} differs from the oracle ({int((mm.bits(got[k]) != mm.bits(w)).sum())} of {got[k].size} words)"

    # ---- the cases; each returns what it measured on the oracle's frame

    def far(self):
        share = tiles_that_miss(self.cams["far"])
        want = self.oracle("far")
        alpha = want["rgba"].reshape(H, W, 4)[..., 3]
        assert 0.2 <= share <= 0.8, f"{self.name}: {share:.2f} of the tiles miss the bounding box"
        assert (alpha > 0).mean() > 0.05, f"{self.name}: the far frame shows nothing"
        self.equal(self.render("far"), want, "(a) far camera")
        return share

    def inside(self):
        want = self.oracle("inside")
        stopped = float((want["rgba"].reshape(H, W, 4)[..., 3] >= 1).mean())
        assert stopped > 0.9, f"{self.name}: {stopped:.2f} of the rays stop early"
        self.equal(self.render("inside"), want, "(b) camera inside")
        return stopped

    def rect(self):
        want = self.oracle("near", RECT)
        assert (want["rgba"][..., 3] > 0).any(), f"{self.name}: the sub-rectangle shows nothing"
        self.equal(self.render("near", RECT), want, "(c) sub-rectangle")

    def tiny(self):
        want = self.oracle("near", TINY)
        assert (want["rgba"][..., 3] > 0).any(), f"{self.name}: the two tiles show nothing"
        self.equal(self.render("near", TINY), want, "(d) two tiles")

    def batch(self):
        poses = ["near", "other0", "other1"]
        want = {k: np.stack([self.oracle(p)[k].reshape(H, W, 4) for p in poses]) for k in mm.FRAME_KEYS}
        for i, p in enumerate(poses):     # three different frames, each with rays that end early and rays that do not
            s = mm.shares(self.oracle(p)["rgba"])
            assert s[2] > 0.5 and s[0] + s[1] > 0.005, (self.name, p, s)
            assert i == 0 or not mm.same(want["rgba"][i], want["rgba"][0]), (self.name, p)
        self.equal(self.render(poses), want, "(e) batch of three")

    def fast(self):
        want = self.oracle("far")["rgba"].reshape(H, W, 4)
        self.mnv.accel_set_colour_math(self.accel, 1)
        try:
            got = self.render("far")["rgba"]
        finally:
            self.mnv.accel_set_colour_math(self.accel, 0)
        d = float(np.abs(got[..., :3] - want[..., :3]).max())
        print(f"\n{self.name} (g) fast colour math: colours within {d:.3g} of the exact frame", flush=True)
        assert mm.same(got[..., 3], want[..., 3]), f"{self.name} (g): alpha of the fast colour math differs from the exact frame"
        assert d <= FAST_BOUND, f"{self.name} (g): colours {d:.3g} from the exact frame (bound {FAST_BOUND})"
        return d


SIGMA = {"far": 30.0, "inside": 3000.0, "rect": 30.0, "tiny": 30.0, "batch": 30.0, "fast": 30.0}


@pytest.fixture(scope="module")
def cases(mnv, orc, torch_gpu):
    made = {}

    def get(b, sigma_max):
        if (b, sigma_max) not in made:
            made[(b, sigma_max)] = Case(mnv, orc, b, sigma_max).to_device(torch_gpu)
        return made[(b, sigma_max)]

    yield get
    made.clear()
    gc.collect()


@pytest.mark.parametrize("what", list(SIGMA))
@pytest.mark.parametrize("b", BASES, ids=[f"SH{b}" for b in BASES])
def test_frames_equal_the_oracle(cases, b, what):
    case = cases(b, SIGMA[what])
    getattr(case, what)()


# ---- the children (test-hook build)


def child_refill():
    import torch

    import mega_nerf_viewer_amd as mnv
    import mnv_oracle as orc

    done = []
    for sigma_max, names in ((30.0, ("far", "rect", "tiny")), (3000.0, ("inside",))):
        case = Case(mnv, orc, 9, sigma_max).to_device(torch)
        for name in names:
            getattr(case, name)()
            assert mnv.last_march_variant() == (9, 0, 1, 0), mnv.last_march_variant()
            done.append(name)
        del case
        gc.collect()
    print("inner-loop child ok: " + json.dumps(dict(frames=done, refill_min=os.environ.get("MNV_REFILL_MIN"), queues=os.environ.get("MNV_QUEUES"))), flush=True)


def child_shape():
    import torch

    import mega_nerf_viewer_amd as mnv
    import mnv_oracle as orc

    mm.PATHS.update({10: (9, 1)})
    t = mm.Truth(mnv, orc, 9, 10, "random")
    sc = mm.Scene(t, torch)          # asserts (grid2_level, brick_levels) == (9, 1)
    far = mnv.Camera(mm.W, mm.H, 190.0).set_pose(*FAR)
    t.cams = list(t.cams) + [far]
    shapes = []

    def one(name, got, want, check=None):
        (check or (lambda g, w, n: sc.equal(g, w, n, mm.FRAME_KEYS)))(got, want, name)
        shapes.append(mnv.last_march_shape())
        assert mnv.last_march_variant()[:1] + mnv.last_march_variant()[2:] == (9, 1, 0), mnv.last_march_variant()

    one("whole frame", sc.frame(), t.frame())
    one("sub-rectangle", sc.frame(tile=mm.TILE), t.frame(tile=mm.TILE))
    two = (24, 16, 16, 8)
    assert (t.frame(tile=two)["rgba"][..., 3] > 0).any()
    one("two tiles", sc.frame(tile=two), t.frame(tile=two))
    assert (t.frame(3)["rgba"][..., 3] > 0).any() and (t.frame(3)["rgba"][..., 3] == 0).mean() > 0.5
    one("far pose", sc.frame(pose=3), t.frame(3))
    t.cams = t.cams[:3]
    one("batch of three", sc.batch(), {k: np.stack([t.frame(p)[k] for p in range(3)]) for k in mm.FRAME_KEYS})
    sc.set_fast(True)
    try:
        got, want = sc.frame(), t.frame()
        d = float(np.abs(got["rgba"][..., :3] - want["rgba"].reshape(got["rgba"].shape)[..., :3]).max())
        print(f"fast colour math on shape 1: colours within {d:.3g} of the exact frame", flush=True)
        assert mm.same(got["rgba"][..., 3], want["rgba"].reshape(got["rgba"].shape)[..., 3]) and d <= FAST_BOUND, d
        shapes.append(mnv.last_march_shape())
        assert mnv.last_march_variant() == (9, 4, 1, 0), mnv.last_march_variant()
    finally:
        sc.set_fast(False)
    print("inner-loop child ok: " + json.dumps(dict(shapes=shapes)), flush=True)


def start_child(*args, **knobs):
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    env = hooks.hooks_env()
    for k in ("MNV_GRID2_LEVEL", "MNV_MARCH_SHAPE", "MNV_LDS_LEVEL", "MNV_BRICK_LEVELS", "MNV_STATS", "MNV_REFILL_MIN", "MNV_QUEUES"):
        env.pop(k, None)
    env.update(knobs)
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), *args], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture(scope="module")
def children(torch_gpu):
    """the three children side by side -> name: (returncode, stdout, stderr)"""
    procs = {"refill 16": start_child("refill", MNV_REFILL_MIN="16", MNV_QUEUES="1"), "refill 56": start_child("refill", MNV_REFILL_MIN="56"),
             "shape": start_child("shape", MNV_GRID2_LEVEL="9")}
    out = {}
    for name, p in procs.items():
        stdout, stderr = p.communicate(timeout=300)
        out[name] = (p.returncode, stdout, stderr)
    return out


def child_result(children, name):
    rc, stdout, stderr = children[name]
    assert rc == 0 and "inner-loop child ok: " in stdout, (stdout[-3000:], stderr[-3000:])
    res = json.loads(stdout.split("inner-loop child ok: ")[1].splitlines()[0])
    print(f"\n{name}: {res}")
    return res


@pytest.mark.parametrize("refill_min", (16, 56))
def test_partial_refills_leave_the_inner_loop_with_lanes_alive(children, refill_min):
    res = child_result(children, f"refill {refill_min}")
    assert res["frames"] == ["far", "rect", "tiny", "inside"] and res["refill_min"] == str(refill_min), res
    assert res["queues"] == ("1" if refill_min == 16 else None), res


def test_fixed_lookup_shape_1_runs_the_inner_loop(children):
    res = child_result(children, "shape")
    assert res["shapes"] == [1] * 6, res


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    child_refill() if sys.argv[1] == "refill" else child_shape()
