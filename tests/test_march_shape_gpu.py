"""The fixed lookup shapes of march_accel_kernel (csrc/mnv_march_accel_kernel.h: LDS grid at level 3, second grid at level 9 with inline
cell words, without / with brick records) against the C oracle, and the launcher's choice of them (csrc/mnv_march_launch.h).

tests/test_march_matrix_gpu.py never launches a fixed shape: its trees are small, and mnv_accel_build gives a tree a level-9 grid (two
arrays of 512 MiB) only when the packed tree itself is that large -- below it the second grid stops at level 8.  So every frame of this file
is rendered in a fresh child process on the test-hook build with MNV_GRID2_LEVEL=9 (this file run as a script; the march units are the
same object files in both libraries, only the knobs unit differs), where the recorder of csrc/mnv_knobs.cpp also says which shape a launch
took (mnv_hook_last_march_shape).  The trees and the calls are march_matrix's: Truth (tree + oracle) and Scene (the entry points).

Trees: RGBA, SH1, SH4, SH9, each random and shell, at depth 10 (no records: shape 1) and depth 12 (records: shape 2); 76 x 52 pixels.
Per tree, in exact and in fast colour mode (MODE 0 and MODE 4; RGBA rows have MODE 0 only): the whole frame, the sub-rectangle
(13, 9, 51, 35), a batch of three cameras, every rank of world 3 put back together, and three more whole frames whose cameras stress the
cell coordinates -- one inside the bounding box, one whose rays leave through the far faces (pos clamps at 1 - 1e-6: the largest
coordinate), one looking along an axis with the principal point on a pixel centre (zero direction components).
MODE 0: float RGBA as uint32 and RGBA8 equal the oracle's.  MODE 4: within the fast colour math's bound of the oracle (march_matrix
fast_close), and bit for bit the frames of the generic instantiation -- a second child with MNV_MARCH_SHAPE=0 renders them.
Generic launches (shape 0), all equal to the oracle: MNV_MARCH_SHAPE=0, MNV_LDS_LEVEL=2 and MNV_GRID2_LEVEL=8 on a depth-10 and a
depth-12 tree; a depth-8 and a depth-6 tree; a tracked frame, a depth image and a ray list on a depth-10 tree."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hooks
import march_matrix as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (-1, 1, 4, 9)
# (refine_prob, seed number) of the depth-12 random trees: the first of a search over refine_prob 0.30 / 0.33 / 0.36 and seeds
# 1200 + basis + 100 k with 5000 .. 150000 chunks, leaves at depth 12 and the three poses' shares (background, partial, stopped) >= 0.05
RANDOM12 = {-1: (0.33, 2), 1: (0.3, 13), 4: (0.3, 5), 9: (0.3, 1)}
# the second grid at level 9: inline cell words alone at depth 10 (records need two levels below the grid), records at depth 12
PATHS9 = {10: (9, 1), 12: (9, 2)}
STRESS = ("inside the bounding box", "through the far faces", "along an axis")


def fmt_name(b):
    return "RGBA" if b < 0 else f"SH{b}"


# ---- the child: everything below runs in the fresh process


def make_truth(mnv, orc, b, depth, kind):
    if not (depth == 12 and kind == "random"):
        return mm.Truth(mnv, orc, b, depth, kind)
    refine, seed = RANDOM12[b]
    table_tree = mm.make_tree

    def random12(mnv_, b_, depth_, kind_):
        fmt = dict(fmt=0) if b_ == -1 else {}
        return mnv_.N3Tree.synth_random(depth=12, basis_dim=b_, refine_prob=refine, empty_prob=0.93, sigma_max=400.0, seed=1200 + b_ + 100 * seed, **fmt), None

    mm.make_tree = random12      # (this process is the child: the table's generator has no depth-12 random tree)
    try:
        t = mm.Truth(mnv, orc, b, 12, "random")
    finally:
        mm.make_tree = table_tree
    assert 5000 <= t.cap <= 150000 and t.chunk_depth.max() == 12, (t.name, t.cap, int(t.chunk_depth.max()))
    return t


def stress_cameras(mnv):
    inside = mnv.Camera(mm.W, mm.H, 190.0).set_pose((-0.9, 0.2, 0.85), (-0.718, 0.159, 0.678))   # (sees something of every tree below)
    far = mnv.Camera(mm.W, mm.H, 190.0).set_pose((-2.5, -2.4, -2.2), (-0.61, -0.585, -0.535))
    # pixel (38, 26) has the ray direction (-1, 0, 0): column 38 and row 26 have one zero component each
    axis = mnv.Camera(mm.W, mm.H, 190.0, cx=38.5, cy=26.5).set_pose((3.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    return [inside, far, axis]


class Run:
    """One child process: the scenes it renders, the shape every launch must report, the MODE 4 frames it keeps for the parent."""

    def __init__(self, mnv, orc, torch, out_dir):
        self.mnv, self.orc, self.torch, self.out_dir = mnv, orc, torch, out_dir
        self.launches = 0

    def shape_is(self, want, what):
        got = self.mnv.last_march_shape()
        assert got == want, f"{what}: the launch took lookup shape {got}, expected {want}"
        self.launches += 1

    def scene(self, b, depth, kind, grid2_level=None):
        t = make_truth(self.mnv, self.orc, b, depth, kind)
        sc = mm.Scene(t, self.torch)      # asserts (grid2_level, brick_levels) against mm.PATHS
        if grid2_level is not None:       # records: when the tree has two levels below the second grid
            assert sc.info["grid2_level"] == grid2_level and (sc.info["brick_levels"] == 2) == (depth >= grid2_level + 2), (t.name, sc.info)
        return sc

    def colour_frames(self, sc, want_shape, stress=True, shapes=True):
        """every launch shape of the plain frame in exact and fast mode; -> the MODE 4 frames by name"""
        t, kept = sc.t, {}
        standard = list(t.cams)
        for pose in range(3):
            assert min(mm.shares(t.frame(pose)["rgba"])) >= 0.05, f"{t.name} pose {pose}: shares {mm.shares(t.frame(pose)['rgba'])}"
        for fast in (False, True):
            sc.set_fast(fast)
            mode4 = fast and t.b >= 1
            try:
                check = sc.frame_check(False)

                def one(name, got, want):
                    check(got, want, f"{name} fast={fast}")
                    self.shape_is(want_shape, f"{t.name} {name} fast={fast}")
                    if mode4:
                        kept[name + "/rgba"], kept[name + "/rgba8"] = got["rgba"], got["rgba8"]

                t.cams = standard
                one("whole frame", sc.frame(), t.frame())
                if shapes:
                    one("sub-rectangle", sc.frame(tile=mm.TILE), t.frame(tile=mm.TILE))
                    one("batch of three", sc.batch(), {k: np.stack([t.frame(p)[k] for p in range(3)]) for k in mm.FRAME_KEYS})
                    one("world 3", sc.frame(part=0), t.frame())
                if stress:
                    t.cams = standard + stress_cameras(self.mnv)
                    for i, name in enumerate(STRESS):
                        want = t.frame(3 + i)
                        assert (want["rgba"][..., 3] > 0).any(), f"{t.name} {name}: the camera sees nothing"
                        one(name, sc.frame(pose=3 + i), want)
            finally:
                t.cams = standard
                sc.set_fast(False)
        return kept

    def other_frames(self, sc):
        """frames that have no fixed shape: tracked, depth image, ray list"""
        t = sc.t
        sc.equal(sc.tracked(), t.frame(tracked=True), "trackers", mm.TRACK_KEYS)
        self.shape_is(0, f"{t.name} tracked frame")
        sc.equal(sc.frame(depth_image=True), t.frame(depth_image=True), "depth image", mm.FRAME_KEYS)
        self.shape_is(0, f"{t.name} depth image")
        sc.equal(sc.rays(), t.rays(), "ray list", mm.FRAME_KEYS)
        self.shape_is(0, f"{t.name} ray list")

    def done(self):
        self.torch.cuda.synchronize()
        gc.collect()


def child(role, b, out_dir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import torch

    import mega_nerf_viewer_amd as mnv
    import mnv_oracle as orc

    assert mm.RECORDING, "the child runs on the test-hook build (MNV_LIB_PATH)"
    assert torch.cuda.is_available()
    run, kept = Run(mnv, orc, torch, out_dir), {}
    if role in ("fixed", "generic"):
        mm.PATHS.update(PATHS9)
        for depth in (10, 12):
            for kind in ("random", "shell"):
                sc = run.scene(b, depth, kind, grid2_level=9)
                want = 0 if role == "generic" else 1 if depth == 10 else 2
                for k, v in run.colour_frames(sc, want).items():
                    kept[f"{sc.t.name}/{k}"] = v
                if role == "fixed" and depth == 10 and kind == "random":
                    run.other_frames(sc)
                del sc
                run.done()
        if role == "fixed":      # shallow trees: second grid at level 7 (depth 8), none (depth 6)
            for depth in (8, 6):
                sc = run.scene(b, depth, "random")
                run.colour_frames(sc, 0, stress=False, shapes=False)
                del sc
                run.done()
    elif role in ("lds2", "grid2_8"):
        mm.PATHS.update(PATHS9 if role == "lds2" else {})
        for bb, depth, kind in ((9, 10, "random"), (4, 12, "shell")):
            sc = run.scene(bb, depth, kind, grid2_level=9 if role == "lds2" else 8)
            run.colour_frames(sc, 0, stress=False)
            del sc
            run.done()
    else:
        raise SystemExit(f"unknown role {role}")
    if kept:
        np.savez(os.path.join(out_dir, f"{role}_{b}.npz"), **kept)
    print("march-shape child ok: " + json.dumps(dict(role=role, basis=b, launches=run.launches, kept=len(kept))), flush=True)


# ---- the parent


ENV = {"fixed": dict(MNV_GRID2_LEVEL="9"), "generic": dict(MNV_GRID2_LEVEL="9", MNV_MARCH_SHAPE="0"),
       "lds2": dict(MNV_GRID2_LEVEL="9", MNV_LDS_LEVEL="2"), "grid2_8": dict(MNV_GRID2_LEVEL="8")}


def run_child(role, b, out_dir):
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    env = hooks.hooks_env()
    for k in ("MNV_GRID2_LEVEL", "MNV_MARCH_SHAPE", "MNV_LDS_LEVEL", "MNV_BRICK_LEVELS"):
        env.pop(k, None)
    env.update(ENV[role])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), role, str(b), str(out_dir)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "march-shape child ok: " in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads(r.stdout.split("march-shape child ok: ")[1].splitlines()[0])
    print(f"\n{role} {fmt_name(b)}: {res}")
    return res


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("march_shape")


@pytest.mark.parametrize("b", FORMATS, ids=[fmt_name(b) for b in FORMATS])
def test_fixed_shapes_render_the_oracles_frames(out_dir, b):
    """shape 1 on the depth-10 trees, shape 2 on the depth-12 trees, in every launch shape and under the stress cameras; shape 0 for the
    tracked frame, the depth image, the ray list and the depth-8 / depth-6 trees"""
    res = run_child("fixed", b, out_dir)
    # per tree and colour mode 4 launch shapes (world 3: its three ranks are one check) + 3 stress cameras; the depth-10 random tree's
    # three other frames; two shallow trees, one frame per mode
    modes = 1 if b < 0 else 2
    assert res["launches"] == 4 * 7 * 2 + 3 + 2 * 2, res
    assert res["kept"] == (modes - 1) * 4 * 7 * 2, res


@pytest.mark.parametrize("b", FORMATS, ids=[fmt_name(b) for b in FORMATS])
def test_the_generic_instantiation_renders_the_same_frames(out_dir, b):
    """MNV_MARCH_SHAPE=0: shape 0 everywhere, the oracle's frames in MODE 0, and MODE 4 bit for bit what the fixed shapes gave"""
    res = run_child("generic", b, out_dir)
    assert res["launches"] == 4 * 7 * 2, res
    if b < 0:
        return      # RGBA rows have no MODE 4
    fixed_file = os.path.join(out_dir, f"fixed_{b}.npz")
    if not os.path.exists(fixed_file):
        run_child("fixed", b, out_dir)
    fixed, generic = np.load(fixed_file), np.load(os.path.join(out_dir, f"generic_{b}.npz"))
    assert sorted(fixed.files) == sorted(generic.files) and len(fixed.files) == 4 * 7 * 2
    for k in fixed.files:
        assert mm.same(fixed[k], generic[k]), f"{fmt_name(b)} {k}: the fixed shape's MODE 4 frame differs from the generic instantiation's"


@pytest.mark.parametrize("role", ["lds2", "grid2_8"])
def test_other_lookup_levels_take_the_generic_instantiation(out_dir, role):
    """MNV_LDS_LEVEL=2 / MNV_GRID2_LEVEL=8 on a depth-10 and a depth-12 tree: shape 0, the oracle's frames (second grid at level 9 / 8)"""
    res = run_child(role, 0, out_dir)
    assert res["launches"] == 2 * 4 * 2, res


if __name__ == "__main__":
    child(sys.argv[1], int(sys.argv[2]), sys.argv[3])
