"""Every instantiation of march_accel_kernel<BASIS, 256, MODE, BRICK, RAYS> outside the diagnostics MODE 1, and every launch shape of the
entry points that reach it, against the C oracle (tests/march_matrix.py holds the table).

Which instantiation a request gets is decided at run time (csrc/mnv_accel_capi.hip launch_accel, csrc/mnv_march_launch.h): by the row
format, by whether the accel carries inline cell words or brick records, by the sign of sigma_thresh, by the outputs asked for, by
render_depth and by the accel's colour math.  This file walks that cross product and, in a child process on the test-hook build, proves
that it did: there launch_march_kernel reports the instantiation it launches (csrc/mnv_knobs.cpp, mnv_hook_last_march_variant), every
cell holds it against the rule restated in march_matrix.predict, and the last test holds the union against march_matrix.VARIANTS (44).

Cells.  Row formats: RGBA, SH1, SH4, SH9, SH16, SH25.  Lookup paths, asserted with mnv.accel_info: P0 depth 6, no second grid; P2 depth 8,
grid2_level 7 with inline cell words; P3 depth 10 (and one depth-12 tree, SH4), grid2_level 8 with brick records; P1 = the node words
below the second grid of the P2 / P3 trees, which frames with sigma_thresh = -0.25 and the colour / tracked frames of SH16 / SH25 take.
Trees: a random tree per (format, depth 6 / 8 / 10) and a shell per (format, depth 8 / 10), 76 x 52 pixels, ray lists of 4097 rays.

  test_whole_frames[format-depth]: on each tree of that (format, depth), whole frame, one camera, float + RGBA8 output:
      (a) plain  (b) plain, fast colour math  (c) depth image  (d) split + sample trackers, counts 0..13 against max_sample_count 9, visit
      marks + parent  (e) = (d) with render_depth  (f) sample emission with trackers and visit marks (need_viewdir / appearance_embedding
      on half of the trees each)  (g) ray list  (h) ray list, depth  (i) = (c) .. (h) with the accel in fast mode, bit for bit
      (j) = (a), (d), (f), (g) with sigma_thresh = -0.25; and the reference-layout kernel (mnv.render_voxels) for (c), (d), (e).
  test_launch_shapes[format-depth-tree]: on SH4 / P2 shell, SH9 / P2 random, SH1 / P3 random, RGBA / P3 shell, SH4 / P3 depth-12 shell,
      SH16 / P2 shell (P1 for its colour and tracked frames), SH25 / P0 random, each in exact and in fast mode:
      (a) / (b), (c): sub-rectangle (13, 9, 51, 35); every rank of world 3 with 16 x 8 macro tiles, root_period 0 and 2, put back together;
                      a batch of three cameras; the on-screen inputs tmax_px + rgba8_init; float + RGBA8 and float alone
      (d), (e):       sub-rectangle; the partition (root_period 0 and 2: _visit_part); the on-screen inputs (_visit_ex)
      (f):            sub-rectangle; the depth attachment tmax_px (_visit_ex)
      (g), (h):       a limit and a pixel under every ray
      (j):            sigma_thresh = -0.25 -- the node words, below the second grid on the P2 / P3 trees (P1) -- in every shape above of
                      (a) / (b) but the batch, of (d), of (f) and of (g)

Everything is compared bit for bit (float RGBA as uint32; RGBA8, tracker rows, visit marks, sample counts, sample rows, cluster ids by
equality) but the colours of MODE 4 frames (SH rows in fast mode; RGBA rows have no MODE 4 and stay bit-identical): those stay within
2e-6 of the oracle (include/mnv.h) with alpha bit-identical, and their RGBA8 pixels must be exactly their own float colours packed as the
reference packs them (truncation of v * 255), so that a byte leaves the oracle's only where a float colour crossed a multiple of 1 / 255;
the run prints how many did.  The conditions under which a cell says anything (march_matrix.Truth.check_conditions) are asserted
on the oracle's output."""
import os
import re
import subprocess
import sys

import pytest

import hooks
import march_matrix as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "test_the_matrix_reaches_every_variant_on_the_test_hook_build"

TREES = {(b, d): (["random"] if d == 6 else ["random", "shell"]) for b in mm.FORMATS for d in mm.DEPTHS}
TREES[(4, 12)] = ["shell"]
SHAPE_TREES = [(4, 8, "shell"), (9, 8, "random"), (1, 10, "random"), (-1, 10, "shell"), (4, 12, "shell"), (16, 8, "shell"), (25, 6, "random")]

largest_fast_diff = [0.0]
fast_bytes = [0, 0]     # RGBA8 colour bytes of MODE 4 frames that differ from the oracle's, of how many


@pytest.fixture(scope="module")
def scenes(mnv, orc, torch_gpu):
    """(format, depth, tree kind) -> Scene: every tree is built, moved to the device and rendered by the oracle once per module"""
    cache = {}

    def get(b, depth, kind):
        if (b, depth, kind) not in cache:
            cache[(b, depth, kind)] = mm.Scene(mm.Truth(mnv, orc, b, depth, kind), torch_gpu)
        return cache[(b, depth, kind)]

    yield get
    torch_gpu.cuda.synchronize()
    cache.clear()


def fmt_name(b):
    return "RGBA" if b < 0 else f"SH{b}"


@pytest.mark.parametrize("b,depth", sorted(TREES), ids=[f"{fmt_name(b)}-d{d}" for b, d in sorted(TREES)])
def test_whole_frames(scenes, b, depth):
    for kind in TREES[(b, depth)]:
        sc = scenes(b, depth, kind)
        fig = mm.run_whole_frame_cells(sc)
        largest_fast_diff[0] = max(largest_fast_diff[0], sc.max_fast_diff)
        fast_bytes[0], fast_bytes[1] = fast_bytes[0] + sc.fast_bytes_off, fast_bytes[1] + sc.fast_bytes
        sc.fast_bytes_off = sc.fast_bytes = 0     # (the scene is used again by test_launch_shapes)
        print(f"\n{sc.t.name}: {sc.t.cap} chunks, {sc.info}, {fig}", flush=True)


@pytest.mark.parametrize("b,depth,kind", SHAPE_TREES, ids=[f"{fmt_name(b)}-d{d}-{k}" for b, d, k in SHAPE_TREES])
def test_launch_shapes(scenes, b, depth, kind):
    sc = scenes(b, depth, kind)
    mm.run_shape_cells(sc)
    largest_fast_diff[0] = max(largest_fast_diff[0], sc.max_fast_diff)
    fast_bytes[0], fast_bytes[1] = fast_bytes[0] + sc.fast_bytes_off, fast_bytes[1] + sc.fast_bytes
    sc.fast_bytes_off = sc.fast_bytes = 0


def test_the_matrix_reaches_every_variant_on_the_test_hook_build():
    """The tests of this file once more in a fresh process on the test-hook build, where every launch is held against the predicted
    instantiation and the union against the list."""
    if mm.RECORDING:   # this process already runs on the test-hook build (it is the child, or MNV_LIB_PATH selects that build): no further process
        return
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    me = os.path.relpath(os.path.abspath(__file__), ROOT)   # (node ids are relative to the directory pytest runs in)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", me, "--deselect", f"{me}::{CHILD}"],
                       env=hooks.hooks_env(), capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    n = len(mm.VARIANTS)
    assert f"variants covered: {n} of {n}" in r.stdout, r.stdout[-3000:]
    print("\n" + "\n".join(re.findall(r"^(?:variants covered|largest fast-colour).*$", r.stdout, flags=re.M)))


def test_every_reachable_variant_was_launched():
    """The table reaches the 44 instantiations; on the test-hook build (the child run of the whole file) the recorder saw every one."""
    assert mm.planned_variants() == set(mm.VARIANTS), sorted(mm.planned_variants() ^ set(mm.VARIANTS))
    print(f"\nlargest fast-colour difference from the oracle: {largest_fast_diff[0]:.3g} (bound {mm.FAST_BOUND:g}); "
          f"{fast_bytes[0]} of {fast_bytes[1]} RGBA8 colour bytes of MODE 4 frames differ from the oracle's")
    if mm.RECORDING:
        assert mm.recorded <= mm.predicted
        missing = sorted(set(mm.VARIANTS) - mm.recorded)
        print(f"variants covered: {len(mm.recorded & set(mm.VARIANTS))} of {len(mm.VARIANTS)}", flush=True)
        assert not missing and mm.recorded == set(mm.VARIANTS), f"never launched (run the whole file): {missing}; not in the list: {sorted(mm.recorded - set(mm.VARIANTS))}"
