"""The diagnostics instantiation of the march (march_accel_kernel<9, 256, 1, BRICK>, csrc/mnv_march_diag.h) and its host half
(csrc/mnv_accel_diag.hip), which tests/march_matrix.py leaves out: the frames it renders, its counters, the tile / wavefront timeline, the
footprint bitmap and the phase clocks.  MODE 1 runs on the test-hook build only (the shipped library reads no knob), so every run is a
fresh child process (tests/march_diag.py) with MNV_LIB_PATH and the knobs in its environment; this process renders the same requests on
the shipped library (MODE 0, which tests/test_march_matrix_gpu.py holds against the oracle) and asks the oracle for its counters.

Scene (tests/march_diag.py): the depth-10 random SH9 tree of march_matrix -- second lookup grid at level 8, brick records -- a 64 x 64
frame and a 64 x 40 rectangle at y0 = 13, rendered on one accel; the counters are the two launches' sums.

Counters against the oracle's (orc_counters: steps, hits), measured on the kernel as it was before the instruments moved into
MarchProbe: lane-level march_step == steps and lane-level dense == hits on the node-word run (MNV_BRICK_LEVELS=0); on the brick run
march_step == steps and dense >= hits (dense also counts the candidates: leaves with sigma != 0 that turn out to be below the threshold).
Figures of this scene, the same before and after the move: oracle steps 74876, hits 4107; march_step 74876 and dense 4107 on both runs
(no candidate of this tree is below the threshold), node_load 13401 on node words and 8507 with bricks."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hooks
import march_diag as md
import march_matrix as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = {   # name -> knobs of the child
    "bricks": dict(MNV_STATS="1"),
    "nodes": dict(MNV_STATS="1", MNV_BRICK_LEVELS="0"),
    "clocks": dict(MNV_STATS="2", MNV_TIMELINE="{dir}/timeline.bin", MNV_FOOTPRINT="{dir}/footprint.json"),
}
STAT = re.compile(r"^\[mnv stats\] (\w+)\s+wave-level (\d+) lane-level (\d+) ", re.M)
PHASES = re.compile(r"^\[mnv phases\] .*lookup ([\d.]+), step arithmetic \+ opacity ([\d.]+), row wait ([\d.]+), colour arithmetic ([\d.]+), "
                    r"other \(refill, ray set-up, flush, loop\) (-?[\d.]+); wave-steps (\d+)$", re.M)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, torch_gpu):
    """name -> dict(dir, stderr, info, frame, tile, stats): the three children, started together"""
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    procs = {}
    for name, knobs in RUNS.items():
        d = str(tmp_path_factory.mktemp(name))
        env = hooks.hooks_env(**{k: v.format(dir=d) for k, v in knobs.items()})
        procs[name] = (d, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "march_diag.py"), d], env=env, cwd=ROOT,
                                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, (d, p) in procs.items():
        stdout, stderr = p.communicate(timeout=300)
        assert p.returncode == 0, (name, stdout[-2000:], stderr[-3000:])
        with open(os.path.join(d, "info.json")) as f:
            info = json.load(f)
        stats = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in STAT.finditer(stderr)}
        print(f"\n{name}: {info}\n" + "\n".join(l for l in stderr.splitlines() if l.startswith("[mnv ")), flush=True)
        out[name] = dict(dir=d, stderr=stderr, info=info, stats=stats, frame=np.load(os.path.join(d, "frame.npy")), tile=np.load(os.path.join(d, "tile.npy")))
    return out


@pytest.fixture(scope="module")
def shipped(mnv, torch_gpu):
    """the two requests on the shipped library in this process (MODE 0), and the tree's capacity"""
    tree, _keep = mm.make_tree(mnv, 9, md.DEPTH, md.KIND)
    tree.move_to_device()
    got = {name: md.render(mnv, torch_gpu, tree.accel, tile)[0] for name, tile in md.REQUESTS}
    got["info"] = dict(mnv.accel_info(tree.accel), capacity=int(tree.host_view().capacity))
    return got


@pytest.fixture(scope="module")
def oracle_counters(mnv, orc):
    """(steps, hits) of the oracle over the two requests"""
    tree, _keep = mm.make_tree(mnv, 9, md.DEPTH, md.KIND)
    otree = orc.tree_from_view(tree.host_view())
    ctr = [orc.render(otree, md.camera(mnv).c, mm.options(mnv), tile)["counters"] for _, tile in md.REQUESTS]
    return sum(int(c.steps) for c in ctr), sum(int(c.hits) for c in ctr)


def test_the_scene_has_a_second_grid_and_brick_records(runs, shipped):
    assert shipped["info"]["grid2_level"] > 3 and shipped["info"]["brick_levels"] == 2, shipped["info"]
    for name in ("bricks", "clocks"):
        assert runs[name]["info"]["grid2_level"] > 3 and runs[name]["info"]["brick_levels"] == 2, runs[name]["info"]
    assert runs["nodes"]["info"]["grid2_level"] > 3 and runs["nodes"]["info"]["brick_levels"] == 0, runs["nodes"]["info"]


@pytest.mark.parametrize("name,brick", [("bricks", 1), ("nodes", 0), ("clocks", 1)])
def test_mode_1_renders_the_frames_of_mode_0(runs, shipped, name, brick):
    r = runs[name]
    assert [tuple(v) for v in r["info"]["variants"]] == [(9, 1, brick, 0)] * len(md.REQUESTS), r["info"]
    for what in ("frame", "tile"):
        assert np.isfinite(shipped[what]).all()
        assert mm.same(r[what], shipped[what]), f"{name}: the {what} of MODE 1 differs from the shipped library's " \
            f"({int((mm.bits(r[what]) != mm.bits(shipped[what])).sum())} of {shipped[what].size} words)"


def test_counters_against_the_oracle(runs, oracle_counters):
    steps, hits = oracle_counters
    nodes, bricks = runs["nodes"]["stats"], runs["bricks"]["stats"]
    print(f"\noracle: steps {steps} hits {hits}; node words: {nodes}; bricks: {bricks}", flush=True)
    assert hits > 0 and steps > hits
    assert set(nodes) == set(bricks) == {"outer_iter", "refill", "march_step", "node_load", "dense", "colour_pass"}
    assert nodes["march_step"][1] == steps
    assert nodes["dense"][1] == hits
    assert bricks["march_step"][1] == steps
    assert bricks["dense"][1] >= hits
    for st in (nodes, bricks):    # these depend on the number of wavefronts
        assert min(st["outer_iter"]) > 0 and min(st["refill"]) > 0, st


def test_timeline(runs):
    h = np.fromfile(os.path.join(runs["clocks"]["dir"], "timeline.bin"), dtype=np.uint64)
    tiles, waves, per_frame = (int(x) for x in h[:3])
    assert tiles == per_frame == (md.SIZE // 8) ** 2      # the last launch: the 64 x 64 frame
    assert waves > 0 and h.size == 3 + tiles * 4 + waves * 2
    rec = h[3:3 + tiles * 4].reshape(tiles, 4)             # t_grab, t_done, wave, iterations
    assert (rec[:, 0] > 0).all() and (rec[:, 1] >= rec[:, 0]).all()
    assert (rec[:, 3] >= 1).all() and (rec[:, 2] < waves).all()
    wv = h[3 + tiles * 4:].reshape(waves, 2)               # t_entry, t_exit
    assert (wv[:, 0] > 0).all() and (wv[:, 1] >= wv[:, 0]).all()


def test_footprint(runs):
    r = runs["clocks"]
    with open(os.path.join(r["dir"], "footprint.json")) as f:
        fp = json.load(f)
    keys = ["grid2_lines", "records_lines", "nodes_lines", "rows_lines", "grid2_vox_lines", "grid_vox_lines"]
    assert set(fp) == set(keys) | {"line_bytes"} and fp["line_bytes"] == 128, fp
    assert fp["rows_lines"] > 0 and fp["grid2_lines"] > 0, fp
    # bytes of the arrays (csrc/mnv_accel.h; the accel reserves the tree's capacity, the top grid is at most level 5)
    cap, cells2 = r["info"]["capacity"], 8 ** r["info"]["grid2_level"]
    size = dict(grid2_lines=cells2 * 4, records_lines=cap * 64, nodes_lines=cap * 8 * 4, rows_lines=cap * 8 * 64, grid2_vox_lines=cells2 * 4,
                grid_vox_lines=8 ** 5 * 4)
    for k in keys:
        assert 0 <= fp[k] <= size[k] // 128 + 1, (k, fp[k], size[k])


def test_phase_clocks(runs):
    m = PHASES.search(runs["clocks"]["stderr"])
    assert m, runs["clocks"]["stderr"][-2000:]
    shares = [float(x) for x in m.groups()[:5]]
    assert all(0.0 <= s <= 1.0 for s in shares), shares
    assert abs(sum(shares) - 1.0) <= 1e-3, shares         # (the printed digits of a sum that is 1 by construction)
    assert int(m.group(6)) > 0
    assert not PHASES.search(runs["bricks"]["stderr"])    # MNV_STATS=1 carries no clocks
