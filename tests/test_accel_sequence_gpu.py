"""The packed accel through prune / refresh SEQUENCES and through the branches of mnv_accel_refresh that no round of random edits takes
(csrc/mnv_accel_refresh_prune.hip).

Sequences: edit, edit, prune (visit marks), edit, prune (synthetic marks), edit, mnv_accel_rebuild, edit -- each edit one mnv_accel_refresh
with 96 splits and 64 rewritten rows around the second lookup grid -- on four trees: records from the start, records that a refresh
allocates and the next prune derives again, three levels under the grid, no second grid.  tests/test_accel_edit_model.py holds, on the
host, that every prune deletes and renumbers around the grid and every refresh after it appends and rewrites there.

Branches: changed / appended lists longer than one pass of accel_patch_plan's scan (1024, 1025, 2049 entries, a 64-item voxel at each
pass boundary), a changed list with voxels split in the same call, duplicates and one voxel first and last, refreshes without a parent
array (each whole-array choice), a path split down to depth 23 and the refusal at depth 24.

Evidence after every step:
  (a) frames -- plain, tracker + visit marks, emitted samples: the patched accel against the reference-layout kernels on the same arrays,
      bit for bit, voxel numbers and marks included (device-derived: both sides read the device arrays);
  (b) node words -- mnv_accel_sample_points at the centre of EVERY leaf against tests/extract_ref.py on the host model's arrays: voxel, depth
      and sigma bits.  It reads the accel's own node words -- every link, every leaf bit and every sigma half -- and is the host-written
      reference for them after a refresh or a renumbering.  (The depth FIELD of a leaf word is not among them: the query reports the levels
      it descended.  The march scales in-leaf coordinates by that field, so the frames of (a) hold it, for the voxels the poses cross.);
  (c) after a prune, the device child / parent / data / sample_counts arrays against the host model's (oracle/refine_oracle.py:prune_tree);
  (d) the lookup levels and brick levels mnv_accel_info reports against the model's.
And once more in ONE child process on the test-hook build with MNV_REFRESH_DEBUG=2, where every refresh and prune ends with a kernel that
holds every lookup word against a fresh derivation from the node words (device-derived: it would agree with a wrong node word -- (b) is
there for that), and the refresh reports its patch items, compared here with the model's restated totals."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # the child process of the last test: the import paths that tests/conftest.py gives the suite
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import accel_edit_model as M  # noqa: E402
import hooks  # noqa: E402
from test_accel_edit_gpu import EditedTree, frames_of, make_grid, same_frames  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 25     # seconds: three times the child run's measured 6.8 s, rounded up


class Bench:
    """One edited tree on the device with what the checks need; counts the refreshes that report on the test-hook build."""

    def __init__(self, mnv, torch, spec, reserve):
        self.mnv, self.torch = mnv, torch
        self.et = EditedTree(mnv, torch, spec, reserve)
        self.cams, self.opt, self.grid = M.poses(mnv), M.frame_options(mnv), make_grid(mnv)
        self.frames = 0
        self.reported = []     # (n_new, n_changed, items of the appended chunks, items of the changed voxels) of every refresh with a second grid

    def close(self):
        self.et.close()

    def frames_of(self, accel, pose):
        return frames_of(self.mnv, self.torch, self.et, self.cams[pose], self.opt, accel, self.grid)

    def refresh(self, old_cap, changed, parent=True):
        et = self.et
        et.upload()
        items = (M.new_chunk_items(et, old_cap), M.changed_items(et, changed) if parent else 0)
        keep = et.tv.parent
        if not parent:
            et.tv.parent = 0
        try:
            et.refresh(old_cap, changed)
        finally:
            et.tv.parent = keep
        if et.L2 > 0:
            self.reported.append((et.cap - old_cap, len(changed)) + items)

    def check(self, what):
        """(a), (b) and (d) on the accel as it is."""
        mnv, torch, et = self.mnv, self.torch, self.et
        info = mnv.accel_info(et.accel)
        assert (info["grid2_level"], info["brick_levels"]) == (et.L2, et.brick_levels), (what, info, et.L2, et.brick_levels)
        pose = self.frames % 2
        self.frames += 1
        bad = same_frames(self.frames_of(et.accel, pose), self.frames_of(None, pose))
        pts = et.leaf_probe_points()
        lv = et.leaves()
        voxel, depth, sigma = et.expected_samples(pts)
        assert np.array_equal(voxel, (lv[:, 0] * 8 + lv[:, 1]).astype(np.int32)) and np.array_equal(depth, et.depth[lv[:, 0]])   # one probe per leaf
        got = [t.cpu().numpy() for t in mnv.sample_points(et.accel, torch.from_numpy(pts).cuda())]
        wrong = {k: int((g != w).sum()) for k, g, w in (("voxel", got[0], voxel), ("depth", got[1], depth), ("sigma", got[2].view(np.uint32), sigma.view(np.uint32)))}
        assert not bad and not any(wrong.values()), (what, "(a) frames that differ from the reference layout's", bad,
                                                     "(b) leaves whose node words differ from the host model", wrong, len(lv), info)

    def prune(self, marks, old_cap):
        """mnv_prune_tree_accel with these marks on the device (the host model is pruned already); (c)."""
        mnv, torch, et = self.mnv, self.torch, self.et
        visited = torch.from_numpy(np.ascontiguousarray(marks, np.int32)).cuda()
        edit = mnv.tree_edit(et.d["child"], et.d["parent"], et.offset, et.scale, old_cap)
        new_cap, n_del = mnv.prune_tree(edit, et.d["data"], et.dd, et.d["counts"], visited, et.max_cap, accel=et.accel)
        torch.cuda.synchronize()
        assert (new_cap, n_del) == (et.cap, old_cap - et.cap)
        for k, want in (("child", et.child), ("parent", et.parent), ("data", et.data.view(np.int16)), ("counts", et.counts)):
            got = et.d[k].cpu().numpy().reshape(want.shape)
            assert got[:new_cap].tobytes() == want[:new_cap].tobytes(), ("after the prune the device array differs from the host model's", k)
        et.upload()    # (what lies behind the new capacity is cleared, as in the model)
        et.d["counts"].copy_(torch.from_numpy(et.counts))


def run_sequence_case(mnv, torch, orc, name, verbose=False):
    b = Bench(mnv, torch, M.sequence_spec(name), M.SEQUENCE_RESERVE)
    et = b.et
    try:
        assert (et.L2 > 0) == (name != "d6_sh4")
        b.check((name, "build"))
        levels = [et.brick_levels]

        def on_step(i, step, info):
            if step == "edit":
                b.refresh(info["old_cap"], info["changed"])
            elif step == "rebuild":
                mnv.accel_rebuild(et.accel, et.tv)
                et.built()
            else:
                if step == "prune_visit":   # the marks are a visit frame's: the device's own frame leaves the same ones
                    seen = b.frames_of(et.accel, 1)["visited"]      # (the device arrays and the accel are still the unpruned tree's)
                    assert np.array_equal(seen != 0, info["marks"] != 0), (name, i, "visit marks of the device frame and of the CPU oracle differ")
                b.prune(info["marks"], info["old_cap"])
            b.check((name, i, step))
            levels.append(et.brick_levels)
            if verbose:
                print(f"{name} step {i} {step}: capacity {et.cap}, {mnv.accel_info(et.accel)}", flush=True)

        M.run_sequence(name, et, orc, on_step)
        # brick levels never drop (check() held the accel's against the model's at every step)
        assert all(y >= x for step, x, y in zip(M.STEPS, levels, levels[1:]) if step != "rebuild"), levels
        if name in M.RECORDS_APPEAR_AT:
            at = M.RECORDS_APPEAR_AT[name]
            assert levels[:at + 1] == [1] * (at + 1) and levels[at + 1:] == [2] * (len(M.STEPS) - at), levels
            assert M.STEPS[at + 1] == "edit" and M.STEPS[at + 2].startswith("prune")
        fresh = mnv.accel_create(et.tv)
        try:
            cov_a, cov_b = mnv.accel_info(et.accel, coverage=True), mnv.accel_info(fresh, coverage=True)
            if cov_a["grid2_level"] == cov_b["grid2_level"]:
                assert cov_a["nonleaf_cells"] == cov_b["nonleaf_cells"] and cov_a["inline_cells"] == cov_b["inline_cells"], (cov_a, cov_b)
            for pose in (0, 1):
                assert not same_frames(b.frames_of(et.accel, pose), b.frames_of(fresh, pose))
        finally:
            mnv.accel_destroy(fresh)
        return b.reported
    finally:
        b.close()


@pytest.mark.parametrize("name", list(M.SEQUENCE_CASES))
def test_the_accel_follows_edits_prunes_and_a_rebuild_in_sequence(mnv, orc, torch_gpu, name):
    run_sequence_case(mnv, torch_gpu, orc, name)


def run_large_lists(mnv, torch):
    b = Bench(mnv, torch, M.sequence_spec("d10_sh4"), M.LARGE_RESERVE)
    et = b.et
    try:
        rng = np.random.default_rng(M.SEQUENCE_SEED)
        used = set()
        for n_new in M.LARGE_NEW:
            old_cap, items = M.large_new_edit(et, rng, n_new, used)
            b.refresh(old_cap, [])
            assert b.reported[-1] == (n_new, 0, items, 0)
            b.check(("appended chunks", n_new))
        for n_changed in M.LARGE_CHANGED:
            changed, items = M.large_changed_edit(et, rng, n_changed, used)
            b.refresh(et.cap, changed)
            assert b.reported[-1] == (0, n_changed, 0, items)
            b.check(("changed voxels", n_changed))
        return b.reported
    finally:
        b.close()


def test_lists_longer_than_one_scan_pass(mnv, torch_gpu):
    run_large_lists(mnv, torch_gpu)


def run_tolerated_list(mnv, torch):
    b = Bench(mnv, torch, M.sequence_spec("d10_sh4"), M.N_SPLIT)
    et = b.et
    try:
        old_cap, changed, _ = M.tolerated_list_edit(et, np.random.default_rng(M.SEQUENCE_SEED))
        assert changed[0] == changed[-1] and any(et.child[e] != 0 for e in changed) and len(set(changed)) < len(changed)
        b.refresh(old_cap, changed)
        b.check("split voxels, duplicates and one voxel first and last in changed_nodes")
        return b.reported
    finally:
        b.close()


def test_changed_nodes_may_name_split_voxels_and_repeat_entries(mnv, torch_gpu):
    run_tolerated_list(mnv, torch_gpu)


def run_no_parent(mnv, torch):
    b = Bench(mnv, torch, M.sequence_spec("d10_sh4"), M.N_SPLIT + 1)
    et = b.et
    try:
        rng = np.random.default_rng(M.SEQUENCE_SEED)
        old_cap, changed = et.edit_host(rng, M.N_SPLIT, M.N_CHANGE, M.wanted_depths(et.L2))     # (leaves of depth L2 + 3 come from this round)
        b.refresh(old_cap, changed)
        b.check("the round before")
        for k, changed in enumerate(M.no_parent_lists(et, rng)):
            M.apply_no_parent_list(et, rng, changed)
            b.refresh(et.cap, changed, parent=False)
            b.check(("no parent array", k, et.last["changed_depths"]))
        # appended chunks need the parent array: refused, and the accel is as it was
        before = [b.frames_of(et.accel, pose) for pose in (0, 1)]
        c, s = M.leaves_of_depth(et, et.L2)[0]
        saved = (et.cap, int(et.child[c, s]))
        nc = et.split(c, s, np.stack([et.random_row(rng, 0.0) for _ in range(8)]))
        et.upload()
        et.tv.parent, keep = 0, et.tv.parent
        try:
            with pytest.raises(mnv.MnvError) as e:
                mnv.accel_refresh(et.accel, et.tv, saved[0])
            assert e.value.code == mnv.MNV_E_INVALID
        finally:
            et.tv.parent = keep
        et.child[c, s], et.parent[nc], et.depth[nc], et.cap = saved[1], 0, 0, saved[0]     # the split is taken back
        et.data[nc] = 0
        et.upload()
        for pose in (0, 1):
            assert not same_frames(b.frames_of(et.accel, pose), before[pose])
        b.check("after the refused call")
        return b.reported
    finally:
        b.close()


def test_refreshes_without_a_parent_array_derive_the_lookup_arrays_whole(mnv, torch_gpu):
    run_no_parent(mnv, torch_gpu)


def run_depth_limit(mnv, torch):
    b = Bench(mnv, torch, M.DEEP_SPEC, M.DEEP_RESERVE)
    et = b.et
    try:
        rng = np.random.default_rng(M.SEQUENCE_SEED)
        at = M.deep_chain_start(et, rng)
        while et.depth[at[0]] < M.K_MAX_DEPTH:
            old_cap, at = M.deep_chain_step(et, rng, *at, min(M.DEEP_CHAIN, M.K_MAX_DEPTH - int(et.depth[at[0]])))
            b.refresh(old_cap, [])
            b.check(("chained splits down to depth", int(et.depth[:et.cap].max())))
        assert et.depth[:et.cap].max() == 23 and et.depth[at[0]] == 23
        old_cap, at = M.deep_chain_step(et, rng, *at, 1)     # depth 24
        et.upload()
        with pytest.raises(mnv.MnvError) as e:
            mnv.accel_refresh(et.accel, et.tv, old_cap)
        assert e.value.code == mnv.MNV_E_UNSUPPORTED
        assert mnv.accel_info(et.accel)["brick_levels"] == 0
        with pytest.raises(mnv.MnvError) as e:
            mnv.accel_rebuild(et.accel, et.tv)
        assert e.value.code == mnv.MNV_E_UNSUPPORTED
        cam = b.cams[0]
        rgba = torch.full((cam.height, cam.width, 4), float("nan"), dtype=torch.float32, device="cuda")
        mnv.render_voxels(et.tv, cam, b.opt, rgba=rgba)      # the arrays still render in the reference layout
        torch.cuda.synchronize()
        assert bool(torch.isfinite(rgba).all()) and float(rgba[..., 3].max()) > 0.0
        return b.reported
    finally:
        b.close()


def test_a_path_split_down_to_depth_23_and_the_refusal_at_24(mnv, torch_gpu):
    run_depth_limit(mnv, torch_gpu)


REFRESH_LINE = re.compile(r"\[mnv refresh\] n_new (\d+) n_changed (\d+) shallowest \d+ grid2_level \d+ patch items (-?\d+) \+ (-?\d+)")


def test_every_patched_lookup_word_on_the_test_hook_build(mnv, torch_gpu):
    """Everything above once more, in one child process on the test-hook build with MNV_REFRESH_DEBUG=2: no refresh or prune leaves a
    lookup word that differs from a fresh derivation, and every refresh patched as many items as the model counts."""
    if not os.path.exists(hooks.HOOKS_LIB):
        pytest.fail("mega-nerf-viewer_amd/testhooks/libmnv.so is missing (make builds it)")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=hooks.hooks_env(MNV_REFRESH_DEBUG="2"), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(f"child run: {time.time() - t0:.1f} s")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "[mnv verify]" not in r.stderr
    oks = [line.split()[1] for line in r.stdout.splitlines() if line.startswith("ok ")]
    assert oks == list(M.SEQUENCE_CASES) + ["large_lists", "tolerated_list", "no_parent", "depth_limit"], r.stdout[-3000:]
    want = [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("refresh ")]
    got = [tuple(int(x) for x in m_.groups()) for m_ in REFRESH_LINE.finditer(r.stderr)]
    assert len(got) == r.stderr.count("[mnv refresh]") and len(want) > 8 * 3
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]      # one line per refresh, with the model's item totals
    for n_new, n_changed in [(n, 0) for n in M.LARGE_NEW] + [(0, n) for n in M.LARGE_CHANGED]:
        assert sum((g[0], g[1]) == (n_new, n_changed) and g[2] + g[3] > 64 for g in got) == 1, (n_new, n_changed)


if __name__ == "__main__":   # the child process of the test above
    import torch

    import mega_nerf_viewer_amd as m
    import mnv_oracle

    assert os.environ.get("MNV_LIB_PATH", "").endswith(os.path.join("testhooks", "libmnv.so"))

    def report(name, reported):
        for row in reported:
            print("refresh", *row, flush=True)
        print("ok", name, flush=True)

    for case in M.SEQUENCE_CASES:
        report(case, run_sequence_case(m, torch, mnv_oracle, case, verbose=True))
    report("large_lists", run_large_lists(m, torch))
    report("tolerated_list", run_tolerated_list(m, torch))
    report("no_parent", run_no_parent(m, torch))
    report("depth_limit", run_depth_limit(m, torch))
