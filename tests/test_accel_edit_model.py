"""The host model of an edited, pruned tree (tests/accel_edit_model.py) and the census of the sequences that
tests/test_accel_sequence_gpu.py runs on the device: what every prune deletes and renumbers, what every refresh appends and rewrites, by
depth around the second lookup grid.  These are conditions, not measurements -- they keep the GPU tests from passing vacuously; the seeds
were picked here so that they hold.  No GPU."""
import numpy as np
import pytest

import accel_edit_model as M
import extract_ref
import refine_oracle


@pytest.fixture(scope="module")
def sequences(mnv, orc):
    """name -> (census, model after the last step) of every sequence, run once on the host."""
    out = {}
    for name in M.SEQUENCE_CASES:
        model = M.EditModel(mnv, M.sequence_spec(name), M.SEQUENCE_RESERVE)
        probes_ok = []

        def on_step(i, kind, info, model=model, probes_ok=probes_ok):
            probes_ok.append(model.probes_hit_their_own_leaves())

        first_ok = model.probes_hit_their_own_leaves()
        levels = (model.L, model.L2, model.brick_levels)
        out[name] = (M.run_sequence(name, model, orc, on_step), model, [first_ok] + probes_ok, levels)
    return out


@pytest.mark.parametrize("name", list(M.SEQUENCE_CASES))
def test_every_sequence_reaches_the_states_it_is_there_for(sequences, name):
    census, model, _, levels = sequences[name]
    for c in census:
        print(name, {k: v for k, v in c.items() if k != "tree_depths_before"})
    assert not M.census_problems(name, census)
    assert [c["kind"] for c in census if c["kind"] != "rebuild"] == [s.split("_")[0] for s in M.STEPS if s != "rebuild"]
    rebuilt, = [c for c in census if c["kind"] == "rebuild"]
    assert rebuilt["L"] == 5 and rebuilt["L2"] == min(rebuilt["max_depth"] - 1, 8)      # (the shallow tree has a second grid from here on)
    # the states of the issue's table
    depth = M.SEQUENCE_CASES[name][0]
    L, L2, bricks = levels
    if name == "d6_sh4":
        assert (L, L2, bricks) == (5, 0, 0)
    else:
        assert (L, L2) == (5, 8) and bricks == (2 if depth >= 10 else 1)
    if name == "d11_rgba":
        assert depth == L2 + 3


def test_records_appear_in_the_named_refresh_and_a_prune_follows(sequences):
    (name, step), = M.RECORDS_APPEAR_AT.items()
    census, model, _, (L, L2, bricks) = sequences[name]
    assert bricks == 1 and M.SEQUENCE_CASES[name][0] < L2 + 2                      # max_depth < L2 + 2 at build: no records
    edits = [c for c in census if c["kind"] == "edit"]
    first = next(c["step"] for c in edits if c["max_depth"] >= L2 + 2)
    assert first == step and M.STEPS[step] == "edit"
    nxt = next(c for c in census if c["kind"] == "prune" and c["step"] > step)
    assert L2 + 1 in nxt["renumbered_depths"] and nxt["max_depth"] >= L2 + 2         # the prune derives records of a tree that still has them


@pytest.mark.parametrize("name", list(M.SEQUENCE_CASES))
def test_leaf_probes_are_one_per_leaf_and_resolve_to_their_own_leaf(mnv, sequences, name):
    model = M.EditModel(mnv, M.sequence_spec(name), 0)                              # the unedited tree
    pts = model.leaf_probe_points()
    lv = model.leaves()
    assert pts.shape == (len(lv), 3) and pts.dtype == np.float32
    data, child, _ = model.tree.host_arrays()
    voxel, depth, sigma = extract_ref.sample_points(data, child, model.offset, model.scale, pts)
    assert np.array_equal(voxel, (lv[:, 0] * 8 + lv[:, 1]).astype(np.int32)) and len(np.unique(voxel)) == len(lv)
    assert np.array_equal(depth, model.depth[lv[:, 0]])
    assert np.array_equal(sigma.view(np.uint32), np.asarray(model.data[lv[:, 0], lv[:, 1], -1], np.float32).view(np.uint32))
    assert all(sequences[name][2]), "after every step of the sequence too"


def test_the_models_pruned_arrays_are_the_oracles_byte_for_byte(mnv, orc):
    name = "d10_sh4"
    model = M.EditModel(mnv, M.sequence_spec(name), 64)
    rng = np.random.default_rng(3)
    model.edit_host(rng, 40, 10, M.wanted_depths(model.L2))
    for marks in (model.visit_marks(orc, M.poses(mnv)[0], M.frame_options(mnv)), None):
        if marks is None:
            marks = model.subtree_marks(rng, [model.L2 - 1, model.L2, model.L2 + 1])
        child, parent, data, counts = model.child.copy(), model.parent.copy(), model.data.copy().view(np.uint16), model.counts.copy()
        visited = marks.copy()
        cap = model.cap
        want_cap, want_del = refine_oracle.prune_tree(orc, child, parent, data, counts, visited, cap, model.max_cap)
        new_cap, n_del = model.prune(marks, orc)
        assert (new_cap, n_del) == (want_cap, want_del) and 0 < n_del < cap
        for got, want in ((model.child, child), (model.parent, parent), (model.data.view(np.uint16), data), (model.counts, counts)):
            assert got[:new_cap].tobytes() == want[:new_cap].tobytes()
        assert np.array_equal(model.depth[:new_cap], M.chunk_depths(model.parent, new_cap)) and not model.depth[new_cap:].any()
        # a tree again: every link names a chunk whose parent word names the link
        inner = np.argwhere(model.child[:new_cap] != 0)
        kids = inner[:, 0] + model.child[inner[:, 0], inner[:, 1]]
        assert (kids < new_cap).all() and np.array_equal(model.parent[kids], inner[:, 0] * 8 + inner[:, 1]) and len(kids) == new_cap - 1
        assert model.probes_hit_their_own_leaves()


def test_synthetic_marks_are_closed_under_ancestors_and_keep_the_root(mnv):
    model = M.EditModel(mnv, M.sequence_spec("d9_sh9"), 0)
    marks = model.subtree_marks(np.random.default_rng(1), [model.L2 - 2, model.L2 - 1, model.L2, model.L2 + 1])
    cap = model.cap
    assert marks[0] == 1 and not marks[cap:].any() and 0 < (marks[:cap] == 0).sum() < cap
    assert (marks[model.parent[1:cap] >> 3] >= marks[1:cap]).all()


def test_expected_levels_restate_the_builds_rule():
    # the budget rule: 8 bytes a cell against max(128 MiB, twice the packed tree); the small grid at 5, the second at 9 at most
    assert M.levels_for(4, 100, 4) == (4, 0)
    assert M.levels_for(6, 1000, 4) == (5, 0)                 # min(max_depth - 1, 9) = 5 is not deeper than the small grid
    assert M.levels_for(7, 1000, 4) == (5, 6)
    assert M.levels_for(9, 1000, 9) == (5, 8)
    assert M.levels_for(12, 1000, 9) == (5, 8)                # level 9 is 1 GiB: over a small tree's budget
    assert M.levels_for(12, 8_000_000, 9) == (5, 9)           # 2 * 64 M voxels * (4 + 64) bytes pay for it
    assert M.levels_for(23, 1000, -1) == (5, 8)
    assert [M.row_bytes_for(b) for b in (-1, 1, 4, 9, 16, 25)] == [8, 8, 32, 64, 128, 256]
    # patch items: 4096 cells each; one item for the cell above a voxel of depth L2 + 1 when there are inline words
    assert [M.patch_items(d, 8, 9) for d in (0, 1, 2, 4, 5, 8, 9, 10)] == [0, 512, 64, 1, 1, 1, 1, 0]
    assert M.patch_items(9, 8, 8) == 0


@pytest.fixture(scope="module")
def large_lists(mnv):
    model = M.EditModel(mnv, M.sequence_spec("d10_sh4"), M.LARGE_RESERVE)
    rng = np.random.default_rng(M.SEQUENCE_SEED)
    used, rounds = set(), []
    for n_new in M.LARGE_NEW:
        old_cap, items = M.large_new_edit(model, rng, n_new, used)
        rounds.append(("new", n_new, old_cap, items, [int(model.depth[model.parent[old_cap + p] >> 3]) for p in M.LARGE_POSITIONS if p < n_new],
                       [M.patch_items(int(model.depth[model.parent[c] >> 3]), model.L2, model.L2 + 1) for c in range(old_cap, model.cap)]))
        model.refreshed()
    for n_changed in M.LARGE_CHANGED:
        changed, items = M.large_changed_edit(model, rng, n_changed, used)
        rounds.append(("changed", n_changed, model.cap, items, [int(model.depth[changed[p][0]]) for p in M.LARGE_POSITIONS if p < n_changed],
                       [M.patch_items(int(model.depth[c]), model.L2, model.L2 + 1) for c, _ in changed]))
        assert len(set(changed)) == n_changed
    return model, rounds


def test_the_large_lists_put_shallow_voxels_around_every_scan_pass_boundary(large_lists):
    model, rounds = large_lists
    assert model.L2 == 8 and model.brick_levels == 2
    assert [(k, n) for k, n, *_ in rounds] == [("new", 1024), ("new", 1025), ("new", 2049), ("changed", 1025), ("changed", 2049)]
    for kind, n, _, items, depths_at, per_voxel in rounds:
        print(kind, n, "patch items", items)
        assert depths_at == [2] * sum(p < n for p in M.LARGE_POSITIONS)           # depth 2: 64 items each at L2 = 8
        assert len(per_voxel) == n and sum(per_voxel) == items
        assert all(per_voxel[p] == 64 for p in M.LARGE_POSITIONS if p < n)
        # the running sum crosses every pass boundary with a carry that is neither zero nor a multiple of the shallow voxels' 64 alone
        for b in range(1024, n, 1024):
            carry = sum(per_voxel[:b])
            assert carry > 64 and carry % 64 != 0, (kind, n, b, carry)
        assert items > 64 * len(depths_at)
    assert model.probes_hit_their_own_leaves()


def test_the_tolerated_list_holds_split_voxels_duplicates_and_one_voxel_first_and_last(mnv):
    model = M.EditModel(mnv, M.sequence_spec("d10_sh4"), M.N_SPLIT)
    old_cap, changed, items = M.tolerated_list_edit(model, np.random.default_rng(M.SEQUENCE_SEED))
    assert len(changed) == 300 and changed[0] == changed[-1] and model.child[changed[0]] == 0
    split_now = [e for e in set(changed) if model.child[e] != 0]
    assert len(split_now) >= 20 and all(M.sigma_bits(model.data[e]) != 0 for e in split_now)
    twice = [e for e in set(changed) if changed.count(e) == 2 and e != changed[0]]
    assert len(twice) >= 30
    assert items == sum(M.patch_items(int(model.depth[c]), 8, 9) for c, s in changed if model.child[c, s] == 0) > 0
    assert model.last["to_zero"] and model.last["from_zero"]


def test_the_lists_without_a_parent_array_reach_each_whole_array_choice(mnv):
    model = M.EditModel(mnv, M.sequence_spec("d10_sh4"), M.N_SPLIT)
    rng = np.random.default_rng(M.SEQUENCE_SEED)
    model.edit_host(rng, M.N_SPLIT, M.N_CHANGE, M.wanted_depths(model.L2))         # (leaves of depth L2 + 3 come from this round)
    model.refreshed()
    L2 = model.L2
    shallowest = []
    for changed in M.no_parent_lists(model, rng):
        M.apply_no_parent_list(model, rng, changed)
        assert all(model.child[e] == 0 for e in changed)
        assert model.last["to_zero"] + model.last["from_zero"] == len(changed) and model.last["to_zero"] and model.last["from_zero"]
        shallowest.append(model.last["changed_depths"][0])
    assert shallowest[0] <= L2 and shallowest[1:] == [L2 + 1, L2 + 2, L2 + 3]


def test_the_deep_chain_reaches_depth_23_with_probes_that_still_resolve(mnv):
    model = M.EditModel(mnv, M.DEEP_SPEC, M.DEEP_RESERVE)
    assert (model.L, model.L2, model.brick_levels) == (5, 0, 0) and model.accel_max_depth == 6
    rng = np.random.default_rng(M.SEQUENCE_SEED)
    at = M.deep_chain_start(model, rng)
    hops = []
    while model.depth[at[0]] < M.K_MAX_DEPTH:
        n = min(M.DEEP_CHAIN, M.K_MAX_DEPTH - int(model.depth[at[0]]))
        _, at = M.deep_chain_step(model, rng, *at, n)
        hops.append(n)
        model.refreshed()
        assert model.probes_hit_their_own_leaves()
    assert hops == [8, 8, 1] and model.accel_max_depth == 23 and model.brick_levels == 0
    _, at = M.deep_chain_step(model, rng, *at, 1)
    assert model.last["max_depth"] == 24
