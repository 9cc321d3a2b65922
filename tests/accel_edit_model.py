"""Host model of a tree that the refinement loop edits and prunes in place, and of what the packed accel must answer for it.  No GPU:
numpy arrays in the reference layout (data / child / parent / sample_counts with a reserve behind the capacity) plus the chunk depths.

  * edit_host      the splits and row rewrites of tests/test_accel_edit_gpu.py's rounds (moved here unchanged; EditedTree adds the device half);
  * prune          the arrays after mnv_prune_tree: oracle/refine_oracle.py:prune_tree on the model's arrays, chunk depths derived again;
  * visit_marks / subtree_marks   the two kinds of marks a prune gets: a visit frame's (the CPU oracle's march), and synthetic ones that
                   drop whole sub-trees under chosen voxels (closed under ancestors, root kept);
  * expected_levels    accel_build's choice of grid_level / grid2_level (csrc/mnv_accel_build.hip) restated;
  * leaf_probe_points / expected_samples   one world-space point per leaf (its centre) and the (voxel, depth, sigma) that
                   tests/extract_ref.py:sample_points answers for it -- the host-written reference for the accel's own node words;
  * patch_items    csrc/mnv_accel_refresh_prune.hip's count of patch items per affected voxel, restated.

Every edit and prune leaves a census (what it touched, by depth) in `last`: tests/test_accel_edit_model.py asserts on it that the GPU
sequences reach the states they are there for."""
import numpy as np

import cases
import extract_ref
import refine_oracle

K_MAX_GRID_LEVEL = 5     # csrc/mnv_accel.h: kMaxGridLevel
K_MAX_GRID2_LEVEL = 9    # kMaxGrid2Level
K_PATCH_CELLS = 4096     # csrc/mnv_accel_refresh_prune.hip: kPatchCells
K_MAX_DEPTH = 23         # the deepest tree an accel describes


def chunk_depths(parent, cap):
    depth = np.zeros(cap, np.int32)
    depth[0] = 1
    pc = parent[:cap] >> 3
    for _ in range(64):   # level by level, whatever order the chunks are numbered in
        todo = (depth == 0) & (depth[pc] > 0)
        todo[0] = False
        if not todo.any():
            break
        depth[todo] = depth[pc[todo]] + 1
    assert (depth > 0).all()
    return depth


def row_bytes_for(basis):
    """csrc/mnv_accel_launch.h: row_bytes_pow2 (basis -1: RGBA rows)."""
    chan = 2 if basis <= 0 else 2 * basis if basis < 16 else ((2 * basis + 3) // 4) * 4
    r = 8
    while r < 3 * chan + 2:
        r *= 2
    return r


def levels_for(max_depth, capacity, basis):
    """accel_build's (grid_level, grid2_level) for a tree of `capacity` chunks whose deepest voxel has depth max_depth: the small grid at
    min(max_depth, 5); the second grid at the deepest level <= min(max_depth - 1, 9) whose two arrays (8 bytes a cell) stay within
    max(128 MiB, twice the packed tree), and none unless it is deeper than the small grid (and at least 2)."""
    L = min(max_depth, K_MAX_GRID_LEVEL)
    L2 = min(max_depth - 1, K_MAX_GRID2_LEVEL)
    nvox = capacity * 8
    budget = max(128 << 20, 2 * (nvox * 4 + nvox * row_bytes_for(basis)))
    while L2 > L and (8 << (3 * L2)) > budget:
        L2 -= 1
    if L2 <= L or L2 < 2:
        L2 = 0
    return L, L2


def patch_items(d, L2, L2i):
    """Patch items of an affected voxel of depth d: its 8^(L2 - d) cells of the level-L2 grid in pieces of 4096, or the one cell above a
    voxel of depth L2 + 1 when the grid has inline words (L2i == L2 + 1); none below that."""
    if 1 <= d <= L2:
        return ((1 << (3 * (L2 - d))) + K_PATCH_CELLS - 1) // K_PATCH_CELLS
    return 1 if (d == L2 + 1 and L2i > L2) else 0


def sigma_bits(row):
    return int(np.asarray(row[-1:], np.float16).view(np.uint16)[0])


class EditModel:
    """Host copy of the reference-layout arrays, edited the way the refinement loop edits them."""

    def __init__(self, mnv, spec, reserve):
        self.mnv = mnv
        tree = cases.make_tree(mnv, spec)
        self.tree = tree
        v = tree.host_view()
        data, child, parent = tree.host_arrays()
        self.cap, self.dd, self.max_cap = v.capacity, v.data_dim, v.capacity + reserve
        self.offset, self.scale = [float(x) for x in v.offset], [float(x) for x in v.scale]
        self.format, self.basis_dim = int(v.format), int(v.basis_dim)
        self.data = np.zeros((self.max_cap, 8, self.dd), np.float16)
        self.child = np.zeros((self.max_cap, 8), np.int32)
        self.parent = np.zeros(self.max_cap, np.int32)
        self.data[:self.cap], self.child[:self.cap], self.parent[:self.cap] = data.view(np.float16).reshape(self.cap, 8, self.dd), child, parent
        self.depth = np.zeros(self.max_cap, np.int32)
        self.depth[:self.cap] = chunk_depths(parent, self.cap)
        self.counts = np.random.default_rng(99).integers(0, 13, (self.max_cap, 8)).astype(np.int16)
        self.last = {}
        self.built()

    # ---- what the accel of this tree holds besides the arrays

    def accel_basis(self):
        return self.basis_dim if (self.format == self.mnv.FORMAT_SH and self.basis_dim >= 0) else -1

    def expected_levels(self):
        """(grid_level, grid2_level) that accel_build chooses for the tree as it is now."""
        return levels_for(int(self.depth[:self.cap].max()), self.cap, self.accel_basis())

    def built(self):
        """An accel was built (or rebuilt) from the tree as it is: levels chosen, records where the tree has two levels below the grid."""
        self.L, self.L2 = self.expected_levels()
        self.accel_max_depth = int(self.depth[:self.cap].max())
        self.brick_levels = 0 if self.L2 == 0 else 2 if self.accel_max_depth >= self.L2 + 2 else 1

    def refreshed(self):
        """A refresh followed the last edit: the accel's max_depth only grows, records appear once it reaches L2 + 2."""
        self.accel_max_depth = max(self.accel_max_depth, int(self.depth[:self.cap].max()))
        if self.accel_max_depth > K_MAX_DEPTH:
            self.brick_levels = 0
        elif self.L2 > 0 and self.accel_max_depth >= self.L2 + 2:
            self.brick_levels = 2

    # ---- edits

    def random_row(self, rng, empty_prob):
        row = (rng.standard_normal(self.dd) * 0.7).astype(np.float16)
        row[self.dd - 1] = np.float16(0.0) if rng.random() < empty_prob else np.float16(rng.uniform(0.02, 40.0))
        return row

    def split(self, c, s, rows):
        """Leaf (c, s) becomes an inner voxel; its eight leaves are the next chunk, with `rows` [8, data_dim]."""
        assert self.child[c, s] == 0 and self.cap < self.max_cap
        nc = self.cap
        self.child[c, s] = nc - c
        self.parent[nc] = c * 8 + s
        self.child[nc] = 0
        self.depth[nc] = self.depth[c] + 1
        self.data[nc] = rows
        self.cap += 1
        return nc

    def edit_host(self, rng, n_split, n_change, depths_wanted, empty_prob=0.5):
        """n_split leaves become inner voxels with eight new leaves each (a third of them under chunks appended in this very round),
        n_change leaf rows are rewritten.  -> (old capacity, [(chunk, slot)] of the rewritten rows)."""
        old_cap = self.cap
        cand_all = np.argwhere(self.child[:self.cap] == 0)    # every leaf, in voxel order; kept current over the splits below
        for k in range(n_split):
            if self.cap >= self.max_cap:
                break
            lo = old_cap if (k % 3 == 2 and self.cap > old_cap) else 0    # chained: a leaf of a chunk that is new in this round
            first = int(np.searchsorted(cand_all[:, 0], lo))
            cand = cand_all[first:]
            want = depths_wanted[k % len(depths_wanted)]
            at = np.flatnonzero(self.depth[cand[:, 0]] == want)
            j = int(at[rng.integers(len(at))]) if len(at) else int(rng.integers(len(cand)))
            c, s = cand[j]
            if self.depth[c] >= 22:
                continue
            nc = self.cap
            self.child[c, s] = nc - c
            self.parent[nc] = c * 8 + s
            self.child[nc] = 0
            self.depth[nc] = self.depth[c] + 1
            for j8 in range(8):
                self.data[nc, j8] = self.random_row(rng, empty_prob)
            self.cap += 1
            cand_all = np.concatenate([cand_all[:first + j], cand_all[first + j + 1:], np.stack([np.full(8, nc), np.arange(8)], axis=1)])
        changed, before, after = [], [], []
        leaves = np.argwhere(self.child[:old_cap] == 0)
        for k in range(n_change):
            want = depths_wanted[k % len(depths_wanted)]
            at = leaves[self.depth[leaves[:, 0]] == want]
            pick = at if len(at) else leaves
            c, s = pick[rng.integers(len(pick))]
            if self.child[c, s] != 0:
                continue   # split in this round
            before.append(sigma_bits(self.data[c, s]))
            self.data[c, s] = self.random_row(rng, empty_prob)
            after.append(sigma_bits(self.data[c, s]))
            changed.append((c, s))
        self.note_edit(old_cap, changed, before, after)
        return old_cap, changed

    def note_edit(self, old_cap, changed, sigma_before, sigma_after):
        """Census of an edit: depths of the appended chunks and of the voxels they hang under, depths of the rewritten leaves, how
        many sigmas went to / came from zero."""
        new = np.arange(old_cap, self.cap)
        b, a = np.asarray(sigma_before, np.int64) & 0x7fff, np.asarray(sigma_after, np.int64) & 0x7fff
        self.last = dict(kind="edit", n_new=len(new), new_depths=sorted(set(self.depth[new].tolist())),
                         split_depths=sorted(set(self.depth[self.parent[new] >> 3].tolist())),
                         n_changed=len(changed), changed_depths=sorted(set(int(self.depth[c]) for c, _ in changed)),
                         to_zero=int(((b != 0) & (a == 0)).sum()), from_zero=int(((b == 0) & (a != 0)).sum()),
                         max_depth=int(self.depth[:self.cap].max()))

    # ---- prunes

    def orc_tree(self, orc):
        t = orc.OrcTree()
        t.data, t.child, t.sample_counts = self.data.ctypes.data, self.child.ctypes.data, self.counts.ctypes.data
        for i in range(3):
            t.offset[i], t.scale[i] = self.offset[i], self.scale[i]
        t.N, t.data_dim, t.format, t.basis_dim, t.capacity = 2, self.dd, self.format, self.basis_dim, self.cap
        return t

    def visit_marks(self, orc, cam, opt):
        """Marks as the loop makes them: the chunks a track_visit frame of `cam` walks through (int32 [max_cap], 0 above the capacity)."""
        marks = np.zeros(self.max_cap, np.int32)
        orc.render(self.orc_tree(orc), cam.c, opt, want_trackers=True, visited=marks, track_visit=True)
        assert marks[0] != 0 and not marks[self.cap:].any()
        return marks

    def subtree_marks(self, rng, depths, per_depth=3):
        """Synthetic marks: everything stays but the sub-trees under `per_depth` inner voxels of each of the given depths (where the
        tree has such voxels).  Closed under ancestors by construction; the root chunk is kept."""
        gone = np.zeros(self.cap, bool)
        inner = np.argwhere(self.child[:self.cap] != 0)
        for d in depths:
            at = inner[self.depth[inner[:, 0]] == d]
            if len(at) == 0:
                continue
            for c, s in at[rng.choice(len(at), size=min(per_depth, len(at)), replace=False)]:
                gone[c + self.child[c, s]] = True
        order = np.argsort(self.depth[:self.cap], kind="stable")   # parents before children
        for c in order[1:]:
            if gone[self.parent[c] >> 3]:
                gone[c] = True
        assert not gone[0]
        marks = np.zeros(self.max_cap, np.int32)
        marks[:self.cap] = ~gone
        return marks

    def prune(self, marks, orc):
        """The arrays after mnv_prune_tree with these marks (oracle/refine_oracle.py:prune_tree), chunk depths derived again.
        -> (new capacity, chunks deleted); the census is left in `last`."""
        cap, L2 = self.cap, self.L2
        visited = np.array(marks, np.int32)
        dele = visited[:cap] == 0
        assert not dele[0], "the root chunk is marked by every visit frame"
        pc = self.parent[:cap] >> 3
        assert not (dele[pc] & ~dele)[1:].any(), "marks are closed under ancestors"
        shifts = np.cumsum(dele)
        old_depth = self.depth[:cap].copy()
        inner = np.argwhere(self.child[:cap] != 0)
        inner = inner[~dele[inner[:, 0]]]
        cut = inner[dele[inner[:, 0] + self.child[inner[:, 0], inner[:, 1]]]]     # surviving voxels whose sub-tree goes: leaves now
        kept = np.flatnonzero(~dele)
        new_cap, n_del = refine_oracle.prune_tree(orc, self.child, self.parent, self.data.view(np.uint16), self.counts, visited, cap, self.max_cap)
        assert new_cap == len(kept) and n_del == int(dele.sum())
        self.cap = new_cap
        self.depth[:] = 0
        if n_del:
            self.depth[:new_cap] = old_depth[kept]
            assert np.array_equal(self.depth[:new_cap], chunk_depths(self.parent, new_cap))   # the renumbering kept every chunk's depth
        else:
            self.depth[:new_cap] = old_depth
        # (rows behind the new capacity are stale copies: nothing reads them before an edit writes them)
        self.child[new_cap:], self.parent[new_cap:] = 0, 0
        renumbered = kept[(shifts[kept] > 0)]
        self.last = dict(kind="prune", n_deleted=n_del, deleted_depths=sorted(set(old_depth[dele].tolist())),
                         cut_depths=sorted(set(old_depth[cut[:, 0]].tolist())),
                         renumbered_depths=sorted(set(old_depth[renumbered].tolist())),
                         tree_depths_before=sorted(set(old_depth.tolist())), max_depth=int(self.depth[:new_cap].max()), L2=L2)
        return new_cap, n_del

    # ---- the host-written reference for the accel's node words

    def leaves(self):
        """(chunk, slot) int64 [n, 2] of every leaf voxel, in voxel order."""
        return np.argwhere(self.child[:self.cap] == 0).astype(np.int64)

    def leaf_probe_points(self):
        """float32 [n, 3]: the centre of every leaf voxel in world coordinates (tree space u = offset + p * scale), one point per leaf
        in the order of leaves()."""
        cap = self.cap
        base = np.zeros((cap, 3), np.int64)     # integer coordinates of the voxel a chunk hangs under, at that voxel's depth
        bits = lambda s: np.stack([(s >> 2) & 1, (s >> 1) & 1, s & 1], axis=-1)   # noqa: E731
        for d in range(2, int(self.depth[:cap].max()) + 1):
            idx = np.flatnonzero(self.depth[:cap] == d)
            pv = self.parent[idx].astype(np.int64)
            base[idx] = base[pv >> 3] * 2 + bits(pv & 7)
        lv = self.leaves()
        c, s = lv[:, 0], lv[:, 1]
        xyz = base[c] * 2 + bits(s)
        u = (xyz.astype(np.float64) + 0.5) / np.exp2(self.depth[c].astype(np.float64))[:, None]
        p = (u - np.asarray(self.offset, np.float64)[None, :]) / np.asarray(self.scale, np.float64)[None, :]
        return np.ascontiguousarray(p.astype(np.float32))

    def expected_samples(self, points=None):
        """(voxel int32 [n], depth int32 [n], sigma float32 [n]) of tests/extract_ref.py:sample_points for the probe points."""
        pts = self.leaf_probe_points() if points is None else points
        return extract_ref.sample_points(self.data[:self.cap].view(np.uint16), self.child[:self.cap], self.offset, self.scale, pts)

    def probes_hit_their_own_leaves(self):
        """The probes are one per leaf and each resolves, in the host reference, to the leaf it was made for (at that leaf's depth)."""
        lv = self.leaves()
        voxel, depth, _ = self.expected_samples()
        return (len(voxel) == len(lv) and np.array_equal(voxel.astype(np.int64), lv[:, 0] * 8 + lv[:, 1])
                and np.array_equal(depth, self.depth[lv[:, 0]]) and len(np.unique(voxel)) == len(voxel))


# ---------------------------------------------------------------- the sequences of tests/test_accel_sequence_gpu.py, on the host

# name -> (depth, basis, format keywords, refine_prob): the shapes of tests/test_accel_edit_gpu.py's EDIT_CASES that reach each state
SEQUENCE_CASES = {
    "d10_sh4": (10, 4, {}, 0.40),               # records from the start: L2 = 8, depth = L2 + 2
    "d9_sh9": (9, 9, {}, 0.40),                 # no records at build; a refresh allocates them, the next prune derives them again
    "d11_rgba": (11, -1, dict(fmt=0), 0.36),    # three levels under the grid
    "d6_sh4": (6, 4, {}, 0.5),                  # no second grid: the small grid and the node words follow the edits
}
STEPS = ("edit", "edit", "prune_visit", "edit", "prune_synth", "edit", "rebuild", "edit")
SEQUENCE_SEED = 7                                                             # of the trees, and of the branch tests' edits
EDIT_SEEDS = {"d10_sh4": 1, "d9_sh9": 1, "d11_rgba": 1, "d6_sh4": 2}          # of each sequence's edits: picked on the host so that census_problems() finds nothing
N_SPLIT, N_CHANGE = 96, 64
SEQUENCE_RESERVE = N_SPLIT * sum(s == "edit" for s in STEPS)
RECORDS_APPEAR_AT = {"d9_sh9": 0}   # the step (a refresh) after which max_depth >= L2 + 2 first holds in the case whose records appear late


def tree_spec(depth, basis, fmt_kw, refine, seed):
    return dict(kind="random", depth=depth, basis_dim=basis, refine_prob=refine, empty_prob=0.9, sigma_max=40.0, seed=500 + seed + depth, **fmt_kw)


def sequence_spec(name):
    return tree_spec(*SEQUENCE_CASES[name], SEQUENCE_SEED)


def poses(mnv):
    return [mnv.Camera(168, 120, 400.0).set_pose((-2.5, 1.4, 1.8), (-0.74, 0.4, 0.54)), mnv.Camera(168, 120, 400.0).set_pose((2.2, -1.9, 1.1), (0.7, -0.6, 0.39))]


def frame_options(mnv):
    opt = mnv.RenderOptions.cli_defaults()
    opt.max_depth, opt.max_sample_count, opt.max_guided_samples = 12, 9, 16
    return opt


def wanted_depths(L2):
    return [L2 - 1, L2, L2 + 1, L2 + 2, L2 + 3, 2, L2 + 1, L2]


def run_sequence(name, model, orc, on_step=None):
    """The step list on the host model.  After each step the model holds the arrays the device must hold; on_step(i, kind, info) then
    does the device half (info: old_cap / changed of an edit, marks of a prune).  -> the census of every step."""
    rng = np.random.default_rng(EDIT_SEEDS[name])
    cams, opt = poses(model.mnv), frame_options(model.mnv)
    census = []
    for i, step in enumerate(STEPS):
        info = {}
        if step == "edit":
            old_cap, changed = model.edit_host(rng, N_SPLIT, N_CHANGE, wanted_depths(model.L2))
            info = dict(old_cap=old_cap, changed=changed)
        elif step == "prune_visit":
            info = dict(marks=model.visit_marks(orc, cams[1], opt), old_cap=model.cap)   # (the pose that sees most of every tree)
            model.prune(info["marks"], orc)
        elif step == "prune_synth":
            L2 = model.L2 if model.L2 > 0 else 3
            info = dict(marks=model.subtree_marks(rng, [L2 - 2, L2 - 1, L2, L2 + 1]), old_cap=model.cap)
            model.prune(info["marks"], orc)
        if step != "rebuild":
            census.append(dict(model.last, step=i, L2=model.L2))
        if on_step:
            on_step(i, step, info)
        if step == "edit":
            model.refreshed()
        elif step == "rebuild":
            model.built()
            census.append(dict(kind="rebuild", step=i, L2=model.L2, L=model.L, max_depth=model.accel_max_depth))
    return census


def census_problems(name, census):
    """The conditions that keep the GPU sequences from passing vacuously (every prune on a tree with a second grid deletes chunks
    around the grid, makes a shallow voxel a leaf and renumbers a chunk one level below the grid; every refresh after a prune appends and
    rewrites around the grid with sigma going both ways).  -> a list of what does not hold."""
    bad = []
    pruned = False
    for c in census:
        L2, i = c["L2"], c["step"]
        if c["kind"] == "prune":
            pruned = True
            if c["n_deleted"] == 0:
                bad.append((name, i, "nothing deleted"))
            if L2 > 0:
                for d in (L2, L2 + 1, L2 + 2):
                    if d in c["tree_depths_before"] and d not in c["deleted_depths"]:
                        bad.append((name, i, f"no chunk of depth {d} deleted"))
                if not any(d <= L2 for d in c["cut_depths"]):
                    bad.append((name, i, "no voxel of depth <= L2 became a leaf"))
                if L2 + 1 not in c["renumbered_depths"]:
                    bad.append((name, i, "no surviving chunk of depth L2 + 1 changed its number"))
        elif c["kind"] == "edit":
            if c["n_new"] == 0:
                bad.append((name, i, "nothing appended"))
            if pruned and L2 > 0:
                for d in (L2 + 1, L2 + 2):
                    if d not in c["new_depths"]:
                        bad.append((name, i, f"no chunk appended at depth {d}"))
                for d in (L2, L2 + 1, L2 + 2):
                    if d not in c["changed_depths"]:
                        bad.append((name, i, f"no leaf row of depth {d} rewritten"))
                if not (c["to_zero"] and c["from_zero"]):
                    bad.append((name, i, "sigma does not go both to and from zero"))
    return bad


# ---------------------------------------------------------------- the refresh branches no round takes, on the host

LARGE_NEW = (1024, 1025, 2049)          # appended chunks of three refreshes: one scan pass exactly, one more, two more
LARGE_CHANGED = (1025, 2049)            # changed voxels of two more
LARGE_POSITIONS = (1023, 1024, 2047)    # where a depth-2 voxel (64 patch items at L2 = 8) sits in each list: around the pass boundaries
LARGE_RESERVE = sum(LARGE_NEW)


def leaves_of_depth(model, d, below=None):
    cap = model.cap if below is None else below
    lv = np.argwhere(model.child[:cap] == 0)
    return lv[model.depth[lv[:, 0]] == d]


def large_new_edit(model, rng, n_new, used):
    """n_new appended chunks; the chunks at LARGE_POSITIONS hang under depth-2 leaves (not in `used`), the others under leaves around
    the grid, a third of them chained.  -> (old_cap, expected items of the appended chunks)."""
    old_cap, L2 = model.cap, model.L2
    wanted = wanted_depths(L2)
    for k in range(n_new):
        if k in LARGE_POSITIONS:
            at = [tuple(v) for v in leaves_of_depth(model, 2, old_cap) if tuple(v) not in used]
            c, s = at[rng.integers(len(at))]
            used.add((c, s))
        else:
            lo = old_cap if (k % 3 == 2 and model.cap > old_cap) else 0
            cand = np.argwhere(model.child[lo:model.cap] == 0)
            cand[:, 0] += lo
            want = wanted[k % len(wanted)]
            at = cand[model.depth[cand[:, 0]] == (want if want > 2 else L2 + 1)]     # (the depth-2 leaves are kept for the positions)
            pick = at if len(at) else cand[model.depth[cand[:, 0]] > 2]
            c, s = pick[rng.integers(len(pick))]
        model.split(c, s, np.stack([model.random_row(rng, 0.5) for _ in range(8)]))
    assert model.cap - old_cap == n_new
    model.note_edit(old_cap, [], [], [])
    return old_cap, new_chunk_items(model, old_cap)


def new_chunk_items(model, old_cap):
    L2, L2i = model.L2, model.L2 + 1 if model.brick_levels >= 1 else model.L2
    return sum(patch_items(int(model.depth[model.parent[c] >> 3]), L2, L2i) for c in range(old_cap, model.cap)) if L2 > 0 else 0


def changed_items(model, changed):
    """Items of a changed list: every entry that is still a leaf counts (a duplicate counts again), a voxel that was split counts nothing."""
    L2, L2i = model.L2, model.L2 + 1 if model.brick_levels >= 1 else model.L2
    return sum(patch_items(int(model.depth[c]), L2, L2i) for c, s in changed if model.child[c, s] == 0) if L2 > 0 else 0


def flip_sigma(model, rng, c, s):
    """Rewrite leaf row (c, s): new colours, sigma to zero if it was not, from zero if it was."""
    was = sigma_bits(model.data[c, s]) & 0x7fff
    model.data[c, s] = model.random_row(rng, 0.0)
    if was:
        model.data[c, s, -1] = np.float16(0.0)
    return was != 0


def large_changed_edit(model, rng, n_changed, used):
    """n_changed distinct rewritten leaves (sigma flipped); those at LARGE_POSITIONS are depth-2 leaves.  -> (changed, expected items)."""
    L2 = model.L2
    shallow = [tuple(v) for v in leaves_of_depth(model, 2)]
    picked = [shallow[i] for i in rng.choice(len(shallow), size=sum(p < n_changed for p in LARGE_POSITIONS), replace=False)]
    used.update(picked)
    lv = model.leaves()
    lv = lv[model.depth[lv[:, 0]] >= L2 - 1]
    rest = lv[rng.choice(len(lv), size=n_changed - len(picked), replace=False)]
    changed, it = [], iter(picked)
    rest = iter(rest)
    for k in range(n_changed):
        c, s = next(it) if k in LARGE_POSITIONS else next(rest)
        changed.append((int(c), int(s)))
    before = [sigma_bits(model.data[c, s]) for c, s in changed]
    for c, s in changed:
        flip_sigma(model, rng, c, s)
    model.note_edit(model.cap, changed, before, [sigma_bits(model.data[c, s]) for c, s in changed])
    return changed, changed_items(model, changed)


def tolerated_list_edit(model, rng, n_list=300, n_split_entries=24, n_twice=30):
    """One round of 96 splits, then a changed list of n_list entries that holds voxels split in this very round (their rows rewritten too,
    with sigma != 0: a kernel that did not skip them would put a leaf word over the link), n_twice entries twice, and one voxel first and last.
    -> (old_cap, changed, expected items of the changed list)."""
    old_cap, _ = model.edit_host(rng, N_SPLIT, 0, wanted_depths(model.L2))
    pv = model.parent[old_cap:model.cap]
    split_now = [(int(v >> 3), int(v & 7)) for v in pv if (v >> 3) < old_cap][:n_split_entries]
    assert len(split_now) == n_split_entries
    lv = np.argwhere(model.child[:old_cap] == 0)
    lv = lv[model.depth[lv[:, 0]] >= max(model.L2 - 1, 2)]
    n_single = n_list - 2 - n_split_entries - 2 * n_twice
    picks = [(int(c), int(s)) for c, s in lv[rng.choice(len(lv), size=1 + n_twice + n_single, replace=False)]]
    ends, twice, single = picks[0], picks[1:1 + n_twice], picks[1 + n_twice:]
    middle = split_now + twice + twice + single
    middle = [middle[i] for i in rng.permutation(len(middle))]
    changed = [ends] + middle + [ends]
    assert len(changed) == n_list
    distinct = sorted(set(changed))
    before = [sigma_bits(model.data[c, s]) for c, s in distinct]
    for c, s in distinct:
        if model.child[c, s] != 0:
            model.data[c, s] = model.random_row(rng, 0.0)      # a link now: the row is rewritten all the same, with sigma != 0
        else:
            flip_sigma(model, rng, c, s)
    model.note_edit(old_cap, distinct, before, [sigma_bits(model.data[c, s]) for c, s in distinct])
    model.last.update(split_entries=len(split_now), twice=n_twice, first_is_last=changed[0] == changed[-1])
    return old_cap, changed, changed_items(model, changed)


def pick_mixed(model, rng, cand, n):
    """n of the leaves `cand`, half of them (where there are that many) with sigma != 0: flipping them sends sigma both ways."""
    dense = (model.data[cand[:, 0], cand[:, 1], -1].view(np.uint16) & 0x7fff) != 0
    a, b = cand[dense], cand[~dense]
    na = min(len(a), n // 2)
    assert na >= 1 and len(b) >= n - na, (len(a), len(b), n)
    return np.concatenate([a[rng.choice(len(a), size=na, replace=False)], b[rng.choice(len(b), size=n - na, replace=False)]])


def no_parent_lists(model, rng):
    """Four changed lists for refreshes without a parent array: the shallowest rewritten leaf is of depth <= L2 (grid2, inline words and
    records derived again whole), exactly L2 + 1 (inline words and records), exactly L2 + 2 (records only), deeper (nothing to derive)."""
    L2 = model.L2
    out = []
    for lo in (L2 - 1, L2 + 1, L2 + 2, L2 + 3):
        lv = model.leaves()
        first = lv[model.depth[lv[:, 0]] == lo]
        more = lv[model.depth[lv[:, 0]] >= max(lo, L2 + 1)]
        picks = np.concatenate([pick_mixed(model, rng, first, 2), pick_mixed(model, rng, more, 12)])
        out.append(sorted(set((int(c), int(s)) for c, s in picks)))
    return out


def apply_no_parent_list(model, rng, changed):
    before = [sigma_bits(model.data[c, s]) for c, s in changed]
    for c, s in changed:
        flip_sigma(model, rng, c, s)
    model.note_edit(model.cap, changed, before, [sigma_bits(model.data[c, s]) for c, s in changed])


DEEP_SPEC = dict(kind="random", depth=6, basis_dim=-1, fmt=0, refine_prob=0.5, empty_prob=0.9, sigma_max=40.0, seed=531)
DEEP_CHAIN = 8          # chained chunks per refresh
DEEP_RESERVE = 24


def deep_chain_start(model, rng):
    """A depth-6 leaf away from the cube's faces (the point query clamps tree-space coordinates at 1 - 1e-6)."""
    pts = model.leaf_probe_points()
    lv = model.leaves()
    inside = (np.abs(pts) < 0.75).all(axis=1) & (model.depth[lv[:, 0]] == 6) & (np.asarray(model.data[lv[:, 0], lv[:, 1], -1], np.float32) > 0)
    at = lv[inside]
    c, s = at[rng.integers(len(at))]
    return int(c), int(s)


def deep_chain_step(model, rng, c, s, n):
    """Split (c, s), then a leaf of the new chunk, and so on: n chained chunks.  -> (old_cap, the leaf to go on from)."""
    old_cap = model.cap
    for _ in range(n):
        nc = model.split(c, s, np.stack([model.random_row(rng, 0.3) for _ in range(8)]))
        c, s = nc, int(rng.integers(8))
    model.note_edit(old_cap, [], [], [])
    return old_cap, (c, s)
