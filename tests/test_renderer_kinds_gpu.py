"""Transitions between the frame kinds of ONE Renderer with frames in flight (host/volume_renderer.cpp: plan, slot, issue).  The other
suites exercise each kind alone or against the pinhole; here one renderer walks through plain, anti-aliased, orthographic,
equirectangular, grid, mesh, guided-in-flight, guided, splitting and plain frames again, three in flight, scored against a target
throughout, and every frame is collected only when its slot is about to be taken again.  Every frame equals -- bytes, score, stats --
what a renderer that never did anything else makes of it, and the slots rotate as volume_renderer.hpp promises.  No tolerance anywhere.
Only the public binding is used: the file runs unchanged against any build of the library (MNV_LIB_PATH)."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

W, H = 64, 48
IN_FLIGHT = 3
SEED = 9
M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15          # frame f of a renderer draws its sample jitter from seed + GOLDEN * f (volume_renderer.hpp: "(seed, f)")
PINHOLE = ((-2.4, 1.1, 1.6), (-0.72, 0.33, 0.48), 224.0)         # the sh4_d6 case's camera at this frame size
ORTHO = ((-1.35, 0.9, 2.25), (-0.45, 0.3, 0.75), 18.0)           # the camera plane outside the volume, 18 pixels per world unit
PANORAMA = ((0.1, -0.2, 0.05), (0.6, 0.64, 0.48), 60.0)          # from inside
N_POSES = 4

PLAIN = dict(aa=1, proj="pinhole", grid=False, mesh=None, model=False, in_flight=False, guided=False, split=False)
# (name, frames, what differs from a plain frame); from "guided_in_flight" on the model is set and stays
WALK = [
    ("plain", 4, {}),
    ("antialiased", 2, dict(aa=4)),
    ("ortho", 2, dict(proj="ortho")),
    ("equirect", 1, dict(proj="equirect")),
    ("plain_again", 2, {}),
    ("grid", 2, dict(grid=True)),
    ("mesh", 2, dict(mesh="visible")),
    ("mesh_hidden", 1, dict(mesh="hidden")),
    ("guided_in_flight", 3, dict(mesh="hidden", model=True, in_flight=True, guided=True)),
    ("guided", 1, dict(mesh="hidden", model=True, guided=True)),
    ("splitting", 3, dict(mesh="hidden", model=True, split=True)),
    ("plain_after", 3, dict(mesh="hidden", model=True)),
]
FIRST_WITH_MODEL = 8


def _cfg(i):
    return dict(PLAIN, **WALK[i][2])


def _overlaps(cfg):
    """volume_renderer.hpp, frames_in_flight / guided_in_flight: frames that leave the tree alone rotate over the slots (the tree
    stays below 3/4 of its capacity here); a guided frame whose count is wanted at once and a splitting frame run alone on slot 0."""
    return not cfg["split"] and (not cfg["guided"] or cfg["in_flight"])


def _pose(cfg, f):
    c, b, fx = {"pinhole": PINHOLE, "ortho": ORTHO, "equirect": PANORAMA}[cfg["proj"]]
    a = np.deg2rad(7.0 * (f % N_POSES))
    cs, sn = float(np.cos(a)), float(np.sin(a))
    rot = lambda v: (cs * v[0] - sn * v[1], sn * v[0] + cs * v[1], v[2])  # noqa: E731
    return rot(c), rot(b), fx


def _mesh(mnv):
    vert = np.zeros((3, 9), np.float32)
    vert[:, :3] = [(-0.8, -0.8, 0.2), (0.9, -0.6, 0.1), (0.0, 0.9, -0.2)]
    vert[:, 3:6] = (0.9, 0.4, 0.1)
    vert[:, 8] = 1.0
    return mnv.Mesh(vert, np.arange(3, dtype=np.uint32), 3)


class _Walker:
    """A Renderer on its own copy of the sh4_d6 tree (with room to grow: the tree stays below 3/4 of max_tree_capacity), scored against
    `target`, that is put into a walk's configurations one after the other."""

    def __init__(self, mnv, target, seed=SEED):
        from test_aa_gpu import _model

        self.mnv = mnv
        self.tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"])
        self.model = _model(mnv, self.tree.host_view())
        r = self.r = mnv.Renderer()
        r.resize(W, H)
        r.set(self.tree, 2 * self.tree.capacity)
        opt = mnv.RenderOptions.cli_defaults()
        bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
        C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
        r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
        for k, v in dict(grid_max_depth=3, max_depth=8, split_batch_size=512, samples_per_corner=4, max_sample_count=24, max_guided_samples=16).items():
            setattr(r.options, k, v)
        r.set_seed(seed)
        r.set_frames_in_flight(IN_FLIGHT)
        r.set_target(target, mnv.METRIC_SSIM)
        self.mesh = None
        self.has_model = self.guided_in_flight = False

    def configure(self, cfg):
        mnv, r = self.mnv, self.r
        r.set_antialiasing(cfg["aa"], mnv.AA_TENT)
        r.set_projection({"pinhole": mnv.PROJ_PINHOLE, "ortho": mnv.PROJ_ORTHO, "equirect": mnv.PROJ_EQUIRECT}[cfg["proj"]])
        r.options.show_grid = cfg["grid"]
        if cfg["mesh"] is not None and self.mesh is None:
            self.mesh = _mesh(mnv)
            r.add_mesh(self.mesh)
        if self.mesh is not None:
            self.mesh.visible = cfg["mesh"] == "visible"
        if cfg["model"] and not self.has_model:
            r.set_model(*self.model)
            self.has_model = True
        if cfg["in_flight"] != self.guided_in_flight:
            r.set_guided_in_flight(cfg["in_flight"])
            self.guided_in_flight = cfg["in_flight"]
        r.options.use_guided_sampling = cfg["guided"]
        r.options.use_splitting = cfg["split"]

    def render(self, cfg, f):
        c, b, fx = _pose(cfg, f)
        self.r.set_camera(c, b, fx=fx)
        return self.r.render()

    def collect(self, slot, guided_in_flight=False):
        f32, u8 = self.r.download_slot(slot, want_rgba8=True)
        return dict(f32=f32.tobytes(), u8=u8.tobytes(), metrics=self.r.metrics(slot), alpha=float((f32[..., 3] > 0).mean()),
                    count=self.r.slot_guided_samples(slot) if guided_in_flight else None)


def _walk(mnv, target, steps, seed=SEED, first_pose=0):
    """Walk through WALK[i] for i in steps, IN_FLIGHT frames in flight: a frame is collected only when the next frame is about to take
    its slot (or at the end).  Returns the frames in order: step, pose number, slot, stats, bytes, score."""
    w = _Walker(mnv, target, seed)
    frames, pending, slot, f = [], {}, 0, first_pose
    for i in steps:
        cfg = _cfg(i)
        w.configure(cfg)
        for _ in range(WALK[i][1]):
            slot = (slot + 1) % IN_FLIGHT if _overlaps(cfg) else 0          # the rotation the header promises
            if slot in pending:
                done = pending.pop(slot)
                done.update(w.collect(slot, done["cfg"]["in_flight"]))
            st = w.render(cfg, f)
            assert w.r.last_slot() == slot, (WALK[i][0], f, w.r.last_slot(), slot)                        # (a)
            frames.append(dict(step=i, cfg=cfg, pose=f, slot=slot, stats=st))
            pending[slot] = frames[-1]
            f += 1
    for s, fr in pending.items():
        fr.update(w.collect(s, fr["cfg"]["in_flight"]))
    return frames


def _same(a, b):
    return a["f32"] == b["f32"] and a["u8"] == b["u8"] and a["metrics"] == b["metrics"]


def test_a_walk_through_the_frame_kinds_with_frames_in_flight(mnv, torch_gpu):
    torch = torch_gpu
    target = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (H, W, 4), dtype=np.uint8)).cuda()
    frames = _walk(mnv, target, range(len(WALK)))
    assert len(frames) == sum(n for _, n, _ in WALK) and {fr["slot"] for fr in frames} == {0, 1, 2}
    for fr in frames:
        assert fr["alpha"] > 0.05 and fr["metrics"]["n_win"] > 0, (WALK[fr["step"]][0], fr["pose"])      # the volume is in view; scored

    # (b) the kinds that do not refine: a fresh renderer that renders only that kind at that pose
    for fr in frames:
        if fr["step"] >= FIRST_WITH_MODEL:
            continue
        x = _Walker(mnv, target)
        x.configure(fr["cfg"])
        st = x.render(fr["cfg"], fr["pose"])
        alone = x.collect(x.r.last_slot())
        assert _same(fr, alone) and fr["stats"] == st, (WALK[fr["step"]][0], fr["pose"])
    by_step = lambda i: [fr for fr in frames if fr["step"] == i]  # noqa: E731
    plain_at = lambda fr: next(p for p in by_step(0) if p["pose"] % N_POSES == fr["pose"] % N_POSES)  # noqa: E731
    # ... and the kinds are other frames than the plain frame of the same pose -- but for the hidden mesh, which asks for nothing
    for i in (1, 5, 6):
        assert all(fr["f32"] != plain_at(fr)["f32"] for fr in by_step(i)), WALK[i][0]
    assert by_step(2)[0]["f32"] != by_step(3)[0]["f32"]
    assert all(fr["f32"] == plain_at(fr)["f32"] for fr in by_step(4) + by_step(7))

    # (c) the refinement steps and the plain frames after them: a twin that, on its own copy of the tree, ran only those steps.  Its
    # frame numbers start at 0, so its seed is advanced by the frames the walk rendered before (seed + GOLDEN * f is what a frame uses)
    tail = [fr for fr in frames if fr["step"] >= FIRST_WITH_MODEL]
    before = len(frames) - len(tail)
    twin = _walk(mnv, target, range(FIRST_WITH_MODEL, len(WALK)), seed=(SEED + GOLDEN * before) & M64, first_pose=before)
    assert [(tw["step"], tw["pose"]) for tw in twin] == [(fr["step"], fr["pose"]) for fr in tail]
    for fr, tw in zip(tail, twin):
        assert _same(fr, tw) and fr["stats"] == tw["stats"], (WALK[fr["step"]][0], fr["pose"], fr["stats"], tw["stats"])
    split = by_step(10)
    assert sum(fr["stats"]["added"] for fr in split) > 0 and all(fr["stats"]["used_accel"] for fr in tail)
    assert [fr["stats"]["fused"] for fr in by_step(8) + by_step(9)] == [1, 1, 1, 1]
    assert all(fr["f32"] != plain_at(fr)["f32"] for fr in by_step(11))                                      # the tree has grown

    # (d) the sample count of a guided frame in flight is the count of the same frame rendered alone on slot 0
    x = _Walker(mnv, target)
    x.configure(_cfg(9))
    for fr in by_step(8):
        st = x.render(_cfg(9), fr["pose"])
        assert x.r.last_slot() == 0 and fr["stats"]["guided_samples"] == -1
        assert fr["count"] == st["guided_samples"] > 0, fr["pose"]
        assert fr["f32"] == x.collect(0)["f32"]


def test_refusals_no_other_suite_covers(mnv, torch_gpu):
    """One case per row of the renderer's refusal table that test_rays_gpu, test_aa_gpu, test_metrics_gpu, test_wireframe_gpu and
    test_mesh_gpu leave out and that the binding can reach: the code, the whole text, and the next permitted render() succeeds.  (Not
    reachable through the binding: an unknown projection / aa_filter and a target together with ranks -- the setters refuse them --
    and a tree without a parent array, which Renderer.set always uploads.)"""
    import mlp_cases
    from test_aa_gpu import _model
    from test_renderer_refine_gpu import make_grid

    def renderer(with_tree=True):
        r = mnv.Renderer()
        r.resize(W, H)
        tree = cases.make_tree(mnv, cases.CASES["sh4_d6"]["tree"]) if with_tree else None
        if with_tree:
            r.set(tree, 2 * tree.capacity)
            r.options.max_depth, r.options.split_batch_size, r.options.samples_per_corner = 8, 64, 2
        r.set_camera(PINHOLE[0], PINHOLE[1], fx=PINHOLE[2])
        return r, tree

    def refused(r, code, text):
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == code and str(e.value) == f"mnv error {code}: {text}", str(e.value)

    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)         # one rank through RCCL
    try:
        # anti-aliasing on several ranks
        r, tree = renderer()
        r.set_ranks(comm)
        r.set_antialiasing(4, mnv.AA_TENT)
        refused(r, mnv.MNV_E_INVALID, "anti-aliasing is for one rank: it cannot be combined with set_ranks")
        r.set_antialiasing(1, mnv.AA_TENT)
        assert r.render()["used_accel"]
        r.set_ranks(None)
        # several ranks without a tree
        r, _ = renderer(with_tree=False)
        r.set_ranks(comm)
        refused(r, mnv.MNV_E_IO, "several ranks need a tree with the packed accel (N == 2, RGBA or SH1/4/9/16/25 rows)")
        r.set_ranks(None)
        r.render()
        # a model whose rows are not the tree's
        r, tree = renderer()
        dd = tree.host_view().data_dim
        desc = mnv.mlp_desc(n_clusters=6, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=64, hidden_layers=2, out_dim=dd + 2)
        r.set_model(desc, mlp_cases.make_params(mnv, desc, seed=21), make_grid(mnv))
        r.render()                                          # a model alone is no obstacle
        r.options.use_splitting = True
        refused(r, mnv.MNV_E_IO, "the model's out_dim must be the tree's data_dim + 1 (cuda_renderer.cpp:255-257)")
        r.options.use_splitting = False
        assert r.render()["used_accel"]
        # depth mode while several ranks refine
        r, tree = renderer()
        r.set_model(*_model(mnv, tree.host_view()))
        r.set_ranks(comm)
        r.options.use_splitting = r.options.render_depth = True
        refused(r, mnv.MNV_E_IO, "several ranks: no depth mode while refining")
        r.options.render_depth = False
        assert r.render()["used_accel"]
        r.set_ranks(None)
        # guided sampling on several ranks with a network the fused kernel does not cover
        r, tree = renderer()
        desc = mnv.mlp_desc(n_clusters=6, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=128, hidden_layers=2, out_dim=dd + 1)
        r.set_model(desc, mlp_cases.make_params(mnv, desc, seed=21), make_grid(mnv))
        r.set_ranks(comm)
        r.options.use_guided_sampling = True
        refused(r, mnv.MNV_E_IO, "several ranks: guided sampling needs a network the fused kernel covers (64 wide, at most 64 encoded inputs)")
        r.options.use_guided_sampling = False
        assert r.render()["used_accel"]
        r.set_ranks(None)
    finally:
        comm.close()
