"""The C-ABI entry points that render on a packed accel (include/mnv.h), called through mnv.lib() directly: every argument check they make
answers with its return code and its mnv_last_error text before anything is launched, and the entry points of one family are the same
frame when the extras of the wider ones are NULL.  Only the public ABI is used, so the file runs unchanged against any build of the
library (MNV_LIB_PATH)."""
import ctypes as C

import numpy as np
import pytest

import mlp_cases
from test_renderer_refine_gpu import make_grid

pytestmark = pytest.mark.gpu

W, H = 20, 12  # ragged 8 x 8 tiles in both axes
MAX_G = 8
WHOLE = (0, 1, 0, 0, 0)

# parameter lists of the sixteen entry points (names of the values in Scene.args)
P = "mnv_render_voxels_accel"
S = "mnv_get_samples_from_voxels_accel"
F = "mnv_render_guided_fused"
TRACK = ["split", "sample", "counts"]
VISIT = TRACK + ["visited", "parent"]
OUT = ["rgba", "rgba8"]
HEAD = ["accel", "cam", "opt", "tile"]
SAMPLES = ["num", "samples", "dim", "clusters", "grid"]
ENTRIES = {
    P: HEAD + OUT + ["stream"],
    P + "_part": HEAD + ["part"] + OUT + ["stream"],
    P + "_ex": HEAD + ["inputs"] + OUT + ["stream"],
    P + "_batch": ["accel", "cam", "n_cams", "opt", "tile", "part"] + OUT + ["stream"],
    P + "_track": HEAD + OUT + TRACK + ["stream"],
    P + "_visit": HEAD + OUT + VISIT + ["stream"],
    P + "_visit_ex": HEAD + ["inputs"] + OUT + VISIT + ["stream"],
    P + "_visit_part": HEAD + ["part"] + OUT + VISIT + ["stream"],
    S: HEAD + TRACK + SAMPLES + ["stream"],
    S + "_visit": HEAD + VISIT + SAMPLES + ["stream"],
    S + "_visit_ex": HEAD + ["inputs"] + VISIT + SAMPLES + ["stream"],
    F: HEAD + ["mlp", "grid"] + OUT + ["counter", "stream"],
    F + "_track": HEAD + ["mlp", "grid"] + OUT + VISIT + ["counter", "stream"],
    F + "_track_ex": HEAD + ["inputs", "mlp", "grid"] + OUT + VISIT + ["counter", "stream"],
    F + "_part": HEAD + ["part", "mlp", "grid"] + OUT + ["counter", "stream"],
    F + "_track_part": HEAD + ["part", "mlp", "grid"] + OUT + VISIT + ["counter", "stream"],
    "mnv_render_rays_accel": ["accel", "origins", "dirs", "width", "height", "opt", "inputs"] + OUT + ["stream"],
}
FRAME_ENTRIES = [n for n in ENTRIES if n.startswith(P)]
SAMPLE_ENTRIES = [n for n in ENTRIES if n.startswith(S)]
FUSED_ENTRIES = [n for n in ENTRIES if n.startswith(F)]
RAYS = "mnv_render_rays_accel"


class Scene:
    def __init__(self, mnv, torch):
        self.mnv, self.torch = mnv, torch
        self.tree = mnv.N3Tree.synth_random(depth=3, basis_dim=1)
        self.tree.move_to_device(need_parent=True)
        self.view = self.tree.device_view()
        self.cam = mnv.orbit_camera(W, H, 14.0, 2.0, 35.0, 25.0)
        self.opt = mnv.RenderOptions.cli_defaults()
        self.opt.max_guided_samples = MAX_G
        self.opt.need_viewdir = 0
        self.opt.appearance_embedding = -1
        self.grid = make_grid(mnv)
        # the smallest 64-wide model shape the fused-frame suite pins (tests/test_guided_fused_gpu.py)
        desc = mnv.mlp_desc(n_clusters=2, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=64, hidden_layers=2, out_dim=self.view.data_dim + 1)
        self.mlp = mnv.Mlp(desc, mlp_cases.make_params(mnv, desc, seed=1))
        mnv.accel_set_fused_kernel(self.tree.accel, 1)  # the one-role kernel: frames do not depend on a producer / consumer schedule
        n = W * H
        self.rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        self.rgba8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        self.visited = torch.zeros(self.view.capacity, dtype=torch.int32, device="cuda")
        self.num = torch.zeros(n, dtype=torch.int16, device="cuda")
        self.samples = torch.zeros((n, MAX_G, 4), dtype=torch.float32, device="cuda")
        self.clusters = torch.zeros((n, MAX_G), dtype=torch.int16, device="cuda")
        self.rays = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda")
        self.rays[1, ..., 2] = 1.0

    def args(self):
        return {"accel": C.c_void_p(self.tree.accel), "cam": C.byref(self.cam.c), "n_cams": 1, "opt": C.byref(self.opt),
                "tile": self.mnv.Rect(0, 0, W, H), "part": self.mnv.Partition(*WHOLE), "inputs": None, "rgba": self.rgba.data_ptr(),
                "rgba8": self.rgba8.data_ptr(), "split": None, "sample": None, "counts": None, "visited": None, "parent": None,
                "num": self.num.data_ptr(), "samples": self.samples.data_ptr(), "dim": 4, "clusters": self.clusters.data_ptr(),
                "grid": C.byref(self.grid), "mlp": self.mlp._h, "counter": None, "stream": None, "origins": self.rays[0].data_ptr(),
                "dirs": self.rays[1].data_ptr(), "width": W, "height": H}

    def call(self, name, **over):
        """(return code, mnv_last_error) of entry point `name` with the scene's valid arguments, `over` replacing some of them"""
        a = self.args()
        assert set(over) <= set(ENTRIES[name]), (name, over)
        a.update(over)
        h = self.mnv.lib()
        rc = getattr(h, name)(*[a[k] for k in ENTRIES[name]])
        return rc, h.mnv_last_error().decode("utf-8", "replace")

    def options(self, **fields):
        o = type(self.opt).from_buffer_copy(self.opt)
        for k, v in fields.items():
            setattr(o, k, v)
        return o


@pytest.fixture(scope="module")
def scene(mnv, torch_gpu):
    s = Scene(mnv, torch_gpu)
    yield s
    torch_gpu.cuda.synchronize()


def refused(scene, name, code, text, **over):
    rc, msg = scene.call(name, **over)
    assert rc == code and text in msg, (name, sorted(over), rc, msg)


def test_every_entry_point_refuses_a_null_accel_options_or_camera(scene):
    inv = scene.mnv.MNV_E_INVALID
    for name in ENTRIES:
        fused = name in FUSED_ENTRIES
        refused(scene, name, inv, "null argument" if fused else "accel is null", accel=None)
        tracked = name == RAYS or any(name.endswith(s) for s in ("_track", "_visit", "_visit_ex", "_visit_part"))
        no_opt = "null argument" if fused or name in SAMPLE_ENTRIES else "options are null" if tracked else "camera/options pointer is null"
        refused(scene, name, inv, no_opt, opt=None)
        if name != RAYS:
            refused(scene, name, inv, "null argument" if fused else "need 1 .. MNV_MAX_BATCH cameras", cam=None)


def test_visit_marks_need_the_parent_array(scene):
    for name, keys in ENTRIES.items():
        if "visited" in keys:
            refused(scene, name, scene.mnv.MNV_E_INVALID, "visit marks on the packed layout need the parent array", visited=scene.visited.data_ptr())


@pytest.mark.parametrize("part", [(2, 2, 8, 8, 0), (0, 2, 12, 8, 0), (0, 2, 8, 8, 1)], ids=["rank_ge_world", "tile_not_multiple_of_8", "root_period_1"])
def test_a_malformed_partition_is_refused(scene, part):
    for name, keys in ENTRIES.items():
        if "part" in keys:
            refused(scene, name, scene.mnv.MNV_E_INVALID, "partition needs 0 <= rank < world", part=scene.mnv.Partition(*part))


def test_a_batch_needs_1_to_64_cameras_of_one_size(scene):
    mnv, inv = scene.mnv, scene.mnv.MNV_E_INVALID
    cams = (mnv.CameraStruct * 65)(*[scene.cam.c] * 65)
    for n in (0, 65):
        refused(scene, P + "_batch", inv, "need 1 .. MNV_MAX_BATCH cameras", cam=cams, n_cams=n)
    cams[1].width = W + 1
    refused(scene, P + "_batch", inv, "all cameras of a batch must have the same image size", cam=cams, n_cams=2)


def test_sample_rows_and_quota_are_checked(scene):
    inv = scene.mnv.MNV_E_INVALID
    no_quota = scene.options(max_guided_samples=0)
    for name in SAMPLE_ENTRIES:
        for dim in (3, 5):
            refused(scene, name, inv, "samples_dim must be 4 + 3 * need_viewdir", dim=dim)
        refused(scene, name, inv, "max_guided_samples must be positive", opt=C.byref(no_quota))
    for name in FUSED_ENTRIES:
        refused(scene, name, inv, "max_guided_samples must be positive", opt=C.byref(no_quota))


def test_the_fused_frame_refuses_depth_mode_and_a_model_that_disagrees_with_the_options(scene):
    depth, viewdir = scene.options(render_depth=1), scene.options(need_viewdir=1)
    for name in FUSED_ENTRIES:
        refused(scene, name, scene.mnv.MNV_E_UNSUPPORTED, "no depth mode", opt=C.byref(depth))
        refused(scene, name, scene.mnv.MNV_E_INVALID, "options.need_viewdir does not match the model", opt=C.byref(viewdir))


def test_a_ray_image_needs_a_size_and_an_output(scene):
    inv = scene.mnv.MNV_E_INVALID
    refused(scene, RAYS, inv, "a ray image needs width >= 1", width=0)
    refused(scene, RAYS, inv, "both outputs are null", rgba=None, rgba8=None)
    refused(scene, RAYS, inv, "ray origins / directions are null", origins=None)


def frame_of(scene, name, **over):
    torch = scene.torch
    scene.rgba.fill_(float("nan"))
    scene.rgba8.fill_(7)
    rc, msg = scene.call(name, **over)
    assert rc == 0, (name, rc, msg)
    torch.cuda.synchronize()
    return scene.rgba.cpu().numpy().view(np.uint32).copy(), scene.rgba8.cpu().numpy().copy()


def test_the_frame_entry_points_are_one_frame_when_their_extras_are_null(scene):
    """mnv_render_voxels_accel, _ex, _batch (one camera, whole image), _part ({0, 1, 0, 0, 0}), _track, _visit and _visit_ex with NULL extras"""
    assert sorted(FRAME_ENTRIES) == sorted(P + s for s in ("", "_ex", "_batch", "_part", "_track", "_visit", "_visit_ex", "_visit_part"))
    ref, ref8 = frame_of(scene, P)
    alpha = ref.view(np.float32)[..., 3]
    assert np.isfinite(alpha).all() and (alpha > 0).any() and (alpha < 1).any(), "the frame shows the tree and its background"
    for name in FRAME_ENTRIES[1:]:
        got, got8 = frame_of(scene, name)
        assert np.array_equal(got, ref) and np.array_equal(got8, ref8), name


def test_the_sample_entry_points_emit_the_same_rows(scene):
    def emit(name):
        scene.num.zero_()  # (the march adds to the counts)
        scene.samples.fill_(-1.0)
        scene.clusters.fill_(-2)
        rc, msg = scene.call(name)
        assert rc == 0, (name, rc, msg)
        scene.torch.cuda.synchronize()
        return scene.num.cpu().numpy().copy(), scene.samples.cpu().numpy().view(np.uint32).copy(), scene.clusters.cpu().numpy().copy()

    num, rows, ids = emit(S)
    assert num.min() >= 0 and num.max() > 0, "some rays emit samples"
    for name in SAMPLE_ENTRIES[1:]:
        got = emit(name)
        assert np.array_equal(got[0], num) and np.array_equal(got[1], rows) and np.array_equal(got[2], ids), name


def test_the_fused_entry_points_are_one_frame_when_their_extras_are_null(scene):
    """mnv_render_guided_fused, _track and _track_ex (and the two _part entry points with the whole-image partition) on fused kernel 1"""
    counter = scene.torch.zeros(1, dtype=scene.torch.int64, device="cuda")
    ref, ref8 = frame_of(scene, F, counter=counter.data_ptr())
    assert int(counter.item()) > 0, "the network ran"
    for name in FUSED_ENTRIES[1:]:
        got, got8 = frame_of(scene, name)
        assert np.array_equal(got, ref) and np.array_equal(got8, ref8), name
    assert scene.mnv.accel_fused_faults(scene.tree.accel) == 0
