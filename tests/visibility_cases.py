"""The cases of the culling tests (tests/test_visibility_ref.py on the CPU, tests/test_visibility_gpu.py on the device): the six trees,
options and 640-ray lists of tests/fit_cases.py (degenerate rays, rays from inside, per-ray limits), and a hand-built WALL tree: a slab
of leaves so dense that one sample ends a ray, in front of refined, non-empty chunks at three depths that only a camera behind the wall
could see."""
import numpy as np

import fit_cases
import rays_ref

NAMES = fit_cases.NAMES
WALL_SIGMA = 60000.0      # d_s >= step_size * delta_scale = 2e-4: att <= exp(-12) < stop_thresh, the first sample ends the ray
WALL_FRAME = 24
# the threshold the mixed-scene counts of tests/test_visibility_ref.py are stated for
MIXED_THRESH = 1e-2


def wall_arrays():
    """(data uint16 [cap, 8, 4], child int32 [cap, 8]) of an SH1 tree over world [-1, 1]^3 (offset 0.5, scale 0.5; tree space below).
    Root voxels with x in [0, 0.5) refine once: their x-low halves are empty, their x-high halves -- the slab x in [0.25, 0.5), over all of
    y and z -- carry WALL_SIGMA.  Root voxels with x in [0.5, 1) refine to chunks of depth 2 whose voxels 0 and 5 refine again (depth 3),
    voxel 3 of the first of those once more (depth 4); every leaf behind the wall has sigma 20."""
    rng = np.random.default_rng(31)
    child_rows, sigma_rows = [np.zeros(8, np.int32)], [np.zeros(8, np.float32)]

    def new_chunk(parent, j, sigma):
        n = len(child_rows)
        child_rows[parent][j] = n - parent
        child_rows.append(np.zeros(8, np.int32))
        sigma_rows.append(np.asarray(sigma, np.float32))
        return n

    for j in range(8):                                                # j = 4 x + 2 y + z
        if j < 4:
            new_chunk(0, j, [0.0] * 4 + [WALL_SIGMA] * 4)
        else:
            c2 = new_chunk(0, j, [20.0] * 8)
            for k in (0, 5):
                c3 = new_chunk(c2, k, [20.0] * 8)
                if k == 0:
                    new_chunk(c3, 3, [20.0] * 8)
    child = np.stack(child_rows)
    cap = child.shape[0]
    vals = rng.normal(0.0, 1.5, size=(cap, 8, 4)).astype(np.float16)
    vals[..., 3] = np.stack(sigma_rows).astype(np.float16)
    return np.ascontiguousarray(vals.view(np.uint16)), child


def wall_tree(mnv):
    data, child = wall_arrays()
    return mnv.N3Tree.from_arrays(data, child, data_format="SH1")


def wall_cameras(mnv, size=WALL_FRAME):
    """two cameras on the wall's side (world x < -1, y and z inside [-1, 1]) that look at the centre: every line of sight to a point behind
    the wall crosses the slab inside the volume"""
    out = []
    for c in ((-3.0, 0.3, -0.2), (-2.5, -0.5, 0.4)):
        c = np.array(c, np.float64)
        back = c / np.linalg.norm(c)
        out.append(mnv.Camera(size, size, 1.25 * size).set_pose(tuple(float(x) for x in c), tuple(float(x) for x in back)))
    return out


def camera_rays(cam):
    """(origins, dirs) float32 [h * w, 3] of a camera's pinhole frame"""
    o, d = rays_ref.pinhole_rays(cam.c)
    return o.reshape(-1, 3), d.reshape(-1, 3)


def wall_ray_list(mnv):
    """the frames of both wall cameras as one list: dict(o, d float32 [1152, 3], tmax None)"""
    rays = [camera_rays(c) for c in wall_cameras(mnv)]
    return dict(o=np.concatenate([r[0] for r in rays]), d=np.concatenate([r[1] for r in rays]), tmax=None)
