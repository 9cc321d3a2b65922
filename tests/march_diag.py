"""The scene of tests/test_march_diag_gpu.py and its child process: `python tests/march_diag.py <out dir>` renders the scene's two
requests on whatever library MNV_LIB_PATH selects (the test: the test-hook build with diagnostics knobs set, so the diagnostics
instantiation of march_accel_kernel, MODE 1, runs), writes frame.npy, tile.npy and info.json into the directory and destroys the accel,
which prints the reports of csrc/mnv_accel_diag.hip."""
import gc
import json
import os
import sys

import numpy as np

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_root, os.path.join(_root, "oracle")):     # (the child process starts here, without the test session's paths)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import march_matrix as mm  # noqa: E402

DEPTH, KIND = 10, "random"     # the smallest SH9 tree of march_matrix with a second lookup grid below the LDS level and brick records (mm.PATHS)
SIZE = 64                      # the frame: 64 x 64 pixels, 8 x 8 ray tiles
TILE = (0, 13, 64, 40)         # x0, y0, w, h: a rectangle at an offset that is no multiple of the ray tile, 8 x 5 ray tiles
REQUESTS = (("tile", TILE), ("frame", None))     # (the frame last: MNV_TIMELINE keeps the last launch)


def camera(mnv):
    return mnv.Camera(SIZE, SIZE, 190.0).set_pose(*mm.RANDOM_POSES[0])


def render(mnv, torch, accel, tile, recording=False):
    """-> (float RGBA frame of the request as numpy, the instantiation that ran if `recording`: the test-hook build records it)"""
    w, h = (tile[2], tile[3]) if tile else (SIZE, SIZE)
    rgba = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(accel, camera(mnv), mm.options(mnv), tile=tile, rgba=rgba)
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), (mnv.last_march_variant() if recording else None)


def main(out_dir):
    import torch

    import mega_nerf_viewer_amd as mnv

    tree, _keep = mm.make_tree(mnv, 9, DEPTH, KIND)
    tree.move_to_device()
    info = dict(mnv.accel_info(tree.accel), capacity=int(tree.host_view().capacity), variants=[])
    for name, tile in REQUESTS:
        got, variant = render(mnv, torch, tree.accel, tile, recording=True)
        np.save(os.path.join(out_dir, name + ".npy"), got)
        info["variants"].append(variant)
    with open(os.path.join(out_dir, "info.json"), "w") as f:
        json.dump(info, f)
    del tree          # mnv_accel_destroy: the reports
    gc.collect()


if __name__ == "__main__":
    main(sys.argv[1])
