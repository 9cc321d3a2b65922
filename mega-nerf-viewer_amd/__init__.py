"""ctypes binding of libmnv.so (include/mnv.h) for the test-suite, bench.py and the
multi-GPU tile driver.

This is plumbing over the C ABI, not a second implementation: every render call goes
through ``mnv_render_voxels`` / ``mnv_render_voxels_accel`` into the hand-written HIP
kernels.  There is no CPU or PyTorch fallback -- if ``libmnv.so`` is missing the import of
the library raises, and a render call on a machine without a HIP device returns the
library's error (``MnvError``).

Reference surface mirrored here (cmusatyalab/mega-nerf-viewer):
  * ``N3Tree``           include/n3tree/n3tree.hpp:17-69
  * ``Camera``           include/camera.hpp:12-87 (pose model + intrinsics)
  * ``RenderOptions``    include/render_options.hpp:9-56
  * ``render_voxels``    include/cuda/renderer_kernel.hpp:23-34
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MNV_LIB_PATH") or os.path.join(_HERE, "libmnv.so")   # MNV_LIB_PATH: A/B builds of the library (tools/build_variant.sh)

MNV_OK = 0
MNV_E_INVALID = -1
MNV_E_UNSUPPORTED = -2
MNV_E_NO_DEVICE = -3
MNV_E_IO = -4
MNV_E_NO_RCCL = -5
MNV_E_RCCL = -6
MNV_E_FAULT = -7
FORMAT_RGBA = 0
FORMAT_SH = 1
BASIS_MAX = 25


class MnvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mnv error {code}: {msg}")
        self.code = code


class TreeView(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("child", C.c_void_p),
        ("parent", C.c_void_p),
        ("sample_counts", C.c_void_p),
        ("offset", C.c_float * 3),
        ("scale", C.c_float * 3),
        ("N", C.c_int32),
        ("data_dim", C.c_int32),
        ("format", C.c_int32),
        ("basis_dim", C.c_int32),
        ("capacity", C.c_int32),
    ]


class CameraStruct(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("c2w", C.c_float * 12),
    ]


class RenderOptions(C.Structure):
    """viewer::RenderOptions, field for field (reference include/render_options.hpp:9-56)."""

    _fields_ = [
        ("step_size", C.c_float),
        ("sigma_thresh", C.c_float),
        ("stop_thresh", C.c_float),
        ("background_brightness", C.c_float),
        ("render_bbox", C.c_float * 6),
        ("basis_minmax", C.c_int32 * 2),
        ("rot_dirs", C.c_float * 3),
        ("show_grid", C.c_bool),
        ("grid_max_depth", C.c_int32),
        ("render_depth", C.c_bool),
        ("use_splitting", C.c_bool),
        ("use_guided_sampling", C.c_bool),
        ("max_depth", C.c_int32),
        ("samples_per_corner", C.c_int32),
        ("split_batch_size", C.c_int32),
        ("nerf_batch_size", C.c_int32),
        ("max_sample_count", C.c_int32),
        ("need_viewdir", C.c_bool),
        ("appearance_embedding", C.c_int32),
        ("max_guided_samples", C.c_int32),
    ]

    @classmethod
    def defaults(cls) -> "RenderOptions":
        o = cls()
        lib().mnv_default_render_options(C.byref(o))
        return o

    @classmethod
    def cli_defaults(cls) -> "RenderOptions":
        o = cls()
        lib().mnv_cli_render_options(C.byref(o))
        return o


class Rect(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class FrameInputs(C.Structure):
    """mnv_frame_inputs: the per-pixel arrays of the reference's offscreen == false call shape (device pointers, either may be NULL)."""
    _fields_ = [("tmax_px", C.c_void_p), ("rgba8_init", C.c_void_p)]


class Partition(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("root_period", C.c_int32)]


class ClusterGrid(C.Structure):
    _fields_ = [("grid_dim", C.c_int32 * 2), ("min_position", C.c_float * 3), ("range", C.c_float * 3)]


class TreeEdit(C.Structure):
    _fields_ = [("child", C.c_void_p), ("parent", C.c_void_p), ("offset", C.c_float * 3), ("scale", C.c_float * 3),
                ("N", C.c_int32), ("capacity", C.c_int32)]


class MlpDesc(C.Structure):
    _fields_ = [("n_clusters", C.c_int32), ("pos_octaves", C.c_int32), ("dir_octaves", C.c_int32), ("need_viewdir", C.c_int32),
                ("n_embeddings", C.c_int32), ("embedding_dim", C.c_int32), ("hidden_width", C.c_int32), ("hidden_layers", C.c_int32),
                ("out_dim", C.c_int32), ("center", C.c_float * 3), ("inv_extent", C.c_float * 3)]


class RendererStats(C.Structure):
    _fields_ = [("track_visit", C.c_int32), ("used_accel", C.c_int32), ("full", C.c_int32), ("split_candidates", C.c_int32),
                ("added", C.c_int32), ("sample_candidates", C.c_int32), ("resampled", C.c_int32), ("pruned", C.c_int32),
                ("guided_samples", C.c_int64), ("capacity", C.c_int64), ("fused", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class FitParams(C.Structure):
    """mnv_fit_params"""
    _fields_ = [("iterations", C.c_int32), ("lr_colour", C.c_float), ("lr_sigma", C.c_float), ("reserved", C.c_int32)]


class AdamParams(C.Structure):
    """mnv_adam_params"""
    _fields_ = [("lr_colour", C.c_float), ("lr_sigma", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("reserved", C.c_int32 * 3)]


class FitParamsEx(C.Structure):
    """mnv_fit_params_ex"""
    _fields_ = [("steps", C.c_int32), ("optimizer", C.c_int32), ("lr_colour", C.c_float), ("lr_sigma", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("batch_rays", C.c_int32), ("tile", C.c_int32), ("seed", C.c_uint64), ("reserved", C.c_int32 * 4)]


FIT_SGD, FIT_ADAM = 0, 1
# Adam's rates for fitting rows (include/mnv.h, mnv_n3tree_fit_ex; the sweep behind them stands in tests/fit_adam_ref.py)
ADAM_DEFAULTS = dict(lr_colour=0.03, lr_sigma=1.0, betas=(0.9, 0.999), eps=1e-8)

FIT_SUMS = ("n_rays", "n_stopped", "n_samples", "n_skipped", "se_q32")   # the first five int64 words of mnv_fit_sums (8 in all)


VIS_SUMS = ("n_rays", "n_stopped", "n_samples", "n_skipped")   # the first four int64 words of mnv_vis_sums (8 in all)


class CullCounts(C.Structure):
    """mnv_cull_counts"""
    _fields_ = [("leaves_seen", C.c_int64), ("leaves_culled", C.c_int64), ("dead_chunks", C.c_int64), ("reserved", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_[:3]}


class MetricSums(C.Structure):
    """mnv_metric_sums: the five int64 words mnv_frame_metrics leaves in device memory."""
    _fields_ = [("n_px", C.c_int64), ("se_q32", C.c_int64), ("n_win", C.c_int64), ("ssim_q32", C.c_int64), ("reserved", C.c_int64)]


class FrameMetricValues(C.Structure):
    """mnv_frame_metric_values: what mnv_metrics_finish makes of the sums."""
    _fields_ = [("mse", C.c_double), ("psnr", C.c_double), ("ssim", C.c_double), ("n_px", C.c_int64), ("n_win", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SynthRandomParams(C.Structure):
    _fields_ = [
        ("depth", C.c_int32),
        ("format", C.c_int32),
        ("basis_dim", C.c_int32),
        ("refine_prob", C.c_float),
        ("empty_prob", C.c_float),
        ("sigma_max", C.c_float),
        ("coef_sd", C.c_float),
        ("offset", C.c_float * 3),
        ("scale", C.c_float * 3),
        ("seed", C.c_uint64),
    ]


class SynthTerrainParams(C.Structure):
    _fields_ = [("depth", C.c_int32), ("basis_dim", C.c_int32), ("bricks_y", C.c_int32), ("bricks_z", C.c_int32),
                ("noise_cells", C.c_int32), ("base", C.c_float), ("amplitude", C.c_float), ("thickness", C.c_float),
                ("sigma_lo", C.c_float), ("sigma_hi", C.c_float), ("offset", C.c_float * 3), ("scale", C.c_float * 3),
                ("seed", C.c_uint64)]


class SynthShellParams(C.Structure):
    _fields_ = [
        ("depth", C.c_int32),
        ("basis_dim", C.c_int32),
        ("radius", C.c_float),
        ("half_thickness", C.c_float),
        ("sigma_lo", C.c_float),
        ("sigma_hi", C.c_float),
        ("offset", C.c_float * 3),
        ("scale", C.c_float * 3),
        ("seed", C.c_uint64),
    ]


class ExtractParams(C.Structure):
    """mnv_extract_params"""
    _fields_ = [("level", C.c_int32), ("iso", C.c_float), ("flags", C.c_int32)]


class SurfaceStats(C.Structure):
    """mnv_surface_stats: bricks of the lattice, bricks the passes visited, device milliseconds per pass."""
    _fields_ = [("bricks", C.c_int64), ("candidate_bricks", C.c_int64), ("ms_candidates", C.c_float), ("ms_count", C.c_float), ("ms_scan", C.c_float),
                ("ms_emit", C.c_float), ("ms_colour", C.c_float), ("ms_total", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


EXTRACT_COLOUR, EXTRACT_ALL_BRICKS = 1, 2


class PointsParams(C.Structure):
    """mnv_points_params"""
    _fields_ = [("offset", C.c_float * 3), ("scale", C.c_float * 3), ("depth", C.c_int32), ("format", C.c_int32), ("basis_dim", C.c_int32),
                ("min_points", C.c_uint32), ("sigma", C.c_float)]


class PointsStats(C.Structure):
    """mnv_points_stats"""
    _fields_ = [("accepted", C.c_int64), ("dropped", C.c_int64), ("distinct_voxels", C.c_int64), ("occupied_voxels", C.c_int64),
                ("chunks_at_depth", C.c_int64 * 24)]

    @property
    def capacity(self) -> int:
        return int(sum(self.chunks_at_depth))

    def as_dict(self):
        return dict(accepted=self.accepted, dropped=self.dropped, distinct_voxels=self.distinct_voxels, occupied_voxels=self.occupied_voxels,
                    chunks_at_depth=list(self.chunks_at_depth), capacity=self.capacity)


MERGE_OVER, MERGE_ADD = 0, 1


class MergeParams(C.Structure):
    """mnv_merge_params"""
    _fields_ = [("level", C.c_int32), ("corner", C.c_int32 * 3), ("mode", C.c_int32), ("reserved", C.c_int32)]


class MergeStats(C.Structure):
    """mnv_merge_stats"""
    _fields_ = [("chunks_at_depth", C.c_int64 * 24), ("capacity", C.c_int64), ("rows_from_a", C.c_int64), ("rows_from_b", C.c_int64),
                ("rows_blended", C.c_int64), ("pushed_a", C.c_int64), ("pushed_b", C.c_int64)]

    def as_dict(self):
        return dict(chunks_at_depth=list(self.chunks_at_depth), capacity=self.capacity, rows_from_a=self.rows_from_a, rows_from_b=self.rows_from_b,
                    rows_blended=self.rows_blended, pushed_a=self.pushed_a, pushed_b=self.pushed_b)


# every symbol include/mnv.h declares (tests/test_capi_symbols.py checks the export list)
_SIGNATURES = {
    "mnv_version": (C.c_int, []),
    "mnv_last_error": (C.c_char_p, []),
    "mnv_source_sha": (C.c_char_p, []),
    "mnv_device_count": (C.c_int, []),
    "mnv_default_render_options": (None, [C.POINTER(RenderOptions)]),
    "mnv_cli_render_options": (None, [C.POINTER(RenderOptions)]),
    "mnv_camera_init": (None, [C.POINTER(CameraStruct), C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float]),
    "mnv_camera_set_pose": (None, [C.POINTER(CameraStruct), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mnv_camera_drag": (None, [C.POINTER(CameraStruct), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                               C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]),
    "mnv_render_voxels": (C.c_int, [C.POINTER(TreeView), C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mnv_render_voxels_ex": (C.c_int, [C.POINTER(TreeView), C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.POINTER(FrameInputs),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mnv_render_voxels_accel_ex": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.POINTER(FrameInputs),
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_accel_create": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.POINTER(C.c_void_p)]),
    "mnv_accel_create_reserved": (C.c_int, [C.POINTER(TreeView), C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mnv_accel_refresh": (C.c_int, [C.c_void_p, C.POINTER(TreeView), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "mnv_accel_rebuild": (C.c_int, [C.c_void_p, C.POINTER(TreeView), C.c_void_p]),
    "mnv_accel_destroy": (None, [C.c_void_p]),
    "mnv_accel_device_bytes": (C.c_size_t, [C.c_void_p]),
    "mnv_accel_grid2_level": (C.c_int32, [C.c_void_p]),
    "mnv_accel_brick_levels": (C.c_int32, [C.c_void_p]),
    "mnv_accel_lookup_coverage": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mnv_accel_set_cu_budget": (C.c_int, [C.c_void_p, C.c_int32]),
    "mnv_stream_create_reserved": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "mnv_stream_destroy": (C.c_int, [C.c_void_p]),
    "mnv_render_voxels_accel": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_partition_local_tiles": (C.c_int32, [Rect, Partition]),
    "mnv_render_voxels_accel_part": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, Partition,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_accel_set_colour_math": (C.c_int, [C.c_void_p, C.c_int]),
    "mnv_accel_set_fused_kernel": (C.c_int, [C.c_void_p, C.c_int]),
    "mnv_accel_set_fused_diag": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mnv_accel_fused_faults": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "mnv_set_tree_cache": (None, [C.c_int]),
    "mnv_tree_invalidate": (None, [C.c_void_p]),
    "mnv_assemble_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, Partition, C.c_int32, C.c_int32, C.c_void_p]),
    "mnv_comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "mnv_comm_init_rank": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mnv_comm_rank": (C.c_int32, [C.c_void_p]),
    "mnv_comm_world": (C.c_int32, [C.c_void_p]),
    "mnv_comm_rccl_version": (C.c_int32, []),
    "mnv_gather_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    "mnv_comm_destroy": (None, [C.c_void_p]),
    "mnv_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mnv_merge_visit_marks": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mnv_render_voxels_accel_visit_part": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, Partition, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_guided_fused_track_part": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, Partition, C.c_void_p,
                                                     C.POINTER(ClusterGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_voxels_accel_batch": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.c_int32, C.POINTER(RenderOptions), Rect,
                                                Partition, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_voxels_accel_track": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_get_samples_from_voxels": (C.c_int, [C.POINTER(TreeView), C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_get_samples_from_voxels_ex": (C.c_int, [C.POINTER(TreeView), C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.POINTER(FrameInputs),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_get_samples_from_voxels_accel_visit_ex": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.POINTER(FrameInputs),
                                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                             C.c_void_p, C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_render_guided_fused_track_ex": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.POINTER(FrameInputs), C.c_void_p,
                                                   C.POINTER(ClusterGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    "mnv_get_samples_from_voxels_accel": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_render_voxels_accel_visit": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_get_samples_from_voxels_accel_visit": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                          C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_render_guided_fused": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.POINTER(ClusterGrid),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_guided_fused_track": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.POINTER(ClusterGrid),
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_guided_fused_part": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, Partition, C.c_void_p,
                                               C.POINTER(ClusterGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_nerf_results": (C.c_int, [C.POINTER(TreeView), C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_add_children_and_generate_samples": (C.c_int, [C.POINTER(TreeEdit), C.POINTER(RenderOptions), C.c_void_p, C.c_int32, C.c_void_p,
                                                        C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_generate_samples": (C.c_int, [C.POINTER(TreeEdit), C.POINTER(RenderOptions), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.POINTER(ClusterGrid), C.c_void_p]),
    "mnv_adjust_parents_and_children": (C.c_int, [C.POINTER(TreeEdit), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_select_split_candidates": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "mnv_select_sample_candidates": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "mnv_apply_split_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mnv_apply_sample_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mnv_prune_tree": (C.c_int, [C.POINTER(TreeEdit), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.c_void_p]),
    "mnv_prune_tree_accel": (C.c_int, [C.POINTER(TreeEdit), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), C.c_void_p]),
    "mnv_mlp_param_count": (C.c_size_t, [C.POINTER(MlpDesc)]),
    "mnv_mlp_create": (C.c_int, [C.POINTER(MlpDesc), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mnv_mlp_destroy": (None, [C.c_void_p]),
    "mnv_query_submodules": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "mnv_fill_uniform": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p]),
    "mnv_compact_guided_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "mnv_renderer_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "mnv_renderer_destroy": (None, [C.c_void_p]),
    "mnv_renderer_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mnv_renderer_load_model": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mnv_renderer_set_model": (C.c_int, [C.c_void_p, C.POINTER(MlpDesc), C.c_void_p, C.c_size_t, C.POINTER(ClusterGrid)]),
    "mnv_renderer_resize": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "mnv_renderer_options": (C.POINTER(RenderOptions), [C.c_void_p]),
    "mnv_renderer_set_camera": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mnv_renderer_set_seed": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32]),
    "mnv_renderer_render": (C.c_int, [C.c_void_p, C.POINTER(RendererStats)]),
    "mnv_renderer_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_renderer_sync_tree": (C.c_int, [C.c_void_p]),
    "mnv_renderer_set_frames_in_flight": (C.c_int, [C.c_void_p, C.c_int32]),
    "mnv_renderer_set_guided_in_flight": (C.c_int, [C.c_void_p, C.c_int]),
    "mnv_renderer_slot_guided_samples": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "mnv_renderer_last_slot": (C.c_int32, [C.c_void_p]),
    "mnv_renderer_set_fused_guided": (C.c_int, [C.c_void_p, C.c_int]),
    "mnv_renderer_set_frame_inputs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_render_voxels_accel_visit_ex": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.POINTER(FrameInputs), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_renderer_set_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "mnv_renderer_download_slot": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mnv_n3tree_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "mnv_n3tree_from_arrays": (C.c_int, [C.POINTER(TreeView), C.POINTER(C.c_void_p)]),
    "mnv_n3tree_free": (None, [C.c_void_p]),
    "mnv_n3tree_host_view": (C.c_int, [C.c_void_p, C.POINTER(TreeView)]),
    "mnv_n3tree_move_to_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mnv_n3tree_device_view": (C.c_int, [C.c_void_p, C.POINTER(TreeView)]),
    "mnv_n3tree_accel": (C.c_void_p, [C.c_void_p]),
    "mnv_n3tree_save_npz": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mnv_data_format_parse": (None, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mnv_data_format_to_string": (C.c_int, [C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "mnv_synth_random_tree": (C.c_int, [C.POINTER(SynthRandomParams), C.POINTER(C.c_void_p)]),
    "mnv_synth_shell_tree": (C.c_int, [C.POINTER(SynthShellParams), C.POINTER(C.c_void_p)]),
    "mnv_synth_terrain_tree": (C.c_int, [C.POINTER(SynthTerrainParams), C.POINTER(C.c_void_p)]),
    "mnv_n3tree_gen_wireframe": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "mnv_wireframe_create": (C.c_int, [C.POINTER(TreeView), C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mnv_wireframe_update": (C.c_int, [C.c_void_p, C.POINTER(TreeView), C.c_int32, C.c_void_p]),
    "mnv_wireframe_destroy": (None, [C.c_void_p]),
    "mnv_wireframe_cube_count": (C.c_int64, [C.c_void_p]),
    "mnv_wireframe_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "mnv_render_wireframe": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_renderer_wireframe": (C.c_void_p, [C.c_void_p]),
    "mnv_renderer_camera": (C.c_int, [C.c_void_p, C.POINTER(CameraStruct)]),
    "mnv_wireframe_set_method": (C.c_int, [C.c_void_p, C.c_int32]),
    "mnv_aa_pattern": (C.c_int, [C.c_int32, C.c_void_p]),
    "mnv_aa_weights": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "mnv_resolve_samples": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_renderer_set_antialiasing": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "mnv_mesh_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    "mnv_mesh_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int]),
    "mnv_mesh_destroy": (None, [C.c_void_p]),
    "mnv_mesh_model_matrix": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mnv_mesh_show": (C.c_int, [C.c_void_p, C.c_int]),
    "mnv_mesh_visible": (C.c_int, [C.c_void_p]),
    "mnv_mesh_vertex_count": (C.c_int64, [C.c_void_p]),
    "mnv_mesh_face_count": (C.c_int64, [C.c_void_p]),
    "mnv_mesh_face_size": (C.c_int32, [C.c_void_p]),
    "mnv_model_matrix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "mnv_obj_read": (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                               C.POINTER(C.c_int32)]),
    "mnv_render_meshes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(CameraStruct), C.POINTER(RenderOptions), Rect, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "mnv_renderer_add_mesh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mnv_renderer_clear_meshes": (C.c_int, [C.c_void_p]),
    "mnv_renderer_mesh_count": (C.c_int32, [C.c_void_p]),
    "mnv_render_rays_accel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RenderOptions), C.POINTER(FrameInputs),
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_generate_rays": (C.c_int, [C.c_int32, C.POINTER(CameraStruct), Rect, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_equirect_tables": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "mnv_renderer_set_projection": (C.c_int, [C.c_void_p, C.c_int32]),
    "mnv_frame_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_ssim_window": (C.c_int, [C.c_void_p]),
    "mnv_metrics_finish": (C.c_int, [C.POINTER(MetricSums), C.POINTER(FrameMetricValues)]),
    "mnv_pnm_read": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mnv_renderer_set_target": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mnv_renderer_slot_metrics": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(FrameMetricValues)]),
    "mnv_accel_sample_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_extract_surface": (C.c_int, [C.c_void_p, C.POINTER(ExtractParams), C.c_void_p, C.POINTER(C.c_void_p)]),
    "mnv_surface_destroy": (None, [C.c_void_p]),
    "mnv_surface_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mnv_surface_stats_get": (C.c_int, [C.c_void_p, C.POINTER(SurfaceStats)]),
    "mnv_surface_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "mnv_surface_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mnv_surface_to_mesh": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mnv_obj_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "mnv_tree_mip_rows": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "mnv_tree_truncate": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_n3tree_make_lod": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "mnv_renderer_set_lod": (C.c_int, [C.c_void_p, C.c_int32]),
    "mnv_tree_select_cut": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "mnv_tree_cut": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_n3tree_make_view_lod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]),
    "mnv_renderer_set_view_lod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_int32]),
    "mnv_renderer_set_lod_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(FitParams)]),
    "mnv_renderer_set_lod_fit_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(FitParamsEx)]),
    "mnv_renderer_set_cull": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float]),
    "mnv_rays_grad": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RenderOptions), C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_rows_master_init": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mnv_rows_sgd_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p]),
    "mnv_n3tree_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(FitParams), C.c_void_p]),
    "mnv_n3tree_fit_to_tree": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RenderOptions), C.POINTER(FitParams), C.c_void_p]),
    "mnv_rows_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(AdamParams), C.c_int64, C.c_void_p]),
    "mnv_ray_batcher_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mnv_ray_batcher_units": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "mnv_ray_batcher_draw": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_ray_batcher_destroy": (None, [C.c_void_p]),
    "mnv_n3tree_fit_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(RenderOptions), C.POINTER(FitParamsEx), C.c_void_p, C.c_void_p]),
    "mnv_n3tree_fit_to_tree_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RenderOptions), C.POINTER(FitParamsEx), C.c_void_p, C.c_void_p]),
    "mnv_rays_visibility": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RenderOptions), C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "mnv_tree_cull": (C.c_int, [C.POINTER(TreeView), C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(CullCounts), C.c_void_p]),
    "mnv_n3tree_make_culled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RenderOptions), C.c_float, C.POINTER(C.c_int64), C.POINTER(CullCounts),
                                         C.POINTER(C.c_void_p)]),
    "mnv_point_tree_create": (C.c_int, [C.POINTER(PointsParams), C.POINTER(C.c_void_p)]),
    "mnv_point_tree_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mnv_point_tree_finish": (C.c_int, [C.c_void_p, C.POINTER(PointsStats), C.c_void_p]),
    "mnv_point_tree_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_point_tree_destroy": (None, [C.c_void_p]),
    "mnv_points_colour_table": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "mnv_points_bounds_to_cube": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_n3tree_from_points": (C.c_int, [C.POINTER(PointsParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(PointsStats), C.POINTER(C.c_void_p)]),
    "mnv_tree_merge_plan": (C.c_int, [C.POINTER(TreeView), C.POINTER(TreeView), C.POINTER(MergeParams), C.POINTER(C.c_void_p), C.POINTER(MergeStats), C.c_void_p]),
    "mnv_tree_merge_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_tree_merge_destroy": (None, [C.c_void_p]),
    "mnv_tree_voxel_cube": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_n3tree_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MergeParams), C.POINTER(MergeStats), C.POINTER(C.c_void_p)]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libmnv.so (built by ``__graft_entry__.build()`` / ``make``); raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
        # One HIP runtime per process: torch ships its own libamdhip64.so.7 and must load it first;
        # libmnv.so (linked against the same SONAME) then binds to that copy.  Loading ours first
        # leaves two half-initialised runtimes and hipGetDeviceCount() == 0.
        import torch  # noqa: F401

        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


class ProbeCamBlock(C.Structure):
    """csrc/mnv_device.h CamBlock, field for field (80 bytes)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("c2w", C.c_float * 12), ("cen", C.c_float * 3),
                ("pad", C.c_float)]


class ProbeFrame(C.Structure):
    """csrc/mnv_device.h FrameParams, field for field (240 bytes, 16-byte aligned): the by-value argument block of the march kernels, as
    mnv_hook_probe_setup_ray takes it.  The four pointers at the end are ignored by the probes."""
    _fields_ = [("cam", ProbeCamBlock), ("x0", C.c_int32), ("y0", C.c_int32), ("tw", C.c_int32), ("th", C.c_int32),
                ("offset", C.c_float * 3), ("scale", C.c_float * 3),
                ("step_size", C.c_float), ("sigma_thresh", C.c_float), ("stop_thresh", C.c_float), ("background_brightness", C.c_float),
                ("render_bbox", C.c_float * 6), ("basis_min", C.c_int32), ("basis_max", C.c_int32), ("render_depth", C.c_int32),
                ("rot_enabled", C.c_int32), ("rot_k", C.c_float * 3), ("rot_cos", C.c_float), ("rot_sin", C.c_float),
                ("rgba", C.c_void_p), ("rgba8", C.c_void_p), ("tmax_px", C.c_void_p), ("rgba8_init", C.c_void_p), ("tail_pad", C.c_uint64)]


# The element-wise probes of mnv_device.h's device functions (csrc/mnv_probe.hip, test-hook build only): device pointers in, device
# pointers out, hip_stream last, an MNV_E_* code back.  tests/test_primitives_gpu.py is their caller.
_PROBE_SIGNATURES = {
    "mnv_hook_probe_frame_size": (C.c_int, []),
    "mnv_hook_probe_cam_size": (C.c_int, []),
    "mnv_hook_live_bytes": (C.c_int64, [C.c_int]),
    "mnv_hook_probe_expf": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_expf_digest": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_expf_variants_differ": (C.c_int, [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_half": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_sigmoid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_sh": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_half_product": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_sh_mix": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_setup_ray": (C.c_int, [C.POINTER(ProbeFrame), C.POINTER(ProbeCamBlock), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                           C.c_void_p, C.c_void_p]),
    "mnv_hook_probe_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # csrc/mnv_points_probe.hip: rocprim::radix_sort_pairs alone, the yardstick of tools/points_bench.py
    "mnv_hook_points_sort_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_int32), C.c_void_p]),
}

_hooks_lib: Optional[C.CDLL] = None
HOOKS_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "testhooks", "libmnv.so")


def hooks_lib() -> C.CDLL:
    """The test-hook build of the library (testhooks/libmnv.so: the same object code but for the knobs / transport units) as a SECOND binding in
    this process -- for what the shipped library does not have: mnv_hook_set_ref_table_min_rays, with which the tests run
    mnv_render_voxels' per-launch lookup table at any frame size, and the mnv_hook_probe_* entry points (_PROBE_SIGNATURES).  (When
    MNV_LIB_PATH already selects the hooks build it is that library.)"""
    global _hooks_lib
    if _hooks_lib is None:
        lib()   # torch's HIP runtime first (see lib())
        if os.path.abspath(LIB_PATH) == os.path.abspath(HOOKS_LIB_PATH):
            h = lib()
        else:
            if not os.path.exists(HOOKS_LIB_PATH):
                raise ImportError(f"{HOOKS_LIB_PATH} is missing (make builds it beside libmnv.so)")
            h = C.CDLL(HOOKS_LIB_PATH)
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(h, name)
                fn.restype = res
                fn.argtypes = args
        h.mnv_hook_set_ref_table_min_rays.restype = None
        h.mnv_hook_set_ref_table_min_rays.argtypes = [C.c_longlong]
        h.mnv_hook_last_march_variant.restype = None
        h.mnv_hook_last_march_variant.argtypes = [C.POINTER(C.c_int32)]
        for name, (res, args) in _PROBE_SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.mnv_hook_probe_frame_size() != C.sizeof(ProbeFrame) or h.mnv_hook_probe_cam_size() != C.sizeof(ProbeCamBlock):
            raise RuntimeError("ProbeFrame / ProbeCamBlock no longer mirror csrc/mnv_device.h's FrameParams / CamBlock")
        _hooks_lib = h
    return _hooks_lib


def last_march_variant():
    """(BASIS, MODE, BRICK, RAYS) of the march_accel_kernel instantiation that the test-hook build launched last (csrc/mnv_knobs.cpp;
    (-2, -1, -1, -1) before the first launch).  Says something about this process's launches only when MNV_LIB_PATH selects that build."""
    out = (C.c_int32 * 4)()
    hooks_lib().mnv_hook_last_march_variant(out)
    return tuple(int(x) for x in out)


def last_march_shape() -> int:
    """Lookup shape of the march_accel_kernel instantiation that the test-hook build launched last (csrc/mnv_march_accel_kernel.h: 0 generic,
    1 / 2 the fixed shape without / with brick records; -1 before the first launch).  As last_march_variant: the hooks build only."""
    f = hooks_lib().mnv_hook_last_march_shape
    f.restype, f.argtypes = C.c_int32, []
    return int(f())


def built_source_sha() -> str:
    """Hash of the sources the loaded libmnv.so was built from (mnv_source_sha)."""
    return lib().mnv_source_sha().decode()


def shipped_source_sha() -> str:
    """The same hash over the sources in this tree (the Makefile's SRC_SHA: sorted relative names, contents concatenated)."""
    import glob
    import hashlib

    here = os.path.dirname(os.path.abspath(__file__))
    names = []
    for pat in ("csrc/*.hip", "csrc/*.h", "csrc/*.cpp", "host/*.cpp", "host/*.hpp", "../include/*.h"):
        names += [os.path.relpath(f, here) for f in glob.glob(os.path.join(here, pat))]
    names = sorted(set(names) - {os.path.join("csrc", "mnv_build_info.cpp")})   # (the unit the hash is compiled INTO is not part of it)
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(here, n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _check(rc: int, h=None) -> None:
    if rc != 0:
        raise MnvError(rc, (h or lib()).mnv_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return int(lib().mnv_device_count())


def parse_data_format(s: str):
    f, b = C.c_int32(), C.c_int32()
    lib().mnv_data_format_parse(s.encode(), C.byref(f), C.byref(b))
    return f.value, b.value


def data_format_to_string(fmt: int, basis_dim: int) -> str:
    buf = C.create_string_buffer(64)
    _check(lib().mnv_data_format_to_string(fmt, basis_dim, buf, 64))
    return buf.value.decode()


def _f3(v: Sequence[float]):
    return (C.c_float * 3)(*[float(x) for x in v])


class Camera:
    """Pose model + intrinsics of viewer::Camera (reference src/camera.cpp:29-130)."""

    def __init__(self, width=256, height=256, fx=1111.0, fy=-1.0, cx=-1.0, cy=-1.0):
        self.c = CameraStruct()
        lib().mnv_camera_init(C.byref(self.c), width, height, fx, fy, cx, cy)

    def set_pose(self, center, v_back, v_world_up=(0.0, 0.0, 1.0)) -> "Camera":
        lib().mnv_camera_set_pose(C.byref(self.c), _f3(center), _f3(v_back), _f3(v_world_up))
        return self

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height

    @property
    def c2w(self) -> np.ndarray:
        return np.array(list(self.c.c2w), dtype=np.float32)


def camera_drag(cam: "Camera", center, v_back, v_world_up, origin, movement_speed, is_pan, about_origin, start_xy, end_xy):
    """Camera::begin_drag / drag_update / end_drag (+ the next frame's _update) on a camera at the given pose: -> (center, v_back, origin, c2w[12])."""
    c, b, u, o = _f3(center), _f3(v_back), _f3(v_world_up), _f3(origin)
    lib().mnv_camera_drag(C.byref(cam.c), c, b, u, o, float(movement_speed), int(is_pan), int(about_origin), float(start_xy[0]), float(start_xy[1]),
                          float(end_xy[0]), float(end_xy[1]))
    return np.float32(list(c)), np.float32(list(b)), np.float32(list(o)), np.float32(list(cam.c.c2w))


def orbit_camera(width, height, fx, radius, azimuth_deg, elevation_deg, fy=-1.0) -> Camera:
    """Camera on a sphere of `radius` around the world origin looking at the origin
    (SURVEY.md 8(d) cfg2 poses).  Pure float64 host trigonometry -> float32 pose vectors."""
    az, el = np.deg2rad(azimuth_deg), np.deg2rad(elevation_deg)
    back = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    center = (radius * back).astype(np.float32)
    return Camera(width, height, fx, fy).set_pose(center, back.astype(np.float32))


class N3Tree:
    """Handle to the C++ viewer::N3Tree (host arrays + optional device copy + accel)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    def __del__(self):
        try:
            if self._h:
                lib().mnv_n3tree_free(self._h)
                self._h = None
        except Exception:
            pass

    @classmethod
    def open(cls, path: str) -> "N3Tree":
        h = C.c_void_p()
        _check(lib().mnv_n3tree_open(os.fsencode(path), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_arrays(cls, data: np.ndarray, child: np.ndarray, *, data_format: str, offset=(0.5, 0.5, 0.5),
                    scale=(0.5, 0.5, 0.5), parent: Optional[np.ndarray] = None) -> "N3Tree":
        data = np.ascontiguousarray(data)
        child = np.ascontiguousarray(child, dtype=np.int32)
        if data.dtype == np.float16:
            data = data.view(np.uint16)
        assert data.dtype == np.uint16
        cap = child.shape[0]
        v = TreeView()
        v.data = data.ctypes.data
        v.child = child.ctypes.data
        if parent is not None:
            parent = np.ascontiguousarray(parent, dtype=np.int32)
            v.parent = parent.ctypes.data
        v.offset = _f3(offset)
        v.scale = _f3(scale)
        v.N = 2
        v.data_dim = data.size // (cap * 8)
        v.format, v.basis_dim = parse_data_format(data_format)
        v.capacity = cap
        h = C.c_void_p()
        _check(lib().mnv_n3tree_from_arrays(C.byref(v), C.byref(h)))
        return cls(h.value)

    @classmethod
    def synth_random(cls, depth=4, basis_dim=1, fmt=FORMAT_SH, refine_prob=0.6, empty_prob=0.5, sigma_max=30.0,
                     coef_sd=1.5, offset=(0.5, 0.5, 0.5), scale=(0.5, 0.5, 0.5), seed=0) -> "N3Tree":
        p = SynthRandomParams(depth, fmt, basis_dim, refine_prob, empty_prob, sigma_max, coef_sd, _f3(offset), _f3(scale), seed)
        h = C.c_void_p()
        _check(lib().mnv_synth_random_tree(C.byref(p), C.byref(h)))
        return cls(h.value)

    @classmethod
    def synth_shell(cls, depth=10, basis_dim=9, radius=0.35, half_thickness=1.5 / 1024, sigma_lo=50.0, sigma_hi=400.0,
                    offset=(0.5, 0.5, 0.5), scale=(0.5, 0.5, 0.5), seed=0) -> "N3Tree":
        p = SynthShellParams(depth, basis_dim, radius, half_thickness, sigma_lo, sigma_hi, _f3(offset), _f3(scale), seed)
        h = C.c_void_p()
        _check(lib().mnv_synth_shell_tree(C.byref(p), C.byref(h)))
        return cls(h.value)

    @classmethod
    def synth_terrain(cls, depth=10, basis_dim=9, bricks_y=4, bricks_z=2, noise_cells=6, base=0.25, amplitude=0.35,
                      thickness=1.5 / 1024, sigma_lo=50.0, sigma_hi=400.0, offset=(0.5, 0.5, 0.5), scale=(0.5, 0.125, 0.125),
                      seed=0) -> "N3Tree":
        p = SynthTerrainParams(depth, basis_dim, bricks_y, bricks_z, noise_cells, base, amplitude, thickness, sigma_lo, sigma_hi,
                               _f3(offset), _f3(scale), seed)
        h = C.c_void_p()
        _check(lib().mnv_synth_terrain_tree(C.byref(p), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_points(cls, xyz, rgb=None, depth: int = 8, sigma: float = 100.0, min_points: int = 1, data_format: str = "RGBA", cube=None,
                    return_stats: bool = False, stream: int = 0):
        """N3Tree::from_points: a tree from a coloured point cloud, on the device with parent, sample counts and the accel, host arrays
        filled (include/mnv.h, "a tree from a coloured point cloud").  xyz: float32 [n, 3], rgb: uint8 [n, 3] or None (white), as numpy
        arrays or torch device tensors.  cube: (offset[3], scale[3]) of the world -> unit cube map, or None for the smallest cube around
        the cloud's finite points, widened by 2^-12 of its edge so that no point sits on its upper faces.  return_stats: also the
        PointsStats."""
        import torch

        def dev(a, dtype, what):
            if a is None:
                return None
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if dtype == torch.float32 else np.uint8))
            if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
                raise MnvError(MNV_E_INVALID, f"{what} must be [n, 3] of {dtype}")
            return t.contiguous().cuda()

        xyz_t = dev(xyz, torch.float32, "xyz")
        n = int(xyz_t.shape[0])
        rgb_t = dev(rgb, torch.uint8, "rgb") if rgb is not None else torch.full((n, 3), 255, dtype=torch.uint8, device=xyz_t.device)
        if int(rgb_t.shape[0]) != n:
            raise MnvError(MNV_E_INVALID, "one colour per point")
        if cube is None:
            good = xyz_t[torch.isfinite(xyz_t).all(dim=1)]
            if good.shape[0] == 0:
                lo = hi = np.zeros(3, np.float32)
            else:
                lo, hi = good.min(dim=0).values.cpu().numpy(), good.max(dim=0).values.cpu().numpy()
            pad = np.float32(max(float((hi - lo).max()), 0.0) / 4096.0) or np.float32(0.5)
            cube = points_bounds_to_cube(lo - pad, hi + pad)
        fmt, basis = parse_data_format(data_format)
        p = PointsParams(_f3(cube[0]), _f3(cube[1]), int(depth), fmt, basis, int(min_points), float(sigma))
        h, st = C.c_void_p(), PointsStats()
        _check(lib().mnv_n3tree_from_points(C.byref(p), xyz_t.data_ptr() if n else None, rgb_t.data_ptr() if n else None, n, C.c_void_p(stream), C.byref(st),
                                            C.byref(h)))
        out = cls(h.value)
        return (out, st) if return_stats else out

    def host_view(self) -> TreeView:
        v = TreeView()
        _check(lib().mnv_n3tree_host_view(self._h, C.byref(v)))
        return v

    def device_view(self) -> TreeView:
        v = TreeView()
        _check(lib().mnv_n3tree_device_view(self._h, C.byref(v)))
        return v

    def host_arrays(self):
        """(data uint16 [cap,8,data_dim], child int32 [cap,8], parent int32 [cap]) views of the C++ arrays."""
        v = self.host_view()
        cap, dd = v.capacity, v.data_dim
        data = np.ctypeslib.as_array(C.cast(v.data, C.POINTER(C.c_uint16)), shape=(cap, 8, dd))
        child = np.ctypeslib.as_array(C.cast(v.child, C.POINTER(C.c_int32)), shape=(cap, 8))
        parent = np.ctypeslib.as_array(C.cast(v.parent, C.POINTER(C.c_int32)), shape=(cap,))
        return data, child, parent

    @property
    def capacity(self) -> int:
        return self.host_view().capacity

    @property
    def data_format(self) -> str:
        v = self.host_view()
        return data_format_to_string(v.format, v.basis_dim)

    def move_to_device(self, max_capacity: int = 0, need_parent=False, need_sample_counts=False, stream: int = 0):
        _check(lib().mnv_n3tree_move_to_device(self._h, max_capacity, int(need_parent), int(need_sample_counts), C.c_void_p(stream)))
        return self

    @property
    def accel(self) -> int:
        a = lib().mnv_n3tree_accel(self._h)
        if not a:
            raise MnvError(MNV_E_INVALID, "tree has no accel (call move_to_device first)")
        return a

    def save_npz(self, path: str) -> None:
        _check(lib().mnv_n3tree_save_npz(self._h, os.fsencode(path)))

    def make_lod(self, depth: int) -> "N3Tree":
        """N3Tree::make_lod: a new tree on the device (with its accel where this one has one) whose interior rows are mipped from their
        children and which is cut at `depth` (the root chunk's voxels have depth 1); its host arrays are filled.  Needs move_to_device."""
        h = C.c_void_p()
        _check(lib().mnv_n3tree_make_lod(self._h, int(depth), C.byref(h)))
        return N3Tree(h.value)

    def make_view_lod(self, views, pixels: float, min_depth: int = 1, max_depth: int = 23, return_counts: bool = False):
        """N3Tree::make_view_lod: a new tree on the device, as make_lod's, cut where `views` -- a sequence of ((x, y, z), focal_px):
        world-space eyes and focal lengths in pixels -- say so: a voxel's children stay when the voxel could cover `pixels` pixels from
        one of the eyes; nothing is cut above min_depth, nothing kept below max_depth.  return_counts: also the kept chunks per depth
        (int64 [24]).  Needs move_to_device."""
        table = lod_views(views)
        h, kept = C.c_void_p(), np.zeros(24, np.int64)
        _check(lib().mnv_n3tree_make_view_lod(self._h, table.ctypes.data, int(table.shape[0]), float(pixels), int(min_depth), int(max_depth),
                                              kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(h)))
        out = N3Tree(h.value)
        return (out, kept) if return_counts else out

    def merge(self, other: "N3Tree", level: int = 0, corner=(0, 0, 0), mode="over", return_stats: bool = False):
        """N3Tree::merge: a new tree on the device, as make_lod's, that is this tree with `other` placed into its depth-`level` voxel with
        integer corner `corner` (include/mnv.h, "merging two trees"): the union of the two structures in canonical breadth-first order;
        mode "over": where `other` holds density its row; "add": where both do, the density-weighted blend.  Both trees need
        move_to_device; neither is changed.  return_stats: also the MergeStats."""
        p = merge_params(level, corner, mode)
        h, st = C.c_void_p(), MergeStats()
        _check(lib().mnv_n3tree_merge(self._h, other._h, C.byref(p), C.byref(st), C.byref(h)))
        out = N3Tree(h.value)
        return (out, st) if return_stats else out

    def voxel_cube(self, level: int, corner):
        """N3Tree::voxel_cube: (offset, scale) a tile must be built with so that it merges into this tree at level : corner."""
        v = self.host_view()
        return tree_voxel_cube(tuple(v.offset), tuple(v.scale), level, corner)

    def make_culled(self, cams, opt: RenderOptions, weight_thresh: float = 0.0):
        """N3Tree::make_culled: a new tree on the device, as make_lod's, without what the pinhole frames of `cams` cannot see: leaves no ray
        of those frames weights above weight_thresh are emptied, chunks left all-empty collapse into an empty leaf (rays_visibility per
        camera, tree_cull, tree_cut).  -> (tree, kept_at_depth int64 [24], counts dict).  Needs move_to_device."""
        n = len(cams)
        if n < 1:
            raise MnvError(MNV_E_INVALID, "at least one camera")
        arr = (CameraStruct * n)(*[c.c for c in cams])
        h, kept, counts = C.c_void_p(), np.zeros(24, np.int64), CullCounts()
        _check(lib().mnv_n3tree_make_culled(self._h, arr, n, C.byref(opt), float(weight_thresh), kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(counts),
                                            C.byref(h)))
        return N3Tree(h.value), kept, counts.as_dict()

    @staticmethod
    def _fit_params_ex(iterations, lr_colour, lr_sigma, optimizer, batch_rays, tile, seed, betas, eps) -> "FitParamsEx":
        """mnv_fit_params_ex of fit's / fit_to's arguments; with optimizer "adam", rates given as None are ADAM_DEFAULTS'"""
        opts = {"sgd": FIT_SGD, "adam": FIT_ADAM}
        if optimizer not in opts:
            raise MnvError(MNV_E_INVALID, "optimizer is 'sgd' or 'adam'")
        if optimizer == "adam":
            lr_colour = ADAM_DEFAULTS["lr_colour"] if lr_colour is None else lr_colour
            lr_sigma = ADAM_DEFAULTS["lr_sigma"] if lr_sigma is None else lr_sigma
        if lr_colour is None or lr_sigma is None:
            raise MnvError(MNV_E_INVALID, "the SGD step needs lr_colour and lr_sigma")
        return FitParamsEx(int(iterations), opts[optimizer], float(lr_colour), float(lr_sigma), float(betas[0]), float(betas[1]), float(eps), int(batch_rays),
                           int(tile), int(seed))

    def fit(self, cams, targets, opt: RenderOptions, iterations: int, lr_colour: Optional[float] = None, lr_sigma: Optional[float] = None, *,
            optimizer: str = "sgd", batch_rays: int = 0, tile: int = 8, seed: int = 0, betas=ADAM_DEFAULTS["betas"], eps: float = ADAM_DEFAULTS["eps"],
            return_counts: bool = False):
        """N3Tree::fit / fit_ex: `iterations` gradient steps on this tree's rows (on the device) against `targets`, one float32 device
        tensor [height, width, 4] per camera of `cams` (alpha 0 excludes a pixel).  optimizer "sgd" (mnv_rows_sgd_step) or "adam"
        (mnv_rows_adam_step with betas / eps; rates left None are ADAM_DEFAULTS').  batch_rays 0: full batch; otherwise every step takes
        batch_rays rays drawn across all cameras in units of tile x tile pixels (RayBatcher with `seed`).  The accel is rebuilt and the host
        arrays are refreshed.  -> int64 [iterations]: se_q32 of each step's rays before its step; with return_counts (se_q32, n_rays)."""
        import torch

        n = len(cams)
        if n < 1 or len(targets) != n:
            raise MnvError(MNV_E_INVALID, "one target frame per camera, at least one camera")
        for c, t in zip(cams, targets):
            if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != c.width * c.height * 4:
                raise MnvError(MNV_E_INVALID, "a target must be a contiguous float32 device tensor [height, width, 4] of its camera's size")
        arr = (CameraStruct * n)(*[c.c for c in cams])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in targets])
        se = np.zeros(max(int(iterations), 0), np.int64)
        if optimizer == "sgd" and batch_rays == 0 and not return_counts and lr_colour is not None and lr_sigma is not None:
            p = FitParams(int(iterations), float(lr_colour), float(lr_sigma), 0)
            _check(lib().mnv_n3tree_fit(self._h, arr, n, ptrs, C.byref(opt), C.byref(p), se.ctypes.data))
            return se
        px = self._fit_params_ex(iterations, lr_colour, lr_sigma, optimizer, batch_rays, tile, seed, betas, eps)
        n_rays = np.zeros_like(se)
        _check(lib().mnv_n3tree_fit_ex(self._h, arr, n, ptrs, C.byref(opt), C.byref(px), se.ctypes.data, n_rays.ctypes.data))
        return (se, n_rays) if return_counts else se

    def fit_to(self, teacher: "N3Tree", cams, opt: RenderOptions, iterations: int, lr_colour: Optional[float] = None, lr_sigma: Optional[float] = None, *,
               optimizer: str = "sgd", batch_rays: int = 0, tile: int = 8, seed: int = 0, betas=ADAM_DEFAULTS["betas"], eps: float = ADAM_DEFAULTS["eps"],
               return_counts: bool = False):
        """N3Tree::fit_to / fit_to_ex: fit against the frames the accel march renders of `teacher` (on the device) at `cams`; as fit otherwise."""
        n = len(cams)
        if n < 1:
            raise MnvError(MNV_E_INVALID, "at least one camera")
        arr = (CameraStruct * n)(*[c.c for c in cams])
        se = np.zeros(max(int(iterations), 0), np.int64)
        if optimizer == "sgd" and batch_rays == 0 and not return_counts and lr_colour is not None and lr_sigma is not None:
            p = FitParams(int(iterations), float(lr_colour), float(lr_sigma), 0)
            _check(lib().mnv_n3tree_fit_to_tree(self._h, teacher._h, arr, n, C.byref(opt), C.byref(p), se.ctypes.data))
            return se
        px = self._fit_params_ex(iterations, lr_colour, lr_sigma, optimizer, batch_rays, tile, seed, betas, eps)
        n_rays = np.zeros_like(se)
        _check(lib().mnv_n3tree_fit_to_tree_ex(self._h, teacher._h, arr, n, C.byref(opt), C.byref(px), se.ctypes.data, n_rays.ctypes.data))
        return (se, n_rays) if return_counts else se

    def gen_wireframe(self, max_depth: int = 100000) -> np.ndarray:
        """N3Tree::gen_wireframe (n3tree.cpp:249-329) on the host arrays: float32 [n_vertices, 9] (position, colour, normal), 24 vertices
        (12 edges) per cube in the reference's order."""
        n = C.c_int64(0)
        _check(lib().mnv_n3tree_gen_wireframe(self._h, int(max_depth), None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        if n.value:
            _check(lib().mnv_n3tree_gen_wireframe(self._h, int(max_depth), out.ctypes.data, out.size, C.byref(n)))
        return out.reshape(-1, 9)


def _ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (or a raw int / None)."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _frame_inputs(tmax_px, rgba8_init, pixels: int):
    """mnv_frame_inputs of the reference's offscreen == false call shape, or None when neither array is given."""
    if tmax_px is None and rgba8_init is None:
        return None
    import torch

    if tmax_px is not None and (not tmax_px.is_cuda or not tmax_px.is_contiguous() or tmax_px.dtype != torch.float32 or tmax_px.numel() < pixels):
        raise MnvError(MNV_E_INVALID, f"tmax_px must be a contiguous float32 device tensor with at least {pixels} elements")
    _check_out("rgba8_init", rgba8_init, pixels, "u8")
    return FrameInputs(tmax_px.data_ptr() if tmax_px is not None else None, rgba8_init.data_ptr() if rgba8_init is not None else None)


def render_voxels(tree_view: TreeView, cam: Camera, opt: RenderOptions, tile=None, rgba=None, rgba8=None,
                  split_track=None, sample_track=None, visited=None, track_visit=False, stream: int = 0, tmax_px=None, rgba8_init=None,
                  table_min_rays: Optional[int] = None) -> None:
    """viewer::render_voxels on reference-layout device arrays (asynchronous on `stream`).  tmax_px / rgba8_init: the depth attachment and
    the image under the volume of the reference's offscreen == false call shape (indexed like the outputs; rgba8_init may be rgba8).
    table_min_rays (tests only): run the call on the test-hook build with its per-launch lookup table forced on (0) / off (-1) / from that
    many rays -- the shipped library has no such switch (65536 rays)."""
    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    h = lib()
    if table_min_rays is not None:
        h = hooks_lib()
        h.mnv_hook_set_ref_table_min_rays(int(table_min_rays))
    inputs = _frame_inputs(tmax_px, rgba8_init, tile[2] * tile[3])
    try:
        with _timed(stream):
            if inputs is not None:
                _check(h.mnv_render_voxels_ex(C.byref(tree_view), C.byref(cam.c), C.byref(opt), Rect(*tile), C.byref(inputs), _ptr(rgba), _ptr(rgba8),
                                              _ptr(split_track), _ptr(sample_track), _ptr(visited), int(track_visit), C.c_void_p(stream)), h)
            else:
                _check(h.mnv_render_voxels(C.byref(tree_view), C.byref(cam.c), C.byref(opt), Rect(*tile), _ptr(rgba), _ptr(rgba8),
                                           _ptr(split_track), _ptr(sample_track), _ptr(visited), int(track_visit), C.c_void_p(stream)), h)
    finally:
        if table_min_rays is not None:
            h.mnv_hook_set_ref_table_min_rays(1 << 16)


def accel_create(tree_view: TreeView, max_capacity: int = 0, stream: int = 0) -> int:
    """Packed accel of a device tree view with room for max_capacity chunks (0: the tree's capacity); free with accel_destroy."""
    h = C.c_void_p()
    _check(lib().mnv_accel_create_reserved(C.byref(tree_view), max(max_capacity, tree_view.capacity), C.c_void_p(stream), C.byref(h)))
    return h.value


def accel_rebuild(accel: int, tree_view: TreeView, stream: int = 0) -> None:
    """Rebuild the accel in place from the tree (after a prune renumbered the chunks)."""
    _check(lib().mnv_accel_rebuild(C.c_void_p(accel), C.byref(tree_view), C.c_void_p(stream)))


def accel_destroy(accel: int) -> None:
    _pinned_fused_kernel.pop(accel, None)
    lib().mnv_accel_destroy(C.c_void_p(accel))


def accel_refresh(accel: int, tree_view: TreeView, old_capacity: int, changed_nodes=None, stream: int = 0) -> None:
    """Patch the accel after chunks [old_capacity, tree_view.capacity) were appended and / or the rows of changed_nodes
    (device int32 [n][2]) were rewritten."""
    n = 0 if changed_nodes is None else int(changed_nodes.shape[0])
    _check(lib().mnv_accel_refresh(C.c_void_p(accel), C.byref(tree_view), old_capacity, _ptr(changed_nodes), n, C.c_void_p(stream)))


def _check_out(name: str, t, pixels: int, dtype_name: str) -> None:
    """An output tensor must be a contiguous device tensor of the right element type with room for `pixels` RGBA pixels: the library
    writes through the raw pointer."""
    if t is None or isinstance(t, int):
        return
    import torch

    want = torch.float32 if dtype_name == "f32" else torch.uint8
    if not t.is_cuda or not t.is_contiguous() or t.dtype != want or t.numel() < pixels * 4:
        raise MnvError(MNV_E_INVALID, f"{name} must be a contiguous {want} device tensor with at least {pixels} RGBA pixels "
                                      f"(got {tuple(t.shape)} {t.dtype}, device {t.device})")


def _pixels(tile, n_frames: int, part) -> int:
    """Pixels the launch may write: frames x tile; under a partition the rank's own macro tiles, or frames x j_max macro tiles for a batch."""
    _, _, w, h = tile
    if part is None or not (part[1] > 1 or (part[1] == 1 and part[2] > 0)):
        return n_frames * w * h
    rank, world, tw, th = part[:4]
    period = part[4] if len(part) > 4 else 0
    if n_frames == 1:
        return partition_local_tiles(tile, rank, world, tw, th, period) * tw * th
    j_max = max(partition_local_tiles(tile, r, world, tw, th, period) for r in range(world))
    return n_frames * j_max * tw * th


def _accel_frame(cam: Camera, tile, rgba, rgba8, tmax_px=None, rgba8_init=None, n_frames: int = 1, part=None):
    """What every wrapper of a packed-layout entry point derives first: the default tile (the camera's image), the output tensors checked
    against the pixels of the launch, and mnv_frame_inputs.  Returns (mnv_rect, inputs by reference or None)."""
    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    px = _pixels(tile, n_frames, part)
    _check_out("rgba", rgba, px, "f32")
    _check_out("rgba8", rgba8, px, "u8")
    inputs = _frame_inputs(tmax_px, rgba8_init, tile[2] * tile[3])
    return Rect(*tile), (C.byref(inputs) if inputs is not None else None)


def _march_accel(accel: int, cam: Camera, opt: RenderOptions, frame, rgba, rgba8, stream: int, split_track=None, sample_track=None, sample_counts=None,
                 visited=None, parent=None, part=None) -> None:
    """The launch behind render_voxels_accel[_track|_visit|_part]: the most general entry point of the whole-frame / the partitioned family,
    NULL for the extras a caller does not use.  frame: what _accel_frame returned."""
    rect, inputs = frame
    extras = (_ptr(rgba), _ptr(rgba8), _ptr(split_track), _ptr(sample_track), _ptr(sample_counts), _ptr(visited), _ptr(parent), C.c_void_p(stream))
    if part is None:
        _check(lib().mnv_render_voxels_accel_visit_ex(C.c_void_p(accel), C.byref(cam.c), C.byref(opt), rect, inputs, *extras))
        return
    if inputs is not None:
        raise MnvError(MNV_E_INVALID, "frame inputs are for whole-frame launches")
    _check(lib().mnv_render_voxels_accel_visit_part(C.c_void_p(accel), C.byref(cam.c), C.byref(opt), rect, Partition(*part), *extras))


def render_voxels_accel(accel: int, cam: Camera, opt: RenderOptions, tile=None, rgba=None, rgba8=None, stream: int = 0, tmax_px=None,
                        rgba8_init=None) -> None:
    """The tuned march on the packed layout (asynchronous on `stream`); tmax_px / rgba8_init as in render_voxels."""
    frame = _accel_frame(cam, tile, rgba, rgba8, tmax_px, rgba8_init)
    with _timed(stream):
        _march_accel(accel, cam, opt, frame, rgba, rgba8, stream)


def render_voxels_accel_track(accel: int, cam: Camera, opt: RenderOptions, tile=None, rgba=None, rgba8=None,
                              split_track=None, sample_track=None, sample_counts=None, stream: int = 0) -> None:
    """The tuned march with the refinement trackers (rows as render_voxels writes them)."""
    frame = _accel_frame(cam, tile, rgba, rgba8)
    with _timed(stream):
        _march_accel(accel, cam, opt, frame, rgba, rgba8, stream, split_track, sample_track, sample_counts)


def render_voxels_accel_visit(accel: int, cam: Camera, opt: RenderOptions, visited, parent, tile=None, rgba=None, rgba8=None, split_track=None,
                              sample_track=None, sample_counts=None, stream: int = 0, part=None, tmax_px=None, rgba8_init=None) -> None:
    """Tracker march on the packed accel that also leaves the reference's visit marks (march marks leaf chunks, closure adds ancestors).
    part = (rank, world, tile_w, tile_h[, root_period]): only that rank's macro tiles, pixels and tracker rows in compact tile order.
    tmax_px / rgba8_init: the reference's offscreen == false inputs (whole-frame launches only)."""
    frame = _accel_frame(cam, tile, rgba, rgba8, tmax_px, rgba8_init, part=part)
    _march_accel(accel, cam, opt, frame, rgba, rgba8, stream, split_track, sample_track, sample_counts, visited, parent, part)


def get_samples_from_voxels_accel_visit(accel: int, cam: Camera, opt: RenderOptions, visited, parent, num_samples, samples, cluster_indices,
                                        grid: ClusterGrid, split_track=None, sample_track=None, sample_counts=None, tile=None, stream: int = 0,
                                        tmax_px=None) -> None:
    """tmax_px: the depth attachment of the reference's offscreen == false call (every ray stops there), indexed like the pixels."""
    rect, inputs = _accel_frame(cam, tile, None, None, tmax_px)
    _check(lib().mnv_get_samples_from_voxels_accel_visit_ex(C.c_void_p(accel), C.byref(cam.c), C.byref(opt), rect, inputs, _ptr(split_track),
                                                            _ptr(sample_track), _ptr(sample_counts), _ptr(visited), _ptr(parent), _ptr(num_samples),
                                                            _ptr(samples), int(samples.shape[-1]), _ptr(cluster_indices), C.byref(grid),
                                                            C.c_void_p(stream)))


def accel_set_colour_math(accel: int, mode: int) -> None:
    """Colour math of ONE accel: 0 exact (bit-identical to the oracle, the default), 1 hardware exp2 / rcp in the colour sigmoid (colours move
    ~1e-7).  There is no process-wide switch."""
    _check(lib().mnv_accel_set_colour_math(C.c_void_p(accel), int(mode)))


# The C library holds the choice of the fused guided-sampling kernel and its diagnostics buffer PER ACCEL (mnv_accel_set_fused_kernel /
# mnv_accel_set_fused_diag).  The two module-level setters below are a convenience of this harness for tests and tools whose trees are
# created deep inside helpers: render_guided_fused* (and Renderer.render) hand the harness's current choice to the accel they launch on,
# unless accel_set_fused_kernel pinned that accel.
_harness_fused_kernel: Optional[int] = None
_harness_fused_diag = None
_harness_diag_used = False
_pinned_fused_kernel: dict = {}


def accel_set_fused_kernel(accel: int, version: int) -> None:
    """Fused guided-sampling kernel of ONE accel: 0 = by network size (default), 1 = one-role wavefronts, 2 = producer / consumer wavefronts;
    negative = un-pin (the harness default of set_fused_kernel applies again)."""
    if version < 0:
        _pinned_fused_kernel.pop(accel, None)
        _check(lib().mnv_accel_set_fused_kernel(C.c_void_p(accel), int(_harness_fused_kernel or 0)))
    else:
        _pinned_fused_kernel[accel] = int(version)
        _check(lib().mnv_accel_set_fused_kernel(C.c_void_p(accel), int(version)))


def accel_set_fused_diag(accel: int, words32=None) -> None:
    """Diagnostics buffer of the fused kernels on ONE accel: a device int64 tensor of at least 32 words, or None.  The library keeps only the
    address: the caller keeps the tensor alive while it is set."""
    if words32 is not None and words32.numel() < 32:
        raise ValueError("the diagnostics buffer holds 32 words")
    _check(lib().mnv_accel_set_fused_diag(C.c_void_p(accel), _ptr(words32)))


def set_fused_kernel(version: int) -> None:
    """Harness default for the accels render_guided_fused* launch on (see above): 0 = by network size, 1, 2."""
    global _harness_fused_kernel
    _harness_fused_kernel = int(version) if version in (1, 2) else None


def set_fused_diag(words32=None) -> None:
    """Harness default: the diagnostics buffer handed to every accel render_guided_fused* launches on from now on (None: none).  The tensor
    is held here, so that a caller that drops its own reference cannot leave the kernels adding into freed memory."""
    global _harness_fused_diag, _harness_diag_used
    if words32 is not None and words32.numel() < 32:
        raise ValueError("the diagnostics buffer holds 32 words")
    _harness_fused_diag = words32
    _harness_diag_used = True


def _fused_defaults(accel: int) -> None:
    if accel not in _pinned_fused_kernel and (_harness_fused_kernel is not None or _harness_diag_used):
        _check(lib().mnv_accel_set_fused_kernel(C.c_void_p(accel), int(_harness_fused_kernel or 0)))
    if _harness_diag_used:
        _check(lib().mnv_accel_set_fused_diag(C.c_void_p(accel), _ptr(_harness_fused_diag)))


def accel_fused_faults(accel: int) -> int:
    """Spin-waits of the producer / consumer kernel that its watchdog abandoned since the accel was created (0 on a healthy build);
    waits for the device."""
    n = C.c_uint32(0)
    _check(lib().mnv_accel_fused_faults(C.c_void_p(accel), C.byref(n)))
    return int(n.value)


def set_tree_cache(enable: bool) -> None:
    """render_voxels (reference layout) keeps the packed re-layout of every tree it has seen (include/mnv.h: mnv_set_tree_cache);
    after editing a tree's arrays in place call tree_invalidate()."""
    lib().mnv_set_tree_cache(1 if enable else 0)


def tree_invalidate(child=None) -> None:
    """Forget the cached re-layout of the tree whose `child` array is this device tensor / address (None: all of them)."""
    if child is None:
        lib().mnv_tree_invalidate(None)
    else:
        lib().mnv_tree_invalidate(C.c_void_p(child if isinstance(child, int) else child.data_ptr()))


def assemble_tiles(gathered, frames, width: int, height: int, world: int, tile_w: int, tile_h: int, n_frames: int = 1, stream: int = 0,
                   root_period: int = 0) -> None:
    """Rank 0's un-permute of the gathered tile buffers into frames (device tensors, RGBA8 or float RGBA)."""
    bpp = gathered.element_size() * 4
    _check(lib().mnv_assemble_tiles(_ptr(gathered), _ptr(frames), width, height, Partition(0, world, tile_w, tile_h, root_period), n_frames, bpp,
                                    C.c_void_p(stream)))


def partition_local_tiles(tile, rank: int, world: int, tile_w: int, tile_h: int, root_period: int = 0) -> int:
    return int(lib().mnv_partition_local_tiles(Rect(*tile), Partition(rank, world, tile_w, tile_h, root_period)))


def render_voxels_accel_part(accel: int, cam: Camera, opt: RenderOptions, rank: int, world: int, tile_w: int, tile_h: int,
                             tile=None, rgba=None, rgba8=None, stream: int = 0, root_period: int = 0) -> None:
    """Render the macro tiles of `rank` (m % world == rank, or the root-relieving deal of mnv_partition.root_period) of `tile` into a
    compact local-tile-major buffer [local_tiles][tile_h][tile_w][4] (see mnv_partition in include/mnv.h)."""
    part = (rank, world, tile_w, tile_h, root_period)
    frame = _accel_frame(cam, tile, rgba, rgba8, part=part)
    with _timed(stream):
        _march_accel(accel, cam, opt, frame, rgba, rgba8, stream, part=part)


def get_samples_from_voxels(tree_view: TreeView, cam: Camera, opt: RenderOptions, num_samples, samples, cluster_indices,
                            grid: ClusterGrid, split_track=None, sample_track=None, visited=None, track_visit=False,
                            tile=None, stream: int = 0, tmax_px=None) -> None:
    """viewer::get_samples_from_voxels (reference include/cuda/renderer_kernel.hpp:36-52).  tmax_px: the depth attachment of its
    offscreen == false call (renderer_kernel.cu:354-357), a float32 device tensor indexed like the pixels."""
    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    inputs = _frame_inputs(tmax_px, None, tile[2] * tile[3])
    if inputs is not None:
        _check(lib().mnv_get_samples_from_voxels_ex(C.byref(tree_view), C.byref(cam.c), C.byref(opt), Rect(*tile), C.byref(inputs), _ptr(split_track),
                                                    _ptr(sample_track), _ptr(visited), int(track_visit), _ptr(num_samples), _ptr(samples),
                                                    int(samples.shape[-1]), _ptr(cluster_indices), C.byref(grid), C.c_void_p(stream)))
        return
    _check(lib().mnv_get_samples_from_voxels(C.byref(tree_view), C.byref(cam.c), C.byref(opt), Rect(*tile), _ptr(split_track),
                                             _ptr(sample_track), _ptr(visited), int(track_visit), _ptr(num_samples), _ptr(samples),
                                             int(samples.shape[-1]), _ptr(cluster_indices), C.byref(grid), C.c_void_p(stream)))


def get_samples_from_voxels_accel(accel: int, cam: Camera, opt: RenderOptions, num_samples, samples, cluster_indices, grid: ClusterGrid,
                                  split_track=None, sample_track=None, sample_counts=None, tile=None, stream: int = 0, tmax_px=None) -> None:
    """get_samples_from_voxels on the packed accel (no visit marks)."""
    get_samples_from_voxels_accel_visit(accel, cam, opt, None, None, num_samples, samples, cluster_indices, grid, split_track, sample_track,
                                        sample_counts, tile, stream, tmax_px)


def render_nerf_results(tree_view: TreeView, cam: Camera, opt: RenderOptions, sample_values, z_vals, offsets, rgba=None,
                        rgba8=None, tile=None, stream: int = 0) -> None:
    """viewer::render_nerf_results (reference include/cuda/renderer_kernel.hpp:12-21)."""
    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    _check(lib().mnv_render_nerf_results(C.byref(tree_view), C.byref(cam.c), C.byref(opt), Rect(*tile), _ptr(sample_values),
                                         int(sample_values.shape[-1]), _ptr(z_vals), _ptr(offsets), _ptr(rgba), _ptr(rgba8),
                                         C.c_void_p(stream)))


def render_guided_fused(accel: int, cam: Camera, opt: RenderOptions, mlp: "Mlp", grid: ClusterGrid, tile=None, rgba=None, rgba8=None,
                        sample_counter=None, split_track=None, sample_track=None, sample_counts=None, visited=None, parent=None,
                        stream: int = 0, tmax_px=None) -> None:
    """The guided-sampling frame as one kernel (mnv_render_guided_fused[_track]).  `sample_counter`: optional device int64 tensor,
    incremented by the number of network evaluations; trackers / visit marks as in render_voxels_accel_visit.  tmax_px: the depth
    attachment of the reference's offscreen == false frame (the image under the volume has weight 0 in that frame: not an input)."""
    rect, inputs = _accel_frame(cam, tile, rgba, rgba8, tmax_px)
    _fused_defaults(accel)
    _check(lib().mnv_render_guided_fused_track_ex(C.c_void_p(accel), C.byref(cam.c), C.byref(opt), rect, inputs, mlp._h, C.byref(grid), _ptr(rgba),
                                                  _ptr(rgba8), _ptr(split_track), _ptr(sample_track), _ptr(sample_counts), _ptr(visited), _ptr(parent),
                                                  _ptr(sample_counter), C.c_void_p(stream)))


def render_guided_fused_part(accel: int, cam: Camera, opt: RenderOptions, mlp: "Mlp", grid: ClusterGrid, part, tile=None, rgba=None, rgba8=None,
                             sample_counter=None, stream: int = 0, split_track=None, sample_track=None, sample_counts=None, visited=None,
                             parent=None) -> None:
    """One rank's macro tiles of the fused guided-sampling frame (part = (rank, world, tile_w, tile_h[, root_period])); with trackers /
    visit marks: mnv_render_guided_fused_track_part (rows in the compact tile order of the pixels)."""
    rect, _ = _accel_frame(cam, tile, rgba, rgba8, part=part)
    _fused_defaults(accel)
    _check(lib().mnv_render_guided_fused_track_part(C.c_void_p(accel), C.byref(cam.c), C.byref(opt), rect, Partition(*part), mlp._h, C.byref(grid),
                                                    _ptr(rgba), _ptr(rgba8), _ptr(split_track), _ptr(sample_track), _ptr(sample_counts), _ptr(visited),
                                                    _ptr(parent), _ptr(sample_counter), C.c_void_p(stream)))


def tree_edit(child, parent, offset, scale, capacity: int) -> TreeEdit:
    e = TreeEdit()
    e.child, e.parent = _ptr(child), _ptr(parent)
    e.offset, e.scale = _f3(offset), _f3(scale)
    e.N, e.capacity = 2, capacity
    return e


def add_children_and_generate_samples(edit: TreeEdit, opt: RenderOptions, parent_nodes, samples, cluster_indices, visited,
                                      grid: ClusterGrid, stream: int = 0) -> None:
    _check(lib().mnv_add_children_and_generate_samples(C.byref(edit), C.byref(opt), _ptr(parent_nodes), int(parent_nodes.shape[0]),
                                                       _ptr(samples), int(samples.shape[-1]), _ptr(cluster_indices), _ptr(visited),
                                                       C.byref(grid), C.c_void_p(stream)))


def generate_samples(edit: TreeEdit, opt: RenderOptions, nodes, samples, cluster_indices, grid: ClusterGrid, stream: int = 0) -> None:
    _check(lib().mnv_generate_samples(C.byref(edit), C.byref(opt), _ptr(nodes), int(nodes.shape[0]), _ptr(samples),
                                      int(samples.shape[-1]), _ptr(cluster_indices), C.byref(grid), C.c_void_p(stream)))


def adjust_parents_and_children(edit: TreeEdit, first_shift_index: int, to_delete, index_shifts, stream: int = 0) -> None:
    _check(lib().mnv_adjust_parents_and_children(C.byref(edit), first_shift_index, _ptr(to_delete), _ptr(index_shifts), C.c_void_p(stream)))


def select_split_candidates(split_track, max_out: int, nodes_out, stream: int = 0):
    """expand_voxels' vote on a [n][3] device tracker -> (pairs written to nodes_out, qualifying candidates)."""
    n_out, n_cand = C.c_int32(0), C.c_int32(0)
    _check(lib().mnv_select_split_candidates(_ptr(split_track), split_track.numel() // 3, max_out, _ptr(nodes_out), C.byref(n_out),
                                             C.byref(n_cand), C.c_void_p(stream)))
    return n_out.value, n_cand.value


def select_sample_candidates(sample_track, max_out: int, nodes_out, stream: int = 0):
    n_out, n_cand = C.c_int32(0), C.c_int32(0)
    _check(lib().mnv_select_sample_candidates(_ptr(sample_track), sample_track.numel() // 3, max_out, _ptr(nodes_out), C.byref(n_out),
                                              C.byref(n_cand), C.c_void_p(stream)))
    return n_out.value, n_cand.value


def apply_split_results(data, sample_counts, capacity: int, num_parents: int, results, samples_per_corner: int, data_dim: int,
                        stream: int = 0) -> None:
    _check(lib().mnv_apply_split_results(_ptr(data), _ptr(sample_counts), capacity, num_parents, _ptr(results), results.shape[-1],
                                         samples_per_corner, data_dim, C.c_void_p(stream)))


def apply_sample_results(data, sample_counts, nodes, results, samples_per_corner: int, data_dim: int, stream: int = 0) -> None:
    _check(lib().mnv_apply_sample_results(_ptr(data), _ptr(sample_counts), _ptr(nodes), nodes.shape[0], _ptr(results), results.shape[-1],
                                          samples_per_corner, data_dim, C.c_void_p(stream)))


def prune_tree(edit: TreeEdit, data, data_dim: int, sample_counts, visited, max_capacity: int, stream: int = 0, accel: int = 0):
    """-> (new_capacity, num_deleted).  `accel`: the tree's packed accel follows the prune in place (mnv_prune_tree_accel)."""
    new_cap, n_del = C.c_int32(0), C.c_int32(0)
    _check(lib().mnv_prune_tree_accel(C.byref(edit), _ptr(data), data_dim, _ptr(sample_counts), _ptr(visited), max_capacity,
                                      C.c_void_p(accel) if accel else None, C.byref(new_cap), C.byref(n_del), C.c_void_p(stream)))
    return new_cap.value, n_del.value


def mlp_desc(n_clusters=1, pos_octaves=4, dir_octaves=2, need_viewdir=False, n_embeddings=0, embedding_dim=0, hidden_width=64,
             hidden_layers=2, out_dim=5, center=(0.0, 0.0, 0.0), inv_extent=(1.0, 1.0, 1.0)) -> MlpDesc:
    d = MlpDesc(n_clusters, pos_octaves, dir_octaves, int(need_viewdir), n_embeddings, embedding_dim, hidden_width, hidden_layers, out_dim)
    d.center, d.inv_extent = _f3(center), _f3(inv_extent)
    return d


class Mlp:
    """Per-sample sub-module network (include/mnv.h: mnv_mlp_*).  `params`: numpy float16/uint16
    [n_clusters * param_count], cluster-major, in the order documented in the header."""

    def __init__(self, desc: MlpDesc, params, stream: int = 0):
        self.desc = desc
        p = np.ascontiguousarray(params).view(np.uint16).reshape(-1)
        h = C.c_void_p()
        _check(lib().mnv_mlp_create(C.byref(desc), p.ctypes.data, p.size, C.c_void_p(stream), C.byref(h)))
        self._h = h

    @staticmethod
    def param_count(desc: MlpDesc) -> int:
        return int(lib().mnv_mlp_param_count(C.byref(desc)))

    def query(self, cluster_indices, samples, results, n=None, stream: int = 0) -> None:
        """cluster_indices int16 [n], samples float32 [n][cols], results float32 [n][>= out_dim] (device tensors)."""
        n = int(samples.shape[0]) if n is None else n
        _check(lib().mnv_query_submodules(self._h, _ptr(cluster_indices), _ptr(samples), samples.stride(0), n, _ptr(results),
                                          results.stride(0), C.c_void_p(stream)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mnv_mlp_destroy(self._h)
                self._h = None
        except Exception:  # interpreter shutdown: module globals may be gone
            pass


def fill_uniform(out, seed: int, stream: int = 0) -> None:
    _check(lib().mnv_fill_uniform(_ptr(out), out.numel(), seed & 0xFFFFFFFFFFFFFFFF, C.c_void_p(stream)))


def compact_guided_samples(num_samples, samples, cluster_indices, offsets, z_vals=None, rows=None, clusters=None, stream: int = 0) -> int:
    """cumsum + packing of the emitted guided samples; returns the total.  With the outputs None only `offsets` is filled."""
    n_rays, max_g, dim = samples.shape
    total = C.c_int64(0)
    _check(lib().mnv_compact_guided_samples(_ptr(num_samples), _ptr(samples), _ptr(cluster_indices), n_rays, max_g, dim, _ptr(offsets),
                                            _ptr(z_vals), _ptr(rows), _ptr(clusters), 0 if z_vals is None else z_vals.shape[0],
                                            C.byref(total), C.c_void_p(stream)))
    return total.value


class Renderer:
    """viewer::VolumeRenderer behind the C ABI (mnv_renderer_*): owns camera + options + stream, runs the
    refinement loop when a model is set."""

    def __init__(self):
        h = C.c_void_p()
        _check(lib().mnv_renderer_create(C.byref(h)))
        self._h = h
        self._tree = None
        self.width = self.height = 0

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mnv_renderer_destroy(self._h)
                self._h = None
        except Exception:  # interpreter shutdown: module globals may be gone
            pass

    @property
    def options(self) -> RenderOptions:
        return lib().mnv_renderer_options(self._h).contents

    def set(self, tree: "N3Tree", max_tree_capacity: int) -> None:
        _check(lib().mnv_renderer_set(self._h, tree._h, max_tree_capacity))
        self._tree = tree  # keep alive

    def load_model(self, path: str) -> None:
        _check(lib().mnv_renderer_load_model(self._h, os.fsencode(path)))

    def set_model(self, desc: MlpDesc, params, grid: ClusterGrid) -> None:
        p = np.ascontiguousarray(params).view(np.uint16).reshape(-1)
        _check(lib().mnv_renderer_set_model(self._h, C.byref(desc), p.ctypes.data, p.size, C.byref(grid)))

    def resize(self, width: int, height: int) -> None:
        _check(lib().mnv_renderer_resize(self._h, width, height))
        if (width, height) != (self.width, self.height) and self.width:   # the renderer dropped a target of the old size
            self._target, self._slot_targets = None, {}
        self.width, self.height = width, height

    def set_camera(self, center, back, up=(0.0, 0.0, 1.0), fx: float = -1.0, fy: float = -1.0) -> None:
        _check(lib().mnv_renderer_set_camera(self._h, fx, fy, _f3(center), _f3(back), _f3(up)))

    def set_seed(self, seed: int, accel_rebuild_after: int = -1) -> None:
        _check(lib().mnv_renderer_set_seed(self._h, seed, accel_rebuild_after))

    def render(self) -> dict:
        st = RendererStats()
        if self._tree is not None and (_harness_fused_kernel is not None or _harness_diag_used):
            a = lib().mnv_n3tree_accel(self._tree._h)
            if a:
                _fused_defaults(a)
        _check(lib().mnv_renderer_render(self._h, C.byref(st)))
        if getattr(self, "_target", None) is not None:   # the frame's slot reads this tensor until it is collected
            self._slot_targets[self.last_slot()] = self._target
        return st.as_dict()

    def download(self, want_rgba8=False):
        rgba = np.empty((self.height, self.width, 4), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        _check(lib().mnv_renderer_download(self._h, rgba.ctypes.data, rgba8.ctypes.data if want_rgba8 else None))
        return (rgba, rgba8) if want_rgba8 else rgba

    def sync_tree(self) -> None:
        _check(lib().mnv_renderer_sync_tree(self._h))

    def set_frames_in_flight(self, count: int) -> None:
        _check(lib().mnv_renderer_set_frames_in_flight(self._h, int(count)))

    def set_guided_in_flight(self, on: bool) -> None:
        """Guided-sampling frames that change nothing rotate over the frame slots like plain frames (default off); their sample count:
        slot_guided_samples(last_slot())."""
        _check(lib().mnv_renderer_set_guided_in_flight(self._h, 1 if on else 0))

    def slot_guided_samples(self, slot: int) -> int:
        n = C.c_int64(0)
        _check(lib().mnv_renderer_slot_guided_samples(self._h, int(slot), C.byref(n)))
        return int(n.value)

    def set_fused_guided(self, enable: bool) -> None:
        _check(lib().mnv_renderer_set_fused_guided(self._h, int(enable)))

    def set_frame_inputs(self, tmax_px=None, rgba8_init=None) -> None:
        """The depth image ([height][width] float32) and the image under the volume ([height][width][4] uint8) of the reference's
        offscreen == false frames: device tensors the caller keeps alive while frames are rendered; None, None = the offline renderer."""
        px = self.width * self.height
        inputs = _frame_inputs(tmax_px, rgba8_init, px)
        self._inputs = (tmax_px, rgba8_init)  # keep the tensors alive
        _check(lib().mnv_renderer_set_frame_inputs(self._h, C.c_void_p(inputs.tmax_px if inputs is not None else None),
                                                   C.c_void_p(inputs.rgba8_init if inputs is not None else None)))

    def set_ranks(self, comm, tile_w: int = 64, tile_h: int = 24) -> None:
        """Several ranks refine one scene in lock step (VolumeRenderer::set_ranks); comm: mnv.Comm or None."""
        self._comm = comm  # keep the communicator alive as long as the renderer uses it
        _check(lib().mnv_renderer_set_ranks(self._h, C.c_void_p(comm.handle) if comm is not None else None, int(tile_w), int(tile_h)))

    def last_slot(self) -> int:
        return int(lib().mnv_renderer_last_slot(self._h))

    def last_camera(self) -> CameraStruct:
        """The camera (matrix and intrinsics) the last render() used."""
        c = CameraStruct()
        _check(lib().mnv_renderer_camera(self._h, C.byref(c)))
        return c

    def set_antialiasing(self, samples: int, filter: int = 1) -> None:
        """VolumeRenderer::aa_samples / aa_filter (AA_BOX / AA_TENT): samples > 1 renders that many jittered sub-frames per frame in one
        launch and resolves them on the device; 1 (the default) is the point-sampled frame, unchanged.  What render() refuses with
        samples > 1 (frame inputs, ranks, refinement, no packed accel, samples > MAX_BATCH) raises there, with MNV_E_INVALID."""
        _check(lib().mnv_renderer_set_antialiasing(self._h, int(samples), int(filter)))

    def set_projection(self, projection: int) -> None:
        """VolumeRenderer::projection (PROJ_PINHOLE / PROJ_ORTHO / PROJ_EQUIRECT): with another projection than the pinhole a frame generates
        its rays on the device and marches them as a ray list; PROJ_PINHOLE (the default) is the camera frame, unchanged.  What render()
        refuses with another projection (frame inputs, ranks, show_grid, a visible mesh, anti-aliasing, refinement, no packed accel)
        raises there, with MNV_E_INVALID."""
        _check(lib().mnv_renderer_set_projection(self._h, int(projection)))

    def set_lod(self, depth: int) -> None:
        """VolumeRenderer::set_lod: depth >= 1 has every frame march N3Tree.make_lod(depth) of the tree that was set (built at the first
        frame that needs it, one kept per depth); 0 (the default) is the full tree, unchanged.  What render() refuses with a level of
        detail (use_splitting, use_guided_sampling, ranks) raises there, with MNV_E_INVALID."""
        _check(lib().mnv_renderer_set_lod(self._h, int(depth)))

    def set_view_lod(self, views=(), pixels: float = 1.0, min_depth: int = 1, max_depth: int = 23) -> None:
        """VolumeRenderer::set_view_lod: every frame marches N3Tree.make_view_lod(views, pixels, min_depth, max_depth) of the tree that was
        set (built at the first frame that needs it, kept until the views or parameters change); an empty list (the default) is the full
        tree, unchanged.  What render() refuses with a view cut (use_splitting, use_guided_sampling, ranks, set_lod above 0) raises
        there, with MNV_E_INVALID."""
        table = lod_views(views)
        _check(lib().mnv_renderer_set_view_lod(self._h, table.ctypes.data if table.shape[0] else None, int(table.shape[0]), float(pixels),
                                               int(min_depth), int(max_depth)))

    def set_cull(self, cams=(), weight_thresh: float = 0.0) -> None:
        """VolumeRenderer::set_cull: every frame marches N3Tree.make_culled(cams, options, weight_thresh) of the tree that was set (built at
        the first frame that needs it, kept until the cameras, the threshold or the march options change); an empty list (the default)
        is the full tree, unchanged.  What render() refuses with a culled tree (use_splitting, use_guided_sampling, ranks, set_lod above
        0, set_view_lod) raises there, with MNV_E_INVALID."""
        cams = list(cams)
        arr = (CameraStruct * max(len(cams), 1))(*[c.c for c in cams])
        _check(lib().mnv_renderer_set_cull(self._h, arr if cams else None, len(cams), float(weight_thresh)))

    def set_lod_fit(self, cams=(), iterations: int = 0, lr_colour: Optional[float] = 0.0, lr_sigma: Optional[float] = 0.0, *, optimizer: str = "sgd",
                    batch_rays: int = 0, tile: int = 8, seed: int = 0, betas=ADAM_DEFAULTS["betas"], eps: float = ADAM_DEFAULTS["eps"]) -> None:
        """VolumeRenderer::set_lod_fit: every tree set_lod / set_view_lod builds from now on is fitted to the full tree at `cams`
        (N3Tree.fit_to, with its keywords) right after it is built; no camera or no iteration (the default) switches it off."""
        cams = list(cams)
        arr = (CameraStruct * max(len(cams), 1))(*[c.c for c in cams])
        if optimizer == "sgd" and batch_rays == 0:
            p = FitParams(int(iterations), float(lr_colour), float(lr_sigma), 0)
            _check(lib().mnv_renderer_set_lod_fit(self._h, arr if cams else None, len(cams), C.byref(p)))
            return
        px = N3Tree._fit_params_ex(iterations, lr_colour, lr_sigma, optimizer, batch_rays, tile, seed, betas, eps)
        _check(lib().mnv_renderer_set_lod_fit_ex(self._h, arr if cams else None, len(cams), C.byref(px)))

    def set_target(self, target=None, flags: int = 0) -> None:
        """VolumeRenderer::set_target: score every frame against `target`, a contiguous uint8 device tensor [height, width, 4], on the
        device (METRIC_QUANTISED / METRIC_MASK_ALPHA / METRIC_SSIM); metrics(slot) collects a frame's score.  The tensor may change per
        frame; this object keeps it alive (and the tensor of every slot's last frame).  None (the default): frames are not scored."""
        if target is None:
            self._target, self._slot_targets = None, {}
            _check(lib().mnv_renderer_set_target(self._h, None, 0))
            return
        import torch

        if not target.is_cuda or not target.is_contiguous() or target.dtype != torch.uint8 or target.numel() != self.width * self.height * 4:
            raise MnvError(MNV_E_INVALID, f"target must be a contiguous uint8 device tensor of {self.height} x {self.width} x 4 elements")
        _check(lib().mnv_renderer_set_target(self._h, C.c_void_p(target.data_ptr()), int(flags)))
        self._target = target
        if not hasattr(self, "_slot_targets"):
            self._slot_targets = {}

    def metrics(self, slot=None) -> dict:
        """mnv_renderer_slot_metrics: wait for the frame of `slot` (None: the last frame's) and return its score as a dict (mse, psnr, ssim,
        n_px, n_win); raises MnvError (MNV_E_INVALID) when that frame was not scored."""
        v = FrameMetricValues()
        _check(lib().mnv_renderer_slot_metrics(self._h, self.last_slot() if slot is None else int(slot), C.byref(v)))
        return v.as_dict()

    def add_mesh(self, mesh: "Mesh") -> None:
        """VolumeRenderer::meshes: while a listed mesh is visible every frame draws the list (over the grid, if show_grid is set) with
        mnv_render_meshes and marches with the two images as its frame inputs.  The Mesh stays the caller's; this object keeps it alive."""
        _check(lib().mnv_renderer_add_mesh(self._h, mesh._h))
        if not hasattr(self, "_meshes"):
            self._meshes = []
        self._meshes.append(mesh)

    def clear_meshes(self) -> None:
        _check(lib().mnv_renderer_clear_meshes(self._h))
        self._meshes = []

    @property
    def mesh_count(self) -> int:
        return int(lib().mnv_renderer_mesh_count(self._h))

    def wireframe(self) -> int:
        """Raw mnv_wireframe handle of the last show_grid frame (0 before the first); owned by the renderer."""
        return lib().mnv_renderer_wireframe(self._h) or 0

    def download_slot(self, slot: int, want_rgba8=False):
        rgba = np.empty((self.height, self.width, 4), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        _check(lib().mnv_renderer_download_slot(self._h, int(slot), rgba.ctypes.data, rgba8.ctypes.data if want_rgba8 else None))
        return (rgba, rgba8) if want_rgba8 else rgba


WIREFRAME_AUTO, WIREFRAME_BINNED, WIREFRAME_GLOBAL = 0, 1, 2


class Wireframe:
    """mnv_wireframe: the grid overlay's edge list on the device, built from a device tree view (N3Tree::gen_wireframe's cubes)."""

    def __init__(self, tree_view: TreeView, max_depth: int, stream: int = 0):
        h = C.c_void_p()
        _check(lib().mnv_wireframe_create(C.byref(tree_view), int(max_depth), C.c_void_p(stream), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mnv_wireframe_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self) -> int:
        return self._h.value

    def update(self, tree_view: TreeView, max_depth: int, stream: int = 0) -> None:
        _check(lib().mnv_wireframe_update(self._h, C.byref(tree_view), int(max_depth), C.c_void_p(stream)))

    def set_method(self, method: int) -> None:
        """WIREFRAME_AUTO / WIREFRAME_BINNED / WIREFRAME_GLOBAL: how mnv_render_wireframe resolves depth (same images either way)."""
        _check(lib().mnv_wireframe_set_method(self._h, int(method)))

    @property
    def cube_count(self) -> int:
        return int(lib().mnv_wireframe_cube_count(self._h))

    def segments(self, stream: int = 0):
        """float32 device tensor [n, 6]: the world endpoints (A, B) of every edge, 12 per cube in _push_wireframe_bb's order."""
        return wireframe_segments(self._h.value, stream)

    def render(self, cam: Camera, opt: RenderOptions, tile=None, tmax_px=None, rgba8=None, stream: int = 0):
        return render_wireframe(self._h.value, cam, opt, tile, tmax_px, rgba8, stream)


def wireframe_segments(wire: int, stream: int = 0):
    """mnv_wireframe_segments of a raw mnv_wireframe handle (e.g. Renderer.wireframe()) into a new float32 device tensor [n, 6]."""
    import torch

    n = C.c_int64(0)
    _check(lib().mnv_wireframe_segments(C.c_void_p(wire), None, 0, C.byref(n), C.c_void_p(stream)))
    out = torch.empty((n.value, 6), dtype=torch.float32, device="cuda")
    if n.value:
        _check(lib().mnv_wireframe_segments(C.c_void_p(wire), out.data_ptr(), n.value, C.byref(n), C.c_void_p(stream)))
    return out


def render_wireframe(wire: int, cam: Camera, opt: RenderOptions, tile=None, tmax_px=None, rgba8=None, stream: int = 0):
    """mnv_render_wireframe: the grid pass into (tmax_px float32 [h, w], rgba8 uint8 [h, w, 4]) device tensors (allocated when None);
    returns both."""
    import torch

    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    w, h = tile[2], tile[3]
    if tmax_px is None:
        tmax_px = torch.empty((h, w), dtype=torch.float32, device="cuda")
    if rgba8 is None:
        rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    if not tmax_px.is_cuda or not tmax_px.is_contiguous() or tmax_px.dtype != torch.float32 or tmax_px.numel() < w * h:
        raise MnvError(MNV_E_INVALID, f"tmax_px must be a contiguous float32 device tensor with at least {w * h} elements")
    _check_out("rgba8", rgba8, w * h, "u8")
    _check(lib().mnv_render_wireframe(C.c_void_p(wire), C.byref(cam.c), C.byref(opt), Rect(*tile), tmax_px.data_ptr(), rgba8.data_ptr(),
                                      C.c_void_p(stream)))
    return tmax_px, rgba8


def model_matrix(rotation=(0.0, 0.0, 0.0), translation=(0.0, 0.0, 0.0), scale: float = 1.0) -> np.ndarray:
    """mnv_model_matrix: the model matrix of the reference's Mesh::draw as float32 [3, 4] (axis-angle rotation, then scale, translation in
    the last column); host arithmetic, no GPU."""
    out = np.empty((3, 4), np.float32)
    _check(lib().mnv_model_matrix(_f3(rotation), _f3(translation), float(scale), out.ctypes.data))
    return out


def obj_read(path: str, color=None):
    """mnv_obj_read: (vert float32 [n, 9], faces uint32 [m, face_size] or None when non-indexed, face_size) of a Wavefront OBJ file, as
    viewer::Mesh::load_obj forms them; a malformed file raises MnvError (MNV_E_IO) naming the line."""
    nf, ni, fs = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    col = _f3(color) if color is not None else None
    _check(lib().mnv_obj_read(os.fsencode(path), col, None, 0, C.byref(nf), None, 0, C.byref(ni), C.byref(fs)))
    vert = np.empty(nf.value, np.float32)
    faces = np.empty(ni.value, np.uint32)
    _check(lib().mnv_obj_read(os.fsencode(path), col, vert.ctypes.data, vert.size, C.byref(nf), faces.ctypes.data, faces.size, C.byref(ni), C.byref(fs)))
    return vert.reshape(-1, 9), (faces.reshape(-1, fs.value) if ni.value else None), int(fs.value)


class Mesh:
    """mnv_mesh / viewer::Mesh: vertices float32 [n, 9] (position, colour, normal), optional indices [m, face_size], face_size 1 / 2 / 3
    (points, lines, triangles), lit or unlit, a model transform (axis-angle rotation, translation, scale) and a visibility flag."""

    def __init__(self, vert, faces=None, face_size: int = 3, unlit: bool = False):
        v = np.ascontiguousarray(vert, np.float32)
        if v.ndim != 2 or v.shape[1] != 9:
            raise MnvError(MNV_E_INVALID, "vert must be [n_verts, 9] (position, colour, normal)")
        f = None if faces is None else np.ascontiguousarray(faces, np.uint32).reshape(-1)
        h = C.c_void_p()
        _check(lib().mnv_mesh_create(v.ctypes.data if v.size else None, v.shape[0], f.ctypes.data if f is not None and f.size else None,
                                     0 if f is None else f.size, int(face_size), int(bool(unlit)), C.byref(h)))
        self._h = h

    @classmethod
    def from_obj(cls, path: str, color=None, unlit: bool = False) -> "Mesh":
        vert, faces, face_size = obj_read(path, color)
        return cls(vert, faces, face_size, unlit)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mnv_mesh_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self) -> int:
        return self._h.value

    def set_matrix(self, matrix) -> None:
        """The model matrix itself, float32 [3, 4] row-major (mnv_mesh_model_matrix)."""
        m = np.ascontiguousarray(matrix, np.float32)
        if m.shape != (3, 4):
            raise MnvError(MNV_E_INVALID, "the model matrix is [3, 4]")
        _check(lib().mnv_mesh_model_matrix(self._h, m.ctypes.data))

    def set_transform(self, rotation=(0.0, 0.0, 0.0), translation=(0.0, 0.0, 0.0), scale: float = 1.0) -> None:
        """The reference's Mesh::rotation (axis-angle) / translation / scale."""
        self.set_matrix(model_matrix(rotation, translation, scale))

    @property
    def visible(self) -> bool:
        return bool(lib().mnv_mesh_visible(self._h))

    @visible.setter
    def visible(self, on: bool) -> None:
        _check(lib().mnv_mesh_show(self._h, int(bool(on))))

    @property
    def vertex_count(self) -> int:
        return int(lib().mnv_mesh_vertex_count(self._h))

    @property
    def face_count(self) -> int:
        return int(lib().mnv_mesh_face_count(self._h))

    @property
    def face_size(self) -> int:
        return int(lib().mnv_mesh_face_size(self._h))


def render_meshes(meshes, cam: Camera, opt: RenderOptions, tile=None, under=None, tmax_px=None, rgba8=None, stream: int = 0):
    """mnv_render_meshes: the mesh pass into (tmax_px float32 [h, w], rgba8 uint8 [h, w, 4]) device tensors (allocated when None); returns
    both.  under: None (the images start cleared) or a (tmax_px, rgba8) pair of an earlier pass to draw over -- it may be the outputs."""
    import torch

    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    w, h = tile[2], tile[3]
    if tmax_px is None:
        tmax_px = torch.empty((h, w), dtype=torch.float32, device="cuda")
    if rgba8 is None:
        rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    if not tmax_px.is_cuda or not tmax_px.is_contiguous() or tmax_px.dtype != torch.float32 or tmax_px.numel() < w * h:
        raise MnvError(MNV_E_INVALID, f"tmax_px must be a contiguous float32 device tensor with at least {w * h} elements")
    _check_out("rgba8", rgba8, w * h, "u8")
    inputs = None
    if under is not None:
        inputs = _frame_inputs(under[0], under[1], w * h)
        if inputs is None:
            inputs = FrameInputs()
    handles = (C.c_void_p * max(len(meshes), 1))(*[m._h.value for m in meshes])
    _check(lib().mnv_render_meshes(handles, len(meshes), C.byref(cam.c), C.byref(opt), Rect(*tile), C.byref(inputs) if inputs is not None else None,
                                   tmax_px.data_ptr(), rgba8.data_ptr(), C.c_void_p(stream)))
    return tmax_px, rgba8


def obj_write(path: str, vert, faces=None, face_size: int = 3) -> None:
    """mnv_obj_write: vert float32 [n, 9] (position, colour, normal) and faces uint32 [m, face_size] (or None) as a Wavefront OBJ file whose
    floats obj_read returns bit for bit."""
    v = np.ascontiguousarray(vert, np.float32).reshape(-1, 9)
    f = None if faces is None else np.ascontiguousarray(faces, np.uint32).reshape(-1)
    _check(lib().mnv_obj_write(os.fsencode(path), v.ctypes.data if v.size else None, v.shape[0], f.ctypes.data if f is not None and f.size else None,
                               0 if f is None else f.size, int(face_size)))


def sample_points(accel: int, points, voxel: bool = True, depth: bool = True, sigma: bool = True, stream: int = 0):
    """mnv_accel_sample_points: the leaf under each world-space point of a float32 device tensor [n, 3].  Returns (voxel int32 [n], depth
    int32 [n], sigma float32 [n]) device tensors; an output that is switched off is None (and NULL in the call).  A point with a
    non-finite coordinate answers (-1, 0, 0)."""
    import torch

    if not points.is_cuda or points.dtype != torch.float32 or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3:
        raise MnvError(MNV_E_INVALID, "points must be a contiguous float32 device tensor [n, 3]")
    n = points.shape[0]
    vo = torch.empty(n, dtype=torch.int32, device="cuda") if voxel else None
    de = torch.empty(n, dtype=torch.int32, device="cuda") if depth else None
    sg = torch.empty(n, dtype=torch.float32, device="cuda") if sigma else None
    _check(lib().mnv_accel_sample_points(C.c_void_p(accel), points.data_ptr(), n, _ptr(vo), _ptr(de), _ptr(sg), C.c_void_p(stream)))
    return vo, de, sg


class Surface:
    """mnv_surface: an extracted iso-surface on the device (extract_surface)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mnv_surface_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def counts(self):
        nv, ni = C.c_int64(0), C.c_int64(0)
        _check(lib().mnv_surface_counts(self._h, C.byref(nv), C.byref(ni)))
        return nv.value, ni.value

    def stats(self) -> dict:
        st = SurfaceStats()
        _check(lib().mnv_surface_stats_get(self._h, C.byref(st)))
        return st.as_dict()

    def vertices(self) -> np.ndarray:
        """float32 [n_verts, 9] on the host: position, colour, normal"""
        nv, _ = self.counts()
        out = np.empty((nv, 9), np.float32)
        _check(lib().mnv_surface_download(self._h, out.ctypes.data if nv else None, out.size, None, 0))
        return out

    def faces(self) -> np.ndarray:
        """uint32 [n_triangles, 3] on the host"""
        _, ni = self.counts()
        out = np.empty((ni // 3, 3), np.uint32)
        _check(lib().mnv_surface_download(self._h, None, 0, out.ctypes.data if ni else None, out.size))
        return out

    def device_pointers(self):
        """(vertices, indices) device addresses of the surface's own arrays (0 when it is empty); they live as long as the surface"""
        v, f = C.c_void_p(), C.c_void_p()
        _check(lib().mnv_surface_device(self._h, C.byref(v), C.byref(f)))
        return v.value or 0, f.value or 0

    def to_mesh(self, unlit: bool = False) -> "Mesh":
        """A device-to-device copy as a Mesh that render_meshes and Renderer.add_mesh draw."""
        h = C.c_void_p()
        _check(lib().mnv_surface_to_mesh(self._h, int(bool(unlit)), C.byref(h)))
        m = Mesh.__new__(Mesh)
        m._h = h
        return m

    def save_obj(self, path: str) -> None:
        obj_write(path, self.vertices(), self.faces(), 3)


def extract_surface(accel: int, level: int, iso: float, colour: bool = True, all_bricks: bool = False, stream: int = 0) -> Surface:
    """mnv_extract_surface: the iso-surface of the density on a lattice of 2^level samples per axis (3 <= level <= 10) as an indexed
    triangle mesh with a normal and a colour per vertex; include/mnv.h states every value.  all_bricks switches the empty-space skip off
    (same bytes)."""
    p = ExtractParams(int(level), float(iso), (EXTRACT_COLOUR if colour else 0) | (EXTRACT_ALL_BRICKS if all_bricks else 0))
    h = C.c_void_p()
    _check(lib().mnv_extract_surface(C.c_void_p(accel), C.byref(p), C.c_void_p(stream), C.byref(h)))
    return Surface(h.value)


def tree_mip_rows(tree_view: TreeView, data_out, chunk_depth_out=None, stream: int = 0) -> np.ndarray:
    """mnv_tree_mip_rows: the rows of a device tree view with every interior row derived from the voxel's children, into data_out (int16 /
    uint16 / float16 device tensor [capacity, 8, data_dim]; never the tree's own array); chunk_depth_out: int32 device tensor [capacity]
    or None.  Returns chunks_at_depth, int64 [24] (entry d: chunks of depth d).  Waits for `stream`."""
    counts = np.zeros(24, np.int64)
    _check(lib().mnv_tree_mip_rows(C.byref(tree_view), _ptr(data_out), _ptr(chunk_depth_out), counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                   C.c_void_p(stream)))
    return counts


def tree_truncate(tree_view: TreeView, chunk_depth, max_depth: int, new_capacity: int, child_out, data_out, parent_out=None,
                  sample_counts_out=None, stream: int = 0) -> None:
    """mnv_tree_truncate (asynchronous on `stream`): the chunks of depth 1 .. max_depth of a device tree view, compacted in order, into
    device tensors of new_capacity chunks (child int32 [n, 8], data 16-bit [n, 8, data_dim], parent int32 [n] or None, sample counts int16
    [n, 8] or None); tree_view.data holds the rows to carry, chunk_depth is tree_mip_rows' array."""
    _check(lib().mnv_tree_truncate(C.byref(tree_view), _ptr(chunk_depth), int(max_depth), int(new_capacity), _ptr(child_out), _ptr(data_out),
                                   _ptr(parent_out), _ptr(sample_counts_out), C.c_void_p(stream)))


def lod_views(views) -> np.ndarray:
    """A sequence of ((x, y, z), focal_px) as the float32 [n, 4] array that is mnv_lod_view[n] (an [n, 4] array passes through)."""
    if isinstance(views, np.ndarray):
        return np.ascontiguousarray(views, np.float32).reshape(-1, 4)
    return np.array([[e[0], e[1], e[2], f] for e, f in views], np.float32).reshape(-1, 4)


def tree_select_cut(tree_view: TreeView, views, pixels: float, min_depth: int, max_depth: int, keep_out, stream: int = 0) -> np.ndarray:
    """mnv_tree_select_cut: which chunks of a device tree view are worth keeping for `views` (lod_views' forms) at `pixels`, into keep_out
    (uint8 device tensor [capacity]: 1 kept, 0 not).  Returns kept_at_depth, int64 [24].  Waits for `stream`."""
    table = lod_views(views)
    kept = np.zeros(24, np.int64)
    _check(lib().mnv_tree_select_cut(C.byref(tree_view), table.ctypes.data if table.shape[0] else None, int(table.shape[0]), float(pixels), int(min_depth),
                                     int(max_depth), _ptr(keep_out), kept.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(stream)))
    return kept


def tree_cut(tree_view: TreeView, keep, new_capacity: int, child_out, data_out, parent_out=None, sample_counts_out=None, stream: int = 0) -> None:
    """mnv_tree_cut (asynchronous on `stream`): the chunks with keep != 0 of a device tree view, compacted in order, into device tensors of
    new_capacity chunks, as tree_truncate's; `keep` (uint8 device tensor [capacity]) must be parent-closed (tree_select_cut's is)."""
    _check(lib().mnv_tree_cut(C.byref(tree_view), _ptr(keep), int(new_capacity), _ptr(child_out), _ptr(data_out), _ptr(parent_out),
                              _ptr(sample_counts_out), C.c_void_p(stream)))


def points_colour_table(data_format: str = "RGBA") -> np.ndarray:
    """mnv_points_colour_table: the binary16 bits an 8-bit colour mean becomes in a row of `data_format` (uint16 [256]); host only."""
    fmt, basis = parse_data_format(data_format)
    out = np.zeros(256, np.uint16)
    _check(lib().mnv_points_colour_table(fmt, basis, out.ctypes.data))
    return out


def points_bounds_to_cube(lo, hi):
    """mnv_points_bounds_to_cube: (offset float32 [3], scale float32 [3]) of the smallest cube around the box [lo, hi], centre at 0.5."""
    lo, hi = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32)
    offset, scale = np.zeros(3, np.float32), np.zeros(3, np.float32)
    _check(lib().mnv_points_bounds_to_cube(lo.ctypes.data, hi.ctypes.data, offset.ctypes.data, scale.ctypes.data))
    return offset, scale


class PointTree:
    """mnv_point_tree: points -> occupancy, structure, first colours (include/mnv.h, "a tree from a coloured point cloud").  add any number
    of times (float32 [n, 3] / uint8 [n, 3] device tensors), finish() -> PointsStats, then write() into device tensors of stats.capacity chunks."""

    def __init__(self, offset, scale, depth: int, sigma: float, min_points: int = 1, data_format: str = "RGBA"):
        fmt, basis = parse_data_format(data_format)
        self.params = PointsParams(_f3(offset), _f3(scale), int(depth), fmt, basis, int(min_points), float(sigma))
        self.data_dim = 4 if fmt == FORMAT_RGBA else 3 * basis + 1
        self._h = C.c_void_p()
        _check(lib().mnv_point_tree_create(C.byref(self.params), C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                lib().mnv_point_tree_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def add(self, xyz, rgb, n=None, stream: int = 0) -> None:
        n = int(xyz.shape[0]) if n is None else int(n)
        _check(lib().mnv_point_tree_add(self._h, _ptr(xyz), _ptr(rgb), n, C.c_void_p(stream)))

    def finish(self, stream: int = 0) -> PointsStats:
        st = PointsStats()
        _check(lib().mnv_point_tree_finish(self._h, C.byref(st), C.c_void_p(stream)))
        return st

    def write(self, child_out, data_out, parent_out=None, sample_counts_out=None, counts_out=None, stream: int = 0) -> None:
        _check(lib().mnv_point_tree_write(self._h, _ptr(child_out), _ptr(data_out), _ptr(parent_out), _ptr(sample_counts_out), _ptr(counts_out),
                                          C.c_void_p(stream)))


def merge_params(level: int = 0, corner=(0, 0, 0), mode="over") -> MergeParams:
    """mnv_merge_params of a placement level : corner and a mode ("over", "add", or MERGE_OVER / MERGE_ADD)."""
    if isinstance(mode, str):
        if mode not in ("over", "add"):
            raise MnvError(MNV_E_INVALID, "mode is 'over' or 'add'")
        mode = MERGE_ADD if mode == "add" else MERGE_OVER
    return MergeParams(int(level), (C.c_int32 * 3)(*[int(c) for c in corner]), int(mode), 0)


def tree_voxel_cube(offset, scale, level: int, corner):
    """mnv_tree_voxel_cube: (offset float32 [3], scale float32 [3]) of the depth-`level` voxel with integer corner `corner` of the cube
    (offset, scale): scale * 2^level and offset * 2^level - corner.  Host only."""
    o, s = np.ascontiguousarray(offset, np.float32), np.ascontiguousarray(scale, np.float32)
    c = np.ascontiguousarray(corner, np.int32)
    if o.shape != (3,) or s.shape != (3,) or c.shape != (3,):
        raise MnvError(MNV_E_INVALID, "offset, scale and corner have three entries")
    offset_out, scale_out = np.zeros(3, np.float32), np.zeros(3, np.float32)
    _check(lib().mnv_tree_voxel_cube(o.ctypes.data, s.ctypes.data, int(level), c.ctypes.data, offset_out.ctypes.data, scale_out.ctypes.data))
    return offset_out, scale_out


class TreeMerge:
    """mnv_tree_merge: the plan of merging device tree view `b` into `a` at level : corner (include/mnv.h, "merging two trees"); waits for
    `stream`.  stats (MergeStats) sizes the outputs: write() fills device tensors of stats.capacity chunks, any number of times.  The two
    views' arrays must stay alive and unchanged while the plan is used."""

    def __init__(self, a: TreeView, b: TreeView, level: int = 0, corner=(0, 0, 0), mode="over", stream: int = 0):
        self._h = C.c_void_p()
        self.params = merge_params(level, corner, mode)
        self.stats = MergeStats()
        self.data_dim = int(a.data_dim)
        _check(lib().mnv_tree_merge_plan(C.byref(a), C.byref(b), C.byref(self.params), C.byref(self._h), C.byref(self.stats), C.c_void_p(stream)))

    def __del__(self):
        try:
            if self._h:
                lib().mnv_tree_merge_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def write(self, child_out, data_out, parent_out=None, sample_counts_out=None, src_a_out=None, src_b_out=None, stream: int = 0) -> None:
        _check(lib().mnv_tree_merge_write(self._h, _ptr(child_out), _ptr(data_out), _ptr(parent_out), _ptr(sample_counts_out), _ptr(src_a_out),
                                          _ptr(src_b_out), C.c_void_p(stream)))


MAX_BATCH = 64
AA_BOX, AA_TENT = 0, 1


def aa_pattern(n: int) -> np.ndarray:
    """mnv_aa_pattern: float32 [n, 2] sub-pixel offsets (dx, dy) in [-0.5, 0.5); n == 1 is (0, 0), else the Halton (2, 3) points k + 1."""
    out = np.zeros((max(int(n), 0), 2), np.float32)
    _check(lib().mnv_aa_pattern(int(n), out.ctypes.data))
    return out


def aa_weights(filter: int, offsets) -> np.ndarray:
    """mnv_aa_weights: the filter table float32 [n, 2r + 1, 2r + 1] (weights[k, j + r, i + r], i along x) of AA_BOX (r = 0) or AA_TENT
    (r = 1) for the offsets of aa_pattern; the radius is weights.shape[1] // 2."""
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 2)
    r, n = C.c_int32(0), C.c_int64(0)
    _check(lib().mnv_aa_weights(int(filter), off.shape[0], off.ctypes.data, C.byref(r), None, 0, C.byref(n)))
    out = np.empty(n.value, np.float32)
    _check(lib().mnv_aa_weights(int(filter), off.shape[0], off.ctypes.data, C.byref(r), out.ctypes.data, out.size, C.byref(n)))
    d = 2 * r.value + 1
    return out.reshape(off.shape[0], d, d)


def resolve_samples(sub, weights, radius: int, rgba=None, rgba8=None, stream: int = 0) -> None:
    """mnv_resolve_samples (asynchronous on `stream`): sub float32 device tensor [n, h, w, 4], weights float32 device tensor
    [n, 2r + 1, 2r + 1] (a numpy table is copied to the device first), rgba float32 [h, w, 4] / rgba8 uint8 [h, w, 4] device tensors."""
    import torch

    if not sub.is_cuda or not sub.is_contiguous() or sub.dtype != torch.float32 or sub.dim() != 4 or sub.shape[3] != 4:
        raise MnvError(MNV_E_INVALID, "sub must be a contiguous float32 device tensor [n, height, width, 4]")
    n, h, w = int(sub.shape[0]), int(sub.shape[1]), int(sub.shape[2])
    if isinstance(weights, np.ndarray):
        weights = torch.from_numpy(np.ascontiguousarray(weights, np.float32)).to(sub.device)
    d = 2 * int(radius) + 1
    if not weights.is_cuda or not weights.is_contiguous() or weights.dtype != torch.float32 or weights.numel() < n * d * d:
        raise MnvError(MNV_E_INVALID, f"weights must be a contiguous float32 device tensor with at least {n * d * d} elements")
    _check_out("rgba", rgba, w * h, "f32")
    _check_out("rgba8", rgba8, w * h, "u8")
    with _timed(stream):
        _check(lib().mnv_resolve_samples(sub.data_ptr(), n, w, h, weights.data_ptr(), int(radius), _ptr(rgba), _ptr(rgba8), C.c_void_p(stream)))


METRIC_QUANTISED, METRIC_MASK_ALPHA, METRIC_SSIM = 1, 2, 4


def ssim_window() -> np.ndarray:
    """mnv_ssim_window: the standard SSIM window, float32 [11] (Gaussian, sigma 1.5, normalised in double, rounded to float)."""
    out = np.zeros(11, np.float32)
    _check(lib().mnv_ssim_window(out.ctypes.data))
    return out


def metrics_finish(sums) -> dict:
    """mnv_metrics_finish: (n_px, se_q32, n_win, ssim_q32[, reserved]) -- a MetricSums, a sequence or the int64 tensor frame_metrics
    returns -- to a dict of mse, psnr, ssim (Python floats; inf / nan as the header states) and the two counts."""
    if not isinstance(sums, MetricSums):
        w = [int(x) for x in (sums.tolist() if hasattr(sums, "tolist") else sums)]
        sums = MetricSums(*(w + [0] * (5 - len(w))))
    v = FrameMetricValues()
    _check(lib().mnv_metrics_finish(C.byref(sums), C.byref(v)))
    return v.as_dict()


def frame_metrics(rgba, target8, flags: int = 0, window=None, sums=None, se_map=None, ssim_map=None, stream: int = 0):
    """mnv_frame_metrics (asynchronous on `stream`): rgba float32 device tensor [h, w, 4] against target8 uint8 device tensor [h, w, 4].
    Returns `sums`, an int64 device tensor [5] (n_px, se_q32, n_win, ssim_q32, 0; allocated when None, zeroed by the call).  window: None
    (the standard one) or 11 floats (host).  se_map float32 [h, w] / ssim_map float32 [h - 10, w - 10, 3]: optional device outputs."""
    import torch

    if not rgba.is_cuda or not rgba.is_contiguous() or rgba.dtype != torch.float32 or rgba.dim() != 3 or rgba.shape[2] != 4:
        raise MnvError(MNV_E_INVALID, "rgba must be a contiguous float32 device tensor [height, width, 4]")
    h, w = int(rgba.shape[0]), int(rgba.shape[1])
    if not target8.is_cuda or not target8.is_contiguous() or target8.dtype != torch.uint8 or target8.numel() != w * h * 4:
        raise MnvError(MNV_E_INVALID, f"target8 must be a contiguous uint8 device tensor of {h} x {w} x 4 elements")
    if sums is None:
        sums = torch.empty(5, dtype=torch.int64, device=rgba.device)
    if not sums.is_cuda or not sums.is_contiguous() or sums.dtype != torch.int64 or sums.numel() < 5:
        raise MnvError(MNV_E_INVALID, "sums must be a contiguous int64 device tensor of 5 elements")
    for name, t, n in (("se_map", se_map, w * h), ("ssim_map", ssim_map, max(w - 10, 0) * max(h - 10, 0) * 3)):
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or t.numel() < n):
            raise MnvError(MNV_E_INVALID, f"{name} must be a contiguous float32 device tensor with at least {n} elements")
    g = None if window is None else np.ascontiguousarray(window, np.float32).reshape(-1)
    if g is not None and g.size != 11:
        raise MnvError(MNV_E_INVALID, "window has 11 entries")
    with _timed(stream):
        _check(lib().mnv_frame_metrics(rgba.data_ptr(), target8.data_ptr(), w, h, int(flags), g.ctypes.data if g is not None else None, sums.data_ptr(),
                                       _ptr(se_map), _ptr(ssim_map), C.c_void_p(stream)))
    return sums


def pnm_read(path: str, expect_width: int = 0, expect_height: int = 0) -> np.ndarray:
    """mnv_pnm_read: a binary PPM (P6) / PGM (P5) file with maxval 255 as uint8 [height, width, channels]; a malformed file, or one of
    another size than expected, raises MnvError (MNV_E_IO)."""
    w, h, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().mnv_pnm_read(os.fsencode(path), int(expect_width), int(expect_height), None, 0, C.byref(w), C.byref(h), C.byref(ch)))
    out = np.empty((h.value, w.value, ch.value), np.uint8)
    _check(lib().mnv_pnm_read(os.fsencode(path), int(expect_width), int(expect_height), out.ctypes.data, out.size, C.byref(w), C.byref(h), C.byref(ch)))
    return out


PROJ_PINHOLE, PROJ_ORTHO, PROJ_EQUIRECT = 0, 1, 2
_equirect_dev = {}   # (width, height, device) -> the device copy of equirect_tables, kept alive for the launches that read it


def equirect_tables(width: int, height: int) -> np.ndarray:
    """mnv_equirect_tables: float32 [width + height, 2] = (sin, cos) of every column's longitude, then of every row's latitude."""
    out = np.zeros((max(int(width), 0) + max(int(height), 0), 2), np.float32)
    _check(lib().mnv_equirect_tables(int(width), int(height), out.ctypes.data))
    return out


def _check_rays(name: str, t, shape=None):
    import torch

    if t is None or not hasattr(t, "is_cuda") or not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or t.dim() not in (2, 3) \
            or t.shape[-1] != 3 or t.numel() == 0 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = f"{tuple(shape)}" if shape is not None else "[height, width, 3] or [n, 3]"
        raise MnvError(MNV_E_INVALID, f"{name} must be a contiguous float32 device tensor {want}"
                                      f" (got {None if t is None else (tuple(t.shape), t.dtype, t.device)})")


def generate_rays(projection: int, cam: Camera, tile=None, origins=None, dirs=None, stream: int = 0):
    """mnv_generate_rays (asynchronous on `stream`): world-space origins and directions, float32 device tensors [tile h, tile w, 3], of the
    rectangle `tile` of cam's image under PROJ_PINHOLE / PROJ_ORTHO / PROJ_EQUIRECT; origins / dirs are allocated when not given.
    -> (origins, dirs)"""
    import torch

    if tile is None:
        tile = (0, 0, cam.width, cam.height)
    shape = (tile[3], tile[2], 3)
    if tile[2] < 1 or tile[3] < 1:
        raise MnvError(MNV_E_INVALID, "the rectangle needs w >= 1 and h >= 1")
    if origins is None:
        origins = torch.empty(shape, dtype=torch.float32, device="cuda")
    if dirs is None:
        dirs = torch.empty(shape, dtype=torch.float32, device="cuda")
    _check_rays("origins", origins, shape)
    _check_rays("dirs", dirs, shape)
    tables = None
    if projection == PROJ_EQUIRECT:
        key = (cam.width, cam.height, str(origins.device))
        if key not in _equirect_dev:
            _equirect_dev[key] = torch.from_numpy(equirect_tables(cam.width, cam.height)).to(origins.device)
        tables = _equirect_dev[key]
    with _timed(stream):
        _check(lib().mnv_generate_rays(int(projection), C.byref(cam.c), Rect(*tile), _ptr(tables), origins.data_ptr(), dirs.data_ptr(),
                                       C.c_void_p(stream)))
    return origins, dirs


def render_rays_accel(accel: int, origins, dirs, opt: RenderOptions, rgba=None, rgba8=None, tmax=None, rgba8_init=None, stream: int = 0) -> None:
    """mnv_render_rays_accel (asynchronous on `stream`): the tuned march on the caller's rays.  origins / dirs: float32 device tensors
    [height, width, 3] (an image of rays) or [n, 3] (a flat list), world space, directions of any length; outputs, tmax (float32, a ray's
    t_max) and rgba8_init (uint8 RGBA, the pixel under the volume) are indexed like the rays."""
    _check_rays("origins", origins)
    _check_rays("dirs", dirs, tuple(origins.shape))
    height, width = (1, int(origins.shape[0])) if origins.dim() == 2 else (int(origins.shape[0]), int(origins.shape[1]))
    _check_out("rgba", rgba, width * height, "f32")
    _check_out("rgba8", rgba8, width * height, "u8")
    inputs = _frame_inputs(tmax, rgba8_init, width * height)
    with _timed(stream):
        _check(lib().mnv_render_rays_accel(C.c_void_p(accel), origins.data_ptr(), dirs.data_ptr(), width, height, C.byref(opt),
                                           C.byref(inputs) if inputs is not None else None, _ptr(rgba), _ptr(rgba8), C.c_void_p(stream)))


def _check_dev(name: str, t, dtype, numel: int):
    if t is None or not hasattr(t, "is_cuda") or not t.is_cuda or not t.is_contiguous() or t.dtype != dtype or t.numel() < numel:
        raise MnvError(MNV_E_INVALID, f"{name} must be a contiguous {dtype} device tensor with at least {numel} elements")


def rays_grad(view: TreeView, origins, dirs, target, opt: RenderOptions, acc, sums, rgba=None, tmax=None, stream: int = 0) -> None:
    """mnv_rays_grad (asynchronous on `stream`): marches the rays (as render_rays_accel takes them) through the DEVICE tree view and ADDS the
    gradient of 1/2 |pixel - target|^2 into acc (int64 [capacity * 8, data_dim], fixed point 2^-32) and the ray counts and squared error into
    sums (int64 [8], FIT_SUMS names the first five); both are the caller's to zero.  target: float32 [.., 4], alpha 0 excludes a ray."""
    import torch

    _check_rays("origins", origins)
    _check_rays("dirs", dirs, tuple(origins.shape))
    height, width = (1, int(origins.shape[0])) if origins.dim() == 2 else (int(origins.shape[0]), int(origins.shape[1]))
    n = width * height
    _check_dev("target", target, torch.float32, n * 4)
    _check_dev("acc", acc, torch.int64, view.capacity * 8 * view.data_dim)
    _check_dev("sums", sums, torch.int64, 8)
    _check_out("rgba", rgba, n, "f32")
    if tmax is not None:
        _check_dev("tmax", tmax, torch.float32, n)
    with _timed(stream):
        _check(lib().mnv_rays_grad(C.byref(view), origins.data_ptr(), dirs.data_ptr(), target.data_ptr(), _ptr(tmax), width, height, C.byref(opt), _ptr(rgba),
                                   acc.data_ptr(), sums.data_ptr(), C.c_void_p(stream)))


def rays_visibility(view: TreeView, origins, dirs, opt: RenderOptions, wmax, sums, tmax=None, stream: int = 0) -> None:
    """mnv_rays_visibility (asynchronous on `stream`): marches the rays (as rays_grad takes them) through the DEVICE tree view and takes, per
    leaf voxel, the maximum of the compositing weights T * (1 - att) its dense samples got into wmax (int32 / uint32 device tensor
    [capacity * 8]: binary32 bit patterns, 0 = never weighted) and adds the ray counts into sums (int64 [8], VIS_SUMS names the first four);
    both are the caller's to zero, calls accumulate."""
    import torch

    _check_rays("origins", origins)
    _check_rays("dirs", dirs, tuple(origins.shape))
    height, width = (1, int(origins.shape[0])) if origins.dim() == 2 else (int(origins.shape[0]), int(origins.shape[1]))
    if wmax is None or not wmax.is_cuda or not wmax.is_contiguous() or wmax.element_size() != 4 or wmax.numel() < view.capacity * 8:
        raise MnvError(MNV_E_INVALID, f"wmax must be a contiguous 32-bit device tensor with at least {view.capacity * 8} elements")
    _check_dev("sums", sums, torch.int64, 8)
    if tmax is not None:
        _check_dev("tmax", tmax, torch.float32, width * height)
    with _timed(stream):
        _check(lib().mnv_rays_visibility(C.byref(view), origins.data_ptr(), dirs.data_ptr(), _ptr(tmax), width, height, C.byref(opt), wmax.data_ptr(),
                                         sums.data_ptr(), C.c_void_p(stream)))


def tree_cull(tree_view: TreeView, wmax, weight_thresh: float, data_out, keep_out, stream: int = 0):
    """mnv_tree_cull: the rows of a device tree view with every leaf whose word of wmax (rays_visibility's array) is not above weight_thresh
    zeroed, into data_out (16-bit device tensor [capacity, 8, data_dim], never the tree's own array), and which chunks stay into keep_out
    (uint8 device tensor [capacity]) -- tree_cut's input.  -> (kept_at_depth int64 [24], counts dict).  Waits for `stream`."""
    kept, counts = np.zeros(24, np.int64), CullCounts()
    _check(lib().mnv_tree_cull(C.byref(tree_view), _ptr(wmax), float(weight_thresh), _ptr(data_out), _ptr(keep_out), kept.ctypes.data_as(C.POINTER(C.c_int64)),
                               C.byref(counts), C.c_void_p(stream)))
    return kept, counts.as_dict()


def rows_master_init(data, master=None, stream: int = 0):
    """mnv_rows_master_init: the float32 master copy of binary16 rows (a uint16 / float16 device tensor); non-finite bit patterns read +0."""
    import torch

    if not data.is_cuda or not data.is_contiguous() or data.element_size() != 2:
        raise MnvError(MNV_E_INVALID, "data must be a contiguous 16-bit device tensor")
    if master is None:
        master = torch.empty(tuple(data.shape), dtype=torch.float32, device=data.device)
    _check_dev("master", master, torch.float32, data.numel())
    _check(lib().mnv_rows_master_init(data.data_ptr(), data.numel(), master.data_ptr(), C.c_void_p(stream)))
    return master


def rows_sgd_step(data, master, acc, data_dim: int, lr_colour: float, lr_sigma: float, n_rows: Optional[int] = None, stream: int = 0) -> None:
    """mnv_rows_sgd_step: one gradient step on the rows whose accumulators are not all zero (master float32, data binary16 and acc int64
    device tensors of n_rows * data_dim elements each; data may be a raw device pointer); clears the accumulators it consumed."""
    import torch

    if n_rows is None:
        n_rows = master.numel() // int(data_dim)
    n = int(n_rows) * int(data_dim)
    _check_dev("master", master, torch.float32, n)
    _check_dev("acc", acc, torch.int64, n)
    if not isinstance(data, int) and (not data.is_cuda or not data.is_contiguous() or data.element_size() != 2 or data.numel() < n):
        raise MnvError(MNV_E_INVALID, f"data must be a contiguous 16-bit device tensor with at least {n} elements")
    _check(lib().mnv_rows_sgd_step(_ptr(data), master.data_ptr(), acc.data_ptr(), int(n_rows), int(data_dim), float(lr_colour), float(lr_sigma),
                                   C.c_void_p(stream)))


def rows_adam_step(data, master, m1, m2, acc, data_dim: int, step: int, lr_colour: float = ADAM_DEFAULTS["lr_colour"], lr_sigma: float = ADAM_DEFAULTS["lr_sigma"],
                   betas=ADAM_DEFAULTS["betas"], eps: float = ADAM_DEFAULTS["eps"], n_rows: Optional[int] = None, stream: int = 0) -> None:
    """mnv_rows_adam_step: step number `step` (from 1) of the lazy Adam on the rows whose accumulators are not all zero (master, m1, m2
    float32, data binary16 and acc int64 device tensors of n_rows * data_dim elements each; data may be a raw device pointer); clears the
    accumulators it consumed."""
    import torch

    if n_rows is None:
        n_rows = master.numel() // int(data_dim)
    n = int(n_rows) * int(data_dim)
    for name, t in (("master", master), ("m1", m1), ("m2", m2)):
        _check_dev(name, t, torch.float32, n)
    _check_dev("acc", acc, torch.int64, n)
    if not isinstance(data, int) and (not data.is_cuda or not data.is_contiguous() or data.element_size() != 2 or data.numel() < n):
        raise MnvError(MNV_E_INVALID, f"data must be a contiguous 16-bit device tensor with at least {n} elements")
    p = AdamParams(float(lr_colour), float(lr_sigma), float(betas[0]), float(betas[1]), float(eps))
    _check(lib().mnv_rows_adam_step(_ptr(data), master.data_ptr(), m1.data_ptr(), m2.data_ptr(), acc.data_ptr(), int(n_rows), int(data_dim), C.byref(p), int(step),
                                    C.c_void_p(stream)))


class RayBatcher:
    """mnv_ray_batcher: batches of rays and targets drawn across a set of cameras and their target images (float32 device tensors
    [height, width, 4], kept alive by this object) in a seeded order that changes with the epoch.  A unit is a pixel (tile 1) or an 8 x 8
    pixel tile (tile 8); `units` is their total, `rays_per_unit` tile * tile."""

    def __init__(self, cams, targets, tile: int = 8, seed: int = 0):
        import torch

        n = len(cams)
        if n < 1 or len(targets) != n:
            raise MnvError(MNV_E_INVALID, "one target image per camera, at least one camera")
        for c, t in zip(cams, targets):
            if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != c.width * c.height * 4:
                raise MnvError(MNV_E_INVALID, "a target must be a contiguous float32 device tensor [height, width, 4] of its camera's size")
        self._targets = list(targets)
        arr = (CameraStruct * n)(*[c.c for c in cams])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in targets])
        h = C.c_void_p()
        _check(lib().mnv_ray_batcher_create(arr, ptrs, n, int(tile), int(seed), C.byref(h)))
        self._h = h
        units, per = C.c_int64(), C.c_int32()
        _check(lib().mnv_ray_batcher_units(self._h, C.byref(units), C.byref(per)))
        self.units, self.rays_per_unit = int(units.value), int(per.value)

    def draw(self, epoch: int, first: int, count: int, origins=None, dirs=None, target=None, stream: int = 0):
        """mnv_ray_batcher_draw (asynchronous on `stream`): the units at places first .. first + count - 1 of the epoch's order, as float32
        device tensors origins, dirs [count * rays_per_unit, 3] and target [count * rays_per_unit, 4] (allocated when not given): what
        rays_grad takes as a flat list.  -> (origins, dirs, target)"""
        import torch

        n = max(int(count), 0) * self.rays_per_unit
        if origins is None:
            origins = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        if dirs is None:
            dirs = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        if target is None:
            target = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        _check_dev("origins", origins, torch.float32, n * 3)
        _check_dev("dirs", dirs, torch.float32, n * 3)
        _check_dev("target", target, torch.float32, n * 4)
        _check(lib().mnv_ray_batcher_draw(self._h, int(epoch), int(first), int(count), origins.data_ptr(), dirs.data_ptr(), target.data_ptr(), C.c_void_p(stream)))
        return origins, dirs, target

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().mnv_ray_batcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_voxels_accel_batch(accel: int, cams, opt: RenderOptions, tile=None, part=None, rgba=None, rgba8=None,
                              stream: int = 0) -> None:
    """Several frames (`cams`: list of Camera, same image size) in one launch; frame f is written at
    rgba[f].  `part` = (rank, world, tile_w, tile_h[, root_period]) selects the interleaved macro-tile partition."""
    n = len(cams)
    if n < 1 or n > MAX_BATCH:
        raise MnvError(MNV_E_INVALID, f"need 1 .. {MAX_BATCH} cameras, got {n}")
    arr = (CameraStruct * n)(*[c.c for c in cams])
    p = Partition(0, 1, 0, 0) if part is None else Partition(*part)
    rect, _ = _accel_frame(cams[0], tile, rgba, rgba8, n_frames=n, part=part)
    with _timed(stream):
        _check(lib().mnv_render_voxels_accel_batch(C.c_void_p(accel), arr, n, C.byref(opt), rect, p, _ptr(rgba), _ptr(rgba8), C.c_void_p(stream)))


def accel_info(accel: int, coverage: bool = False) -> dict:
    """Device bytes of the packed layout, the level of its second lookup grid, the levels below it answered by inline cell words / brick records;
    coverage=True adds mnv_accel_lookup_coverage (a pass over the grid: waits for the device)."""
    d = {"device_bytes": int(lib().mnv_accel_device_bytes(accel)), "grid2_level": int(lib().mnv_accel_grid2_level(accel)),
         "brick_levels": int(lib().mnv_accel_brick_levels(C.c_void_p(accel)))}
    if coverage:
        out = (C.c_int64 * 4)()
        _check(lib().mnv_accel_lookup_coverage(C.c_void_p(accel), out))
        d.update(nonleaf_cells=int(out[0]), inline_cells=int(out[1]), inline_lost_to_chunk_field=int(out[2]), record_chunks=int(out[3]))
    return d


def accel_set_cu_budget(accel: int, num_cus: int) -> None:
    """Compute units the tuned kernel fills (0 = all); for launches on a CU-masked stream."""
    _check(lib().mnv_accel_set_cu_budget(accel, int(num_cus)))


def stream_create_reserved(reserve_cus: int):
    """(stream handle, enabled compute units): a HIP stream that leaves `reserve_cus` units free for other streams' kernels."""
    h, n = C.c_void_p(), C.c_int32()
    _check(lib().mnv_stream_create_reserved(int(reserve_cus), C.byref(h), C.byref(n)))
    return h.value, n.value


def stream_destroy(stream: int) -> None:
    _check(lib().mnv_stream_destroy(C.c_void_p(stream)))


COMM_ID_BYTES = 128


def comm_get_unique_id() -> bytes:
    """The 128-byte RCCL id one rank draws and hands to the others (any side channel)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().mnv_comm_get_unique_id(buf))
    return buf.raw


class Comm:
    """RCCL communicator of the tile gather (mnv_comm_*): one process per GPU, bound to the current device."""

    def __init__(self, unique_id: bytes, world: int, rank: int):
        if len(unique_id) != COMM_ID_BYTES:
            raise MnvError(MNV_E_INVALID, "unique id must be 128 bytes")
        h = C.c_void_p()
        _check(lib().mnv_comm_init_rank(C.create_string_buffer(unique_id, COMM_ID_BYTES), int(world), int(rank), C.byref(h)))
        self.handle, self.world, self.rank = h.value, int(world), int(rank)

    def gather_tiles(self, local, gathered, root: int = 0, stream: int = 0) -> None:
        """local: contiguous device tensor; gathered (root only): contiguous device tensor [world, *local.shape]."""
        nbytes = local.numel() * local.element_size()
        if not local.is_contiguous() or not local.is_cuda:
            raise MnvError(MNV_E_INVALID, "local must be a contiguous device tensor")
        if self.rank == root:
            if gathered is None or not gathered.is_contiguous() or not gathered.is_cuda or gathered.numel() * gathered.element_size() != nbytes * self.world:
                raise MnvError(MNV_E_INVALID, "gathered must be a contiguous device tensor of world x local bytes")
        _check(lib().mnv_gather_tiles(C.c_void_p(self.handle), _ptr(local), _ptr(gathered) if gathered is not None else None, nbytes, int(root),
                                      C.c_void_p(stream)))

    def allgather(self, table, stream: int = 0) -> None:
        """table: contiguous device tensor [world, ...]; this rank has written table[rank]; afterwards every rank holds every block."""
        if not table.is_contiguous() or not table.is_cuda or table.shape[0] != self.world:
            raise MnvError(MNV_E_INVALID, "table must be a contiguous device tensor [world, ...]")
        _check(lib().mnv_allgather(C.c_void_p(self.handle), _ptr(table), table.numel() * table.element_size() // self.world, C.c_void_p(stream)))

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().mnv_comm_destroy(C.c_void_p(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_visit_marks(table, visited, stream: int = 0) -> None:
    """visited[c] = max over ranks of table[r][c] (int32 device tensors [world, capacity] and [capacity])."""
    _check(lib().mnv_merge_visit_marks(_ptr(table), int(table.shape[0]), int(table.shape[1]), _ptr(visited), C.c_void_p(stream)))


def rccl_version() -> int:
    return int(lib().mnv_comm_rccl_version())


# ---- device times of the launches made through this binding: HIP events on the launch stream, recorded HERE (the library records nothing itself)
class _Timing:
    on = False
    pairs: list = []
    hip = None


def _hip():
    if _Timing.hip is None:
        lib()
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        h = C.CDLL(path or "libamdhip64.so")
        for name, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]), ("hipEventSynchronize", [C.c_void_p]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]), ("hipEventDestroy", [C.c_void_p])):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = C.c_int, args
        _Timing.hip = h
    return _Timing.hip


class _timed:
    """with _timed(stream): <one launch> -- two events around it when set_timing(True) is active"""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        self.e0 = None
        if _Timing.on:
            h = _hip()
            self.e0, self.e1 = C.c_void_p(), C.c_void_p()
            if h.hipEventCreate(C.byref(self.e0)) or h.hipEventCreate(C.byref(self.e1)):
                raise MnvError(MNV_E_FAULT, "hipEventCreate failed")
            h.hipEventRecord(self.e0, C.c_void_p(self.stream))
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.e0 is not None:
            _hip().hipEventRecord(self.e1, C.c_void_p(self.stream))
            _Timing.pairs.append((self.e0, self.e1))
        return False


def set_timing(enable: bool) -> None:
    """Start / stop timing the march launches made through render_voxels / render_voxels_accel[_track|_part|_batch] (HIP events on their streams)."""
    h = _hip()
    for e0, e1 in _Timing.pairs:
        h.hipEventDestroy(e0)
        h.hipEventDestroy(e1)
    _Timing.pairs = []
    _Timing.on = bool(enable)


def take_timing():
    """(sum of the device times in ms, launches) since the last call; waits for the launches."""
    h = _hip()
    total, n = 0.0, 0
    for e0, e1 in _Timing.pairs:
        if h.hipEventSynchronize(e1):
            raise MnvError(MNV_E_FAULT, "hipEventSynchronize failed")
        ms = C.c_float()
        if h.hipEventElapsedTime(C.byref(ms), e0, e1):
            raise MnvError(MNV_E_FAULT, "hipEventElapsedTime failed")
        total += ms.value
        n += 1
        h.hipEventDestroy(e0)
        h.hipEventDestroy(e1)
    _Timing.pairs = []
    return total, n
