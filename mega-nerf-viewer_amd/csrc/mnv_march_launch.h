// mnv_march_launch.h -- the one launcher of march_accel_kernel and the choice of its MODE, for the units that instantiate the kernel
// (mnv_accel_march.hip: node words; mnv_accel_march_brick.hip: inline cell words / brick records; mnv_accel_march_rays.hip: ray lists).
// A unit instantiates what its calls of launch_march_mode name: the BASIS values of its switch times the MODEs below -- and, for the
// plain colour frames of the brick unit (MODE 0 / 4), times the lookup shapes of mnv_march_accel_kernel.h.
#pragma once

#include "mnv_knobs.h"
#include "mnv_march_accel_kernel.h"

namespace mnv {

template <int BASIS, int MODE, bool BRICK, bool RAYS, int SHAPE>
static int launch_march_instance(const LaunchBlock<RAYS> &K, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    constexpr int BLOCK = 256;
    auto kern = march_accel_kernel<BASIS, BLOCK, MODE, BRICK, RAYS, SHAPE>;
    if (lds_bytes > 65536) {  // diagnostics only (MNV_LDS_LEVEL=5); the attribute is per device, so set it on every such launch
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    note_march_variant(BASIS, MODE, BRICK, RAYS);  // empty in the shipped build (mnv_knobs.cpp)
    note_march_shape(SHAPE);
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(BLOCK), lds_bytes, stream, K);
    return (int)hipGetLastError();
}

// Lookup shape of a launch: a fixed one when the launch block says exactly what that instantiation assumes -- LDS grid at level 3, second
// grid at level 9, inline cell words -- with or without brick records; anything else (shallow trees, MNV_LDS_LEVEL / MNV_GRID2_LEVEL /
// MNV_BRICK_LEVELS of the test-hook build, and MNV_MARCH_SHAPE=0 there) is the generic instantiation.
static int march_shape_of(const AccelLaunch &K) {
    static const bool env_generic = knob_int(KNOB_MARCH_SHAPE, 1) == 0;
    if (env_generic || K.lds_level != kShapeLdsLevel || K.A.grid2_level != kShapeGrid2Level || !K.A.grid2i) return kShapeGeneric;
    return K.A.recs ? kShapeL3G9Recs : kShapeL3G9;
}

template <int BASIS, int MODE, bool BRICK, bool RAYS>
static int launch_march_kernel(const LaunchBlock<RAYS> &K, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    if constexpr (BRICK && !RAYS && (MODE == 0 || MODE == 4)) {
        const int shape = march_shape_of(K);
        if (shape == kShapeL3G9) return launch_march_instance<BASIS, MODE, BRICK, RAYS, kShapeL3G9>(K, n_blocks, lds_bytes, stream);
        if (shape == kShapeL3G9Recs) return launch_march_instance<BASIS, MODE, BRICK, RAYS, kShapeL3G9Recs>(K, n_blocks, lds_bytes, stream);
    }
    return launch_march_instance<BASIS, MODE, BRICK, RAYS, kShapeGeneric>(K, n_blocks, lds_bytes, stream);
}

// MODE of a launch: statistics -> 1, emitted samples -> 3, trackers / visit marks -> 2, depth image -> 5, fast colour math -> 4, else 0.
// Modes 1, 3 and 5 exist for BASIS 9 only: 1 is the diagnostics build (MNV_STATS / MNV_ABLATE ...) of the headline variant, 3 and 5 read
// no colour rows, so one instantiation serves every row format.  Ray lists have the plain march and the depth image.
template <int BASIS, bool BRICK, bool RAYS>
static int launch_march_mode(const LaunchBlock<RAYS> &K, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    if constexpr (!RAYS) {
        if constexpr (BASIS == 9) {
            if (K.diag.stats) return launch_march_kernel<BASIS, 1, BRICK, RAYS>(K, n_blocks, lds_bytes, stream);
            if (K.samples) return launch_march_kernel<BASIS, 3, BRICK, RAYS>(K, n_blocks, lds_bytes, stream);
        }
        if (K.split_track || K.sample_track || K.visited) return launch_march_kernel<BASIS, 2, BRICK, RAYS>(K, n_blocks, lds_bytes, stream);
    }
    if constexpr (BASIS == 9) {
        if (K.P.render_depth) return launch_march_kernel<BASIS, 5, BRICK, RAYS>(K, n_blocks, lds_bytes, stream);
    }
    if constexpr (!RAYS && BASIS >= 1) {
        if (K.fast_colour) return launch_march_kernel<BASIS, 4, BRICK, RAYS>(K, n_blocks, lds_bytes, stream);
    }
    return launch_march_kernel<BASIS, 0, BRICK, RAYS>(K, n_blocks, lds_bytes, stream);
}

}  // namespace mnv
