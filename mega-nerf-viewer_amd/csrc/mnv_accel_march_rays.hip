// mnv_accel_march_rays.hip -- the instantiations of march_accel_kernel that march the CALLER's rays (RAYS = true: origin and direction of
// every image position from two device arrays, mnv_render_rays_accel) instead of a pinhole camera's: the plain march (MODE 0) for every row
// format and the colourless depth march (MODE 5), each on node words and -- the per-lane row formats -- on inline cell words / brick records.
// No trackers, visit marks, sample emission, partitions, batches or fast colour math for ray lists.
#include "mnv_march_accel_kernel.h"

namespace mnv {

template <int BASIS, int MODE, bool BRICK>
static int launch_rays2(const AccelLaunchRays &K, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    constexpr int BLOCK = 256;
    auto kern = march_accel_kernel<BASIS, BLOCK, MODE, BRICK, true>;
    if (lds_bytes > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(BLOCK), lds_bytes, stream, K);
    return (int)hipGetLastError();
}

template <bool BRICK>
static int launch_rays(const AccelLaunchRays &K, int b, bool colourless, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    if (colourless) return launch_rays2<9, 5, BRICK>(K, n_blocks, lds_bytes, stream);  // (reads no colour rows: serves every row format)
    switch (b) {
        case -1: return launch_rays2<-1, 0, BRICK>(K, n_blocks, lds_bytes, stream);
        case 1: return launch_rays2<1, 0, BRICK>(K, n_blocks, lds_bytes, stream);
        case 4: return launch_rays2<4, 0, BRICK>(K, n_blocks, lds_bytes, stream);
        case 9: return launch_rays2<9, 0, BRICK>(K, n_blocks, lds_bytes, stream);
        default: break;
    }
    if constexpr (!BRICK) {  // (SH16 / SH25: the cooperative colour pass has no brick variant)
        if (b == 16) return launch_rays2<16, 0, false>(K, n_blocks, lds_bytes, stream);
        if (b == 25) return launch_rays2<25, 0, false>(K, n_blocks, lds_bytes, stream);
    }
    return kUnsupportedBasis;
}

int launch_march_rays(const AccelLaunch &K, const float *ray_origins, const float *ray_dirs, int b, bool colourless, bool brick, int n_blocks,
                      size_t lds_bytes, hipStream_t stream) {
    if (!ray_origins || !ray_dirs || K.n_frames != 1 || K.part_world > 0) return (int)hipErrorInvalidValue;
    AccelLaunchRays R;
    static_cast<AccelLaunch &>(R) = K;
    R.ray_origins = ray_origins;
    R.ray_dirs = ray_dirs;
    return brick ? launch_rays<true>(R, b, colourless, n_blocks, lds_bytes, stream) : launch_rays<false>(R, b, colourless, n_blocks, lds_bytes, stream);
}

}  // namespace mnv
