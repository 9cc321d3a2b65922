// mnv_accel_march_rays.hip -- the instantiations of march_accel_kernel that march the CALLER's rays (RAYS = true: origin and direction of
// every image position from two device arrays, mnv_render_rays_accel) instead of a pinhole camera's: the plain march (MODE 0) for every row
// format and the colourless depth march (MODE 5), each on node words and -- the per-lane row formats -- on inline cell words / brick records.
// No trackers, visit marks, sample emission, partitions, batches or fast colour math for ray lists (launch_march_mode<.., RAYS>).
#include "mnv_march_launch.h"

namespace mnv {

template <bool BRICK>
static int launch_rays(const AccelLaunchRays &K, int b, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    switch (b) {
        case -1: return launch_march_mode<-1, BRICK, true>(K, n_blocks, lds_bytes, stream);
        case 1: return launch_march_mode<1, BRICK, true>(K, n_blocks, lds_bytes, stream);
        case 4: return launch_march_mode<4, BRICK, true>(K, n_blocks, lds_bytes, stream);
        case 9: return launch_march_mode<9, BRICK, true>(K, n_blocks, lds_bytes, stream);
        default: break;
    }
    if constexpr (!BRICK) {  // (the brick kernels are not instantiated for SH16 / SH25)
        if (b == 16) return launch_march_mode<16, false, true>(K, n_blocks, lds_bytes, stream);
        if (b == 25) return launch_march_mode<25, false, true>(K, n_blocks, lds_bytes, stream);
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
    if (colourless) b = 9;
    return brick ? launch_rays<true>(R, b, n_blocks, lds_bytes, stream) : launch_rays<false>(R, b, n_blocks, lds_bytes, stream);
}

}  // namespace mnv
