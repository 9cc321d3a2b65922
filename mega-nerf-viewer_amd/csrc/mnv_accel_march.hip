// mnv_accel_march.hip -- the instantiations of march_accel_kernel that walk the node words: every MODE of mnv_march_launch.h for every row format.
#include "mnv_march_launch.h"

namespace mnv {

int launch_march(const AccelLaunch &K, int b, bool colourless, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    if (colourless) b = 9;
    switch (b) {
        case -1: return launch_march_mode<-1, false, false>(K, n_blocks, lds_bytes, stream);
        case 1: return launch_march_mode<1, false, false>(K, n_blocks, lds_bytes, stream);
        case 4: return launch_march_mode<4, false, false>(K, n_blocks, lds_bytes, stream);
        case 9: return launch_march_mode<9, false, false>(K, n_blocks, lds_bytes, stream);
        case 16: return launch_march_mode<16, false, false>(K, n_blocks, lds_bytes, stream);
        case 25: return launch_march_mode<25, false, false>(K, n_blocks, lds_bytes, stream);
        default: break;
    }
    return kUnsupportedBasis;
}

}  // namespace mnv
