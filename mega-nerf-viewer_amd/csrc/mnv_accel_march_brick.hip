// mnv_accel_march_brick.hip -- the instantiations of march_accel_kernel on inline cell words (AccelView::grid2i) and brick records
// (AccelView::recs: the two levels below the second lookup grid from one 64-byte record per chunk): every MODE of mnv_march_launch.h for
// the per-lane row formats (RGBA, SH1 / 4 / 9), the plain colour frames (MODE 0 / 4) also in the two fixed lookup shapes.  launch_accel sends SH16 / SH25 trees and frames with a negative sigma_thresh to the node
// words (mnv_accel_march.hip): every other lookup array says the same.
#include "mnv_march_launch.h"

namespace mnv {

int launch_march_brick(const AccelLaunch &K, int b, bool colourless, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    if (colourless) b = 9;
    switch (b) {
        case -1: return launch_march_mode<-1, true, false>(K, n_blocks, lds_bytes, stream);
        case 1: return launch_march_mode<1, true, false>(K, n_blocks, lds_bytes, stream);
        case 4: return launch_march_mode<4, true, false>(K, n_blocks, lds_bytes, stream);
        case 9: return launch_march_mode<9, true, false>(K, n_blocks, lds_bytes, stream);
        default: break;
    }
    return kUnsupportedBasis;
}

}  // namespace mnv
