// merge.cpp -- viewer::N3Tree::merge: two trees on the device as one new tree (mnv_tree_merge_plan / write), N3Tree::voxel_cube and
// mnv_tree_voxel_cube.
// A unit of its own: it is the one place where the tree model calls the merge entry points of the C ABI.
#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>

#include "../csrc/mnv_error.h"
#include "n3tree.hpp"

namespace viewer {

namespace {
void status(int rc, const char *what) {
    if (rc != MNV_OK) throw StatusError(rc, std::string(what) + ": " + mnv_last_error());
}
struct Handle {  // destroyed on every way out
    mnv_tree_merge *h = nullptr;
    ~Handle() { mnv_tree_merge_destroy(h); }
};
}  // namespace

std::unique_ptr<N3Tree> N3Tree::merge(const N3Tree &other, const mnv_merge_params &params, void *hip_stream, mnv_merge_stats *stats) const {
    auto out = std::make_unique<N3Tree>();
    merge_into(*out, other, params, hip_stream, stats);
    return out;
}

void N3Tree::merge_into(N3Tree &o, const N3Tree &other, const mnv_merge_params &params, void *hip_stream, mnv_merge_stats *stats) const {
    if (&o == this || &o == &other) throw StatusError(MNV_E_INVALID, "merge: the result must be another tree");
    if (!on_device() || !other.on_device()) throw StatusError(MNV_E_INVALID, "merge: both trees must be on the device (move_to_device)");
    const mnv_tree_view av = device_view(), bv = other.device_view();
    Handle H;
    mnv_merge_stats st;
    status(mnv_tree_merge_plan(&av, &bv, &params, &H.h, &st, hip_stream), "mnv_tree_merge_plan");
    compact_into(o, st.capacity, [&](int32_t *child_out, uint16_t *data_out, int32_t *parent_out, int16_t *counts_out) {
        status(mnv_tree_merge_write(H.h, child_out, data_out, parent_out, counts_out, nullptr, nullptr, hip_stream), "mnv_tree_merge_write");
    }, hip_stream);  // (waits for the stream: the handle may go)
    if (stats) *stats = st;
}

void N3Tree::voxel_cube(int level, const std::array<int32_t, 3> &corner, std::array<float, 3> &offset_out, std::array<float, 3> &scale_out) const {
    status(mnv_tree_voxel_cube(offset.data(), scale.data(), level, corner.data(), offset_out.data(), scale_out.data()), "mnv_tree_voxel_cube");
}

}  // namespace viewer

extern "C" int mnv_tree_voxel_cube(const float offset[3], const float scale[3], int32_t level, const int32_t corner[3], float offset_out[3], float scale_out[3]) {
    if (!offset || !scale || !corner || !offset_out || !scale_out) return mnv::set_error(MNV_E_INVALID, "mnv_tree_voxel_cube: null argument");
    if (level < 0 || level > 22) return mnv::set_error(MNV_E_INVALID, "mnv_tree_voxel_cube: level outside 0 .. 22");
    const float two = (float)((int64_t)1 << level);
    for (int k = 0; k < 3; ++k)
        if (corner[k] < 0 || (int64_t)corner[k] >= ((int64_t)1 << level)) return mnv::set_error(MNV_E_INVALID, "mnv_tree_voxel_cube: a corner outside [0, 2^level)");
    for (int k = 0; k < 3; ++k) {
        const float s = scale[k] * two, m = offset[k] * two;  // (offset_out may be offset)
        scale_out[k] = s;
        offset_out[k] = m - (float)corner[k];
    }
    return MNV_OK;
}
