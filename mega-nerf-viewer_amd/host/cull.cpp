// cull.cpp -- viewer::N3Tree::make_culled: a tree without what a set of cameras cannot see, as a new tree on the device
// (mnv_generate_rays + mnv_rays_visibility per camera, mnv_tree_cull, mnv_tree_cut; include/mnv.h, "culling a tree to a pose set").
// A unit of its own, like lod.cpp and fit.cpp: the one place where the tree model calls the culling entry points of the C ABI.
#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>

#include "n3tree.hpp"

namespace viewer {

namespace {
void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
void status(int rc, const char *what) {
    if (rc != MNV_OK) throw StatusError(rc, std::string(what) + ": " + mnv_last_error());
}
}  // namespace

std::unique_ptr<N3Tree> N3Tree::make_culled(const std::vector<mnv_camera> &cams, const mnv_render_options &opt, float weight_thresh, void *hip_stream,
                                            int64_t *kept_at_depth, mnv_cull_counts *counts) const {
    auto out = std::make_unique<N3Tree>();
    make_culled_into(*out, cams, opt, weight_thresh, hip_stream, kept_at_depth, counts);
    return out;
}

void N3Tree::make_culled_into(N3Tree &o, const std::vector<mnv_camera> &cams, const mnv_render_options &opt, float weight_thresh, void *hip_stream,
                              int64_t *kept_at_depth, mnv_cull_counts *counts) const {
    if (&o == this) throw StatusError(MNV_E_INVALID, "make_culled: the result must be another tree");
    if (!on_device()) throw StatusError(MNV_E_INVALID, "make_culled: the tree is not on the device (move_to_device)");
    if (cams.empty()) throw StatusError(MNV_E_INVALID, "make_culled: no camera");
    int64_t largest = 0;
    for (const mnv_camera &c : cams) {
        if (c.width < 1 || c.height < 1) throw StatusError(MNV_E_INVALID, "make_culled: a camera has no pixels");
        const int64_t n = (int64_t)c.width * c.height;
        if (n > ((int64_t)1 << 22)) throw StatusError(MNV_E_INVALID, "make_culled: a camera of more than 2^22 pixels");
        largest = n > largest ? n : largest;
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    mnv_tree_view dv = device_view();
    // the largest weight per leaf over every camera's frame
    mnv::Buffer<uint32_t> wmax;
    mnv::Buffer<mnv_vis_sums> sums;
    mnv::Buffer<float> origins, dirs;
    hip_check(wmax.alloc((size_t)capacity * N3_), "hipMalloc(leaf weights)");
    hip_check(sums.alloc(1), "hipMalloc(visibility sums)");
    hip_check(origins.alloc((size_t)largest * 3), "hipMalloc(ray origins)");
    hip_check(dirs.alloc((size_t)largest * 3), "hipMalloc(ray directions)");
    hip_check(hipMemsetAsync(wmax.get(), 0, wmax.bytes(), stream), "clear leaf weights");
    hip_check(hipMemsetAsync(sums.get(), 0, sums.bytes(), stream), "clear visibility sums");
    for (const mnv_camera &c : cams) {
        status(mnv_generate_rays(MNV_PROJ_PINHOLE, &c, mnv_rect{0, 0, c.width, c.height}, nullptr, origins.get(), dirs.get(), hip_stream), "mnv_generate_rays");
        status(mnv_rays_visibility(&dv, origins.get(), dirs.get(), nullptr, c.width, c.height, &opt, wmax.get(), sums.get(), hip_stream), "mnv_rays_visibility");
    }
    // the culled rows and which chunks stay, then the cut
    mnv::Buffer<uint16_t> culled;
    mnv::Buffer<uint8_t> keep;
    hip_check(culled.alloc((size_t)capacity * N3_ * data_dim), "hipMalloc(culled rows)");
    hip_check(keep.alloc((size_t)capacity), "hipMalloc(keep)");
    int64_t kept[24];
    mnv_cull_counts cc;
    status(mnv_tree_cull(&dv, wmax.get(), weight_thresh, culled.get(), keep.get(), kept, &cc, hip_stream), "mnv_tree_cull");
    int64_t new_cap = 0;
    for (int d = 1; d < 24; ++d) new_cap += kept[d];
    if (kept_at_depth)
        for (int d = 0; d < 24; ++d) kept_at_depth[d] = kept[d];
    if (counts) *counts = cc;
    dv.data = culled.get();
    compact_into(o, new_cap, [&](int32_t *child_out, uint16_t *data_out, int32_t *parent_out, int16_t *counts_out) {
        status(mnv_tree_cut(&dv, keep.get(), (int32_t)new_cap, child_out, data_out, parent_out, counts_out, hip_stream), "mnv_tree_cut");
    }, hip_stream);
}

}  // namespace viewer
