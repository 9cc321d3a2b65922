// lod.cpp -- viewer::N3Tree::make_lod / make_view_lod: a level of detail of a tree as a new tree on the device (mnv_tree_mip_rows, then
// mnv_tree_truncate at a depth or mnv_tree_select_cut + mnv_tree_cut for a list of viewpoints).
// A unit of its own: it is the one place where the tree model calls the level-of-detail entry points of the C ABI.
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

std::unique_ptr<N3Tree> N3Tree::make_lod(int max_depth, void *hip_stream) const {
    auto out = std::make_unique<N3Tree>();
    make_lod_into(*out, max_depth, hip_stream);
    return out;
}

std::unique_ptr<N3Tree> N3Tree::make_view_lod(const std::vector<mnv_lod_view> &views, float pixels, int min_depth, int max_depth, void *hip_stream,
                                              int64_t *kept_at_depth) const {
    auto out = std::make_unique<N3Tree>();
    make_view_lod_into(*out, views, pixels, min_depth, max_depth, hip_stream, kept_at_depth);
    return out;
}

void N3Tree::compact_into(N3Tree &o, int64_t new_cap, const std::function<void(int32_t *, uint16_t *, int32_t *, int16_t *)> &cut, void *hip_stream) const {
    o.free_device();
    o.N = N, o.N2_ = N2_, o.N3_ = N3_;
    o.data_dim = data_dim;
    o.data_format = data_format;
    o.scale = scale;
    o.offset = offset;
    o.capacity = (int)new_cap;
    hip_check(o.device.data.alloc((size_t)new_cap * N3_ * data_dim), "hipMalloc(data)");
    hip_check(o.device.child.alloc((size_t)new_cap * N3_), "hipMalloc(child)");
    hip_check(o.device.parent.alloc((size_t)new_cap), "hipMalloc(parent)");
    if (device.sample_counts) hip_check(o.device.sample_counts.alloc((size_t)new_cap * N3_), "hipMalloc(sample_counts)");
    o.device.max_capacity = (long)new_cap;
    cut(o.device.child.get(), o.device.data.get(), o.device.parent.get(), o.device.sample_counts.get());
    o.parent.assign((size_t)new_cap, -1);  // (copy_from_device sizes the other arrays)
    o.sample_counts.assign((size_t)new_cap * N3_, 8);
    o.copy_from_device(hip_stream);  // waits for the stream: what `cut` reads may go
    if (device.accel) {
        const mnv_tree_view ov = o.device_view();
        status(mnv_accel_create_reserved(&ov, new_cap, hip_stream, &o.device.accel), "mnv_accel_create");
        hip_check(hipStreamSynchronize((hipStream_t)hip_stream), "make_lod");
    }
}

void N3Tree::make_lod_into(N3Tree &o, int max_depth, void *hip_stream) const {
    if (&o == this) throw StatusError(MNV_E_INVALID, "make_lod: the result must be another tree");
    if (!on_device()) throw StatusError(MNV_E_INVALID, "make_lod: the tree is not on the device (move_to_device)");
    if (max_depth < 1) throw StatusError(MNV_E_INVALID, "make_lod: max_depth must be at least 1");
    mnv_tree_view dv = device_view();
    // the mipped rows and the chunk depths of the whole tree
    mnv::Buffer<uint16_t> mipped;
    mnv::Buffer<int32_t> depth;
    hip_check(mipped.alloc((size_t)capacity * N3_ * data_dim), "hipMalloc(mipped rows)");
    hip_check(depth.alloc((size_t)capacity), "hipMalloc(chunk depths)");
    int64_t at_depth[24];
    status(mnv_tree_mip_rows(&dv, mipped.get(), depth.get(), at_depth, hip_stream), "mnv_tree_mip_rows");
    int64_t new_cap = 0;
    for (int d = 1; d < 24 && d <= max_depth; ++d) new_cap += at_depth[d];
    dv.data = mipped.get();
    compact_into(o, new_cap, [&](int32_t *child_out, uint16_t *data_out, int32_t *parent_out, int16_t *counts_out) {
        status(mnv_tree_truncate(&dv, depth.get(), max_depth, (int32_t)new_cap, child_out, data_out, parent_out, counts_out, hip_stream), "mnv_tree_truncate");
    }, hip_stream);
}

void N3Tree::make_view_lod_into(N3Tree &o, const std::vector<mnv_lod_view> &views, float pixels, int min_depth, int max_depth, void *hip_stream,
                                int64_t *kept_at_depth) const {
    if (&o == this) throw StatusError(MNV_E_INVALID, "make_view_lod: the result must be another tree");
    if (!on_device()) throw StatusError(MNV_E_INVALID, "make_view_lod: the tree is not on the device (move_to_device)");
    mnv_tree_view dv = device_view();
    // the mipped rows of the whole tree, then which chunks stay
    mnv::Buffer<uint16_t> mipped;
    mnv::Buffer<uint8_t> keep;
    hip_check(mipped.alloc((size_t)capacity * N3_ * data_dim), "hipMalloc(mipped rows)");
    hip_check(keep.alloc((size_t)capacity), "hipMalloc(keep)");
    int64_t at_depth[24], kept[24];
    status(mnv_tree_mip_rows(&dv, mipped.get(), nullptr, at_depth, hip_stream), "mnv_tree_mip_rows");
    status(mnv_tree_select_cut(&dv, views.data(), (int32_t)views.size(), pixels, min_depth, max_depth, keep.get(), kept, hip_stream), "mnv_tree_select_cut");
    int64_t new_cap = 0;
    for (int d = 1; d < 24; ++d) new_cap += kept[d];
    if (kept_at_depth)
        for (int d = 0; d < 24; ++d) kept_at_depth[d] = kept[d];
    dv.data = mipped.get();
    compact_into(o, new_cap, [&](int32_t *child_out, uint16_t *data_out, int32_t *parent_out, int16_t *counts_out) {
        status(mnv_tree_cut(&dv, keep.get(), (int32_t)new_cap, child_out, data_out, parent_out, counts_out, hip_stream), "mnv_tree_cut");
    }, hip_stream);
}

}  // namespace viewer
