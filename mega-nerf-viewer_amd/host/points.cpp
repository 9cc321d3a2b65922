// points.cpp -- viewer::N3Tree::from_points: a tree from a coloured point cloud as a new tree on the device (mnv_point_tree_create / add /
// finish / write), and mnv_points_bounds_to_cube.
// A unit of its own: it is the one place where the tree model calls the point entry points of the C ABI.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "../csrc/mnv_error.h"
#include "n3tree.hpp"

namespace viewer {

namespace {
void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
void status(int rc, const char *what) {
    if (rc != MNV_OK) throw StatusError(rc, std::string(what) + ": " + mnv_last_error());
}
struct Handle {  // destroyed on every way out
    mnv_point_tree *h = nullptr;
    ~Handle() { mnv_point_tree_destroy(h); }
};
constexpr int64_t kUploadTile = (int64_t)1 << 22;  // points per add of the host overload
}  // namespace

std::unique_ptr<N3Tree> N3Tree::from_points(const mnv_points_params &params, const float *xyz_dev, const uint8_t *rgb_dev, int64_t n, void *hip_stream,
                                            mnv_points_stats *stats) {
    auto out = std::make_unique<N3Tree>();
    from_points_into(*out, params, xyz_dev, rgb_dev, n, hip_stream, stats);
    return out;
}

std::unique_ptr<N3Tree> N3Tree::from_points(const mnv_points_params &params, const std::vector<float> &xyz, const std::vector<uint8_t> &rgb, void *hip_stream,
                                            mnv_points_stats *stats) {
    auto out = std::make_unique<N3Tree>();
    from_points_into(*out, params, xyz, rgb, hip_stream, stats);
    return out;
}

void N3Tree::finish_points_into(N3Tree &o, const mnv_points_params &params, mnv_point_tree *handle, void *hip_stream, mnv_points_stats *stats) {
    mnv_points_stats st;
    status(mnv_point_tree_finish(handle, &st, hip_stream), "mnv_point_tree_finish");
    int64_t cap = 0;
    for (int d = 1; d < 24; ++d) cap += st.chunks_at_depth[d];
    o.free_device();
    o.N = 2, o.N2_ = 4, o.N3_ = 8;
    o.data_format.format = params.format == MNV_FORMAT_SH ? DataFormat::SH : DataFormat::RGBA;
    o.data_format.basis_dim = params.format == MNV_FORMAT_SH ? params.basis_dim : -1;
    o.data_dim = params.format == MNV_FORMAT_SH ? 3 * params.basis_dim + 1 : 4;
    for (int k = 0; k < 3; ++k) o.offset[k] = params.offset[k], o.scale[k] = params.scale[k];
    o.capacity = (int)cap;
    hip_check(o.device.data.alloc((size_t)cap * 8 * o.data_dim), "hipMalloc(data)");
    hip_check(o.device.child.alloc((size_t)cap * 8), "hipMalloc(child)");
    hip_check(o.device.parent.alloc((size_t)cap), "hipMalloc(parent)");
    hip_check(o.device.sample_counts.alloc((size_t)cap * 8), "hipMalloc(sample_counts)");
    o.device.max_capacity = (long)cap;
    status(mnv_point_tree_write(handle, o.device.child.get(), o.device.data.get(), o.device.parent.get(), o.device.sample_counts.get(), nullptr, hip_stream),
           "mnv_point_tree_write");
    o.copy_from_device(hip_stream);  // waits for the stream: the handle may go
    const mnv_tree_view ov = o.device_view();
    status(mnv_accel_create_reserved(&ov, cap, hip_stream, &o.device.accel), "mnv_accel_create");
    hip_check(hipStreamSynchronize((hipStream_t)hip_stream), "from_points");
    if (stats) *stats = st;
}

void N3Tree::from_points_into(N3Tree &o, const mnv_points_params &params, const float *xyz_dev, const uint8_t *rgb_dev, int64_t n, void *hip_stream,
                              mnv_points_stats *stats) {
    Handle H;
    status(mnv_point_tree_create(&params, &H.h), "mnv_point_tree_create");
    status(mnv_point_tree_add(H.h, xyz_dev, rgb_dev, n, hip_stream), "mnv_point_tree_add");
    finish_points_into(o, params, H.h, hip_stream, stats);
}

void N3Tree::from_points_into(N3Tree &o, const mnv_points_params &params, const std::vector<float> &xyz, const std::vector<uint8_t> &rgb, void *hip_stream,
                              mnv_points_stats *stats) {
    if (xyz.size() % 3 != 0) throw StatusError(MNV_E_INVALID, "from_points: three floats per point");
    const int64_t n = (int64_t)(xyz.size() / 3);
    if (!rgb.empty() && rgb.size() != xyz.size()) throw StatusError(MNV_E_INVALID, "from_points: three colour bytes per point, or none");
    Handle H;
    status(mnv_point_tree_create(&params, &H.h), "mnv_point_tree_create");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t tile = std::min<int64_t>(kUploadTile, std::max<int64_t>(n, 1));
    mnv::Buffer<float> xyz_dev;
    mnv::Buffer<uint8_t> rgb_dev;
    hip_check(xyz_dev.alloc((size_t)tile * 3), "hipMalloc(points)");
    hip_check(rgb_dev.alloc((size_t)tile * 3), "hipMalloc(colours)");
    if (rgb.empty()) hip_check(hipMemsetAsync(rgb_dev.get(), 0xff, (size_t)tile * 3, stream), "white colours");
    for (int64_t at = 0; at < n; at += tile) {
        const int64_t m = std::min(tile, n - at);
        hip_check(hipMemcpyAsync(xyz_dev.get(), xyz.data() + at * 3, (size_t)m * 12, hipMemcpyHostToDevice, stream), "upload points");
        if (!rgb.empty()) hip_check(hipMemcpyAsync(rgb_dev.get(), rgb.data() + at * 3, (size_t)m * 3, hipMemcpyHostToDevice, stream), "upload colours");
        status(mnv_point_tree_add(H.h, xyz_dev.get(), rgb_dev.get(), m, hip_stream), "mnv_point_tree_add");  // (waits: the tile may be refilled)
    }
    finish_points_into(o, params, H.h, hip_stream, stats);
}

}  // namespace viewer

extern "C" int mnv_points_bounds_to_cube(const float lo[3], const float hi[3], float offset[3], float scale[3]) {
    if (!lo || !hi || !offset || !scale) return mnv::set_error(MNV_E_INVALID, "mnv_points_bounds_to_cube: null argument");
    float L = 0.f;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || hi[k] < lo[k]) return mnv::set_error(MNV_E_INVALID, "mnv_points_bounds_to_cube: a box needs finite lo <= hi");
        const float ext = hi[k] - lo[k];
        L = ext > L ? ext : L;
    }
    if (L == 0.f) L = 1.f;
    const float s = 1.f / L;
    for (int k = 0; k < 3; ++k) {
        const float centre = 0.5f * (lo[k] + hi[k]), m = s * centre;
        scale[k] = s;
        offset[k] = 0.5f - m;
    }
    return MNV_OK;
}
