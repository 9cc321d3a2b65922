// fit.cpp -- viewer::N3Tree::fit / fit_to: optimise the rows of a tree that is on the device against target frames (mnv_generate_rays,
// mnv_rays_grad, mnv_rows_sgd_step; include/mnv.h, "fitting a tree's rows").  A unit of its own, like lod.cpp: the one place where the tree
// model calls the fitting entry points of the C ABI.
#include <hip/hip_runtime_api.h>

#include <cmath>
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

std::vector<int64_t> N3Tree::fit(const std::vector<mnv_camera> &cams, const std::vector<const float *> &targets, const mnv_render_options &opt,
                                 const mnv_fit_params &params, void *hip_stream) {
    if (!on_device()) throw StatusError(MNV_E_INVALID, "fit: the tree is not on the device (move_to_device)");
    if (cams.empty() || cams.size() != targets.size()) throw StatusError(MNV_E_INVALID, "fit: one target frame per camera, at least one camera");
    if (params.iterations < 0) throw StatusError(MNV_E_INVALID, "fit: negative iteration count");
    if (!std::isfinite(params.lr_colour) || !std::isfinite(params.lr_sigma) || params.lr_colour < 0.f || params.lr_sigma < 0.f)
        throw StatusError(MNV_E_INVALID, "fit: the learning rates must be finite and not negative");
    int64_t total = 0, largest = 0;
    for (size_t i = 0; i < cams.size(); ++i) {
        if (!targets[i]) throw StatusError(MNV_E_INVALID, "fit: a target frame is null");
        if (cams[i].width < 1 || cams[i].height < 1) throw StatusError(MNV_E_INVALID, "fit: a camera has no pixels");
        const int64_t n = (int64_t)cams[i].width * cams[i].height;
        if (n > ((int64_t)1 << 22)) throw StatusError(MNV_E_INVALID, "fit: a camera of more than 2^22 pixels");
        total += n;
        largest = n > largest ? n : largest;
    }
    if (total > ((int64_t)1 << 24)) throw StatusError(MNV_E_INVALID, "fit: the cameras' pixels together pass 2^24 (the accumulators' headroom between two clears)");
    hipStream_t stream = (hipStream_t)hip_stream;
    const mnv_tree_view dv = device_view();
    const size_t n_rows = (size_t)capacity * N3_, n_words = n_rows * data_dim;
    mnv::Buffer<float> master, origins, dirs;
    mnv::Buffer<int64_t> acc;
    mnv::Buffer<mnv_fit_sums> sums;
    hip_check(master.alloc(n_words), "hipMalloc(master rows)");
    hip_check(acc.alloc(n_words), "hipMalloc(row accumulators)");
    hip_check(sums.alloc((size_t)(params.iterations > 0 ? params.iterations : 1)), "hipMalloc(fit sums)");
    hip_check(origins.alloc((size_t)largest * 3), "hipMalloc(ray origins)");
    hip_check(dirs.alloc((size_t)largest * 3), "hipMalloc(ray directions)");
    hip_check(hipMemsetAsync(acc.get(), 0, acc.bytes(), stream), "clear accumulators");
    hip_check(hipMemsetAsync(sums.get(), 0, sums.bytes(), stream), "clear sums");
    status(mnv_rows_master_init(device.data.get(), (int64_t)n_words, master.get(), hip_stream), "mnv_rows_master_init");
    for (int it = 0; it < params.iterations; ++it) {
        for (size_t i = 0; i < cams.size(); ++i) {
            const mnv_camera &c = cams[i];
            status(mnv_generate_rays(MNV_PROJ_PINHOLE, &c, mnv_rect{0, 0, c.width, c.height}, nullptr, origins.get(), dirs.get(), hip_stream), "mnv_generate_rays");
            status(mnv_rays_grad(&dv, origins.get(), dirs.get(), targets[i], nullptr, c.width, c.height, &opt, nullptr, acc.get(), sums.get() + it, hip_stream),
                   "mnv_rays_grad");
        }
        status(mnv_rows_sgd_step(device.data.get(), master.get(), acc.get(), (int64_t)n_rows, data_dim, params.lr_colour, params.lr_sigma, hip_stream),
               "mnv_rows_sgd_step");
    }
    std::vector<mnv_fit_sums> host((size_t)params.iterations);
    if (params.iterations > 0)
        hip_check(hipMemcpyAsync(host.data(), sums.get(), host.size() * sizeof(mnv_fit_sums), hipMemcpyDeviceToHost, stream), "download fit sums");
    if (device.accel) rebuild_accel(hip_stream);
    copy_from_device(hip_stream);  // waits for the stream
    std::vector<int64_t> se((size_t)params.iterations);
    for (size_t i = 0; i < se.size(); ++i) se[i] = host[i].se_q32;
    return se;
}

std::vector<int64_t> N3Tree::fit_to(const N3Tree &teacher, const std::vector<mnv_camera> &cams, const mnv_render_options &opt, const mnv_fit_params &params,
                                    void *hip_stream) {
    if (&teacher == this) throw StatusError(MNV_E_INVALID, "fit_to: the teacher must be another tree");
    if (!teacher.on_device() || !teacher.device.accel) throw StatusError(MNV_E_INVALID, "fit_to: the teacher is not on the device with its accel");
    if (cams.empty()) throw StatusError(MNV_E_INVALID, "fit_to: no camera");
    std::vector<mnv::Buffer<float>> frames(cams.size());
    std::vector<const float *> targets(cams.size());
    for (size_t i = 0; i < cams.size(); ++i) {
        const mnv_camera &c = cams[i];
        if (c.width < 1 || c.height < 1) throw StatusError(MNV_E_INVALID, "fit_to: a camera has no pixels");
        hip_check(frames[i].alloc((size_t)c.width * c.height * 4), "hipMalloc(teacher frame)");
        status(mnv_render_voxels_accel(teacher.device.accel, &c, &opt, mnv_rect{0, 0, c.width, c.height}, frames[i].get(), nullptr, hip_stream),
               "mnv_render_voxels_accel (teacher)");
        targets[i] = frames[i].get();
    }
    return fit(cams, targets, opt, params, hip_stream);  // (same stream: the frames are written before they are read)
}

}  // namespace viewer
