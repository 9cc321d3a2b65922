// fit.cpp -- viewer::N3Tree::fit / fit_to and their _ex forms: optimise the rows of a tree that is on the device against target frames
// (mnv_generate_rays or mnv_ray_batcher_draw, mnv_rays_grad, mnv_rows_sgd_step or mnv_rows_adam_step; include/mnv.h, "fitting a tree's rows"
// and "fitting on a photo set").  A unit of its own, like lod.cpp: the one place where the tree
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

namespace {
mnv_fit_params_ex sgd_full_batch(const mnv_fit_params &p) {
    mnv_fit_params_ex e = {};
    e.steps = p.iterations;
    e.optimizer = MNV_FIT_SGD;
    e.lr_colour = p.lr_colour;
    e.lr_sigma = p.lr_sigma;
    e.tile = 8;
    return e;
}
std::vector<int64_t> se_of(const std::vector<mnv_fit_sums> &sums) {
    std::vector<int64_t> se(sums.size());
    for (size_t i = 0; i < se.size(); ++i) se[i] = sums[i].se_q32;
    return se;
}
constexpr int64_t kMaxRays = (int64_t)1 << 22;  // mnv_rays_grad's limit
// what the loop refuses in its parameters alone: before any allocation or launch, the teacher's frames of fit_to_ex included
void check_params(const mnv_fit_params_ex &params) {
    if (params.steps < 0) throw StatusError(MNV_E_INVALID, "fit: negative iteration count");
    if (!std::isfinite(params.lr_colour) || !std::isfinite(params.lr_sigma) || params.lr_colour < 0.f || params.lr_sigma < 0.f)
        throw StatusError(MNV_E_INVALID, "fit: the learning rates must be finite and not negative");
    const bool adam = params.optimizer == MNV_FIT_ADAM;
    if (!adam && params.optimizer != MNV_FIT_SGD) throw StatusError(MNV_E_INVALID, "fit: the optimizer is 0 (SGD) or 1 (Adam)");
    if (adam && (!(params.beta1 >= 0.f && params.beta1 < 1.f) || !(params.beta2 >= 0.f && params.beta2 < 1.f) || !std::isfinite(params.eps) || !(params.eps > 0.f)))
        throw StatusError(MNV_E_INVALID, "fit: Adam needs beta1 and beta2 in [0, 1) and a finite eps > 0");
    if (params.tile != 1 && params.tile != 8) throw StatusError(MNV_E_INVALID, "fit: a batch unit is a pixel (tile 1) or an 8 x 8 tile (tile 8)");
    const int64_t per = (int64_t)params.tile * params.tile;
    if (params.batch_rays < 0 || params.batch_rays % per != 0 || params.batch_rays > kMaxRays)
        throw StatusError(MNV_E_INVALID, "fit: batch_rays must be 0 (full batch) or a multiple of tile * tile up to 2^22");
}
struct Batcher {  // the handle goes with its scope
    mnv_ray_batcher *h = nullptr;
    ~Batcher() { mnv_ray_batcher_destroy(h); }
};
}  // namespace

std::vector<int64_t> N3Tree::fit(const std::vector<mnv_camera> &cams, const std::vector<const float *> &targets, const mnv_render_options &opt,
                                 const mnv_fit_params &params, void *hip_stream) {
    return se_of(fit_ex(cams, targets, opt, sgd_full_batch(params), hip_stream));
}

std::vector<mnv_fit_sums> N3Tree::fit_ex(const std::vector<mnv_camera> &cams, const std::vector<const float *> &targets, const mnv_render_options &opt,
                                         const mnv_fit_params_ex &params, void *hip_stream) {
    if (!on_device()) throw StatusError(MNV_E_INVALID, "fit: the tree is not on the device (move_to_device)");
    if (cams.empty() || cams.size() != targets.size()) throw StatusError(MNV_E_INVALID, "fit: one target frame per camera, at least one camera");
    check_params(params);
    const bool adam = params.optimizer == MNV_FIT_ADAM;
    const int64_t per = (int64_t)params.tile * params.tile, max_rays = kMaxRays;
    const bool batched = params.batch_rays > 0;
    int64_t total = 0, largest = 0;
    for (size_t i = 0; i < cams.size(); ++i) {
        if (!targets[i]) throw StatusError(MNV_E_INVALID, "fit: a target frame is null");
        if (cams[i].width < 1 || cams[i].height < 1) throw StatusError(MNV_E_INVALID, "fit: a camera has no pixels");
        const int64_t n = (int64_t)cams[i].width * cams[i].height;
        if (!batched && n > max_rays) throw StatusError(MNV_E_INVALID, "fit: a camera of more than 2^22 pixels");
        total += n;
        largest = n > largest ? n : largest;
    }
    if (!batched && total > ((int64_t)1 << 24))
        throw StatusError(MNV_E_INVALID, "fit: the cameras' pixels together pass 2^24 (the accumulators' headroom between two clears)");
    hipStream_t stream = (hipStream_t)hip_stream;
    Batcher batcher;
    int64_t units = 0;
    if (batched) {
        status(mnv_ray_batcher_create(cams.data(), targets.data(), (int32_t)cams.size(), params.tile, params.seed, &batcher.h), "mnv_ray_batcher_create");
        status(mnv_ray_batcher_units(batcher.h, &units, nullptr), "mnv_ray_batcher_units");
    }
    const int64_t B = batched ? params.batch_rays / per : 0, nb = batched ? (units + B - 1) / B : 0;
    const size_t n_ray_slots = (size_t)(batched ? params.batch_rays : largest);
    const mnv_tree_view dv = device_view();
    const size_t n_rows = (size_t)capacity * N3_, n_words = n_rows * data_dim;
    mnv::Buffer<float> master, m1, m2, origins, dirs, batch_target;
    mnv::Buffer<int64_t> acc;
    mnv::Buffer<mnv_fit_sums> sums;
    hip_check(master.alloc(n_words), "hipMalloc(master rows)");
    hip_check(acc.alloc(n_words), "hipMalloc(row accumulators)");
    hip_check(sums.alloc((size_t)(params.steps > 0 ? params.steps : 1)), "hipMalloc(fit sums)");
    hip_check(origins.alloc(n_ray_slots * 3), "hipMalloc(ray origins)");
    hip_check(dirs.alloc(n_ray_slots * 3), "hipMalloc(ray directions)");
    if (batched) hip_check(batch_target.alloc(n_ray_slots * 4), "hipMalloc(batch targets)");
    if (adam) {
        hip_check(m1.alloc(n_words), "hipMalloc(first moments)");
        hip_check(m2.alloc(n_words), "hipMalloc(second moments)");
        hip_check(hipMemsetAsync(m1.get(), 0, m1.bytes(), stream), "clear first moments");
        hip_check(hipMemsetAsync(m2.get(), 0, m2.bytes(), stream), "clear second moments");
    }
    hip_check(hipMemsetAsync(acc.get(), 0, acc.bytes(), stream), "clear accumulators");
    hip_check(hipMemsetAsync(sums.get(), 0, sums.bytes(), stream), "clear sums");
    status(mnv_rows_master_init(device.data.get(), (int64_t)n_words, master.get(), hip_stream), "mnv_rows_master_init");
    mnv_adam_params ap = {};
    ap.lr_colour = params.lr_colour, ap.lr_sigma = params.lr_sigma, ap.beta1 = params.beta1, ap.beta2 = params.beta2, ap.eps = params.eps;
    for (int it = 0; it < params.steps; ++it) {
        if (batched) {
            const int64_t b = it % nb, first = b * B, count = units - first < B ? units - first : B;
            status(mnv_ray_batcher_draw(batcher.h, it / nb, first, count, origins.get(), dirs.get(), batch_target.get(), hip_stream), "mnv_ray_batcher_draw");
            status(mnv_rays_grad(&dv, origins.get(), dirs.get(), batch_target.get(), nullptr, (int32_t)(count * per), 1, &opt, nullptr, acc.get(), sums.get() + it,
                                 hip_stream),
                   "mnv_rays_grad");
        } else {
            for (size_t i = 0; i < cams.size(); ++i) {
                const mnv_camera &c = cams[i];
                status(mnv_generate_rays(MNV_PROJ_PINHOLE, &c, mnv_rect{0, 0, c.width, c.height}, nullptr, origins.get(), dirs.get(), hip_stream), "mnv_generate_rays");
                status(mnv_rays_grad(&dv, origins.get(), dirs.get(), targets[i], nullptr, c.width, c.height, &opt, nullptr, acc.get(), sums.get() + it, hip_stream),
                       "mnv_rays_grad");
            }
        }
        if (adam)
            status(mnv_rows_adam_step(device.data.get(), master.get(), m1.get(), m2.get(), acc.get(), (int64_t)n_rows, data_dim, &ap, (int64_t)it + 1, hip_stream),
                   "mnv_rows_adam_step");
        else
            status(mnv_rows_sgd_step(device.data.get(), master.get(), acc.get(), (int64_t)n_rows, data_dim, params.lr_colour, params.lr_sigma, hip_stream),
                   "mnv_rows_sgd_step");
    }
    std::vector<mnv_fit_sums> host((size_t)params.steps);
    if (params.steps > 0)
        hip_check(hipMemcpyAsync(host.data(), sums.get(), host.size() * sizeof(mnv_fit_sums), hipMemcpyDeviceToHost, stream), "download fit sums");
    if (device.accel) rebuild_accel(hip_stream);
    copy_from_device(hip_stream);  // waits for the stream
    return host;
}

std::vector<int64_t> N3Tree::fit_to(const N3Tree &teacher, const std::vector<mnv_camera> &cams, const mnv_render_options &opt, const mnv_fit_params &params,
                                    void *hip_stream) {
    return se_of(fit_to_ex(teacher, cams, opt, sgd_full_batch(params), hip_stream));
}

std::vector<mnv_fit_sums> N3Tree::fit_to_ex(const N3Tree &teacher, const std::vector<mnv_camera> &cams, const mnv_render_options &opt,
                                            const mnv_fit_params_ex &params, void *hip_stream) {
    if (&teacher == this) throw StatusError(MNV_E_INVALID, "fit_to: the teacher must be another tree");
    if (!teacher.on_device() || !teacher.device.accel) throw StatusError(MNV_E_INVALID, "fit_to: the teacher is not on the device with its accel");
    if (cams.empty()) throw StatusError(MNV_E_INVALID, "fit_to: no camera");
    check_params(params);
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
    return fit_ex(cams, targets, opt, params, hip_stream);  // (same stream: the frames are written before they are read)
}

}  // namespace viewer
