// host_capi.cpp -- extern "C" wrappers of include/mnv.h over the C++ host data model.
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>

#include "../../include/mnv.h"
#include "../csrc/mnv_error.h"
#include "camera.hpp"
#include "mesh.hpp"
#include "n3tree.hpp"
#include "render_options.hpp"
#include "volume_renderer.hpp"

namespace viewer::synth {
void random_tree(const mnv_synth_random_params &p, N3Tree &out);
void shell_tree(const mnv_synth_shell_params &p, N3Tree &out);
void terrain_tree(const mnv_synth_terrain_params &p, N3Tree &out);
}  // namespace viewer::synth

struct mnv_n3tree {
    viewer::N3Tree tree;
};

struct mnv_renderer {
    viewer::VolumeRenderer rend;
};

namespace {
template <typename F>
int guarded(F f) {
    try {
        return f();
    } catch (const viewer::StatusError &e) {  // e.g. show_grid with frame inputs (MNV_E_INVALID), a grid of an N != 2 tree (MNV_E_UNSUPPORTED)
        return mnv::set_error(e.code, e.what());
    } catch (const std::exception &e) {
        return mnv::set_error(MNV_E_IO, e.what());
    } catch (...) {
        return mnv::set_error(MNV_E_IO, "unknown C++ exception");
    }
}
}  // namespace

extern "C" {

void mnv_default_render_options(mnv_render_options *opt) {
    const viewer::RenderOptions d;
    std::memcpy(opt, &d, sizeof(*opt));
}

void mnv_cli_render_options(mnv_render_options *opt) {
    // src/opts.cpp:17-32 defaults mapped as in :49-67
    viewer::RenderOptions d;
    d.background_brightness = 0.f;
    d.step_size = 1e-4f;
    d.stop_thresh = 1e-2f;
    d.sigma_thresh = 1e-2f;
    d.split_batch_size = 4096;
    d.nerf_batch_size = 4096;
    d.samples_per_corner = 8;
    d.appearance_embedding = -1;
    d.max_guided_samples = 128;
    std::memcpy(opt, &d, sizeof(*opt));
}

void mnv_camera_init(mnv_camera *cam, int32_t width, int32_t height, float fx, float fy, float cx, float cy) {
    const viewer::Camera c(width, height, fx, fy, cx, cy);
    *cam = c.c_abi();
}

void mnv_camera_set_pose(mnv_camera *cam, const float center[3], const float v_back[3], const float v_world_up[3]) {
    viewer::Camera c(cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy);
    c.center = {center[0], center[1], center[2]};
    c.v_back = {v_back[0], v_back[1], v_back[2]};
    c.v_world_up = {v_world_up[0], v_world_up[1], v_world_up[2]};
    c._update();
    std::memcpy(cam->c2w, c.transform, sizeof(cam->c2w));
}

void mnv_camera_drag(mnv_camera *cam, float center[3], float v_back[3], const float v_world_up[3], float origin[3], float movement_speed,
                     int is_pan, int about_origin, float x0, float y0, float x1, float y1) {
    viewer::Camera c(cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy);
    c.center = {center[0], center[1], center[2]};
    c.v_back = {v_back[0], v_back[1], v_back[2]};
    c.v_world_up = {v_world_up[0], v_world_up[1], v_world_up[2]};
    c.origin = {origin[0], origin[1], origin[2]};
    c.movement_speed = movement_speed;
    c._update();
    c.begin_drag(x0, y0, is_pan != 0, about_origin != 0);
    c.drag_update(x1, y1);
    c.end_drag();
    c._update();  // what the next frame does (VolumeRenderer::render -> camera._update)
    for (int i = 0; i < 3; ++i) {
        center[i] = c.center[i];
        v_back[i] = c.v_back[i];
        origin[i] = c.origin[i];
    }
    std::memcpy(cam->c2w, c.transform, sizeof(cam->c2w));
}

int mnv_n3tree_open(const char *npz_path, mnv_n3tree **out) {
    if (!npz_path || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        auto *t = new mnv_n3tree();
        try {
            t->tree.open(npz_path);
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
        return MNV_OK;
    });
}

int mnv_n3tree_from_arrays(const mnv_tree_view *host_view, mnv_n3tree **out) {
    if (!host_view || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        auto *t = new mnv_n3tree();
        try {
            t->tree.assign(*host_view);
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
        return MNV_OK;
    });
}

void mnv_n3tree_free(mnv_n3tree *t) { delete t; }

int mnv_n3tree_host_view(const mnv_n3tree *t, mnv_tree_view *view) {
    if (!t || !view) return mnv::set_error(MNV_E_INVALID, "null argument");
    *view = t->tree.host_view();
    return MNV_OK;
}

int mnv_n3tree_move_to_device(mnv_n3tree *t, int64_t max_capacity, int need_parent, int need_sample_counts,
                              void *hip_stream) {
    if (!t) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (mnv_device_count() <= 0) return mnv::set_error(MNV_E_NO_DEVICE, "no HIP device visible");
    return guarded([&] {
        t->tree.move_to_device((long)max_capacity, need_parent != 0, need_sample_counts != 0, hip_stream);
        return MNV_OK;
    });
}

int mnv_n3tree_device_view(const mnv_n3tree *t, mnv_tree_view *view) {
    if (!t || !view) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (!t->tree.on_device()) return mnv::set_error(MNV_E_INVALID, "tree is not on the device");
    *view = t->tree.device_view();
    return MNV_OK;
}

const mnv_accel *mnv_n3tree_accel(const mnv_n3tree *t) { return t ? t->tree.device.accel : nullptr; }

int mnv_n3tree_save_npz(const mnv_n3tree *t, const char *npz_path) {
    if (!t || !npz_path) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        t->tree.save_npz(npz_path);
        return MNV_OK;
    });
}

int mnv_n3tree_gen_wireframe(const mnv_n3tree *t, int32_t max_depth, float *out, int64_t cap_floats, int64_t *n_floats) {
    if (n_floats) *n_floats = 0;
    if (!t) return mnv::set_error(MNV_E_INVALID, "null tree");
    if (cap_floats < 0 || (cap_floats > 0 && !out)) return mnv::set_error(MNV_E_INVALID, "invalid output buffer");
    return guarded([&] {
        const int64_t n = t->tree.gen_wireframe_floats(max_depth);  // counts, builds nothing
        if (n_floats) *n_floats = n;
        if (!out && cap_floats == 0) return (int)MNV_OK;
        if (cap_floats < n) return mnv::set_error(MNV_E_INVALID, "buffer too small (n_floats holds the length)");
        t->tree.gen_wireframe_into(max_depth, out);
        return (int)MNV_OK;
    });
}

int mnv_n3tree_make_lod(mnv_n3tree *t, int32_t max_depth, mnv_n3tree **out) {
    if (!t || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    *out = nullptr;
    return guarded([&] {
        auto *h = new mnv_n3tree();
        try {
            t->tree.make_lod_into(h->tree, max_depth);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return MNV_OK;
    });
}

int mnv_n3tree_make_view_lod(mnv_n3tree *t, const mnv_lod_view *views, int32_t n_views, float pixels, int32_t min_depth, int32_t max_depth,
                             int64_t *kept_at_depth, mnv_n3tree **out) {
    if (!t || !out || !views) return mnv::set_error(MNV_E_INVALID, "null argument");
    *out = nullptr;
    if (n_views < 1 || n_views > 4096) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_make_view_lod: n_views outside [1, 4096]");
    return guarded([&] {
        auto *h = new mnv_n3tree();
        try {
            t->tree.make_view_lod_into(h->tree, std::vector<mnv_lod_view>(views, views + n_views), pixels, min_depth, max_depth, nullptr, kept_at_depth);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return MNV_OK;
    });
}

int mnv_n3tree_make_culled(mnv_n3tree *t, const mnv_camera *cams, int32_t n_cams, const mnv_render_options *opt, float weight_thresh, int64_t *kept_at_depth,
                           mnv_cull_counts *counts, mnv_n3tree **out) {
    if (!t || !out || !cams || !opt) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_make_culled: null argument");
    *out = nullptr;
    if (n_cams < 1) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_make_culled: no camera");
    return guarded([&] {
        auto *h = new mnv_n3tree();
        try {
            t->tree.make_culled_into(h->tree, std::vector<mnv_camera>(cams, cams + n_cams), *opt, weight_thresh, nullptr, kept_at_depth, counts);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return MNV_OK;
    });
}

int mnv_n3tree_from_points(const mnv_points_params *p, const float *xyz, const uint8_t *rgb, int64_t n, void *hip_stream, mnv_points_stats *stats,
                           mnv_n3tree **out) {
    if (!p || !out) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_from_points: null argument");
    *out = nullptr;
    return guarded([&] {
        auto *h = new mnv_n3tree();
        try {
            viewer::N3Tree::from_points_into(h->tree, *p, xyz, rgb, n, hip_stream, stats);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return MNV_OK;
    });
}

int mnv_n3tree_merge(mnv_n3tree *a, const mnv_n3tree *b, const mnv_merge_params *p, mnv_merge_stats *stats, mnv_n3tree **out) {
    if (!a || !b || !p || !out) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_merge: null argument");
    *out = nullptr;
    return guarded([&] {
        auto *h = new mnv_n3tree();
        try {
            a->tree.merge_into(h->tree, b->tree, *p, nullptr, stats);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return MNV_OK;
    });
}

int mnv_n3tree_fit(mnv_n3tree *t, const mnv_camera *cams, int32_t n_cams, const float *const *targets, const mnv_render_options *opt,
                   const mnv_fit_params *params, int64_t *se_q32_out) {
    if (!t || !cams || !targets || !opt || !params) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit: null argument");
    if (n_cams < 1) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit: no camera");
    return guarded([&] {
        const std::vector<int64_t> se = t->tree.fit(std::vector<mnv_camera>(cams, cams + n_cams), std::vector<const float *>(targets, targets + n_cams), *opt, *params);
        if (se_q32_out) std::copy(se.begin(), se.end(), se_q32_out);
        return MNV_OK;
    });
}

int mnv_n3tree_fit_to_tree(mnv_n3tree *t, const mnv_n3tree *teacher, const mnv_camera *cams, int32_t n_cams, const mnv_render_options *opt,
                           const mnv_fit_params *params, int64_t *se_q32_out) {
    if (!t || !teacher || !cams || !opt || !params) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit_to_tree: null argument");
    if (n_cams < 1) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit_to_tree: no camera");
    return guarded([&] {
        const std::vector<int64_t> se = t->tree.fit_to(teacher->tree, std::vector<mnv_camera>(cams, cams + n_cams), *opt, *params);
        if (se_q32_out) std::copy(se.begin(), se.end(), se_q32_out);
        return MNV_OK;
    });
}

namespace {
void copy_fit_sums(const std::vector<mnv_fit_sums> &sums, int64_t *se_q32_out, int64_t *n_rays_out) {
    for (size_t i = 0; i < sums.size(); ++i) {
        if (se_q32_out) se_q32_out[i] = sums[i].se_q32;
        if (n_rays_out) n_rays_out[i] = sums[i].n_rays;
    }
}
}  // namespace

int mnv_n3tree_fit_ex(mnv_n3tree *t, const mnv_camera *cams, int32_t n_cams, const float *const *targets, const mnv_render_options *opt,
                      const mnv_fit_params_ex *p, int64_t *se_q32_out, int64_t *n_rays_out) {
    if (!t || !cams || !targets || !opt || !p) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit_ex: null argument");
    if (n_cams < 1) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit_ex: no camera");
    return guarded([&] {
        copy_fit_sums(t->tree.fit_ex(std::vector<mnv_camera>(cams, cams + n_cams), std::vector<const float *>(targets, targets + n_cams), *opt, *p), se_q32_out,
                      n_rays_out);
        return MNV_OK;
    });
}

int mnv_n3tree_fit_to_tree_ex(mnv_n3tree *t, const mnv_n3tree *teacher, const mnv_camera *cams, int32_t n_cams, const mnv_render_options *opt,
                              const mnv_fit_params_ex *p, int64_t *se_q32_out, int64_t *n_rays_out) {
    if (!t || !teacher || !cams || !opt || !p) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit_to_tree_ex: null argument");
    if (n_cams < 1) return mnv::set_error(MNV_E_INVALID, "mnv_n3tree_fit_to_tree_ex: no camera");
    return guarded([&] {
        copy_fit_sums(t->tree.fit_to_ex(teacher->tree, std::vector<mnv_camera>(cams, cams + n_cams), *opt, *p), se_q32_out, n_rays_out);
        return MNV_OK;
    });
}

void mnv_data_format_parse(const char *str, int32_t *format, int32_t *basis_dim) {
    viewer::DataFormat f;
    f.parse(str ? str : "");
    if (format) *format = f.format == viewer::DataFormat::SH ? MNV_FORMAT_SH : MNV_FORMAT_RGBA;
    if (basis_dim) *basis_dim = f.basis_dim;
}

int mnv_data_format_to_string(int32_t format, int32_t basis_dim, char *buf, size_t buflen) {
    viewer::DataFormat f;
    f.format = format == MNV_FORMAT_SH ? viewer::DataFormat::SH : viewer::DataFormat::RGBA;
    f.basis_dim = basis_dim;
    const std::string s = f.to_string();
    if (!buf || buflen <= s.size()) return mnv::set_error(MNV_E_INVALID, "buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return MNV_OK;
}

/* ---- anti-aliasing: the sample pattern and the filter tables (the recipes are stated in include/mnv.h; the tests restate them) */

int mnv_aa_pattern(int32_t n_samples, float *offsets_xy) {
    if (n_samples < 1 || n_samples > MNV_MAX_BATCH) return mnv::set_error(MNV_E_INVALID, "mnv_aa_pattern: need 1 .. MNV_MAX_BATCH samples");
    if (!offsets_xy) return mnv::set_error(MNV_E_INVALID, "mnv_aa_pattern: null output");
    viewer::aa_pattern(n_samples, offsets_xy);
    return MNV_OK;
}

int mnv_aa_weights(int32_t filter, int32_t n_samples, const float *offsets_xy, int32_t *radius_out, float *weights, int64_t cap_floats,
                   int64_t *n_floats) {
    if (n_floats) *n_floats = 0;
    if (radius_out) *radius_out = 0;
    if (filter != MNV_AA_BOX && filter != MNV_AA_TENT) return mnv::set_error(MNV_E_INVALID, "mnv_aa_weights: unknown filter");
    if (n_samples < 1 || n_samples > MNV_MAX_BATCH) return mnv::set_error(MNV_E_INVALID, "mnv_aa_weights: need 1 .. MNV_MAX_BATCH samples");
    if (!offsets_xy) return mnv::set_error(MNV_E_INVALID, "mnv_aa_weights: null offsets");
    if (cap_floats < 0 || (cap_floats > 0 && !weights)) return mnv::set_error(MNV_E_INVALID, "invalid output buffer");
    const int r = viewer::aa_filter_radius(filter);
    const int64_t n = (int64_t)n_samples * (2 * r + 1) * (2 * r + 1);
    if (radius_out) *radius_out = r;
    if (n_floats) *n_floats = n;
    if (!weights && cap_floats == 0) return MNV_OK;
    if (cap_floats < n) return mnv::set_error(MNV_E_INVALID, "buffer too small (n_floats holds the length)");
    viewer::aa_weights(filter, n_samples, offsets_xy, weights);
    return MNV_OK;
}

int mnv_synth_random_tree(const mnv_synth_random_params *p, mnv_n3tree **out) {
    if (!p || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        auto *t = new mnv_n3tree();
        try {
            viewer::synth::random_tree(*p, t->tree);
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
        return MNV_OK;
    });
}

int mnv_synth_terrain_tree(const mnv_synth_terrain_params *p, mnv_n3tree **out) {
    if (!p || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        auto *t = new mnv_n3tree();
        try {
            viewer::synth::terrain_tree(*p, t->tree);
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
        return MNV_OK;
    });
}

int mnv_synth_shell_tree(const mnv_synth_shell_params *p, mnv_n3tree **out) {
    if (!p || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        auto *t = new mnv_n3tree();
        try {
            viewer::synth::shell_tree(*p, t->tree);
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
        return MNV_OK;
    });
}

/* ---- viewer::VolumeRenderer behind the C ABI (include/renderer/renderer.hpp:9-39) */

int mnv_renderer_create(mnv_renderer **out) {
    if (!out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        *out = new mnv_renderer();
        return MNV_OK;
    });
}

void mnv_renderer_destroy(mnv_renderer *r) { delete r; }

int mnv_renderer_set(mnv_renderer *r, mnv_n3tree *tree, int64_t max_tree_capacity) {
    if (!r || !tree) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (max_tree_capacity < tree->tree.capacity) return mnv::set_error(MNV_E_INVALID, "max_tree_capacity is smaller than the tree");
    return guarded([&] {
        r->rend.set(tree->tree, (long)max_tree_capacity);
        return MNV_OK;
    });
}

int mnv_renderer_load_model(mnv_renderer *r, const char *npz_path) {
    if (!r || !npz_path) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.load_model(npz_path);
        return MNV_OK;
    });
}

int mnv_renderer_set_model(mnv_renderer *r, const mnv_mlp_desc *desc, const uint16_t *params, size_t n_halfs, const mnv_cluster_grid *grid) {
    if (!r || !desc || !params || !grid) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.set_model(*desc, params, n_halfs, *grid);
        return MNV_OK;
    });
}

int mnv_renderer_resize(mnv_renderer *r, int32_t width, int32_t height) {
    if (!r || width < 1 || height < 1) return mnv::set_error(MNV_E_INVALID, "invalid size");
    return guarded([&] {
        r->rend.resize(width, height);
        return MNV_OK;
    });
}

mnv_render_options *mnv_renderer_options(mnv_renderer *r) { return r ? reinterpret_cast<mnv_render_options *>(&r->rend.options) : nullptr; }

int mnv_renderer_set_camera(mnv_renderer *r, float fx, float fy, const float center[3], const float v_back[3], const float v_world_up[3]) {
    if (!r || !center || !v_back || !v_world_up) return mnv::set_error(MNV_E_INVALID, "null argument");
    viewer::Camera &c = r->rend.camera;
    if (fx > 0.f) c.fx = c.default_fx = fx;
    if (fy > 0.f) c.fy = c.default_fy = fy;
    else if (fx > 0.f) c.fy = c.default_fy = fx;
    c.center = {center[0], center[1], center[2]};
    c.v_back = {v_back[0], v_back[1], v_back[2]};
    c.v_world_up = {v_world_up[0], v_world_up[1], v_world_up[2]};
    return MNV_OK;
}

int mnv_renderer_set_seed(mnv_renderer *r, uint64_t seed, int32_t accel_rebuild_after) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    r->rend.seed = seed;
    if (accel_rebuild_after >= 0) r->rend.accel_rebuild_after = accel_rebuild_after;
    return MNV_OK;
}

int mnv_renderer_render(mnv_renderer *r, mnv_renderer_stats *stats) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.render();
        if (stats) {
            const auto &s = r->rend.stats;
            stats->track_visit = s.track_visit;
            stats->used_accel = s.used_accel;
            stats->full = s.full;
            stats->split_candidates = s.split_candidates;
            stats->added = s.added;
            stats->sample_candidates = s.sample_candidates;
            stats->resampled = s.resampled;
            stats->pruned = s.pruned;
            stats->guided_samples = s.guided_samples;
            stats->capacity = s.capacity;
            stats->fused = s.fused;
            stats->reserved = 0;
        }
        return MNV_OK;
    });
}

int mnv_renderer_download(mnv_renderer *r, float *rgba, uint8_t *rgba8) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        std::vector<float> f;
        std::vector<uint8_t> u;
        r->rend.download(rgba ? &f : nullptr, rgba8 ? &u : nullptr);
        if (rgba) std::memcpy(rgba, f.data(), f.size() * sizeof(float));
        if (rgba8) std::memcpy(rgba8, u.data(), u.size());
        return MNV_OK;
    });
}

int mnv_renderer_set_frames_in_flight(mnv_renderer *r, int32_t count) {
    if (!r || count < 1 || count > 16) return mnv::set_error(MNV_E_INVALID, "frames in flight: 1 .. 16");
    return guarded([&] {
        r->rend.sync_tree_streams();
        r->rend.frames_in_flight = count;
        return MNV_OK;
    });
}

int mnv_renderer_set_guided_in_flight(mnv_renderer *r, int enable) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.sync_tree_streams();
        r->rend.guided_in_flight = enable != 0;
        return MNV_OK;
    });
}

int mnv_renderer_slot_guided_samples(mnv_renderer *r, int32_t slot, int64_t *count_out) {
    if (!r || !count_out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        *count_out = (int64_t)r->rend.slot_guided_samples(slot);
        return MNV_OK;
    });
}

int mnv_renderer_set_fused_guided(mnv_renderer *r, int enable) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    r->rend.use_fused_guided = enable != 0;
    return MNV_OK;
}

int mnv_renderer_set_frame_inputs(mnv_renderer *r, const float *tmax_px, const uint8_t *rgba8_init) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.set_frame_inputs(tmax_px, rgba8_init);
        return MNV_OK;
    });
}

int mnv_renderer_set_ranks(mnv_renderer *r, mnv_comm *comm, int32_t tile_w, int32_t tile_h) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (comm && (tile_w < 8 || tile_h < 8 || tile_w % 8 || tile_h % 8)) return mnv::set_error(MNV_E_INVALID, "macro tiles are multiples of 8 pixels");
    return guarded([&] {
        r->rend.set_ranks(comm, tile_w, tile_h);
        return MNV_OK;
    });
}

int32_t mnv_renderer_last_slot(const mnv_renderer *r) { return r ? r->rend.last_slot() : -1; }

int mnv_renderer_download_slot(mnv_renderer *r, int32_t slot, float *rgba, uint8_t *rgba8) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        std::vector<float> f;
        std::vector<uint8_t> u;
        r->rend.download_slot(slot, rgba ? &f : nullptr, rgba8 ? &u : nullptr);
        if (rgba) std::memcpy(rgba, f.data(), f.size() * sizeof(float));
        if (rgba8) std::memcpy(rgba8, u.data(), u.size());
        return MNV_OK;
    });
}

int mnv_renderer_sync_tree(mnv_renderer *r) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.sync_tree();
        return MNV_OK;
    });
}

const mnv_wireframe *mnv_renderer_wireframe(const mnv_renderer *r) { return r ? r->rend.wireframe() : nullptr; }

int mnv_renderer_camera(const mnv_renderer *r, mnv_camera *out) {
    if (!r || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    *out = r->rend.last_camera();
    return MNV_OK;
}

int mnv_renderer_set_antialiasing(mnv_renderer *r, int32_t samples, int32_t filter) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (filter != MNV_AA_BOX && filter != MNV_AA_TENT) return mnv::set_error(MNV_E_INVALID, "anti-aliasing: unknown filter");
    r->rend.aa_samples = samples;  // (a count render() cannot use is refused there, like the other combinations it refuses)
    r->rend.aa_filter = filter;
    return MNV_OK;
}

int mnv_renderer_set_projection(mnv_renderer *r, int32_t projection) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (projection != MNV_PROJ_PINHOLE && projection != MNV_PROJ_ORTHO && projection != MNV_PROJ_EQUIRECT)
        return mnv::set_error(MNV_E_INVALID, "projection: unknown projection");
    r->rend.projection = projection;  // (a combination render() cannot serve is refused there)
    return MNV_OK;
}

int mnv_renderer_set_target(mnv_renderer *r, const uint8_t *rgba8_device, int32_t flags) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.set_target(rgba8_device, flags);
        return MNV_OK;
    });
}

int mnv_renderer_set_lod(mnv_renderer *r, int32_t max_depth) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.set_lod(max_depth);
        return MNV_OK;
    });
}

int mnv_renderer_set_view_lod(mnv_renderer *r, const mnv_lod_view *views, int32_t n_views, float pixels, int32_t min_depth, int32_t max_depth) {
    if (!r || (n_views > 0 && !views)) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (n_views < 0 || n_views > 4096) return mnv::set_error(MNV_E_INVALID, "mnv_renderer_set_view_lod: n_views outside [0, 4096]");
    return guarded([&] {
        r->rend.set_view_lod(n_views ? std::vector<mnv_lod_view>(views, views + n_views) : std::vector<mnv_lod_view>(), pixels, min_depth, max_depth);
        return MNV_OK;
    });
}

int mnv_renderer_set_cull(mnv_renderer *r, const mnv_camera *cams, int32_t n_cams, float weight_thresh) {
    if (!r || (n_cams > 0 && !cams)) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (n_cams < 0) return mnv::set_error(MNV_E_INVALID, "mnv_renderer_set_cull: negative camera count");
    return guarded([&] {
        r->rend.set_cull(n_cams ? std::vector<mnv_camera>(cams, cams + n_cams) : std::vector<mnv_camera>(), weight_thresh);
        return MNV_OK;
    });
}

int mnv_renderer_set_lod_fit(mnv_renderer *r, const mnv_camera *cams, int32_t n_cams, const mnv_fit_params *params) {
    if (!r || !params || (n_cams > 0 && !cams)) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (n_cams < 0) return mnv::set_error(MNV_E_INVALID, "mnv_renderer_set_lod_fit: negative camera count");
    return guarded([&] {
        r->rend.set_lod_fit(n_cams ? std::vector<mnv_camera>(cams, cams + n_cams) : std::vector<mnv_camera>(), *params);
        return MNV_OK;
    });
}

int mnv_renderer_set_lod_fit_ex(mnv_renderer *r, const mnv_camera *cams, int32_t n_cams, const mnv_fit_params_ex *params) {
    if (!r || !params || (n_cams > 0 && !cams)) return mnv::set_error(MNV_E_INVALID, "null argument");
    if (n_cams < 0) return mnv::set_error(MNV_E_INVALID, "mnv_renderer_set_lod_fit_ex: negative camera count");
    return guarded([&] {
        r->rend.set_lod_fit(n_cams ? std::vector<mnv_camera>(cams, cams + n_cams) : std::vector<mnv_camera>(), *params);
        return MNV_OK;
    });
}

int mnv_renderer_slot_metrics(mnv_renderer *r, int32_t slot, mnv_frame_metric_values *out) {
    if (!r || !out) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.slot_metrics(slot, out);
        return MNV_OK;
    });
}

int mnv_model_matrix(const float rotation[3], const float translation[3], float scale, float *matrix3x4_out) {
    if (!rotation || !translation || !matrix3x4_out) return mnv::set_error(MNV_E_INVALID, "mnv_model_matrix: null argument");
    viewer::model_matrix(rotation, translation, scale, matrix3x4_out);
    return MNV_OK;
}

int mnv_obj_read(const char *path, const float *default_color, float *vert, int64_t cap_floats, int64_t *n_floats, uint32_t *faces,
                 int64_t cap_indices, int64_t *n_indices, int32_t *face_size) {
    if (!path) return mnv::set_error(MNV_E_INVALID, "mnv_obj_read: null path");
    return guarded([&] {
        const viewer::Mesh m = viewer::Mesh::load_obj(path, default_color);
        if (n_floats) *n_floats = (int64_t)m.vert.size();
        if (n_indices) *n_indices = (int64_t)m.faces.size();
        if (face_size) *face_size = m.face_size;
        if (!vert && !faces) return cap_floats == 0 && cap_indices == 0 ? MNV_OK : mnv::set_error(MNV_E_INVALID, "mnv_obj_read: null buffers");
        if ((!vert && !m.vert.empty()) || cap_floats < (int64_t)m.vert.size() || (!faces && !m.faces.empty()) || cap_indices < (int64_t)m.faces.size())
            return mnv::set_error(MNV_E_INVALID, "mnv_obj_read: buffer too small (n_floats / n_indices hold the sizes)");
        if (!m.vert.empty()) std::memcpy(vert, m.vert.data(), m.vert.size() * sizeof(float));
        if (!m.faces.empty()) std::memcpy(faces, m.faces.data(), m.faces.size() * sizeof(uint32_t));
        return MNV_OK;
    });
}

int mnv_obj_write(const char *path, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size) {
    if (!path) return mnv::set_error(MNV_E_INVALID, "mnv_obj_write: null path");
    return guarded([&] {
        viewer::write_obj(path, vert, n_verts, faces, n_indices, face_size);
        return MNV_OK;
    });
}

int mnv_renderer_add_mesh(mnv_renderer *r, const mnv_mesh *mesh) {
    if (!r || !mesh) return mnv::set_error(MNV_E_INVALID, "null argument");
    r->rend.meshes.push_back(mesh);
    return MNV_OK;
}

int mnv_renderer_clear_meshes(mnv_renderer *r) {
    if (!r) return mnv::set_error(MNV_E_INVALID, "null argument");
    return guarded([&] {
        r->rend.sync_tree_streams();  // frames in flight draw the listed meshes
        r->rend.meshes.clear();
        return MNV_OK;
    });
}

int32_t mnv_renderer_mesh_count(const mnv_renderer *r) { return r ? (int32_t)r->rend.meshes.size() : 0; }

}  // extern "C"
