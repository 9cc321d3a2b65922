#include "volume_renderer.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "npz.hpp"

namespace viewer {

namespace {
void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
void mnv_check(int rc, const char *what) {
    if (rc != MNV_OK) throw std::runtime_error(std::string(what) + ": " + mnv_last_error());
}
double radical_inverse(int i, int b) {  // include/mnv.h, mnv_aa_pattern
    double f = 1, r = 0;
    while (i > 0) {
        f = f / b;
        r = r + f * (i % b);
        i = i / b;
    }
    return r;
}
}  // namespace

void aa_pattern(int n_samples, float *offsets_xy) {
    if (n_samples == 1) {
        offsets_xy[0] = offsets_xy[1] = 0.f;
        return;
    }
    for (int k = 0; k < n_samples; ++k) {
        offsets_xy[2 * k] = (float)(radical_inverse(k + 1, 2) - 0.5);
        offsets_xy[2 * k + 1] = (float)(radical_inverse(k + 1, 3) - 0.5);
    }
}

int aa_filter_radius(int filter) { return filter == MNV_AA_TENT ? 1 : 0; }

void aa_weights(int filter, int n_samples, const float *offsets_xy, float *weights) {
    if (filter != MNV_AA_TENT) {  // box
        for (int k = 0; k < n_samples; ++k) weights[k] = 1.f;
        return;
    }
    for (int k = 0; k < n_samples; ++k)
        for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i) {
                const double wx = std::max(0.0, 1.0 - std::fabs((double)i + (double)offsets_xy[2 * k]));
                const double wy = std::max(0.0, 1.0 - std::fabs((double)j + (double)offsets_xy[2 * k + 1]));
                weights[(k * 3 + (j + 1)) * 3 + (i + 1)] = (float)(wx * wy);
            }
}

// a grow-only refinement buffer as `count` elements of T
using Bytes = mnv::Buffer<uint8_t>;
template <typename T>
T *sized(Bytes &b, size_t count) {
    const size_t need = count * sizeof(T);
    hip_check(mnv::grow(b, need, need + need / 8, nullptr, false), "hipMalloc(refinement buffer)");
    return reinterpret_cast<T *>(b.get());
}

// a device / pinned pair; a failure carries the text of the half that failed
template <typename T>
void alloc_pair(mnv::Mirrored<T> &m, const char *dev_text, const char *pinned_text) {
    bool pinned = false;
    const hipError_t e = m.alloc(1, &pinned);
    hip_check(e, pinned ? pinned_text : dev_text);
}

// What the next render() does, decided from the renderer's state and options alone (VolumeRenderer::plan()).  render() issues exactly
// this; overlaps_next() / next_slot() report it.
struct VolumeRenderer::FramePlan {
    enum Kind {
        BACKGROUND,        // no tree: the background (over the meshes) on slot 0
        PLAIN,             // the march on the packed accel, beside the frames in flight
        GUIDED_IN_FLIGHT,  // the fused guided kernel with nothing but the picture wanted from it, beside the frames in flight
        TREE,              // alone on slot 0, may edit the tree: march() names the entry points
        RANKS,             // this rank's share of a frame of several ranks (set_ranks), alone on slot 0
        AA,                // aa_samples jittered sub-frames and their resolve
        PROJECTED          // the ray list of an orthographic / equirectangular camera
    } kind = BACKGROUND;
    bool overlaps = false;   // takes the next slot beside the frames in flight; false: waits for them and runs alone on slot 0
    bool show_grid = false;  // draws its own inputs: the grid pass, ...
    bool draws_inputs = false;  // ... the visible meshes, or both
    bool refines = false;    // a TREE / RANKS frame with a model and use_splitting / use_guided_sampling: trackers, visit marks, tree edits
    // TREE: which march.  Whether the frame takes visit marks is known only once the prelude has read camera.has_changed(), a latch that
    // frames which pass their refusals alone may consume; marks on the packed layout need the tree's parent array, a marks frame of a
    // tree without one reads the reference layout.
    bool guided = false, fused = false, packed = false, has_parent = false;
    enum March { FUSED_GUIDED, FOUR_STEP_GUIDED, TRACKED_ACCEL, REFERENCE_LAYOUT };
    bool on_accel(bool track_visit) const { return packed && (!track_visit || has_parent); }  // (FOUR_STEP_GUIDED: its sample march)
    March march(bool track_visit) const {
        if (guided) return fused && on_accel(track_visit) ? FUSED_GUIDED : FOUR_STEP_GUIDED;
        return on_accel(track_visit) ? TRACKED_ACCEL : REFERENCE_LAYOUT;
    }
    const char *refusal = nullptr;   // refused (nothing else of the plan is filled in) ...
    bool refusal_is_status = false;  // ... with StatusError(MNV_E_INVALID); false: std::runtime_error
};

struct VolumeRenderer::Impl {
    N3Tree *tree = nullptr;
    long max_tree_capacity = 0;
    mnv_frame_inputs inputs = {nullptr, nullptr};  // offscreen == false: the caller's depth image and image (set_frame_inputs); the _ex entry
                                                   // points take a block of two nulls as offscreen == true
    // Frames in flight.  The reference calls render_voxels once per frame on one stream (cuda_renderer.cpp:141-142); a single
    // 1080p launch of the march ends in a tail of a few wavefronts finishing the longest rays (a third of the wave slots idle
    // on average), so plain frames rotate over `slots` -- each with its own stream and frame buffers -- and the tail of frame k
    // overlaps frames k+1, k+2.  Frames that refine the tree run one at a time on slot 0 (they mutate what the next one reads).
    struct Slot {
        hipStream_t stream = nullptr;
        mnv::Buffer<float> rgba;
        mnv::Buffer<uint8_t> rgba8;
        mnv::Mirrored<unsigned long long> count;  // guided frames in flight: this slot's sample counter and its pinned copy
        bool counted = false;                     // ... which a frame on this slot has written (or is about to)
        mnv::Buffer<float> grid_tmax;             // show_grid: this slot's depth image and image under the volume
        mnv::Buffer<uint8_t> grid_rgba8;
        mnv::Buffer<float> aa_sub;                // aa_samples > 1: this slot's K float sub-frames
        mnv::Buffer<float> ray_origins, ray_dirs;  // projection != pinhole: this slot's rays, [height][width][3] each
        mnv::Mirrored<mnv_metric_sums> sums;      // set_target: this slot's sums and their pinned copy
        bool scored = false;                      // ... which the last frame on this slot has written (or is about to)
    };
    std::vector<Slot> slots;
    int cur = 0;            // slot of the most recent render()
    bool overlapped = false;  // plain frames may still be running on slots other than 0
    bool tree_stream_dirty = false;  // slot 0's stream may still be editing the tree / accel (a frame other than a plain one ran last)
    hipStream_t stream = nullptr;  // = slots[0].stream: refinement, tree upload, accel patches
    float *rgba = nullptr;         // = slots[cur]
    uint8_t *rgba8 = nullptr;
    int width = 0, height = 0;
    bool initial_resize = true;
    const uint8_t *target = nullptr;  // set_target: the caller's device image every frame is scored against, and the flags of the score
    int target_flags = 0;
    void clear_target() {
        target = nullptr;
        for (Slot &s : slots) s.scored = false;
    }

    // refinement state (cuda_renderer.cpp:441-468,571-600)
    mnv_mlp *mlp = nullptr;
    mnv_mlp_desc mlp_desc{};
    mnv_cluster_grid grid{};
    Bytes split_tracker, sample_tracker, visit_tracker, num_samples, cluster_indices, guided_samples;
    Bytes offsets, z_vals, sample_rows, sample_clusters, nerf_results;
    Bytes nodes, rand_sample, rand_clusters, results, fused_counter;
    // several ranks (set_ranks): this rank's share of the frame in compact tile-major order, the gather table on rank 0, the marks table
    mnv_comm *comm = nullptr;
    mnv_partition part = {0, 1, 0, 0, 0};
    int64_t rank_px = 0;  // pixels per rank in the compact layout: j_max macro tiles
    Bytes local, local8, table, table8, marks_table;
    int64_t tracker_rows() const { return comm ? rank_px * part.world : (int64_t)width * height; }
    bool fused_inputs_ok = false;  // the model's encoded input fits the fused guided kernel (<= 64 features)
    bool prune_happened = false, can_reuse_results = false;
    bool marks_fresh = false, want_marks = false;  // see render(): prune only after a track_visit frame
    long reuse_total = 0;
    uint64_t frame = 0;
    // show_grid: the device edge list, the depth and the tree structure it was made for (tree_version counts set / splits / prunes)
    mnv_wireframe *wire = nullptr;
    mnv_camera last_camera{};  // the camera of the last render()
    int wire_depth = 0;
    uint64_t tree_version = 0, wire_version = 0;
    // anti-aliasing: what the device weight table (shared by the slots) and the slots' sub-frame buffers were made for
    int aa_k = 1, aa_filter = -1, aa_radius = 0;
    mnv::Buffer<float> aa_weights_dev;
    std::vector<float> aa_offsets;
    void free_aa() {  // (the streams are idle)
        for (Slot &s : slots) s.aa_sub.reset();
        aa_weights_dev.reset();
        aa_k = 1;
        aa_filter = -1;
    }
    // projection == MNV_PROJ_EQUIRECT: the device table of mnv_equirect_tables (shared by the slots) and the size it was made for
    mnv::Buffer<float> equirect_dev;
    int equirect_w = 0, equirect_h = 0;
    // set_lod: the depth frames are cut at (0: off), the truncated trees built so far (one per depth) and the structure of `tree` they
    // were made from (tree_version), and the tree this frame marches (set by update_shared; null: `tree` itself)
    int lod = 0, wire_lod = 0;
    struct LodTree {
        int depth;
        std::unique_ptr<N3Tree> tree;
    };
    std::vector<LodTree> lod_trees;
    uint64_t lod_version = 0;
    N3Tree *lod_tree = nullptr;
    // set_view_lod: the viewpoints (empty: off) and parameters of the view-dependent cut, the tree built for them (until they change or
    // the trees above go), and a number that changes with every call (the grid overlay's edge list belongs to one of them)
    std::vector<mnv_lod_view> view_lod_views;
    float view_lod_pixels = 1.f;
    int view_lod_min = 1, view_lod_max = 23;
    std::unique_ptr<N3Tree> view_lod_tree;
    int view_lod_gen = 0, wire_view_gen = 0;
    int view_lod_token() const { return view_lod_views.empty() ? 0 : view_lod_gen; }
    // set_cull: the cameras (empty: off) and the threshold of the culled tree, the tree built for them with the march options it was built
    // under (until cameras, threshold or those options change, or the trees above go), and a number that changes with every call
    std::vector<mnv_camera> cull_cams;
    float cull_thresh = 0.f;
    std::unique_ptr<N3Tree> cull_tree;
    mnv_render_options cull_opt{};
    int cull_gen = 0, wire_cull_gen = 0;
    int cull_token() const { return cull_cams.empty() ? 0 : cull_gen; }
    // the options the visibility march depends on (render_depth changes no weight and is switched off for it)
    static bool same_march(const mnv_render_options &a, const mnv_render_options &b) {
        return a.step_size == b.step_size && a.sigma_thresh == b.sigma_thresh && a.stop_thresh == b.stop_thresh &&
               std::memcmp(a.render_bbox, b.render_bbox, sizeof(a.render_bbox)) == 0;
    }
    // set_lod_fit: the cameras and parameters every level of detail is fitted with when it is built (no iterations: off)
    std::vector<mnv_camera> lod_fit_cams;
    mnv_fit_params_ex lod_fit{};
    void fit_lod(N3Tree &cut, const RenderOptions &o) {
        if (lod_fit.steps > 0 && !lod_fit_cams.empty()) cut.fit_to_ex(*tree, lod_fit_cams, *o.c_abi(), lod_fit, stream);
    }
    N3Tree &march_tree() const { return lod_tree ? *lod_tree : *tree; }
    void drop_lod_trees() {  // (frames in flight may march them)
        if (!lod_trees.empty() || view_lod_tree || cull_tree) sync_all();
        lod_trees.clear();
        view_lod_tree.reset();
        cull_tree.reset();
        lod_tree = nullptr;
    }
    // what draws this frame's inputs (set by render()): the grid, the visible meshes of VolumeRenderer::meshes, or both
    bool pass_grid = false;
    std::vector<const mnv_mesh *> pass_meshes;
    // the grid pass and / or the mesh pass of this frame into slot S's images on `st`, returned as the frame's inputs (the edge list is
    // current); the meshes are drawn over the grid, in place
    mnv_frame_inputs grid_inputs(Slot &S, hipStream_t st, const mnv_camera &cv, const RenderOptions &o) {
        if (!S.grid_tmax || !S.grid_rgba8) {
            hip_check(S.grid_tmax.alloc((size_t)width * height), "hipMalloc(grid depth image)");
            hip_check(S.grid_rgba8.alloc((size_t)width * height * 4), "hipMalloc(grid image)");
        }
        const mnv_frame_inputs in = {S.grid_tmax.get(), S.grid_rgba8.get()};
        if (pass_grid) mnv_check(mnv_render_wireframe(wire, &cv, o.c_abi(), {0, 0, width, height}, S.grid_tmax.get(), S.grid_rgba8.get(), st), "mnv_render_wireframe");
        if (!pass_meshes.empty())
            mnv_check(mnv_render_meshes(pass_meshes.data(), (int32_t)pass_meshes.size(), &cv, o.c_abi(), {0, 0, width, height}, pass_grid ? &in : nullptr,
                                        S.grid_tmax.get(), S.grid_rgba8.get(), st),
                      "mnv_render_meshes");
        return in;
    }
    // the inputs of a frame on the slot it has taken: drawn by the frame itself, or the caller's (set_frame_inputs)
    mnv_frame_inputs frame_inputs(const FramePlan &P, const mnv_camera &cv, const RenderOptions &o) {
        return P.draws_inputs ? grid_inputs(slots[cur], slots[cur].stream, cv, o) : inputs;
    }
    // the fused guided kernel's sample count: copied to pinned memory behind the kernel and read at the frame's LAST wait (the vote's,
    // the tree edit's) instead of at a wait of its own right behind the march -- 20-40 us of a refinement frame
    mnv::PinnedBuffer<unsigned long long> count_host;
    bool count_pending = false;
    void read_count_later(const unsigned long long *counter) {
        if (!count_host) hip_check(count_host.alloc(1), "hipHostMalloc(sample count)");
        hip_check(hipMemcpyAsync(count_host.get(), counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "read sample counter");
        count_pending = true;
    }
    void finish_count(FrameStats &st) {
        if (!count_pending) return;
        hip_check(hipStreamSynchronize(stream), "guided frame");
        st.guided_samples = (long)*count_host.get();
        count_pending = false;
    }

    Impl() {
        slots.resize(1);
        hip_check(hipStreamCreate(&slots[0].stream), "hipStreamCreate");
        stream = slots[0].stream;
    }
    ~Impl() {
        free_frame();  // (waits for every stream)
        if (wire) mnv_wireframe_destroy(wire);
        if (mlp) mnv_mlp_destroy(mlp);
        for (Slot &s : slots)
            if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    void sync_all() {
        for (Slot &s : slots) hip_check(hipStreamSynchronize(s.stream), "hipStreamSynchronize");
        overlapped = false;
    }
    void free_frame() {
        for (Slot &s : slots) {
            if (s.stream) (void)hipStreamSynchronize(s.stream);
            s.rgba.reset();
            s.rgba8.reset();
            s.grid_tmax.reset();
            s.grid_rgba8.reset();
            s.aa_sub.reset();
            s.ray_origins.reset();
            s.ray_dirs.reset();
        }
        rgba = nullptr;
        rgba8 = nullptr;
    }
    // make `n` slots exist, each with a stream and frame buffers of the current size
    void ensure_slots(int n) {
        if (n < 1) n = 1;
        while ((int)slots.size() < n) {
            Slot s;
            hip_check(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "hipStreamCreate");
            slots.push_back(std::move(s));
        }
        for (int i = 0; i < n; ++i) {
            Slot &s = slots[i];
            if ((!s.rgba || !s.rgba8) && width > 0 && height > 0) {
                hip_check(s.rgba.alloc((size_t)width * height * 4), "hipMalloc(frame)");
                hip_check(s.rgba8.alloc((size_t)width * height * 4), "hipMalloc(frame8)");
            }
        }
    }
    void use_slot(int i) {
        cur = i;
        rgba = slots[i].rgba.get();
        rgba8 = slots[i].rgba8.get();
    }
    // The frame's slot: the next one beside the frames in flight, or slot 0 alone once they have finished.
    Slot &take_slot(const FramePlan &P, int frames_in_flight) {
        if (P.overlaps) {
            // Slot streams are not ordered among each other.  Whatever slot 0's stream still holds from a frame that changed the tree
            // or its accel (splits, resampled leaves, accel patches, a prune's renumbering: asynchronous on that stream) must be
            // finished before a frame on another stream reads those arrays: once, on the way from such frames to overlapped ones.
            if (tree_stream_dirty) {
                hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
                tree_stream_dirty = false;
            }
            ensure_slots(frames_in_flight);
            use_slot((cur + 1) % frames_in_flight);
            overlapped = true;
        } else {
            if (overlapped) sync_all();
            use_slot(0);
            // What follows runs on slot 0's stream and may edit the tree.  Anti-aliased and projected frames only read it; they never
            // raised the flag, and raising it now would add a wait on the way back to frames in flight (frames_in_flight raised since).
            if (P.kind != FramePlan::AA && P.kind != FramePlan::PROJECTED) tree_stream_dirty = true;
        }
        slots[cur].counted = false;  // (a guided frame in flight raises it; every other kind's sample count is in `stats`)
        return slots[cur];
    }
    void fill_f32(float *p, size_t n, float v) {
        uint32_t bits;
        std::memcpy(&bits, &v, 4);
        hip_check(hipMemsetD32Async((hipDeviceptr_t)p, (int)bits, n, stream), "fill");
    }
    mnv_tree_edit edit() const {
        mnv_tree_edit e{};
        e.child = tree->device.child.get();
        e.parent = tree->device.parent.get();
        for (int i = 0; i < 3; ++i) {
            e.offset[i] = tree->offset[i];
            e.scale[i] = tree->scale[i];
        }
        e.N = tree->N;
        e.capacity = tree->capacity;
        return e;
    }
    int sample_cols(const RenderOptions &o) const { return 3 + (o.need_viewdir ? 3 : 0) + (o.appearance_embedding != -1 ? 1 : 0); }

    // The refinement prelude of a TREE / RANKS frame (cuda_renderer.cpp:97-107): whether the frame takes visit marks, and the tracker
    // rows of the whole frame (tracker_rows(); on several ranks block r holds rank r's rows), of which this frame writes those from
    // `first_row` on.
    struct Trackers {
        bool track_visit = false;
        float *split = nullptr, *sample = nullptr, *my_split = nullptr, *my_sample = nullptr;  // null: no splitting
        int32_t *visited = nullptr;
    };
    Trackers begin_refinement(const FramePlan &P, Camera &camera, const RenderOptions &o, FrameStats &st, int64_t first_row) {
        Trackers T;
        const bool camera_has_changed = camera.has_changed();
        T.track_visit = P.refines && ((camera_has_changed && tree->capacity > max_tree_capacity * 3 / 4) || prune_happened || want_marks);
        if (camera_has_changed) can_reuse_results = false;
        st.track_visit = T.track_visit;
        T.visited = sized<int32_t>(visit_tracker, (size_t)std::max<long>(max_tree_capacity, 1));
        if (P.refines && o.use_splitting) {
            const int64_t rows = tracker_rows();
            T.split = sized<float>(split_tracker, rows * 3);
            T.sample = sized<float>(sample_tracker, rows * 3);
            // The fused kernel writes all three words of both rows for every pixel it renders, so a healthy fused frame does not need
            // the fill (50 us of a 3 ms configs[4] frame) -- but a wavefront that its watchdog abandoned (MNV_E_FAULT, reported by the
            // NEXT fused call) leaves its pixels' rows unwritten, and refine_after_frame edits the tree from these rows in this same
            // frame: stale (chunk, child) pairs of an earlier frame may name chunks a prune has renumbered since.  -1 rows name nothing.
            fill_f32(T.split, rows * 3, -1.f);
            fill_f32(T.sample, rows * 3, -1.f);
            T.my_split = T.split + first_row * 3;
            T.my_sample = T.sample + first_row * 3;
        }
        return T;
    }
    // ... and the epilogue of every frame of a tree: the vote and the tree edits of a refinement frame, the frame's last wait
    void finish_frame(const FramePlan &P, RenderOptions &o, FrameStats &st, uint64_t seed, bool track_visit) {
        if (P.refines) refine_after_frame(o, st, seed, track_visit);
        finish_count(st);
        ++frame;
        st.capacity = tree->capacity;
    }

    // cuda_renderer.cpp:205-272
    void expand_voxels(RenderOptions &o, FrameStats &st, uint64_t seed);
    // cuda_renderer.cpp:274-333
    void get_more_samples(RenderOptions &o, FrameStats &st, uint64_t seed);
    // cuda_renderer.cpp:335-381
    void prune_tree(FrameStats &st);
    // query_submodules for the samples of a refinement step.  On several ranks (set_ranks) every rank evaluates its share of the rows
    // -- the samples are a pure function of (seed, frame), so every rank holds them all -- and the results are all-gathered: what
    // stays replicated of the step is the vote and the tree edit, not the networks ("broadcast new rows").
    float *query_rows(const int16_t *d_clusters, const float *d_rand, int dim, int64_t rows, int stride);
    void refine_after_frame(RenderOptions &o, FrameStats &st, uint64_t seed, bool track_visit);
};

float *VolumeRenderer::Impl::query_rows(const int16_t *d_clusters, const float *d_rand, int dim, int64_t rows, int stride) {
    const int world = comm ? part.world : 1, rank = comm ? part.rank : 0;
    if (world <= 1) {
        float *d_results = sized<float>(results, (size_t)rows * stride);
        mnv_check(mnv_query_submodules(mlp, d_clusters, d_rand, dim, rows, d_results, stride, stream), "mnv_query_submodules");
        return d_results;
    }
    const int64_t per = (rows + world - 1) / world;  // equal blocks (the last one ragged): the all-gather's table is [world][per rows]
    float *d_results = sized<float>(results, (size_t)per * world * stride);
    const int64_t lo = std::min<int64_t>(rows, per * rank), hi = std::min<int64_t>(rows, per * (rank + 1));
    if (hi > lo)
        mnv_check(mnv_query_submodules(mlp, d_clusters + lo, d_rand + lo * dim, dim, hi - lo, d_results + lo * stride, stride, stream), "mnv_query_submodules");
    mnv_check(mnv_allgather(comm, d_results, (size_t)per * stride * sizeof(float), stream), "mnv_allgather");
    return d_results;
}

void VolumeRenderer::Impl::expand_voxels(RenderOptions &o, FrameStats &st, uint64_t seed) {
    const int64_t n_px = tracker_rows();
    int32_t n = 0, n_cand = 0;
    int32_t *d_nodes = sized<int32_t>(nodes, (size_t)std::max(o.split_batch_size, 1) * 2);
    mnv_check(mnv_select_split_candidates(sized<float>(split_tracker, n_px * 3), n_px, o.split_batch_size, d_nodes, &n, &n_cand, stream),
              "mnv_select_split_candidates");
    st.split_candidates = n_cand;
    if (n_cand == 0) {
        get_more_samples(o, st, seed);
        return;
    }
    if (n == 0) return;
    if (tree->capacity + n > max_tree_capacity) {
        st.full = true;  // "Full"
        return;
    }
    const int dim = sample_cols(o), spc = o.samples_per_corner, dd = tree->data_dim;
    const int64_t children = (int64_t)n * 8, rows = children * spc;
    float *d_rand = sized<float>(rand_sample, (size_t)rows * dim);
    int16_t *d_clusters = sized<int16_t>(rand_clusters, (size_t)rows);
    mnv_check(mnv_fill_uniform(d_rand, rows * dim, seed, stream), "mnv_fill_uniform");
    const mnv_tree_edit e = edit();
    mnv_check(mnv_add_children_and_generate_samples(&e, o.c_abi(), d_nodes, n, d_rand, dim, d_clusters, sized<int32_t>(visit_tracker, max_tree_capacity),
                                                    &grid, stream),
              "mnv_add_children_and_generate_samples");
    float *d_results = query_rows(d_clusters, d_rand, dim, rows, dd + 1);
    mnv_check(mnv_apply_split_results(tree->device.data.get(), tree->device.sample_counts.get(), tree->capacity, n, d_results, dd + 1, spc, dd, stream),
              "mnv_apply_split_results");
    const int old_capacity = tree->capacity;
    tree->capacity += n;
    ++tree_version;
    st.added = n;
    can_reuse_results = false;
    tree->refresh_accel(old_capacity, nullptr, 0, stream);  // the packed layout follows the split
}

void VolumeRenderer::Impl::get_more_samples(RenderOptions &o, FrameStats &st, uint64_t seed) {
    const int64_t n_px = tracker_rows();
    int32_t n = 0, n_cand = 0;
    int32_t *d_nodes = sized<int32_t>(nodes, (size_t)std::max(o.split_batch_size, 1) * 2);
    mnv_check(mnv_select_sample_candidates(sized<float>(sample_tracker, n_px * 3), n_px, o.split_batch_size, d_nodes, &n, &n_cand, stream),
              "mnv_select_sample_candidates");
    st.sample_candidates = n_cand;
    if (n == 0) return;
    // The reference draws 3 columns here whatever the model needs (cuda_renderer.cpp:298-301) while its kernel
    // writes the view-direction / embedding columns as well; the row is sized like expand_voxels' instead.
    const int dim = sample_cols(o), spc = o.samples_per_corner, dd = tree->data_dim;
    const int64_t rows = (int64_t)n * spc;
    float *d_rand = sized<float>(rand_sample, (size_t)rows * dim);
    int16_t *d_clusters = sized<int16_t>(rand_clusters, (size_t)rows);
    mnv_check(mnv_fill_uniform(d_rand, rows * dim, seed ^ 0x5a5a5a5a5a5a5a5aull, stream), "mnv_fill_uniform");
    const mnv_tree_edit e = edit();
    mnv_check(mnv_generate_samples(&e, o.c_abi(), d_nodes, n, d_rand, dim, d_clusters, &grid, stream), "mnv_generate_samples");
    float *d_results = query_rows(d_clusters, d_rand, dim, rows, dd + 1);
    mnv_check(mnv_apply_sample_results(tree->device.data.get(), tree->device.sample_counts.get(), d_nodes, n, d_results, dd + 1, spc, dd, stream),
              "mnv_apply_sample_results");
    st.resampled = n;
    can_reuse_results = false;
    tree->refresh_accel(tree->capacity, d_nodes, n, stream);  // new sigma / colour rows of the resampled leaves
}

void VolumeRenderer::Impl::prune_tree(FrameStats &st) {
    const mnv_tree_edit e = edit();
    int32_t new_cap = tree->capacity, n_del = 0;
    // sample_counts is compacted with the other arrays; the reference forgets it (cuda_renderer.cpp:357-369)
    // A prune renumbers the chunks; the packed accel follows in place (mnv_prune_tree_accel: renumbered node words and lookup grids,
    // compacted colour rows), so that the next frame -- a visit-mark frame, cuda_renderer.cpp:101-102 -- runs on the tuned kernel as well.
    mnv_check(mnv_prune_tree_accel(&e, tree->device.data.get(), tree->data_dim, tree->device.sample_counts.get(), sized<int32_t>(visit_tracker, max_tree_capacity),
                                   (int32_t)max_tree_capacity, tree->device.accel, &new_cap, &n_del, stream),
              "mnv_prune_tree_accel");
    st.pruned = n_del > 0 ? n_del : -1;
    if (n_del > 0) {
        tree->capacity = new_cap;
        ++tree_version;
        can_reuse_results = false;
    }
}

// cuda_renderer.cpp:144-155: what follows the march of a refinement frame
void VolumeRenderer::Impl::refine_after_frame(RenderOptions &options, FrameStats &stats, uint64_t seed, bool track_visit) {
    Impl &I = *this;
    N3Tree &tree = *I.tree;
    // The capacity check runs only while splitting is on: the reference's unconditional
    // check would prune a tree that was merely loaded with max_tree_capacity close to its size.
    if (options.use_splitting) {
        I.expand_voxels(options, stats, seed + 0x9e3779b97f4a7c15ull * I.frame);
        if (track_visit) I.marks_fresh = true;
        I.want_marks = false;
        if (I.max_tree_capacity - tree.capacity < options.split_batch_size) {
            // The reference prunes here with whatever marks exist (cuda_renderer.cpp:148-150); with a camera that
            // has not moved since the tree was small that is no marks at all and the whole tree goes.  Here a
            // prune waits for one track_visit frame since the marks were last cleared.
            if (I.marks_fresh) {
                I.prune_tree(stats);
                I.prune_happened = true;
                I.marks_fresh = false;
            } else {
                I.want_marks = true;
                I.prune_happened = false;
            }
        } else {
            I.prune_happened = false;
        }
    }
}

VolumeRenderer::VolumeRenderer() : impl_(std::make_unique<Impl>()) {}
VolumeRenderer::~VolumeRenderer() {}

void VolumeRenderer::set(N3Tree &tree, long max_tree_capacity) {
    impl_->sync_all();
    impl_->drop_lod_trees();
    tree.move_to_device(max_tree_capacity, true, true, impl_->stream);
    impl_->tree = &tree;
    impl_->max_tree_capacity = max_tree_capacity;
    ++impl_->tree_version;
    // visit_tracker = zeros, [0] = 1 (cuda_renderer.cpp:504-506)
    int32_t *visited = sized<int32_t>(impl_->visit_tracker, (size_t)max_tree_capacity);
    hip_check(hipMemsetAsync(visited, 0, (size_t)max_tree_capacity * 4, impl_->stream), "clear visit marks");
    const int32_t one = 1;
    hip_check(hipMemcpyAsync(visited, &one, 4, hipMemcpyHostToDevice, impl_->stream), "mark root");
    hip_check(hipStreamSynchronize(impl_->stream), "set");
    impl_->prune_happened = impl_->can_reuse_results = impl_->marks_fresh = impl_->want_marks = false;
    options.basis_minmax[0] = 0;
    options.basis_minmax[1] = std::max(tree.data_format.basis_dim - 1, 0);
}

void VolumeRenderer::set_model(const mnv_mlp_desc &desc, const uint16_t *params, size_t n_halfs, const mnv_cluster_grid &grid) {
    mnv_mlp *m = nullptr;
    mnv_check(mnv_mlp_create(&desc, params, n_halfs, impl_->stream, &m), "mnv_mlp_create");
    if (impl_->mlp) mnv_mlp_destroy(impl_->mlp);
    impl_->mlp = m;
    impl_->mlp_desc = desc;
    {
        const int in_dim = 3 + 6 * desc.pos_octaves + (desc.need_viewdir ? 3 + 6 * desc.dir_octaves : 0) + (desc.n_embeddings > 0 ? desc.embedding_dim : 0);
        impl_->fused_inputs_ok = in_dim <= 64;
    }
    impl_->grid = grid;
    // cuda_renderer.cpp:534-537
    options.need_viewdir = desc.need_viewdir != 0;
    if (options.appearance_embedding == -1 && desc.n_embeddings > 0) options.appearance_embedding = 0;
    if (desc.n_embeddings <= 0) options.appearance_embedding = -1;
    impl_->can_reuse_results = false;
}

bool VolumeRenderer::has_model() const { return impl_->mlp != nullptr; }

void VolumeRenderer::load_model(const std::string &npz_path) {
    npz::Archive a = npz::load(npz_path);
    auto need = [&](const char *name) -> npz::Array & {
        auto it = a.find(name);
        if (it == a.end()) throw std::runtime_error(std::string("model container lacks '") + name + "'");
        return it->second;
    };
    auto ints = [&](const char *name, size_t count, int32_t *out) {
        npz::Array &arr = need(name);
        if (arr.num_vals() != count || (arr.kind != 'i' && arr.kind != 'u')) throw std::runtime_error(std::string(name) + " has an unexpected shape");
        for (size_t i = 0; i < count; ++i) out[i] = arr.word_size == 8 ? (int32_t)arr.data<int64_t>()[i] : arr.data<int32_t>()[i];
    };
    auto floats = [&](const char *name, size_t count, float *out) {
        npz::Array &arr = need(name);
        if (arr.num_vals() != count || arr.kind != 'f') throw std::runtime_error(std::string(name) + " has an unexpected shape");
        for (size_t i = 0; i < count; ++i) out[i] = arr.word_size == 8 ? (float)arr.data<double>()[i] : arr.data<float>()[i];
    };
    int32_t d[9];
    ints("mlp_desc", 9, d);
    mnv_mlp_desc desc{};
    desc.n_clusters = d[0];
    desc.pos_octaves = d[1];
    desc.dir_octaves = d[2];
    desc.need_viewdir = d[3];
    desc.n_embeddings = d[4];
    desc.embedding_dim = d[5];
    desc.hidden_width = d[6];
    desc.hidden_layers = d[7];
    desc.out_dim = d[8];
    floats("mlp_center", 3, desc.center);
    floats("mlp_inv_extent", 3, desc.inv_extent);
    mnv_cluster_grid grid{};
    ints("grid_dim", 2, grid.grid_dim);
    float max_position[3];
    floats("min_position", 3, grid.min_position);
    floats("max_position", 3, max_position);
    for (int i = 0; i < 3; ++i) grid.range[i] = max_position[i] - grid.min_position[i];  // cuda_renderer.cpp:527
    npz::Array &p = need("mlp_params");
    if (p.word_size != 2) throw std::runtime_error("mlp_params must be binary16");
    set_model(desc, p.data<uint16_t>(), p.num_vals(), grid);
}

void VolumeRenderer::set_lod(int max_depth) {
    if (max_depth < 0) throw StatusError(MNV_E_INVALID, "set_lod: the depth must be 0 (off) or at least 1");
    impl_->lod = max_depth;
}
int VolumeRenderer::lod() const { return impl_->lod; }

void VolumeRenderer::set_view_lod(const std::vector<mnv_lod_view> &views, float pixels, int min_depth, int max_depth) {
    Impl &I = *impl_;
    if (views.size() > 4096) throw StatusError(MNV_E_INVALID, "set_view_lod: at most 4096 viewpoints");
    if (!views.empty()) {
        if (!std::isfinite(pixels) || pixels < 0.f) throw StatusError(MNV_E_INVALID, "set_view_lod: pixels must be finite and not negative");
        if (min_depth < 1 || max_depth < min_depth) throw StatusError(MNV_E_INVALID, "set_view_lod: need 1 <= min_depth <= max_depth");
        for (const mnv_lod_view &v : views)
            if (!std::isfinite(v.eye[0]) || !std::isfinite(v.eye[1]) || !std::isfinite(v.eye[2]) || !std::isfinite(v.focal_px) || !(v.focal_px > 0.f))
                throw StatusError(MNV_E_INVALID, "set_view_lod: an eye must be finite, focal_px finite and positive");
    }
    if (I.view_lod_tree) {  // (frames in flight may march it)
        I.sync_all();
        I.view_lod_tree.reset();
        I.lod_tree = nullptr;
    }
    I.view_lod_views = views;
    I.view_lod_pixels = pixels;
    I.view_lod_min = min_depth;
    I.view_lod_max = max_depth;
    ++I.view_lod_gen;
}
bool VolumeRenderer::view_lod() const { return !impl_->view_lod_views.empty(); }

void VolumeRenderer::set_cull(const std::vector<mnv_camera> &cams, float weight_thresh) {
    Impl &I = *impl_;
    if (!cams.empty()) {
        if (!std::isfinite(weight_thresh) || weight_thresh < 0.f) throw StatusError(MNV_E_INVALID, "set_cull: weight_thresh must be finite and not negative");
        for (const mnv_camera &c : cams)
            if (c.width < 1 || c.height < 1 || (int64_t)c.width * c.height > ((int64_t)1 << 22))
                throw StatusError(MNV_E_INVALID, "set_cull: a camera needs 1 .. 2^22 pixels");
    }
    if (I.cull_tree) {  // (frames in flight may march it)
        I.sync_all();
        I.cull_tree.reset();
        I.lod_tree = nullptr;
    }
    I.cull_cams = cams;
    I.cull_thresh = weight_thresh;
    ++I.cull_gen;
}
bool VolumeRenderer::cull() const { return !impl_->cull_cams.empty(); }

void VolumeRenderer::set_lod_fit(const std::vector<mnv_camera> &cams, const mnv_fit_params &params) {
    mnv_fit_params_ex ex = {};  // SGD, full batch: N3Tree::fit_to_ex with these is N3Tree::fit_to
    ex.steps = params.iterations;
    ex.optimizer = MNV_FIT_SGD;
    ex.lr_colour = params.lr_colour;
    ex.lr_sigma = params.lr_sigma;
    ex.tile = 8;
    set_lod_fit(cams, ex);
}

void VolumeRenderer::set_lod_fit(const std::vector<mnv_camera> &cams, const mnv_fit_params_ex &params) {
    if (params.steps < 0) throw StatusError(MNV_E_INVALID, "set_lod_fit: negative iteration count");
    if (!std::isfinite(params.lr_colour) || !std::isfinite(params.lr_sigma) || params.lr_colour < 0.f || params.lr_sigma < 0.f)
        throw StatusError(MNV_E_INVALID, "set_lod_fit: the learning rates must be finite and not negative");
    Impl &I = *impl_;
    I.drop_lod_trees();  // (trees fitted otherwise, or not at all, go: the next frame builds its tree again)
    I.lod_fit_cams = cams;
    I.lod_fit = params;
}

void VolumeRenderer::clear() {
    impl_->drop_lod_trees();
    impl_->tree = nullptr;
    ++impl_->tree_version;
}

const mnv_wireframe *VolumeRenderer::wireframe() const { return impl_->wire; }
const mnv_camera &VolumeRenderer::last_camera() const { return impl_->last_camera; }

const mnv_mlp *VolumeRenderer::model() const { return impl_->mlp; }
const mnv_cluster_grid &VolumeRenderer::cluster_grid() const { return impl_->grid; }

void VolumeRenderer::set_frame_inputs(const float *tmax_px_device, const uint8_t *rgba8_init_device) {
    Impl &I = *impl_;
    if (I.comm && (tmax_px_device || rgba8_init_device)) throw std::runtime_error("frame inputs (offscreen == false) are for one rank");
    I.sync_all();
    I.inputs.tmax_px = tmax_px_device;
    I.inputs.rgba8_init = rgba8_init_device;
    I.can_reuse_results = false;  // the samples of the last guided frame were limited by the previous depth image
}

void VolumeRenderer::set_ranks(mnv_comm *comm, int tile_w, int tile_h) {
    Impl &I = *impl_;
    if (comm && I.target) throw StatusError(MNV_E_INVALID, "set_target scores the frame of one rank: it cannot be combined with set_ranks");
    if (comm && (I.inputs.tmax_px || I.inputs.rgba8_init)) throw std::runtime_error("frame inputs (offscreen == false) are for one rank");
    I.sync_all();
    I.comm = comm;
    if (!comm) {
        I.part = {0, 1, 0, 0, 0};
        return;
    }
    I.part = {mnv_comm_rank(comm), mnv_comm_world(comm), tile_w, tile_h, 0};
}

void VolumeRenderer::resize(int width, int height) {
    if (impl_->width == width && impl_->height == height && impl_->rgba) return;
    if (!impl_->initial_resize && camera.width > 0 && camera.height > 0) {
        const float wr = (float)width / camera.width, hr = (float)height / camera.height;
        camera.fx *= wr;
        camera.default_fx *= wr;
        camera.fy *= hr;
        camera.default_fy *= hr;
        if (camera.default_cx != -1) camera.cx *= wr;
        if (camera.default_cy != -1) camera.cy *= hr;
    }
    if (!impl_->initial_resize) impl_->clear_target();  // an image of the old size (the first call only sets the size, also when render() makes it)
    impl_->initial_resize = false;
    camera.width = width;
    camera.height = height;
    if (camera.default_cx == -1) camera.cx = (float)(width / 2);   // "-1 = use width / 2" (main.cpp:496)
    if (camera.default_cy == -1) camera.cy = (float)(height / 2);
    impl_->free_frame();
    impl_->width = width;
    impl_->height = height;
    impl_->ensure_slots(1);
    impl_->use_slot(0);
}

void VolumeRenderer::set_target(const uint8_t *rgba8_device, int flags) {
    Impl &I = *impl_;
    if (!rgba8_device) {
        I.clear_target();
        return;
    }
    if ((flags & ~(MNV_METRIC_QUANTISED | MNV_METRIC_MASK_ALPHA | MNV_METRIC_SSIM)) != 0) throw StatusError(MNV_E_INVALID, "set_target: unknown flag bits");
    if (I.comm) throw StatusError(MNV_E_INVALID, "set_target scores the frame of one rank: it cannot be combined with set_ranks");
    I.target = rgba8_device;
    I.target_flags = flags;
}

void VolumeRenderer::slot_metrics(int slot, mnv_frame_metric_values *out) {
    Impl &I = *impl_;
    if (slot < 0 || slot >= (int)I.slots.size() || !I.slots[slot].scored)
        throw StatusError(MNV_E_INVALID, "slot_metrics: the last frame of this slot was not scored (set_target)");
    hip_check(hipStreamSynchronize(I.slots[slot].stream), "slot_metrics");
    mnv_check(mnv_metrics_finish(I.slots[slot].sums.host.get(), out), "mnv_metrics_finish");
}

// the frame, then its score: on the frame's slot and stream, whatever kind of frame it was
void VolumeRenderer::render() {
    Impl &I = *impl_;
    const uint8_t *target = I.target;
    render_frame();
    Impl::Slot &S = I.slots[I.cur];
    S.scored = false;
    if (!target) return;
    if (!S.sums) alloc_pair(S.sums, "hipMalloc(metric sums)", "hipHostMalloc(metric sums)");
    const int rc = mnv_frame_metrics(S.rgba.get(), target, I.width, I.height, I.target_flags, nullptr, S.sums.dev.get(), nullptr, nullptr, S.stream);
    if (rc != MNV_OK) throw StatusError(rc, std::string("mnv_frame_metrics: ") + mnv_last_error());
    hip_check(hipMemcpyAsync(S.sums.host.get(), S.sums.dev.get(), sizeof(mnv_metric_sums), hipMemcpyDeviceToHost, S.stream), "read metric sums");
    S.scored = true;
}

VolumeRenderer::FramePlan VolumeRenderer::plan() const {
    const Impl &I = *impl_;
    FramePlan P;
    const N3Tree *tree = I.tree != nullptr && I.tree->N > 0 ? I.tree : nullptr;
    const bool packed = tree && tree->device.accel;  // a tree with the packed accel: N == 2, RGBA or SH1/4/9/16/25 rows
    const bool model_on = I.mlp != nullptr && (options.use_splitting || options.use_guided_sampling);
    const bool guided = I.mlp != nullptr && options.use_guided_sampling;
    // the network is one the fused guided kernel covers
    const bool covered = tree && I.mlp_desc.hidden_width == 64 && I.fused_inputs_ok &&
                         (tree->data_format.format != DataFormat::SH || tree->data_format.basis_dim == 1 || tree->data_format.basis_dim == 4 ||
                          tree->data_format.basis_dim == 9 || tree->data_format.basis_dim == 16);
    const bool out_dim_differs = tree && model_on && I.mlp_desc.out_dim != tree->data_dim + 1;
    const bool inputs_set = I.inputs.tmax_px || I.inputs.rgba8_init;
    const bool lod = tree && I.lod > 0, view_lod = tree && !I.view_lod_views.empty(), cull = tree && !I.cull_cams.empty();
    bool mesh_visible = false;
    for (const mnv_mesh *m : meshes) mesh_visible = mesh_visible || (m && mnv_mesh_visible(m));
    const bool projected = projection != MNV_PROJ_PINHOLE, aa = !projected && aa_samples != 1, ranks = !projected && !aa && I.comm;
    P.kind = projected ? FramePlan::PROJECTED : aa ? FramePlan::AA : ranks ? FramePlan::RANKS : tree ? FramePlan::TREE : FramePlan::BACKGROUND;
    // show_grid / meshes: the grid pass and the mesh pass produce this frame's inputs (cuda_renderer.cpp:68-90 draws them before the march)
    P.show_grid = !projected && options.show_grid && tree;
    P.draws_inputs = !projected && (P.show_grid || mesh_visible);
    const bool grid_draws = P.draws_inputs && P.show_grid, meshes_draw = P.draws_inputs && !P.show_grid;

    // Every combination render() cannot serve; the first row that holds is reported.
    const struct {
        bool holds, is_status;
        const char *text;
    } refusals[] = {
        {I.target && I.comm, true, "set_target scores the frame of one rank: it cannot be combined with set_ranks"},
        {lod && (options.use_splitting || options.use_guided_sampling), true,
         "set_lod: frames of a truncated tree cannot edit or vote on the tree (use_splitting / use_guided_sampling)"},
        {lod && I.comm, true, "set_lod is for one rank: it cannot be combined with set_ranks"},
        {view_lod && (options.use_splitting || options.use_guided_sampling), true,
         "set_view_lod: frames of a cut tree cannot edit or vote on the tree (use_splitting / use_guided_sampling)"},
        {view_lod && I.comm, true, "set_view_lod is for one rank: it cannot be combined with set_ranks"},
        {view_lod && lod, true, "set_view_lod and set_lod choose the tree a frame marches: only one of them can be on"},
        {cull && (options.use_splitting || options.use_guided_sampling), true,
         "set_cull: frames of a culled tree cannot edit or vote on the tree (use_splitting / use_guided_sampling)"},
        {cull && I.comm, true, "set_cull is for one rank: it cannot be combined with set_ranks"},
        {cull && (lod || view_lod), true, "set_cull and set_lod / set_view_lod choose the tree a frame marches: only one of them can be on"},
        {projected && projection != MNV_PROJ_ORTHO && projection != MNV_PROJ_EQUIRECT, true, "projection: unknown projection"},
        {projected && inputs_set, true, "projection: set_frame_inputs holds images of a pinhole camera; it cannot be combined with another projection"},
        {projected && I.comm, true, "projection: orthographic / equirectangular frames are for one rank (set_ranks)"},
        {projected && options.show_grid, true, "projection: the grid pass draws through a pinhole camera (show_grid)"},
        {projected && mesh_visible, true, "projection: the mesh pass draws through a pinhole camera (a visible mesh)"},
        {projected && aa_samples != 1, true, "projection: anti-aliasing jitters a pinhole camera (aa_samples > 1)"},
        {projected && model_on, true, "projection: use_splitting / use_guided_sampling march a pinhole camera's rays"},
        {projected && !packed, true, "projection: ray lists need a tree with the packed accel (N == 2, RGBA or SH1/4/9/16/25 rows)"},
        {aa && (aa_samples < 1 || aa_samples > MNV_MAX_BATCH), true, "anti-aliasing: aa_samples must be 1 .. MNV_MAX_BATCH"},
        {aa && aa_filter != MNV_AA_BOX && aa_filter != MNV_AA_TENT, true, "anti-aliasing: unknown aa_filter"},
        {aa && inputs_set, true, "anti-aliasing jitters the camera: it cannot be combined with set_frame_inputs (images of one fixed camera)"},
        {aa && I.comm, true, "anti-aliasing is for one rank: it cannot be combined with set_ranks"},
        {aa && model_on, true, "anti-aliasing cannot be combined with use_splitting / use_guided_sampling (refinement votes per ray of one camera)"},
        {aa && !packed, true, "anti-aliasing needs a tree with the packed accel (N == 2, RGBA or SH1/4/9/16/25 rows)"},
        {grid_draws && inputs_set, true, "show_grid draws the frame inputs itself: it cannot be combined with set_frame_inputs"},
        {meshes_draw && inputs_set, true, "a mesh list draws the frame inputs itself: it cannot be combined with set_frame_inputs"},
        {grid_draws && I.comm, true, "show_grid is for one rank: it cannot be combined with set_ranks"},
        {meshes_draw && I.comm, true, "a mesh list is for one rank: it cannot be combined with set_ranks"},
        {ranks && !packed, false, "several ranks need a tree with the packed accel (N == 2, RGBA or SH1/4/9/16/25 rows)"},
        {!projected && !aa && out_dim_differs, false, "the model's out_dim must be the tree's data_dim + 1 (cuda_renderer.cpp:255-257)"},
        {ranks && options.render_depth && model_on, false, "several ranks: no depth mode while refining"},
        {ranks && guided && !covered, false, "several ranks: guided sampling needs a network the fused kernel covers (64 wide, at most 64 encoded inputs)"},
    };
    for (const auto &r : refusals)
        if (r.holds) {
            P.refusal = r.text;
            P.refusal_is_status = r.is_status;
            return P;
        }

    // A frame that leaves the tree alone takes the next slot beside the frames in flight; everything else runs alone on slot 0.  With
    // a model switched on that is a guided-sampling frame that wants nothing but the picture: the fused kernel, no splitting, no visit
    // marks (a tree below 3/4 of its capacity and no prune pending: track_visit is then false whatever the camera did).
    const bool leaves_tree_alone = !model_on || (guided_in_flight && use_fused_guided && guided && !options.use_splitting && !options.render_depth && covered &&
                                                 !I.prune_happened && !I.want_marks && tree->capacity <= I.max_tree_capacity * 3 / 4);
    P.overlaps = !I.comm && frames_in_flight > 1 && packed && leaves_tree_alone;
    if (P.kind == FramePlan::TREE && P.overlaps) P.kind = guided ? FramePlan::GUIDED_IN_FLIGHT : FramePlan::PLAIN;
    P.refines = model_on && (P.kind == FramePlan::TREE || P.kind == FramePlan::RANKS);
    P.guided = guided;
    P.fused = guided && use_fused_guided && !options.render_depth && covered;
    P.packed = packed;
    P.has_parent = tree && tree->device.parent.get();
    return P;
}

bool VolumeRenderer::overlaps_next() const { return plan().overlaps; }
int VolumeRenderer::next_slot() const { return plan().overlaps ? (impl_->cur + 1) % frames_in_flight : 0; }

// What the slots share is brought up to date before the frame takes its slot: each step that replaces something frames in flight read
// or write waits for them first (sync_all clears `overlapped`, so none of this may follow take_slot).
void VolumeRenderer::update_shared(const FramePlan &P) {
    Impl &I = *impl_;
    // set_lod: the tree this frame marches.  Trees made from another structure of the renderer's tree go (the refusals keep a frame with a
    // level of detail from editing it, a frame without one may have); a missing one is built on slot 0's stream, which holds those edits.
    I.lod_tree = nullptr;
    if (I.lod > 0 && P.kind != FramePlan::BACKGROUND) {
        if (I.lod_version != I.tree_version) I.drop_lod_trees();
        I.lod_version = I.tree_version;
        for (auto &e : I.lod_trees)
            if (e.depth == I.lod) I.lod_tree = e.tree.get();
        if (!I.lod_tree) {
            I.sync_all();
            I.lod_trees.push_back({I.lod, I.tree->make_lod(I.lod, I.stream)});
            I.lod_tree = I.lod_trees.back().tree.get();
            I.fit_lod(*I.lod_tree, options);
        }
    }
    if (!I.view_lod_views.empty() && P.kind != FramePlan::BACKGROUND) {  // set_view_lod: the same with the one tree of the current views
        if (I.lod_version != I.tree_version) I.drop_lod_trees();
        I.lod_version = I.tree_version;
        if (!I.view_lod_tree) {
            I.sync_all();
            I.view_lod_tree = I.tree->make_view_lod(I.view_lod_views, I.view_lod_pixels, I.view_lod_min, I.view_lod_max, I.stream);
            I.fit_lod(*I.view_lod_tree, options);
        }
        I.lod_tree = I.view_lod_tree.get();
    }
    if (!I.cull_cams.empty() && P.kind != FramePlan::BACKGROUND) {  // set_cull: the same with the one tree of the current cameras
        if (I.lod_version != I.tree_version) I.drop_lod_trees();
        I.lod_version = I.tree_version;
        mnv_render_options march = *options.c_abi();
        march.render_depth = false;
        if (I.cull_tree && !Impl::same_march(march, I.cull_opt)) {  // built under other march options: frames in flight may march it
            I.sync_all();
            I.cull_tree.reset();
            ++I.cull_gen;
        }
        if (!I.cull_tree) {
            I.sync_all();
            I.cull_tree = I.tree->make_culled(I.cull_cams, march, I.cull_thresh, I.stream);
            I.cull_opt = march;
        }
        I.lod_tree = I.cull_tree.get();
    }
    if (P.kind == FramePlan::PROJECTED) {  // (draws no inputs; anti-aliasing buffers of earlier frames stay until the next pinhole frame)
        if (projection == MNV_PROJ_EQUIRECT && (!I.equirect_dev || I.equirect_w != I.width || I.equirect_h != I.height)) {
            I.sync_all();  // frames in flight read the old table
            I.equirect_dev.reset();
            std::vector<float> table(((size_t)I.width + I.height) * 2);
            mnv_check(mnv_equirect_tables(I.width, I.height, table.data()), "mnv_equirect_tables");
            hip_check(I.equirect_dev.alloc(table.size()), "hipMalloc(equirectangular table)");
            hip_check(hipMemcpy(I.equirect_dev.get(), table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice), "upload equirectangular table");
            I.equirect_w = I.width;
            I.equirect_h = I.height;
        }
        return;
    }
    if (P.kind != FramePlan::AA && I.aa_k != 1) {  // the buffers of earlier anti-aliased frames go; from here on render() is what it is without the feature
        I.sync_all();
        I.free_aa();
    }
    I.pass_grid = P.show_grid;
    I.pass_meshes.clear();
    for (const mnv_mesh *m : meshes)
        if (m && mnv_mesh_visible(m)) I.pass_meshes.push_back(m);
    if (!I.pass_meshes.empty()) I.can_reuse_results = false;  // (a mesh may have moved: the samples of the last guided frame were limited by it)
    if (P.show_grid && (!I.wire || I.wire_depth != options.grid_max_depth || I.wire_version != I.tree_version || I.wire_lod != I.lod ||
                        I.wire_view_gen != I.view_lod_token() || I.wire_cull_gen != I.cull_token())) {
        I.sync_all();  // frames in flight read the old edge list; slot 0's stream holds the tree edits the new one must see
        const mnv_tree_view dv = I.march_tree().device_view();
        const int rc = I.wire ? mnv_wireframe_update(I.wire, &dv, options.grid_max_depth, I.stream)
                              : mnv_wireframe_create(&dv, options.grid_max_depth, I.stream, &I.wire);
        if (rc != MNV_OK) throw StatusError(rc, std::string("show_grid: ") + mnv_last_error());  // keeps the code (N != 2: unsupported)
        I.wire_depth = options.grid_max_depth;
        I.wire_version = I.tree_version;
        I.wire_lod = I.lod;
        I.wire_view_gen = I.view_lod_token();
        I.wire_cull_gen = I.cull_token();
        I.can_reuse_results = false;  // the samples of the last guided frame were limited by the previous grid
    }
    if (P.kind == FramePlan::AA && (aa_samples != I.aa_k || aa_filter != I.aa_filter)) {
        const int K = aa_samples;
        I.sync_all();  // frames in flight read the old table and write the old sub-frame buffers
        if (K != I.aa_k || !I.aa_weights_dev) {
            I.free_aa();
            hip_check(I.aa_weights_dev.alloc((size_t)K * 25), "hipMalloc(filter weights)");
        }
        I.aa_offsets.resize((size_t)K * 2);
        aa_pattern(K, I.aa_offsets.data());
        I.aa_radius = aa_filter_radius(aa_filter);
        std::vector<float> w((size_t)K * (2 * I.aa_radius + 1) * (2 * I.aa_radius + 1));
        aa_weights(aa_filter, K, I.aa_offsets.data(), w.data());
        hip_check(hipMemcpy(I.aa_weights_dev.get(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice), "upload filter weights");
        I.aa_k = K;
        I.aa_filter = aa_filter;
    }
}

void VolumeRenderer::render_frame() {
    Impl &I = *impl_;
    if (!I.slots[0].rgba) resize(camera.width, camera.height);
    camera._update();
    const mnv_camera cv = camera.c_abi();
    I.last_camera = cv;
    stats = FrameStats();
    const FramePlan P = plan();
    if (P.refusal) {  // before a slot, a stream or a buffer is touched: the same call renders once the obstacle is gone
        if (P.refusal_is_status) throw StatusError(MNV_E_INVALID, P.refusal);
        throw std::runtime_error(P.refusal);
    }
    update_shared(P);
    I.take_slot(P, frames_in_flight);
    bool track_visit = false;
    switch (P.kind) {
        case FramePlan::BACKGROUND: issue_background(P, cv); return;  // (no tree: nothing to refine or count)
        case FramePlan::PLAIN: issue_plain(P, cv); break;
        case FramePlan::GUIDED_IN_FLIGHT: issue_guided_in_flight(P, cv); break;
        case FramePlan::TREE: track_visit = issue_tree(P, cv); break;
        case FramePlan::RANKS: track_visit = issue_ranks(P, cv); break;
        case FramePlan::AA: issue_aa(P, cv); break;
        case FramePlan::PROJECTED: issue_projected(cv); break;
    }
    I.finish_frame(P, options, stats, seed, track_visit);
}

void VolumeRenderer::issue_background(const FramePlan &P, const mnv_camera &cv) {
    Impl &I = *impl_;
    mnv_tree_view empty = {};  // N == 0: background only (renderer_kernel.cu:266)
    const mnv_frame_inputs in = I.frame_inputs(P, cv, options);
    mnv_check(mnv_render_voxels_ex(&empty, &cv, options.c_abi(), {0, 0, I.width, I.height}, &in, I.rgba, I.rgba8, nullptr, nullptr, nullptr, 0, I.stream),
              "mnv_render_voxels_ex");
}

void VolumeRenderer::issue_plain(const FramePlan &P, const mnv_camera &cv) {
    Impl &I = *impl_;
    const mnv_frame_inputs in = I.frame_inputs(P, cv, options);
    mnv_check(mnv_render_voxels_accel_ex(I.march_tree().device.accel, &cv, options.c_abi(), {0, 0, I.width, I.height}, &in, I.rgba, I.rgba8, I.slots[I.cur].stream),
              "mnv_render_voxels_accel_ex");
    stats.used_accel = true;
}

void VolumeRenderer::issue_guided_in_flight(const FramePlan &P, const mnv_camera &cv) {
    Impl &I = *impl_;
    Impl::Slot &S = I.slots[I.cur];
    const mnv_frame_inputs in = I.frame_inputs(P, cv, options);
    if (!S.count) alloc_pair(S.count, "hipMalloc(sample counter)", "hipHostMalloc(sample count)");
    hip_check(hipMemsetAsync(S.count.dev.get(), 0, sizeof(unsigned long long), S.stream), "clear sample counter");
    mnv_check(mnv_render_guided_fused_track_ex(I.tree->device.accel, &cv, options.c_abi(), {0, 0, I.width, I.height}, &in, I.mlp, &I.grid, I.rgba, I.rgba8,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, S.count.dev.get(), S.stream),
              "mnv_render_guided_fused_track_ex");
    hip_check(hipMemcpyAsync(S.count.host.get(), S.count.dev.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, S.stream), "read sample counter");
    S.counted = true;
    stats.used_accel = true;
    stats.fused = true;
    stats.guided_samples = -1;  // in flight: slot_guided_samples(last_slot())
}

// a frame alone on slot 0 that may refine the tree; returns whether it took visit marks
bool VolumeRenderer::issue_tree(const FramePlan &P, const mnv_camera &cv) {
    Impl &I = *impl_;
    N3Tree &tree = I.march_tree();
    const mnv_rect full = {0, 0, I.width, I.height};
    const mnv_frame_inputs in = I.frame_inputs(P, cv, options);
    const Impl::Trackers T = I.begin_refinement(P, camera, options, stats, 0);
    const bool track_visit = T.track_visit;
    const mnv_tree_view dv = tree.device_view();
    switch (P.march(track_visit)) {
        case FramePlan::FUSED_GUIDED: {
            // the guided-sampling frame as ONE kernel (march + networks + composite, no sample buffer); with refinement on as well
            // (configs[4]) the same kernel also writes the trackers and the visit marks
            unsigned long long *counter = sized<unsigned long long>(I.fused_counter, 1);
            hip_check(hipMemsetAsync(counter, 0, sizeof(unsigned long long), I.stream), "clear sample counter");
            mnv_check(mnv_render_guided_fused_track_ex(tree.device.accel, &cv, options.c_abi(), full, &in, I.mlp, &I.grid, I.rgba, I.rgba8, T.split, T.sample,
                                                       T.split ? tree.device.sample_counts.get() : nullptr, track_visit ? T.visited : nullptr, tree.device.parent.get(),
                                                       counter, I.stream),
                      "mnv_render_guided_fused_track_ex");
            I.read_count_later(counter);
            stats.used_accel = true;
            stats.fused = true;
            I.can_reuse_results = false;
            break;
        }
        case FramePlan::FOUR_STEP_GUIDED: {
            // cuda_renderer.cpp:109-139
            const int64_t n_px = (int64_t)I.width * I.height;
            const int samples_dim = 1 + I.sample_cols(options), max_g = options.max_guided_samples, dd = tree.data_dim;
            int64_t *offsets = sized<int64_t>(I.offsets, n_px);
            if (!I.can_reuse_results) {
                int16_t *num = sized<int16_t>(I.num_samples, n_px);
                int16_t *clusters = sized<int16_t>(I.cluster_indices, n_px * max_g);
                float *guided = sized<float>(I.guided_samples, (size_t)n_px * max_g * samples_dim);
                hip_check(hipMemsetAsync(num, 0, n_px * 2, I.stream), "clear num_samples");
                if (P.on_accel(track_visit)) {
                    // visit marks on the packed layout: the march marks leaf chunks, a closure pass adds their ancestors
                    stats.used_accel = true;
                    mnv_check(mnv_get_samples_from_voxels_accel_visit_ex(tree.device.accel, &cv, options.c_abi(), full, &in, T.split, T.sample,
                                                                         tree.device.sample_counts.get(), track_visit ? T.visited : nullptr, tree.device.parent.get(), num,
                                                                         guided, samples_dim, clusters, &I.grid, I.stream),
                              "mnv_get_samples_from_voxels_accel_visit_ex");
                } else {
                    mnv_check(mnv_get_samples_from_voxels_ex(&dv, &cv, options.c_abi(), full, &in, T.split, T.sample, T.visited, track_visit, num, guided,
                                                             samples_dim, clusters, &I.grid, I.stream),
                              "mnv_get_samples_from_voxels_ex");
                }
                // one call in the steady state: the packed buffers keep the size of the previous frames and grow when a frame
                // emits more (the call then reports the total it needs)
                int64_t total = 0, cap_rows = (int64_t)(I.z_vals.bytes() / sizeof(float));
                float *z = nullptr, *rows = nullptr, *values = nullptr;
                int16_t *row_clusters = nullptr;
                for (int attempt = 0; attempt < 2; ++attempt) {
                    z = sized<float>(I.z_vals, (size_t)std::max<int64_t>(cap_rows, 1));
                    rows = sized<float>(I.sample_rows, (size_t)std::max<int64_t>(cap_rows, 1) * (samples_dim - 1));
                    row_clusters = sized<int16_t>(I.sample_clusters, (size_t)std::max<int64_t>(cap_rows, 1));
                    const int rc = mnv_compact_guided_samples(num, guided, clusters, n_px, max_g, samples_dim, offsets, z, rows, row_clusters, cap_rows,
                                                              &total, I.stream);
                    if (rc == MNV_OK) break;
                    if (total <= cap_rows || attempt == 1) mnv_check(rc, "mnv_compact_guided_samples");
                    cap_rows = total + total / 8;
                }
                values = sized<float>(I.nerf_results, (size_t)std::max<int64_t>(total, 1) * (dd + 1));
                if (total > 0)
                    mnv_check(mnv_query_submodules(I.mlp, row_clusters, rows, samples_dim - 1, total, values, dd + 1, I.stream), "mnv_query_submodules");
                I.reuse_total = total;
                I.can_reuse_results = true;
            }
            stats.guided_samples = I.reuse_total;
            mnv_check(mnv_render_nerf_results(&dv, &cv, options.c_abi(), full, sized<float>(I.nerf_results, 1), tree.data_dim + 1, sized<float>(I.z_vals, 1), offsets,
                                              I.rgba, I.rgba8, I.stream),
                      "mnv_render_nerf_results");
            break;
        }
        case FramePlan::TRACKED_ACCEL:
            stats.used_accel = true;
            mnv_check(mnv_render_voxels_accel_visit_ex(tree.device.accel, &cv, options.c_abi(), full, &in, I.rgba, I.rgba8, T.split, T.sample,
                                                       tree.device.sample_counts.get(), track_visit ? T.visited : nullptr, tree.device.parent.get(), I.stream),
                      "mnv_render_voxels_accel_visit_ex");
            break;
        case FramePlan::REFERENCE_LAYOUT:
            mnv_check(mnv_render_voxels_ex(&dv, &cv, options.c_abi(), full, &in, I.rgba, I.rgba8, T.split, T.sample, T.visited, track_visit, I.stream),
                      "mnv_render_voxels_ex");
            break;
    }
    return track_visit;
}

// aa_samples > 1: K jittered sub-frames on the frame's slot and stream, then the resolve into the slot's frame
void VolumeRenderer::issue_aa(const FramePlan &P, const mnv_camera &cv) {
    Impl &I = *impl_;
    Impl::Slot &S = I.slots[I.cur];
    const int K = aa_samples;
    const size_t frame_floats = (size_t)I.width * I.height * 4;
    if (!S.aa_sub) hip_check(S.aa_sub.alloc((size_t)K * frame_floats), "hipMalloc(sub-frames)");
    const mnv_rect full = {0, 0, I.width, I.height};
    mnv_camera cams[MNV_MAX_BATCH];
    for (int k = 0; k < K; ++k) {
        cams[k] = cv;
        cams[k].cx = cv.cx - I.aa_offsets[2 * k];
        cams[k].cy = cv.cy - I.aa_offsets[2 * k + 1];
    }
    if (P.draws_inputs) {  // the batch call has no per-pixel inputs: grid pass + march per camera, in stream order (the slot's two grid images are reused)
        for (int k = 0; k < K; ++k) {
            const mnv_frame_inputs in = I.grid_inputs(S, S.stream, cams[k], options);
            mnv_check(mnv_render_voxels_accel_ex(I.march_tree().device.accel, &cams[k], options.c_abi(), full, &in, S.aa_sub.get() + (size_t)k * frame_floats, nullptr, S.stream),
                      "mnv_render_voxels_accel_ex");
        }
    } else {
        const mnv_partition whole = {0, 1, 0, 0, 0};
        mnv_check(mnv_render_voxels_accel_batch(I.march_tree().device.accel, cams, K, options.c_abi(), full, whole, S.aa_sub.get(), nullptr, S.stream),
                  "mnv_render_voxels_accel_batch");
    }
    mnv_check(mnv_resolve_samples(S.aa_sub.get(), K, I.width, I.height, I.aa_weights_dev.get(), I.aa_radius, I.rgba, I.rgba8, S.stream), "mnv_resolve_samples");
    stats.used_accel = true;
}

// an orthographic or equirectangular projection: the frame's rays on the frame's slot and stream, then the ray march into the slot's frame
void VolumeRenderer::issue_projected(const mnv_camera &cv) {
    Impl &I = *impl_;
    Impl::Slot &S = I.slots[I.cur];
    const size_t ray_floats = (size_t)I.width * I.height * 3;
    if (!S.ray_origins || !S.ray_dirs) {
        hip_check(S.ray_origins.alloc(ray_floats), "hipMalloc(ray origins)");
        hip_check(S.ray_dirs.alloc(ray_floats), "hipMalloc(ray directions)");
    }
    mnv_check(mnv_generate_rays(projection, &cv, {0, 0, I.width, I.height}, projection == MNV_PROJ_EQUIRECT ? I.equirect_dev.get() : nullptr,
                                S.ray_origins.get(), S.ray_dirs.get(), S.stream),
              "mnv_generate_rays");
    mnv_check(mnv_render_rays_accel(I.march_tree().device.accel, S.ray_origins.get(), S.ray_dirs.get(), I.width, I.height, options.c_abi(), nullptr, I.rgba, I.rgba8, S.stream),
              "mnv_render_rays_accel");
    stats.used_accel = true;
}

// one rank of several (set_ranks); returns whether the frame took visit marks
bool VolumeRenderer::issue_ranks(const FramePlan &P, const mnv_camera &cv) {
    Impl &I = *impl_;
    N3Tree &tree = *I.tree;
    const mnv_rect full = {0, 0, I.width, I.height};
    const int world = I.part.world, rank = I.part.rank;
    int32_t j_max = 0;
    for (int r = 0; r < world; ++r) {
        const mnv_partition pr = {r, world, I.part.tile_w, I.part.tile_h, 0};
        j_max = std::max(j_max, mnv_partition_local_tiles(full, pr));
    }
    I.rank_px = (int64_t)j_max * I.part.tile_w * I.part.tile_h;
    const int64_t rows = I.rank_px * world;
    float *local = sized<float>(I.local, (size_t)I.rank_px * 4);
    uint8_t *local8 = sized<uint8_t>(I.local8, (size_t)I.rank_px * 4);
    // the same decisions on every rank: they depend on the camera and on the (replicated) tree only
    const Impl::Trackers T = I.begin_refinement(P, camera, options, stats, (int64_t)rank * I.rank_px);
    const bool track_visit = T.track_visit;
    // (not a row of plan()'s table: it takes the camera latch to know; every tree VolumeRenderer::set uploads has the array)
    if (track_visit && !P.has_parent) throw std::runtime_error("several ranks: visit marks need the tree's parent array");
    stats.used_accel = true;
    if (P.guided) {
        unsigned long long *counter = sized<unsigned long long>(I.fused_counter, 1);
        hip_check(hipMemsetAsync(counter, 0, sizeof(unsigned long long), I.stream), "clear sample counter");
        mnv_check(mnv_render_guided_fused_track_part(tree.device.accel, &cv, options.c_abi(), full, I.part, I.mlp, &I.grid, local, local8, T.my_split,
                                                     T.my_sample, T.split ? tree.device.sample_counts.get() : nullptr, track_visit ? T.visited : nullptr,
                                                     tree.device.parent.get(), counter, I.stream),
                  "mnv_render_guided_fused_track_part");
        I.read_count_later(counter);  // (this rank's share)
        stats.fused = true;
    } else {
        mnv_check(mnv_render_voxels_accel_visit_part(tree.device.accel, &cv, options.c_abi(), full, I.part, local, local8, T.my_split, T.my_sample,
                                                     tree.device.sample_counts.get(), track_visit ? T.visited : nullptr, tree.device.parent.get(), I.stream),
                  "mnv_render_voxels_accel_visit_part");
    }
    // the picture: tiles to rank 0, un-permuted there
    float *table = rank == 0 ? sized<float>(I.table, (size_t)rows * 4) : nullptr;
    uint8_t *table8 = rank == 0 ? sized<uint8_t>(I.table8, (size_t)rows * 4) : nullptr;
    mnv_check(mnv_gather_tiles(I.comm, local, table, (size_t)I.rank_px * 16, 0, I.stream), "mnv_gather_tiles");
    mnv_check(mnv_gather_tiles(I.comm, local8, table8, (size_t)I.rank_px * 4, 0, I.stream), "mnv_gather_tiles");
    if (rank == 0) {
        mnv_check(mnv_assemble_tiles(table, I.rgba, I.width, I.height, I.part, 1, 16, I.stream), "mnv_assemble_tiles");
        mnv_check(mnv_assemble_tiles(table8, I.rgba8, I.width, I.height, I.part, 1, 4, I.stream), "mnv_assemble_tiles");
    }
    // the votes need every rank's tracker rows, a prune every rank's marks
    if (T.split) {
        mnv_check(mnv_allgather(I.comm, T.split, (size_t)I.rank_px * 12, I.stream), "mnv_allgather");
        mnv_check(mnv_allgather(I.comm, T.sample, (size_t)I.rank_px * 12, I.stream), "mnv_allgather");
    }
    if (track_visit && world > 1) {
        // the marks of the chunks that exist: the replicas agree on tree.capacity, and a chunk beyond it cannot be marked (the table is
        // sized once for the largest tree -- reallocation would stall the frame -- but only cap words per rank travel and merge)
        const size_t cap = (size_t)tree.capacity;
        int32_t *marks = sized<int32_t>(I.marks_table, (size_t)I.max_tree_capacity * world);
        hip_check(hipMemcpyAsync(marks + cap * rank, T.visited, cap * 4, hipMemcpyDeviceToDevice, I.stream), "copy marks");
        mnv_check(mnv_allgather(I.comm, marks, cap * 4, I.stream), "mnv_allgather");
        mnv_check(mnv_merge_visit_marks(marks, world, (int32_t)cap, T.visited, I.stream), "mnv_merge_visit_marks");
    }
    return track_visit;
}

const char *VolumeRenderer::get_backend() { return "HIP gfx950"; }

void VolumeRenderer::download(std::vector<float> *rgba, std::vector<uint8_t> *rgba8) {
    download_slot(impl_->cur, rgba, rgba8);
}

int VolumeRenderer::last_slot() const { return impl_->cur; }

long VolumeRenderer::slot_guided_samples(int slot) {
    Impl &I = *impl_;
    if (slot < 0 || slot >= (int)I.slots.size()) throw std::runtime_error("slot_guided_samples: no such frame slot");
    Impl::Slot &S = I.slots[slot];
    if (!S.counted) return slot == I.cur ? stats.guided_samples : 0;
    hip_check(hipStreamSynchronize(S.stream), "slot_guided_samples");
    return (long)*S.count.host.get();
}

void VolumeRenderer::download_slot(int slot, std::vector<float> *rgba, std::vector<uint8_t> *rgba8) {
    if (slot < 0 || slot >= (int)impl_->slots.size() || !impl_->slots[slot].rgba) throw std::runtime_error("download_slot: no such frame slot");
    const size_t n = (size_t)impl_->width * impl_->height * 4;
    hip_check(hipStreamSynchronize(impl_->slots[slot].stream), "render");
    if (rgba) {
        rgba->resize(n);
        hip_check(hipMemcpy(rgba->data(), impl_->slots[slot].rgba.get(), n * sizeof(float), hipMemcpyDeviceToHost), "download rgba");
    }
    if (rgba8) {
        rgba8->resize(n);
        hip_check(hipMemcpy(rgba8->data(), impl_->slots[slot].rgba8.get(), n, hipMemcpyDeviceToHost), "download rgba8");
    }
}

void VolumeRenderer::sync_tree_streams() { impl_->sync_all(); }

void VolumeRenderer::sync_tree() {
    impl_->sync_all();
    if (impl_->tree) impl_->tree->copy_from_device(impl_->stream);
}

const float *VolumeRenderer::device_rgba() const { return impl_->rgba; }
const uint8_t *VolumeRenderer::device_rgba8() const { return impl_->rgba8; }

}  // namespace viewer
