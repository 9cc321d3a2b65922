// volume_renderer.hpp -- viewer::VolumeRenderer for offline batch rendering.
//
// Same role and member names as the reference facade (reference include/renderer/renderer.hpp:9-39,
// src/renderer/cuda_renderer.cpp:68-163,383-516): it owns a Camera and RenderOptions, `set()` moves a
// tree to the device, `resize()` sizes the frame, `render()` launches the march for the current
// camera.  The GL framebuffers / CUDA-GL interop / blit of the reference are replaced by a linear
// device frame (float RGBA + RGBA8) that `download()` copies to the host.
//
// With a model loaded (load_model / set_model) render() also runs the reference's refinement loop
// (cuda_renderer.cpp:98-156,205-381): options.use_guided_sampling composites per-sample network outputs
// instead of tree colours, options.use_splitting grows the tree from the per-ray trackers
// (expand_voxels / get_more_samples) and prunes unvisited chunks when it is nearly full (prune_tree).
// Every step is a device-resident libmnv entry point; the host only sequences them.  The networks are the
// build's own small MLPs (include/mnv.h, mnv_mlp_desc) -- the reference's TorchScript containers are not
// part of its repository.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "camera.hpp"
#include "n3tree.hpp"
#include "render_options.hpp"

namespace viewer {

// The sample pattern and the filter tables of anti-aliased frames (host arithmetic; the recipes are stated in include/mnv.h at
// mnv_aa_pattern / mnv_aa_weights, which check their arguments and call these).
void aa_pattern(int n_samples, float *offsets_xy);  // [n_samples][2]
int aa_filter_radius(int filter);
void aa_weights(int filter, int n_samples, const float *offsets_xy, float *weights);  // [n_samples][2r+1][2r+1]

struct VolumeRenderer {
    explicit VolumeRenderer();
    ~VolumeRenderer();

    // Render the currently set tree with `camera` and `options` (asynchronous on the internal stream).
    void render();
    // Set volumetric data to render: tree.move_to_device(max_tree_capacity, true, true) and
    // basis_minmax = {0, max(basis_dim - 1, 0)} as cuda_renderer.cpp:498-516.
    void set(N3Tree &tree, long max_tree_capacity);
    // Clear the volumetric data
    void clear();
    // Resize the frame.  The first call only sets the size; later calls rescale the intrinsics
    // (fx, fy, cx, cy each scaled once -- the reference scales cy twice, cuda_renderer.cpp:398,404-406).
    void resize(int width, int height);
    // Name identifying the renderer backend
    const char *get_backend();

    // Wait for the last render() and copy the frame to the host ([height][width][4]).
    void download(std::vector<float> *rgba, std::vector<uint8_t> *rgba8);
    // Frames in flight: plain frames (no refinement, a tree with the packed accel) rotate over this many slots, each with its own HIP stream
    // and frame buffers, so that the tail of one launch overlaps the next launches (1 = the reference's one-stream behaviour).
    // render() returns at once; last_slot() names the slot it used and download_slot() waits for that slot's frame only --
    // a caller that wants overlap downloads frame k after it has issued frames k+1 .. k+frames_in_flight-1.
    int frames_in_flight = 3;
    // Guided-sampling frames that change nothing (use_guided_sampling without use_splitting, the fused kernel, a tree below 3/4 of its
    // capacity) may rotate over the slots as well (default off: such a frame's sample count is then not known when render() returns --
    // stats.guided_samples is -1 and slot_guided_samples() waits for it).  1.20 -> 1.09 ms per 1080p frame on cfg2 with three in flight.
    bool guided_in_flight = false;
    long slot_guided_samples(int slot);
    int last_slot() const;
    int next_slot() const;       // the slot the next render() will take (with the options, tree and camera as they are now)
    bool overlaps_next() const;  // ... and whether that frame runs beside the previous ones (a plain frame on the packed accel)
    void download_slot(int slot, std::vector<float> *rgba, std::vector<uint8_t> *rgba8);
    // Wait for every frame in flight.
    void sync_tree_streams();
    // Device pointers of the current frame (valid until the next resize()).
    const float *device_rgba() const;
    const uint8_t *device_rgba8() const;
    // Average device time per render() since the last call, in ms (HIP events).

    // Role of load_model (cuda_renderer.cpp:518-539): read a model container.  Here an .npz with
    //   mlp_desc int32[9] (n_clusters, pos_octaves, dir_octaves, need_viewdir, n_embeddings, embedding_dim,
    //   hidden_width, hidden_layers, out_dim), mlp_center f32[3], mlp_inv_extent f32[3], mlp_params f16/u16 [..],
    //   grid_dim int32[2], min_position f32[3], max_position f32[3]
    // Sets options.need_viewdir / appearance_embedding from the description as the reference does.
    void load_model(const std::string &npz_path);
    void set_model(const mnv_mlp_desc &desc, const uint16_t *params, size_t n_halfs, const mnv_cluster_grid &grid);
    bool has_model() const;
    // The loaded model as the C ABI sees it (for callers that drive libmnv entry points themselves, e.g. the multi-GPU mode of mnv_render).
    const mnv_mlp *model() const;
    const mnv_cluster_grid &cluster_grid() const;
    // Copy the (refined) device tree back into the N3Tree's host arrays, e.g. before N3Tree::save_npz.
    void sync_tree();

    // Several ranks, one process per GPU, render and refine ONE scene in lock step (BASELINE.json configs[4] on several GPUs; SURVEY.md
    // 8(e): "identical deterministic refinement on every rank").  Every rank holds the whole tree and the networks.  render() then
    //   * marches only the macro tiles of this rank (pixels, tracker rows and visit marks: mnv_render_voxels_accel_visit_part /
    //     mnv_render_guided_fused_track_part),
    //   * all-gathers the tracker rows (mnv_allgather) -- the votes of cuda_renderer.cpp:205-227 count candidates over the whole frame and
    //     do not depend on the order of the rows -- and, on a visit-mark frame, the marks (mnv_merge_visit_marks),
    //   * runs the same split / resample / prune on every rank (same candidates, same jitter seed, same network): the replicas stay
    //     identical chunk for chunk, and equal to what one GPU makes of the same camera path,
    //   * gathers the tiles to rank 0 (mnv_gather_tiles) and un-permutes them there: rank 0's frame is the whole picture.
    // Needs the packed accel; guided sampling needs a network the fused kernel covers.  `comm` stays the caller's.
    void set_ranks(mnv_comm *comm, int tile_w = 64, int tile_h = 24);
    // The reference's render loop calls its three launchers with offscreen == false (cuda_renderer.cpp:111-113,135-136,141-142): rays stop at the
    // depth attachment of the GL pass, the frame is composited over its image.  Here the two attachments are device arrays of the caller
    // ([height][width] float, [height][width][4] uint8; either may be null) that stay valid while frames are rendered; both null (the default) is
    // the offline renderer.  One rank only.
    void set_frame_inputs(const float *tmax_px_device, const uint8_t *rgba8_init_device);
    // options.show_grid: every frame first draws the octree grid of options.grid_max_depth (the edges of N3Tree::gen_wireframe) with
    // mnv_render_wireframe into images of its own frame slot, on the slot's stream, and the march then runs with them as its frame inputs
    // (offscreen == false), whatever the frame kind -- what the reference's window shows with "Show Grid" on.  The edge list is
    // regenerated when the depth or the tree's structure changed (set, splits, prunes).  Refused (StatusError, MNV_E_INVALID) together with
    // set_frame_inputs or set_ranks.  wireframe(): the edge list of the last grid frame, null before the first.
    const mnv_wireframe *wireframe() const;
    // Meshes under the volume (the reference's Mesh::draw before the march): device handles of viewer::Mesh::update() / mnv_mesh_create,
    // not owned.  While any of them is visible, every frame draws the grid first (if options.show_grid), then the visible meshes over it
    // with mnv_render_meshes, into the frame slot's two images on the slot's stream, and marches with them as its frame inputs -- for every
    // frame kind the grid works for; with aa_samples > 1 the sub-frames are issued one by one, as with the grid.  Refused like the grid
    // together with set_frame_inputs or set_ranks.  With no visible mesh render() is what it is without this field.  Wait for the frames
    // in flight (sync_tree_streams) before a listed mesh is destroyed.
    std::vector<const mnv_mesh *> meshes;
    // The camera the last render() used (Camera::_update renormalises v_back on every call: the matrix may move by an ulp between frames).
    const mnv_camera &last_camera() const;

    // Anti-aliased frames (the reference has none: it point-samples into a window).  aa_samples == 1: render() is what it is without these
    // fields.  aa_samples = K > 1: a plain frame takes its slot as usual (overlaps_next(); slot 0 otherwise) and, on the slot's stream,
    // marches K cameras equal to the frame's but for cx - dx_k, cy - dy_k (aa_pattern) with ONE mnv_render_voxels_accel_batch launch into a
    // per-slot sub-frame buffer (float RGBA, K * W * H * 16 bytes: allocated at the first such frame, freed by resize() and when K changes)
    // and resolves them into the slot's rgba / rgba8 with mnv_resolve_samples through the device weight table of aa_filter (rebuilt when K
    // or the filter changes).  With options.show_grid the K sub-frames are issued one by one -- mnv_render_wireframe with camera k, then
    // mnv_render_voxels_accel_ex -- because the batch call takes no per-pixel inputs: slower, and the lines are what gains most.
    // Refused (StatusError, MNV_E_INVALID) with aa_samples > 1: set_frame_inputs (a depth image of the caller's fixed camera cannot follow
    // the jitter), set_ranks, a model with use_splitting / use_guided_sampling (refinement votes per ray of ONE camera), a tree without
    // a packed accel, aa_samples outside 1 .. MNV_MAX_BATCH, an unknown aa_filter.
    int aa_samples = 1;
    int aa_filter = MNV_AA_TENT;
    // Other projections than the pinhole camera (the reference has none).  MNV_PROJ_PINHOLE: render() is what it is without this field.
    // MNV_PROJ_ORTHO (camera.fx / fy: pixels per world unit; put the camera plane outside the volume) / MNV_PROJ_EQUIRECT (a panorama from
    // camera.center): the frame takes its slot as a plain frame does and, on the slot's stream, generates its rays with mnv_generate_rays
    // into per-slot buffers (width * height * 24 bytes, allocated at the first such frame, freed by resize()) and marches them with
    // mnv_render_rays_accel into the slot's rgba / rgba8; the equirectangular table is rebuilt when the size changes.  With
    // options.render_depth an orthographic frame from above is a height map.
    // Refused (StatusError, MNV_E_INVALID) with another projection than the pinhole: set_frame_inputs, set_ranks, options.show_grid, a
    // visible mesh, aa_samples > 1, a model with use_splitting / use_guided_sampling, a tree without a packed accel, an unknown projection.
    int projection = MNV_PROJ_PINHOLE;
    // Score every frame against a target image on the device (mnv_frame_metrics; the reference has none).  Null (the default): render() is
    // what it is without this call.  Otherwise every render() -- whatever the frame kind -- is followed, on the frame slot's stream, by
    // mnv_frame_metrics(flags, the standard window) of the slot's float frame against `rgba8_device` ([height][width][4] uint8) into the
    // slot's own device sums and by a 40-byte copy of them to pinned host memory; the frame itself does not change.  The pointer is sampled
    // at render(): it may change per frame, and the caller keeps an array valid until its slot was collected.  slot_metrics() waits for
    // that slot only and finishes the sums (mnv_metrics_finish); StatusError(MNV_E_INVALID) when the slot's last frame was not scored.
    // A resize() that changes the size clears the target (the first one only sets the size); so does a null pointer, together with the
    // scores not yet collected.
    // Refused (StatusError, MNV_E_INVALID): unknown flag bits; a target together with set_ranks, in either order.
    void set_target(const uint8_t *rgba8_device, int flags = 0);
    void slot_metrics(int slot, mnv_frame_metric_values *out);
    // Levels of detail (the reference has none).  0 (the default): render() is what it is without this call.  D >= 1: every frame marches
    // N3Tree::make_lod(D) of the tree that was set -- interior rows mipped from their children, the tree cut at depth D -- instead of the
    // tree itself: plain frames with or without frames in flight, anti-aliased and projected frames, the grid overlay (the grid of the
    // truncated tree) and meshes.  The truncated tree is built at the first frame that needs it (the frames in flight are waited for),
    // kept per depth, and all of them are dropped when set() gets a tree, clear() is called, or the tree was edited since.
    // Refused by render() (StatusError, MNV_E_INVALID) with D >= 1, because such a frame would edit or vote on the tree:
    // options.use_splitting, options.use_guided_sampling (hence visit marks), set_ranks.  A negative D is refused here.
    void set_lod(int max_depth);
    int lod() const;
    // View-dependent levels of detail.  An empty list (the default): render() is what it is without this call.  Otherwise every frame
    // marches N3Tree::make_view_lod(views, pixels, min_depth, max_depth) of the tree that was set: full depth where a voxel could cover
    // `pixels` pixels from one of the listed eyes, coarser elsewhere.  The CALLER names the viewpoints the cut must serve -- an offline
    // renderer knows its poses up front, and a cut that serves all of them is built once: nothing is re-cut per frame.  Same frame
    // kinds as set_lod; the tree is built at the first frame that needs it, kept until the views or parameters change, and dropped
    // where set_lod's trees are.  Refused by render() (StatusError, MNV_E_INVALID) with options.use_splitting,
    // options.use_guided_sampling, set_ranks, and set_lod(D > 0) at the same time.  Refused here: more than 4096 views, an eye or
    // focal length that is not finite, focal_px <= 0, pixels negative or not finite, min_depth < 1, max_depth < min_depth.
    void set_view_lod(const std::vector<mnv_lod_view> &views, float pixels, int min_depth = 1, int max_depth = 23);
    bool view_lod() const;
    // Culling to a pose set.  An empty list (the default): render() is what it is without this call.  Otherwise every frame marches
    // N3Tree::make_culled(cameras, options, weight_thresh) of the tree that was set: the tree without the leaves no ray of the listed
    // cameras' frames weights above weight_thresh, chunks left all-empty collapsed.  The CALLER names the poses, as with set_view_lod; a
    // frame from another pose shows what the listed ones left.  Same frame kinds as set_lod; the tree is built at the first frame that
    // needs it, kept until the cameras, the threshold or the march options (step_size, sigma_thresh, stop_thresh, render_bbox) change, and
    // dropped where set_lod's trees are.  Refused by render() (StatusError, MNV_E_INVALID) with options.use_splitting,
    // options.use_guided_sampling, set_ranks, and set_lod(D > 0) or set_view_lod at the same time.  Refused here: a threshold that is
    // negative or not finite, a camera without pixels or of more than 2^22.
    void set_cull(const std::vector<mnv_camera> &cameras, float weight_thresh = 0.f);
    bool cull() const;
    // Fit the level of detail to the full tree (N3Tree::fit_to; mnv_n3tree_fit_to_tree).  params.iterations == 0 or an empty list (the
    // default): nothing changes.  Otherwise every tree set_lod / set_view_lod builds from now on is fitted, right after it is built, to the
    // frames of the tree that was set at the listed cameras; trees built before are dropped, so the next frame builds and fits anew.
    // Refused wherever set_lod is (render() says so).  Refused here: negative iterations, learning rates that are not finite or negative.
    void set_lod_fit(const std::vector<mnv_camera> &cams, const mnv_fit_params &params);
    // The same with a choice of row step and batching (N3Tree::fit_to_ex; mnv_n3tree_fit_to_tree_ex); the overload above is this one with
    // SGD and full batch.  The optimizer's and the batching's own refusals surface at the frame that builds the tree.
    void set_lod_fit(const std::vector<mnv_camera> &cams, const mnv_fit_params_ex &params);

    // What the last render() did (the reference prints these to stdout).
    struct FrameStats {
        bool track_visit = false, used_accel = false, full = false;
        bool fused = false;                         // the guided-sampling frame ran as one kernel (mnv_render_guided_fused)
        int split_candidates = 0, added = 0;        // expand_voxels
        int sample_candidates = 0, resampled = 0;   // get_more_samples
        int pruned = 0;                             // prune_tree (-1: ran, nothing to prune)
        long guided_samples = 0;                    // rows sent to the networks by guided sampling
        long capacity = 0;
    } stats;
    // Seed of the sample-position jitter (torch::rand in the reference); frame f uses (seed, f).
    uint64_t seed = 0;
    // Guided-sampling frames run as one fused kernel when nothing but the picture is wanted from them (false: always the
    // four-step path of the reference, cuda_renderer.cpp:107-139).
    bool use_fused_guided = true;
    // No longer read: the packed accel follows every tree edit in place (splits, resampled leaves, prunes).  Kept for the C ABI.
    int accel_rebuild_after = 4;

    // Camera instance
    Camera camera;
    // Rendering options
    RenderOptions options;

private:
    // A frame is decided once, then issued.  plan() reads the renderer's state and options -- it makes no HIP call and changes nothing --
    // and answers: the kind of frame (background only; plain or guided beside the frames in flight; a tree frame alone on slot 0 that
    // may refine, with its march: fused guided, four-step guided, tracked on the accel, reference layout; ranks; anti-aliased;
    // projected), whether it takes the next slot, whether it draws its own inputs (grid, visible meshes), whether it refines, and
    // whether it is refused, by the one table of the combinations render() cannot serve.  overlaps_next() and next_slot() read the
    // same function, so what they predict is what render() does.  Which refusal is reported when several hold is not part of the contract.
    // render_frame() (render() but for the score): prepare the camera, plan, refuse, bring what the slots share up to date
    // (update_shared), take the slot, issue the kind's entry points, then the refinement epilogue.
    struct FramePlan;
    FramePlan plan() const;
    void render_frame();
    void update_shared(const FramePlan &P);
    void issue_background(const FramePlan &P, const mnv_camera &cv);
    void issue_plain(const FramePlan &P, const mnv_camera &cv);
    void issue_guided_in_flight(const FramePlan &P, const mnv_camera &cv);
    bool issue_tree(const FramePlan &P, const mnv_camera &cv);
    bool issue_ranks(const FramePlan &P, const mnv_camera &cv);
    void issue_aa(const FramePlan &P, const mnv_camera &cv);
    void issue_projected(const mnv_camera &cv);
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

}  // namespace viewer
