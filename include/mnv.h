/*
 * mnv.h -- C ABI of the MI355X-native N3Tree (PlenOctree) ray-march path.
 *
 * This is the drop-in boundary for ONE path of cmusatyalab/mega-nerf-viewer:
 * the per-ray octree traversal + spherical-harmonic evaluation + front-to-back
 * alpha compositing that the reference launches through
 *
 *     viewer::render_voxels(N3Tree&, const Camera&, const RenderOptions&, ...)
 *         reference: include/cuda/renderer_kernel.hpp:23-34
 *                    src/cuda/renderer_kernel.cu:396-437 (launcher), :243-292 (kernel)
 *
 * Conventions kept from the reference: non-owning views, caller-owned output
 * buffers, POD structs by value/pointer, asynchronous on a caller stream.
 * Conventions changed on purpose: every entry point returns
 * an int status (0 = ok, otherwise a hipError_t or MNV_E_* code) instead of
 * cuda_assert's exit(); the c2w matrix travels by value inside mnv_camera
 * (no hidden default-stream memcpy, camera.cpp:113-123); an explicit tile
 * rectangle selects the pixels to render (multi-GPU partition); float RGBA is
 * the primary output, RGBA8 (renderer_kernel.cu:237) an optional second one.
 *
 * All pointers named "device" must be HIP device pointers on the current
 * device.  No torch types cross this boundary.
 *
 * HOW THIS HEADER IS ORGANISED.  The DROP-IN CORE is the 30 entry points below, one per function / method of the reference's interface for
 * this path -- a maintainer who replaces src/cuda + the loaders binds exactly these (include/mnv_reference_binding.hpp does, inside a build of
 * the reference).  Everything else in this file is an EXTENSION the reference has no counterpart for, grouped by purpose further down: the
 * packed layout ("accel": mnv_accel_*, mnv_render_voxels_accel*, mnv_render_guided_fused*), multi-GPU (mnv_partition*, mnv_comm_*,
 * mnv_gather_tiles, mnv_assemble_tiles, ...), the device-side forms of the host logic between frames (mnv_select_*, mnv_apply_*,
 * mnv_prune_tree*, mnv_query_submodules, mnv_mlp_*), synthetic trees (mnv_synth_*).  No call's result depends on process-wide state, with
 * one opt-in exception that is documented where it is declared (mnv_set_tree_cache).
 *
 *   reference                                                   drop-in core (tests/test_capi_symbols.py: CORE)
 *   include/cuda/renderer_kernel.hpp:23-34  render_voxels        mnv_render_voxels, mnv_render_voxels_ex (offscreen == false)
 *   :36-52  get_samples_from_voxels                              mnv_get_samples_from_voxels, mnv_get_samples_from_voxels_ex
 *   :12-21  render_nerf_results                                  mnv_render_nerf_results
 *   :54-63  add_children_and_generate_samples                    mnv_add_children_and_generate_samples
 *   :65-73  generate_samples                                     mnv_generate_samples
 *   :75-79  adjust_parents_and_children                          mnv_adjust_parents_and_children
 *   include/renderer/renderer.hpp:9-39  VolumeRenderer           mnv_renderer_create, _destroy, _set, _load_model, _resize, _options,
 *                                                                _set_camera, _render, _download
 *   include/n3tree/n3tree.hpp:17-69  N3Tree                      mnv_n3tree_open, _free, _move_to_device, _host_view, _device_view
 *   include/data_format.hpp:7-22  DataFormat                     mnv_data_format_parse, mnv_data_format_to_string
 *   include/camera.hpp:12-87  Camera                             mnv_camera_init, mnv_camera_set_pose, mnv_camera_drag
 *   include/render_options.hpp:9-56, src/opts.cpp:17-32          mnv_default_render_options, mnv_cli_render_options
 *   src/cuda/common.cu:8-20  cuda_assert (exit)                  status codes + mnv_last_error
 */
#ifndef MNV_H
#define MNV_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNV_VERSION 1
#define MNV_BASIS_MAX 25 /* reference include/render_options.hpp:4 */

/* status codes (positive values are hipError_t) */
#define MNV_OK 0
#define MNV_E_INVALID (-1)     /* bad argument */
#define MNV_E_UNSUPPORTED (-2) /* e.g. N != 2, basis_dim not in {-1,0,1,4,9,16,25} */
#define MNV_E_NO_DEVICE (-3)   /* no HIP device / extension unusable */
#define MNV_E_IO (-4)          /* file / npz errors */
#define MNV_E_NO_RCCL (-5)     /* mnv_comm_*: librccl.so.1 cannot be loaded */
#define MNV_E_RCCL (-6)        /* mnv_comm_*: an RCCL call failed (text in mnv_last_error) */
#define MNV_E_FAULT (-7)       /* an EARLIER asynchronous frame on this object is known to be wrong (mnv_render_guided_fused*: watchdog) */

#define MNV_FORMAT_RGBA 0 /* reference include/data_format.hpp:8-12 */
#define MNV_FORMAT_SH 1

/*
 * Non-owning view of an N3Tree in the reference's own array layout
 * (replaces viewer::internal::TreeSpec, include/data_spec.hpp:25-50).
 */
typedef struct mnv_tree_view {
    const uint16_t *data;         /* [capacity][N^3][data_dim] binary16, n3tree.cpp:183-188 */
    const int32_t *child;         /* [capacity][N^3] relative chunk offsets, 0 = leaf, n3tree.cpp:92-97 */
    const int32_t *parent;        /* [capacity], may be NULL, n3tree.cpp:99-107 */
    const int16_t *sample_counts; /* [capacity][N^3], may be NULL, n3tree.cpp:191-193 */
    float offset[3];
    float scale[3];
    int32_t N;         /* spatial branching factor per axis.  N = 2 (every PlenOctree file) everywhere; mnv_render_voxels also takes
                          3 <= N <= 16 (arrays [capacity][N^3]...) through a general walk, as the reference's descent multiplies by tree.N
                          (rt_core.cuh:137-143; its loader warns about N != 2, n3tree.cpp:85-87).  The packed accel, the sample march and the
                          refinement entry points answer MNV_E_UNSUPPORTED for N != 2 (generate_samples is N == 2 in the reference too) */
    int32_t data_dim;  /* halfs per voxel row; sigma is column data_dim-1 */
    int32_t format;    /* MNV_FORMAT_* */
    int32_t basis_dim; /* SH basis functions per channel, -1 if none */
    int32_t capacity;  /* chunks in use */
} mnv_tree_view;

/* Replaces viewer::internal::CameraSpec (include/data_spec.hpp:9-23). */
typedef struct mnv_camera {
    int32_t width, height;
    float fx, fy, cx, cy;
    float c2w[12]; /* column-major [right | up | back | center], camera.cpp:55-82 */
} mnv_camera;

/* viewer::RenderOptions, field for field (include/render_options.hpp:9-56). */
typedef struct mnv_render_options {
    float step_size;
    float sigma_thresh;
    float stop_thresh;
    float background_brightness;
    float render_bbox[6];
    int32_t basis_minmax[2];
    float rot_dirs[3];
    bool show_grid;
    int32_t grid_max_depth;
    bool render_depth;
    bool use_splitting;
    bool use_guided_sampling;
    int32_t max_depth;
    int32_t samples_per_corner;
    int32_t split_batch_size;
    int32_t nerf_batch_size;
    int32_t max_sample_count;
    bool need_viewdir;
    int32_t appearance_embedding;
    int32_t max_guided_samples;
} mnv_render_options;

/* Tile of the camera image; the full frame is {0, 0, width, height}. */
typedef struct mnv_rect {
    int32_t x0, y0, w, h;
} mnv_rect;

/* ------------------------------------------------------------------ misc */

int mnv_version(void);
/* Thread-local description of the last non-zero status returned on this thread. */
const char *mnv_last_error(void);
/* first 16 hex digits of the SHA-256 over the library's sources (csrc/, host/, include/ in the Makefile's order) at build time */
const char *mnv_source_sha(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int mnv_device_count(void);
/* struct defaults of include/render_options.hpp:9-56 */
void mnv_default_render_options(mnv_render_options *opt);
/* CLI defaults of src/opts.cpp:17-32,49-67 (--bg 0, split/nerf batch 4096) */
void mnv_cli_render_options(mnv_render_options *opt);
/* Camera::Camera + Camera::_update pose math (src/camera.cpp:29-82):
 * fy<0 -> fx, cx<0 -> width/2, cy<0 -> height/2 (integer division as in the reference). */
void mnv_camera_init(mnv_camera *cam, int32_t width, int32_t height, float fx, float fy, float cx, float cy);
void mnv_camera_set_pose(mnv_camera *cam, const float center[3], const float v_back[3],
                         const float v_world_up[3]);
/* Camera's drag helpers (include/camera.hpp:22-25, src/camera.cpp:132-187) as one stateless call for hosts without the C++ struct: the
 * pose (center, v_back, origin; updated in place) after begin_drag(x0, y0, is_pan, about_origin); drag_update(x1, y1); end_drag(); and the
 * _update() of the next frame; cam->c2w receives the new matrix.  The C++ host model (host/camera.hpp) has the four members themselves. */
void mnv_camera_drag(mnv_camera *cam, float center[3], float v_back[3], const float v_world_up[3], float origin[3], float movement_speed,
                     int is_pan, int about_origin, float x0, float y0, float x1, float y1);

/* ------------------------------------------------- the hot path (device) */

/*
 * Direct replacement of viewer::render_voxels (offscreen branch,
 * renderer_kernel.cu:225-229,260,277-280) on the reference array layout.
 *   tree        device view (all array pointers are device pointers)
 *   tile        pixels [x0,x0+w) x [y0,y0+h) of cam's image
 *   rgba_out    device float [tile.h][tile.w][4]: rgb after background
 *               composite, a = accumulated opacity (the four floats the
 *               reference holds just before its u8 cast); may be NULL
 *   rgba8_out   device uint8 [tile.h][tile.w][4], renderer_kernel.cu:237; may be NULL
 *   split_track device float [tile.h][tile.w][3] (priority, chunk, child) or NULL
 *   sample_track same for the sample tracker or NULL (rt_core.cuh:237-252,308-321);
 *               the caller pre-fills both with -1 as cuda_renderer.cpp:97-98 does
 *   visited     device int32 [capacity] or NULL; marked when track_visit != 0
 *   hip_stream  hipStream_t; the call is asynchronous on it
 */
int mnv_render_voxels(const mnv_tree_view *tree, const mnv_camera *cam, const mnv_render_options *opt,
                      mnv_rect tile, float *rgba_out, uint8_t *rgba8_out, float *split_track,
                      float *sample_track, int32_t *visited, int track_visit, void *hip_stream);

/*
 * The reference's LIVE call shape.  VolumeRenderer::Impl::render passes offscreen == false to all three launchers
 * (src/renderer/cuda_renderer.cpp:111-113,135-136,141-142): the kernels then read, per pixel, a ray limit from the depth attachment
 * (float t_max = surf2Dread(surf_obj_depth), renderer_kernel.cu:277-280,354-357) and composite over the pixel that is already in
 * the image instead of over background_brightness (renderer_kernel.cu:230-234,260-264) -- how the volume goes behind / in front of
 * the wireframe mesh the GL pass drew.  The two cudaArray_t attachments become two linear device arrays, indexed like the outputs:
 */
typedef struct mnv_frame_inputs {
    const float *tmax_px;       /* device float [tile.h][tile.w]: t_max of every pixel; NULL = 1e9f everywhere (offscreen == true) */
    const uint8_t *rgba8_init;  /* device uint8 [tile.h][tile.w][4]: the image under the volume; NULL = background_brightness
                                   (offscreen == true).  May be the same buffer as rgba8_out (the reference reads and writes one surface). */
} mnv_frame_inputs;
/* mnv_render_voxels with the inputs of offscreen == false; inputs == NULL (or both members NULL) is mnv_render_voxels exactly. */
int mnv_render_voxels_ex(const mnv_tree_view *tree, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                         const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track,
                         int32_t *visited, int track_visit, void *hip_stream);

/*
 * Packed device re-layout of a tree ("accel"): one 32-bit word per voxel
 * (child link or leaf sigma), colour rows padded to 64 B, plus a dense
 * top-of-tree lookup grid.  Built once per tree upload -- the counterpart of
 * N3Tree::move_to_device (n3tree.cpp:207-246); results are bit-identical to
 * mnv_render_voxels.
 */
typedef struct mnv_accel mnv_accel;
int mnv_accel_create(const mnv_tree_view *device_tree, void *hip_stream, mnv_accel **out);
/* The same with room for max_capacity chunks, so that mnv_accel_refresh can follow a tree that grows by refinement. */
int mnv_accel_create_reserved(const mnv_tree_view *device_tree, int64_t max_capacity, void *hip_stream, mnv_accel **out);
/*
 * Bring the accel up to date after a refinement step on the same device arrays, without rebuilding it:
 *   tree           the view with its NEW capacity; chunks [old_capacity, tree->capacity) were appended under existing
 *                  leaves (mnv_add_children_and_generate_samples + mnv_apply_split_results); needs tree->parent then
 *   changed_nodes  device int32 [n_changed][2] (chunk, child) of existing leaves whose data row was rewritten
 *                  (mnv_apply_sample_results), or NULL.  An entry may name a voxel that was split in the same step (it is
 *                  skipped: the voxel is a link now, its new chunk is patched as an appended one), and an entry may
 *                  appear more than once (every copy writes the same words).  Without tree->parent (allowed when no
 *                  chunk was appended) the lookup arrays that a changed leaf reaches are derived again whole.
 * Node words, colour rows and chunk depths of the affected voxels are patched, and of the lookup grids exactly the cells
 * those voxels cover; the inline cell words and the brick records (mnv_accel_brick_levels) are patched in place with
 * them, and records are allocated and derived here when the tree first reaches two levels below the second grid.  A
 * tree that an edit takes past depth 23 is refused with MNV_E_UNSUPPORTED: the accel then describes no frame (its
 * brick levels read 0) until mnv_accel_rebuild accepts a tree again; mnv_render_voxels still renders the arrays.
 * After mnv_prune_tree, which renumbers chunks, call mnv_accel_rebuild (or prune with mnv_prune_tree_accel, which
 * renumbers the accel in place).
 * Ordering: all work is queued on hip_stream.  The call waits for hip_stream only up to the read-back of its flags
 * (chunk depths, node words and colour rows are then written); the kernels that patch the lookup grids, inline words
 * and records are queued behind that and are NOT waited for.  Work queued on hip_stream afterwards is ordered behind
 * them; a frame on another stream needs its own wait on hip_stream.
 */
int mnv_accel_refresh(mnv_accel *accel, const mnv_tree_view *tree, int32_t old_capacity, const int32_t *changed_nodes,
                      int32_t n_changed, void *hip_stream);
/* Rebuild every derived array from the tree in place (e.g. after mnv_prune_tree renumbered the chunks): the reserved arrays are
 * reused, nothing is reallocated unless the lookup-grid levels change.  Synchronises hip_stream. */
int mnv_accel_rebuild(mnv_accel *accel, const mnv_tree_view *tree, void *hip_stream);
void mnv_accel_destroy(mnv_accel *accel);
size_t mnv_accel_device_bytes(const mnv_accel *accel);
/* level of the brick-ordered second lookup grid (0: none): what a report names beside the bytes above */
int32_t mnv_accel_grid2_level(const mnv_accel *accel);
/* levels below that grid which every frame kind resolves WITHOUT walking node words: 1 = the last level is folded into the grid's cell words
 * (a depth-10 tree under a level-9 grid reads no node word at all in plain frames), 2 = the next two levels also come from 64-byte brick
 * records (trees with leaves two or more levels below the grid), 0 = neither (shallow trees).  mnv_accel_refresh patches both with the tree edit,
 * a prune derives them again: the value does not drop between frames of the refinement loop.  Frames are bit-identical either way. */
int32_t mnv_accel_brick_levels(const mnv_accel *accel);
/* How much of the tree those words cover -- a gauge for the one limit they have: an inline cell word names its chunk in 22 bits, relative to
 * the smallest chunk number of that depth (4.19 M numbers from there on); a chunk outside that span is not inline (records / node words
 * answer, bit-identical, one more dependent load).  out4: [0] non-leaf cells of the second grid (= chunks one level below it), [1] of them
 * inline, [2] of them NOT inline although all eight children are leaves (lost to the chunk field; 0 on every tree of the test suite up to
 * 12.7 M chunks), [3] chunks with a brick record.  Waits for the device. */
int mnv_accel_lookup_coverage(const mnv_accel *accel, int64_t out4[4]);
/* Compute units the tuned kernel may fill with its persistent workgroups (8 per unit).  Default (and num_cus <= 0): every unit
 * of the device.  A caller that launches on a stream created with hipExtStreamCreateWithCUMask -- to leave units free for
 * the RCCL kernels of the tile gather, which cannot become resident next to a full set of persistent workgroups -- passes
 * the number of units its mask enables.  New; the reference has no counterpart (auto_cuda_threads, renderer_kernel.cu:14-28,
 * sizes a non-persistent launch). */
int mnv_accel_set_cu_budget(mnv_accel *accel, int32_t num_cus);
int mnv_render_voxels_accel(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt,
                            mnv_rect tile, float *rgba_out, uint8_t *rgba8_out, void *hip_stream);
/* the same with the per-pixel inputs of the reference's offscreen == false call shape (mnv_frame_inputs above) */
int mnv_render_voxels_accel_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                               const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, void *hip_stream);

/*
 * Interleaved macro-tile partition of `tile` for multi-GPU rendering: the
 * rectangle is cut into macro tiles of tile_w x tile_h pixels (multiples of 8), numbered
 * row-major; this call renders the macro tiles m with m % world == rank.  Outputs are compact
 * and local-tile-major: local tile j = m / world is stored at
 * rgba_out[j][tile_h][tile_w][4] (pixels outside `tile` are left untouched), which is the
 * contiguous buffer each rank hands to the RCCL gather.  world <= 1 with tile_w == 0 is the plain call; world == 1 with a
 * tile size gives the same macro-tile-major layout from a single rank.
 */
typedef struct mnv_partition {
    int32_t rank, world;
    int32_t tile_w, tile_h;
    /* 0: macro tile m belongs to rank m % world (local index m / world).  M >= 2: tiles are still dealt in rounds of `world`, but every
     * M-th round leaves rank 0 out -- rank 0 renders (M - 1) / M of a plain share.  For the rank that also receives the gather and
     * un-permutes the frames (measured on one MI355X for world 8: that work stretches its march by 19 %, tools/root_emulation.py). */
    int32_t root_period;
} mnv_partition;
/* number of local macro tiles of `rank` (the leading dimension of its output buffer) */
int32_t mnv_partition_local_tiles(mnv_rect tile, mnv_partition part);
int mnv_render_voxels_accel_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt,
                                 mnv_rect tile, mnv_partition part, float *rgba_out, uint8_t *rgba8_out,
                                 void *hip_stream);

/*
 * Colour arithmetic of the tuned SH march, per accel (default 0).  0: every value is computed exactly as the arithmetic
 * specification says and frames are bit-identical to the oracle.  1: the colour sigmoid
 * weight / (1 + exp(-dot)) uses the hardware exp2 and reciprocal (about 1 ulp each).  Opacity, transmittance, step sizes and
 * every branch stay exact -- SURVEY.md section 7: colour-only arithmetic is continuous and feeds no control flow -- so alpha and
 * the step sequence are unchanged and colours move by ~1e-7 (bound asserted in the tests: 2e-6; contract 1e-4).
 * Trackers, sample emission, depth mode and RGBA-format trees are unaffected.
 */
/* mode 0 exact, 1 fast.  Two renderers of one process can differ; launches already queued keep the mode they were launched with.  (There is no
 * process-wide switch: no call's arithmetic depends on state outside its arguments.) */
int mnv_accel_set_colour_math(mnv_accel *accel, int mode);

/*
 * (mnv_render_voxels builds, in front of every launch of at least 65536 rays, a dense level-7 lookup table of the tree on the caller's stream --
 * stream-ordered scratch memory, about 10 us, 16 MB; csrc/mnv_march_ref_layout.hip -- because the caller's arrays may change between calls and
 * nothing is kept.  Smaller launches (tiles) derive a 512-cell table per workgroup instead.  Frames are bit-identical either way; the threshold
 * is not a switch of this library -- the test-hook build alone can move it, so that the tests run either path at any size.)
 */
/*
 * A memory for the stateless entry point.  viewer::render_voxels (renderer_kernel.hpp:23-34) takes the tree's arrays with every call
 * and keeps nothing, because its caller may edit them in between (the refinement of cuda_renderer.cpp:205-381 does); mnv_render_voxels
 * honours that by default and pays for it: it walks the reference's arrays (one stream: 0.62 ms per 1080p frame of cfg2 against 0.46 ms on
 * the packed re-layout).  mnv_set_tree_cache(1) (process-wide, default 0) lets it keep, per tree -- identified by the addresses of
 * `child` and `data`, `capacity` and the row format; up to four trees, least recently used out -- the packed re-layout of
 * mnv_accel_create, built on the caller's stream at the first call (tens of milliseconds, once) and used for every later plain frame
 * -- with the refinement trackers as well (the reference passes both tensors with every call, cuda_renderer.cpp:141-142; sample counts from
 * the call's view); only frames that ask for visit marks walk the arrays.  Frames and tracker rows are bit-identical either way.
 *   THE RULE: after changing the contents of a cached tree's arrays in place, call mnv_tree_invalidate(child) (NULL: every tree) before the
 *   next frame; a tree that moved or grew (other addresses, other capacity) is a new tree by itself.  Both calls wait for the device.
 *   FREEING a cached tree's arrays counts as changing them: an allocator that hands the same addresses to the next tree of the same
 *   capacity and row format (torch's caching allocator does) would otherwise be answered with the old tree's frames -- invalidate when a
 *   tree dies.  offset / scale are not part of a tree's identity: every frame uses the ones of the view it was called with.
 *   A tree whose re-layout cannot be built (deeper than 23 levels, out of memory) is remembered as such and rendered on the stateless
 *   path without another attempt until it is invalidated.
 * Memory: the re-layout is about 3.6 x the tree (cfg2: 2.6 GB beside 0.72 GB).
 */
void mnv_set_tree_cache(int enable);
void mnv_tree_invalidate(const void *child);

/*
 * The un-permute step on the gathering rank: `gathered` is what the RCCL gather of the ranks'
 * compact buffers produces, [world][n_frames][ceil(macro tiles / world)][tile_h][tile_w] pixels (n_frames = 1 for
 * mnv_render_voxels_accel_part), `frames` receives [n_frames][height][width] pixels.  bytes_per_pixel: 4 (RGBA8) or
 * 16 (float RGBA).  part.rank is ignored; part.root_period must be the one the ranks rendered with.
 */
int mnv_assemble_tiles(const void *gathered, void *frames, int32_t width, int32_t height, mnv_partition part, int32_t n_frames,
                       int32_t bytes_per_pixel, void *hip_stream);

/*
 * The gather that precedes it: the only collective of the path, RCCL over xGMI, one process per GPU (the
 * reference renders on one device, src/renderer/cuda_renderer.cpp:68-163, so there is no reference interface to cite).
 * RCCL (librccl.so.1) is bound at the first mnv_comm_* call; MNV_E_NO_RCCL when it cannot be loaded.
 *
 *   mnv_comm_get_unique_id   one rank (the root) draws the 128-byte id; the host program hands it to the other ranks
 *                            (pipe, shared memory, torch.distributed store -- the library does not care)
 *   mnv_comm_init_rank       collective over the `world` ranks; binds the communicator to the calling thread's current device
 *   mnv_gather_tiles         asynchronous on `hip_stream`: rank r's `local` (bytes_per_rank bytes, device) lands at
 *                            gathered + r * bytes_per_rank on the root (`gathered` is ignored elsewhere): grouped ncclRecv on the
 *                            root, one ncclSend on every other rank, a device copy for the root's own share (a send / receive
 *                            to itself when world == 1, so that a one-GPU box runs the RCCL path for real)
 * A communicator is used from one host thread at a time; calls on it are ordered like RCCL calls (same order on every rank).
 */
#define MNV_COMM_ID_BYTES 128
typedef struct mnv_comm mnv_comm;
int mnv_comm_get_unique_id(void *id_out /* MNV_COMM_ID_BYTES */);
int mnv_comm_init_rank(const void *id, int32_t world, int32_t rank, mnv_comm **out);
int32_t mnv_comm_rank(const mnv_comm *comm);
int32_t mnv_comm_world(const mnv_comm *comm);
int32_t mnv_comm_rccl_version(void); /* ncclGetVersion of the library that was bound, 0 if none */
int mnv_gather_tiles(mnv_comm *comm, const void *local, void *gathered, size_t bytes_per_rank, int32_t root, void *hip_stream);
/*
 * Refinement on several ranks (BASELINE.json configs[4]; SURVEY.md 8(e): "run identical deterministic refinement on every rank"): every
 * rank holds the whole tree, renders its macro tiles of the tracker frame and then needs ALL tracker rows to cast the same votes
 * (cuda_renderer.cpp:205-227 counts candidates over the whole frame; the count does not depend on the order of the rows).
 *   mnv_allgather            in place, asynchronous on `hip_stream`: `table` is [world][bytes_per_rank] on every rank, rank r has written
 *                            block r; afterwards every rank holds every block (grouped ncclSend / ncclRecv between all pairs: on xGMI
 *                            each pair has its own link)
 *   mnv_merge_visit_marks    visited[c] = max over r of table[r][c]: the union of the ranks' visit marks (each rank marks the chunks ITS
 *                            rays went through; a prune needs the frame's), after mnv_allgather of the per-rank mark arrays
 */
int mnv_allgather(mnv_comm *comm, void *table, size_t bytes_per_rank, void *hip_stream);
int mnv_merge_visit_marks(const int32_t *table, int32_t world, int32_t capacity, int32_t *visited, void *hip_stream);
void mnv_comm_destroy(mnv_comm *comm);

/*
 * Several frames in ONE launch: cams[0 .. n_cams) (same image size, same options, same tile /
 * partition); frame f is written at rgba_out + f * frame_elems * 4 (frame_elems = tile.w * tile.h, or
 * ceil(macro_tiles / world) * tile_w * tile_h under a partition -- the same on every rank, so that
 * the per-rank buffers have one shape even when a rank owns one tile fewer).  The ray queues span the frames of the
 * batch (frame-major), so wavefronts that finish their share of one frame carry on with the next: the tail of a frame overlaps
 * the start of the next -- for a camera path this is ~2x faster than one launch per frame.  n_cams <= MNV_MAX_BATCH.
 */
#define MNV_MAX_BATCH 64
int mnv_render_voxels_accel_batch(const mnv_accel *accel, const mnv_camera *cams, int32_t n_cams,
                                  const mnv_render_options *opt, mnv_rect tile, mnv_partition part, float *rgba_out,
                                  uint8_t *rgba8_out, void *hip_stream);

/*
 * The tuned march with the refinement trackers of render_voxels_trace_ray
 * (include/cuda/rt_core.cuh:179-180,237-252,308-321; consumed by cuda_renderer.cpp:150-175):
 * split_track / sample_track are [tile.h][tile.w][3] float rows (priority, chunk, child) exactly
 * as mnv_render_voxels writes them; sample_counts is the tree's live [capacity][N^3] int16 array in
 * the reference layout (it changes between frames, so it is not part of the accel) or NULL.
 * opt->max_depth / opt->max_sample_count bound the candidates.  The `visited` marks
 * (track_visit): mnv_render_voxels_accel_visit.
 * Either tracker may be NULL; with both NULL this is mnv_render_voxels_accel.
 */
int mnv_render_voxels_accel_track(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt,
                                  mnv_rect tile, float *rgba_out, uint8_t *rgba8_out, float *split_track,
                                  float *sample_track, const int16_t *sample_counts, void *hip_stream);

/* ------------------------------------------------ guided sampling kernels (BASELINE config 5) */

/* Cluster grid over world y,z used to route samples to sub-module MLPs
 * (model attributes grid_dim / min_position / range, cuda_renderer.cpp:524-539). */
typedef struct mnv_cluster_grid {
    int32_t grid_dim[2];
    float min_position[3];
    float range[3];
} mnv_cluster_grid;

/*
 * viewer::get_samples_from_voxels (include/cuda/renderer_kernel.hpp:36-52,
 * src/cuda/renderer_kernel.cu:329-363,439-485; rt_core.cuh:418-576), offscreen: the same march as
 * render_voxels, but every dense step emits (z, world xyz[, view dir][, embedding]) instead of colour.
 *   num_samples     device int16 [h*w], in/out; the caller zero-fills it (cuda_renderer.cpp:109)
 *   samples         device float [h*w][opt->max_guided_samples][samples_dim]; only emitted rows are
 *                   written (the caller pre-fills column 0 with -1, cuda_renderer.cpp:110)
 *   samples_dim     4 + 3 * need_viewdir + (appearance_embedding != -1)
 *   cluster_indices device int16 [h*w][max_guided_samples]
 *   split_track / sample_track / visited as in mnv_render_voxels
 */
int mnv_get_samples_from_voxels(const mnv_tree_view *tree, const mnv_camera *cam, const mnv_render_options *opt,
                                mnv_rect tile, float *split_track, float *sample_track, int32_t *visited,
                                int track_visit, int16_t *num_samples, float *samples, int32_t samples_dim,
                                int16_t *cluster_indices, const mnv_cluster_grid *grid, void *hip_stream);

/* ... with the depth attachment of the reference's offscreen == false call (renderer_kernel.cu:354-357: `float t_max = surf2Dread(surf_obj_depth)`):
 * inputs->tmax_px [tile.h][tile.w] limits every ray; inputs == NULL or tmax_px == NULL is the call above.  rgba8_init is not read (no image is written). */
int mnv_get_samples_from_voxels_ex(const mnv_tree_view *tree, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                   const mnv_frame_inputs *inputs, float *split_track, float *sample_track, int32_t *visited, int track_visit,
                                   int16_t *num_samples, float *samples, int32_t samples_dim, int16_t *cluster_indices,
                                   const mnv_cluster_grid *grid, void *hip_stream);

/* The same march on the packed accel (visit marks: mnv_get_samples_from_voxels_accel_visit below); sample_counts is the tree's
 * live [capacity][8] array or NULL.  Bit-identical rows. */
int mnv_get_samples_from_voxels_accel(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                      float *split_track, float *sample_track, const int16_t *sample_counts, int16_t *num_samples,
                                      float *samples, int32_t samples_dim, int16_t *cluster_indices, const mnv_cluster_grid *grid,
                                      void *hip_stream);

/*
 * Both tracker marches on the packed accel WITH visit marks (the role of render_voxels / get_samples_from_voxels called with
 * track_visit = true, cuda_renderer.cpp:101-102,112-114,141-142).  The reference marks every chunk of every descent
 * (query_single_from_root, rt_core.cuh:132-134); the packed layout skips most of the descent, so the march marks the chunk of every
 * leaf it steps through and a second small kernel closes the marks under `parent` -- the same array, element for element.
 * `visited` NULL = the plain tracker entry points; `parent` is the tree's device parent array [capacity].
 */
int mnv_render_voxels_accel_visit(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, float *rgba_out,
                                  uint8_t *rgba8_out, float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited,
                                  const int32_t *parent, void *hip_stream);
/* ... in the reference's LIVE call shape (mnv_frame_inputs, offscreen == false: the tracker frame of cuda_renderer.cpp:141-142 with its depth
 * image and the image under the volume); trackers and `visited` may be NULL (then mnv_render_voxels_accel_ex) */
int mnv_render_voxels_accel_visit_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                     const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track,
                                     const int16_t *sample_counts, int32_t *visited, const int32_t *parent, void *hip_stream);
int mnv_get_samples_from_voxels_accel_visit(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                            float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited,
                                            const int32_t *parent, int16_t *num_samples, float *samples, int32_t samples_dim,
                                            int16_t *cluster_indices, const mnv_cluster_grid *grid, void *hip_stream);
/* ... and with the ray limits of offscreen == false (as mnv_get_samples_from_voxels_ex) */
int mnv_get_samples_from_voxels_accel_visit_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                               const mnv_frame_inputs *inputs, float *split_track, float *sample_track, const int16_t *sample_counts,
                                               int32_t *visited, const int32_t *parent, int16_t *num_samples, float *samples, int32_t samples_dim,
                                               int16_t *cluster_indices, const mnv_cluster_grid *grid, void *hip_stream);
/* The tracker frame of one rank of a multi-GPU run: pixels AND tracker rows of the macro tiles `part` assigns to the rank, both in the
 * compact tile-major order of mnv_render_voxels_accel_part (row p of a tracker belongs to pixel p of the rank's buffer); rows of tiles a
 * ragged partition leaves out are not written (pre-fill with -1 as for a frame).  `visited` receives the marks of this rank's rays. */
int mnv_render_voxels_accel_visit_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, mnv_partition part,
                                       float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track, const int16_t *sample_counts,
                                       int32_t *visited, const int32_t *parent, void *hip_stream);

/*
 * viewer::render_nerf_results (include/cuda/renderer_kernel.hpp:12-21,
 * src/cuda/renderer_kernel.cu:294-327,365-394; rt_core.cuh:334-416), offscreen: composites
 * per-sample network outputs along every ray.
 *   tree          only offset/scale/format/basis_dim are read (host or device view alike)
 *   sample_values device float [n][value_stride]; sigma is column 3 (rt_core.cuh:365)
 *   z_vals        device float [n]
 *   offsets       device int64 [h*w]: inclusive prefix sums of the per-ray sample counts
 */
int mnv_render_nerf_results(const mnv_tree_view *tree, const mnv_camera *cam, const mnv_render_options *opt,
                            mnv_rect tile, const float *sample_values, int32_t value_stride, const float *z_vals,
                            const int64_t *offsets, float *rgba_out, uint8_t *rgba8_out, void *hip_stream);

/* --------------------------------------------- refinement kernels (BASELINE config 5) */

/* Mutable device view of the tree topology for the refinement kernels (the arrays a TreeSpec exposes
 * non-const, include/data_spec.hpp:26-28). */
typedef struct mnv_tree_edit {
    int32_t *child;   /* [max_capacity][8] */
    int32_t *parent;  /* [max_capacity] */
    float offset[3];
    float scale[3];
    int32_t N;        /* 2 */
    int32_t capacity; /* chunks in use BEFORE the call */
} mnv_tree_edit;

/*
 * viewer::add_children_and_generate_samples (include/cuda/renderer_kernel.hpp:54-63,
 * src/cuda/renderer_kernel.cu:170-198,487-510): appends num_parents chunks at [capacity, capacity +
 * num_parents), links them under parent_nodes[i] = (chunk, child), copies the visit mark, and turns the
 * caller's uniform [0,1) numbers in samples[num_parents*8][samples_per_corner][samples_dim] into
 * world-space sample points inside each new voxel (+ view dir / embedding columns, + cluster ids).
 */
int mnv_add_children_and_generate_samples(const mnv_tree_edit *tree, const mnv_render_options *opt,
                                          const int32_t *parent_nodes, int32_t num_parents, float *samples,
                                          int32_t samples_dim, int16_t *cluster_indices, int32_t *visited,
                                          const mnv_cluster_grid *grid, void *hip_stream);
/* viewer::generate_samples (renderer_kernel.hpp:65-73, renderer_kernel.cu:200-213,512-534): the same
 * sample generation for existing voxels nodes[i] = (chunk, child). */
int mnv_generate_samples(const mnv_tree_edit *tree, const mnv_render_options *opt, const int32_t *nodes,
                         int32_t num_items, float *samples, int32_t samples_dim, int16_t *cluster_indices,
                         const mnv_cluster_grid *grid, void *hip_stream);
/* viewer::adjust_parents_and_children (renderer_kernel.hpp:75-79, renderer_kernel.cu:63-86,536-549):
 * fixes relative child offsets and parent ids of chunks [first_shift_index, capacity) before compaction;
 * to_delete is a bool (1 byte) array, index_shifts an int32 array, both [capacity]. */
int mnv_adjust_parents_and_children(const mnv_tree_edit *tree, int32_t first_shift_index, const uint8_t *to_delete,
                                    const int32_t *index_shifts, void *hip_stream);

/* --------------------------- refinement: what the reference does with the trackers between frames
 * (VolumeRenderer::Impl::expand_voxels / get_more_samples / prune_tree, src/renderer/cuda_renderer.cpp:205-381,
 * there a chain of libtorch tensor ops; here device-resident, one call per step).  These calls
 * synchronise `hip_stream` before returning because they hand counts back to the host, as the
 * reference's `.size(0)` / `.item()` reads do. */

/*
 * expand_voxels' vote (cuda_renderer.cpp:205-227): among the rows (priority, chunk, child) of split_track
 * with chunk >= 0, count identical rows, keep those proposed by >= 2 rays, order by (count descending,
 * priority, chunk, child ascending) -- torch::unique_dim's lexicographic order on (-count, row) -- and write
 * the first min(max_out, n) as int32 (chunk, child) pairs to nodes_out (device, [max_out][2]).
 *   n_out         host: pairs written            n_candidates  host: rows that qualified ("Split candidates: N")
 * Rows hold integer-valued floats (|priority| < 32768, 0 <= chunk < 2^31, 0 <= child < 8), which is what the
 * march writes.  max_out = opt.split_batch_size.
 */
int mnv_select_split_candidates(const float *split_track, int64_t n_rows, int32_t max_out, int32_t *nodes_out,
                                int32_t *n_out, int32_t *n_candidates, void *hip_stream);
/* get_more_samples' selection (cuda_renderer.cpp:281-296): unique rows of sample_track with chunk >= 0 in
 * ascending (priority, chunk, child) order, no vote threshold; first min(max_out, n) as (chunk, child). */
int mnv_select_sample_candidates(const float *sample_track, int64_t n_rows, int32_t max_out, int32_t *nodes_out,
                                 int32_t *n_out, int32_t *n_candidates, void *hip_stream);
/*
 * cuda_renderer.cpp:262-270: rows [capacity*8, (capacity + num_parents)*8) of data (device binary16,
 * [max_capacity][8][data_dim]) become the mean over samples_per_corner of results[num_parents*8]
 * [samples_per_corner][result_stride] (device float, result_stride >= data_dim; the reference's is
 * data_dim + 1); sample_counts (may be NULL) of the new chunks is set to samples_per_corner.  `capacity` is
 * the chunk count BEFORE the split; the caller then adds num_parents to it.  Mean = fp32 sum in sample order /
 * n, rounded once to binary16 (torch's reduction order is unspecified: agreement is to 1 binary16 ulp).
 */
int mnv_apply_split_results(uint16_t *data, int16_t *sample_counts, int32_t capacity, int32_t num_parents,
                            const float *results, int32_t result_stride, int32_t samples_per_corner, int32_t data_dim,
                            void *hip_stream);
/*
 * cuda_renderer.cpp:307-332: running average of existing voxels nodes[i] = (chunk, child) with
 * samples_per_corner new network outputs each: data += (sum_new - half(n_new * data)) / (count + n_new),
 * count += n_new.  The reference expression stops at index_add_ (binary16 self, fp32 source is rejected by
 * libtorch), so the last rounding is this build's choice: one rounding of (old + update) to binary16.
 */
int mnv_apply_sample_results(uint16_t *data, int16_t *sample_counts, const int32_t *nodes, int32_t num_items,
                             const float *results, int32_t result_stride, int32_t samples_per_corner, int32_t data_dim,
                             void *hip_stream);
/*
 * prune_tree (cuda_renderer.cpp:335-381): chunks of [0, tree->capacity) whose visit mark is 0 are deleted,
 * the survivors are compacted in order (child offsets and parent ids fixed up by
 * mnv_adjust_parents_and_children with first_shift_index 0), and all marks but the root's are cleared over
 * [1, max_capacity).  data / tree->child / tree->parent are compacted; sample_counts too when non-NULL (the
 * reference leaves sample_counts uncompacted -- pass NULL for that behaviour).
 *   new_capacity  host: chunks in use after the call     num_deleted  host: 0 = "Nothing can be pruned"
 * Returns MNV_E_INVALID when the root itself is unmarked (no track_visit frame was rendered).
 */
int mnv_prune_tree(const mnv_tree_edit *tree, uint16_t *data, int32_t data_dim, int16_t *sample_counts, int32_t *visited,
                   int32_t max_capacity, int32_t *new_capacity, int32_t *num_deleted, void *hip_stream);
/* The same, and the packed accel of the tree follows in place (NULL: plain mnv_prune_tree): surviving chunks are renumbered in the node
 * words and both lookup grids, voxels whose sub-tree went become leaves, the colour rows are compacted -- about 0.9 ms of traffic for
 * the 1.5 M-chunk tree instead of the 2.9 ms of mnv_accel_rebuild.  The accel must describe the tree as it is before the call. */
int mnv_prune_tree_accel(const mnv_tree_edit *tree, uint16_t *data, int32_t data_dim, int16_t *sample_counts, int32_t *visited,
                         int32_t max_capacity, mnv_accel *accel, int32_t *new_capacity, int32_t *num_deleted, void *hip_stream);

/* torch::rand's role in expand_voxels / get_more_samples (cuda_renderer.cpp:247-250,298-301): n uniform numbers in
 * [0, 1) with 24 random bits each, a pure function of (seed, index) -- reproducible, unlike the reference. */
int mnv_fill_uniform(float *out, int64_t n, uint64_t seed, void *hip_stream);
/*
 * The step between mnv_get_samples_from_voxels and the network (cuda_renderer.cpp:116-121,135):
 * offsets_out[ray] = inclusive prefix sum of num_samples (device int64 [n_rays], what mnv_render_nerf_results
 * takes), and the emitted rows of samples[n_rays][max_guided_samples][samples_dim] packed in ray order:
 * z_vals_out[total] = column 0, rows_out[total][samples_dim - 1] = the remaining columns,
 * clusters_out[total].  total_out (host) = offsets_out[n_rays - 1]; returns MNV_E_INVALID when it exceeds
 * rows_capacity.  With all three outputs NULL only offsets_out and total_out are produced (to size the buffers).
 * Synchronises hip_stream (the total sizes the network launch).
 */
int mnv_compact_guided_samples(const int16_t *num_samples, const float *samples, const int16_t *cluster_indices, int64_t n_rays,
                               int32_t max_guided_samples, int32_t samples_dim, int64_t *offsets_out, float *z_vals_out,
                               float *rows_out, int16_t *clusters_out, int64_t rows_capacity, int64_t *total_out,
                               void *hip_stream);

/* ------------------------------------------------ per-sample sub-module network
 *
 * Stands in for VolumeRenderer::Impl::query_submodules (src/renderer/cuda_renderer.cpp:165-203): every sample
 * row is routed to the network of its cluster and the outputs are scattered back in input order.  The
 * reference loads its networks as TorchScript files that are not part of its repository (model_path,
 * cuda_renderer.cpp:518-539), so PARITY IS UNPINNED for the arithmetic: this is the build's own small MLP
 * (triangle-wave position encoding, `hidden_layers` x `hidden_width` ReLU layers with binary16 activations
 * and fp32 accumulation on the matrix cores, linear fp32 output), checked against its own CPU restatement.
 */
typedef struct mnv_mlp_desc {
    int32_t n_clusters;     /* sub-modules; cluster ids 0 .. n_clusters-1 (cuda_renderer.cpp:529-533) */
    int32_t pos_octaves;    /* encoded position: 3 + 6 * pos_octaves features */
    int32_t dir_octaves;    /* encoded direction: 3 + 6 * dir_octaves features when need_viewdir */
    int32_t need_viewdir;   /* sample rows are xyz, dir[3] (opt.need_viewdir) */
    int32_t n_embeddings;   /* > 0: rows end with an appearance-embedding index (opt.appearance_embedding != -1) */
    int32_t embedding_dim;  /* features per embedding (1 .. 64) */
    int32_t hidden_width;   /* 64 or 128 */
    int32_t hidden_layers;  /* >= 1 */
    int32_t out_dim;        /* tree data_dim + 1 (cuda_renderer.cpp:255-257), <= hidden_width */
    float center[3];        /* position normalisation p = (xyz - center) * inv_extent */
    float inv_extent[3];
} mnv_mlp_desc;
typedef struct mnv_mlp mnv_mlp;
/* binary16 parameters per cluster, in this order, all row-major: W0[hidden][in], b0[hidden], then
 * (hidden_layers - 1) x { W[hidden][hidden], b[hidden] }, Wout[out][hidden], bout[out],
 * embedding[n_embeddings][embedding_dim]; in = 3 + 6 pos_octaves (+ 3 + 6 dir_octaves) (+ embedding_dim). */
size_t mnv_mlp_param_count(const mnv_mlp_desc *desc);
/* params: host, n_clusters * mnv_mlp_param_count() binary16 values, cluster-major. */
int mnv_mlp_create(const mnv_mlp_desc *desc, const uint16_t *params, size_t n_halfs, void *hip_stream, mnv_mlp **out);
void mnv_mlp_destroy(mnv_mlp *mlp);
/*
 * samples: device float [n][samples_stride], columns xyz[, dir][, embedding index] first (the layout
 * mnv_get_samples_from_voxels writes after its z column and the refinement kernels write from column 0);
 * cluster_indices: device int16 [n]; results: device float [n][result_stride], columns [0, out_dim) written.
 * Rows whose cluster id is outside [0, n_clusters) get zeros.  Asynchronous on hip_stream; the handle holds the
 * launch scratch, so one handle serves one stream at a time.
 * Arithmetic, for every p whose octaves p 2^k are finite float32 values: encoded inputs and hidden activations are binary16
 * values (round to nearest even, subnormals kept: the matrix instruction does not flush them); the embedding index is
 * truncated toward zero and clamped to the table.  A
 * coordinate or activation beyond binary16's range is an infinity, and an infinity that meets a zero weight, or one of the
 * other sign, makes the accumulator NaN: a hidden layer's ReLU sends a NaN accumulator to +0, as it sends a negative one and -0
 * (the matrix instruction's NaN carries the sign bit, so the kernel's clamp needs no instruction for it); the output layer has
 * no ReLU and returns it.  On networks whose fp32 partial sums are all exact the result equals the CPU restatement in every bit
 * (tests/test_mlp_exact_gpu.py); elsewhere it differs by the order of the fp32 sums.
 */
int mnv_query_submodules(mnv_mlp *mlp, const int16_t *cluster_indices, const float *samples, int32_t samples_stride,
                         int64_t n, float *results, int32_t result_stride, void *hip_stream);

/*
 * The guided-sampling frame as ONE kernel (BASELINE.json configs[4]): what the reference does with get_samples_from_voxels,
 * a cumsum / boolean-mask compaction, query_submodules and render_nerf_results (src/renderer/cuda_renderer.cpp:107-139) --
 * and this library's own four entry points above do the same way -- happens inside the march: every lane marches its ray on
 * the packed accel and releases its samples into a per-wavefront pool in LDS; the wavefront evaluates the sub-module network for
 * 64 pooled samples at a time on the matrix cores (weights of the samples' cluster as the MFMA A operand), and the lane that owns a
 * ray composites its samples in ray order.  No sample buffer exists in global memory.  The frame is bit-identical to mnv_get_samples_from_voxels_accel -> mnv_compact_guided_samples ->
 * mnv_query_submodules -> mnv_render_nerf_results (same march, same MFMA sequence, same composite arithmetic).
 * Restrictions (MNV_E_UNSUPPORTED otherwise; use the four-step path): 64-wide networks with at most 64 encoded inputs,
 * RGBA / SH1/4/9/16 trees, no render_depth.  Refinement trackers and visit marks: mnv_render_guided_fused_track.
 *   sample_counter  optional device counter, ONE word: += network evaluations (= what the four-step path reports as guided samples)
 * Two kernels serve these entry points (csrc/mnv_guided_fused2.h, csrc/mnv_guided_fused.h), same frames bit for bit: when the weights
 * of one sub-module fit a workgroup's LDS beside the sample rings (every 64-wide network of up to about 6 layers), a workgroup
 * is three wavefronts that only march and push their samples into rings in LDS plus one wavefront that only evaluates the
 * network -- weights resident in LDS, results handed back through the rings, the owning lanes composite; otherwise every
 * wavefront does both jobs in turn (weights from L2).  mnv_accel_set_fused_kernel selects one explicitly.
 */
int mnv_render_guided_fused(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, const mnv_mlp *mlp,
                            const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out, unsigned long long *sample_counter,
                            void *hip_stream);
/* Which kernel the mnv_render_guided_fused* entry points launch on THIS accel: 0 = choose by the network's size (default),
 * 1 = the one-role kernel (every wavefront marches and evaluates), 2 = producer / consumer wavefronts wherever the rings, the
 * rays' constants and the weights of enough sub-modules fit a workgroup's LDS (the one-role kernel otherwise). */
int mnv_accel_set_fused_kernel(mnv_accel *accel, int version);
/* Diagnostics of the fused kernels on THIS accel: `words32` = NULL (default, none) or a device buffer of 32 64-bit words the
 * kernels add run counts and per-phase times to (tools/guided_bench.py names them).  Costs a few per cent while set.  The library keeps
 * only the address: the buffer must outlive every launch made while it is set (pass NULL before freeing it). */
int mnv_accel_set_fused_diag(mnv_accel *accel, unsigned long long *words32);
/* The producer / consumer kernel waits with s_sleep polls under a watchdog (a bug ends in wrong pixels, never in a hung device).  A
 * wait the watchdog abandons is counted in a device word of the accel -- always, with or without mnv_accel_set_fused_diag.  The frame's own
 * call has long returned (the entry points are asynchronous), so: the NEXT mnv_render_guided_fused* call on this accel prints one line
 * on stderr and returns MNV_E_FAULT once per fault, and mnv_accel_fused_faults reads the count since mnv_accel_create (it waits for
 * the device).  No wait has ever been abandoned in a test or stress run; the count is 0 on a healthy build. */
int mnv_accel_fused_faults(const mnv_accel *accel, uint32_t *count_out);
/* The same frame when refinement is on as well (BASELINE.json configs[4] has both switches on: cuda_renderer.cpp:107-156): the fused
 * kernel also writes the refinement trackers (rows pre-filled with -1 by the caller, as cuda_renderer.cpp:97-98) and, with `visited` +
 * `parent`, the visit marks -- what get_samples_from_voxels produces besides the samples (rt_core.cuh:475-507,561-574).  A ray that
 * has emitted max_guided_samples samples keeps marching here (its trackers follow the remaining steps); the picture is the same. */
int mnv_render_guided_fused_track(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, const mnv_mlp *mlp,
                                  const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track,
                                  const int16_t *sample_counts, int32_t *visited, const int32_t *parent, unsigned long long *sample_counter,
                                  void *hip_stream);
/* The fused frame in the reference's LIVE call shape (offscreen == false in get_samples_from_voxels and render_nerf_results,
 * cuda_renderer.cpp:111-113,135-136): every ray stops at inputs->tmax_px (renderer_kernel.cu:354-357).  inputs->rgba8_init is not read:
 * render_nerf_results_kernel leaves out[3] at 1 (renderer_kernel.cu:316), so composite_and_write adds the image under the volume with
 * weight 1 - 1 = 0 (:224-234) -- with or without it the frame is the same.  Tracker arguments may be NULL as in mnv_render_guided_fused. */
int mnv_render_guided_fused_track_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                     const mnv_frame_inputs *inputs, const mnv_mlp *mlp, const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out,
                                     float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited, const int32_t *parent,
                                     unsigned long long *sample_counter, void *hip_stream);
/* The fused frame of one rank of a multi-GPU run: the macro tiles `part` assigns to the rank, written tile-major like
 * mnv_render_voxels_accel_part (guided sampling reads the tree only, so the ranks need no exchange but the usual tile gather). */
int mnv_render_guided_fused_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, mnv_partition part,
                                 const mnv_mlp *mlp, const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out,
                                 unsigned long long *sample_counter, void *hip_stream);
/* ... with the tracker rows and visit marks of mnv_render_guided_fused_track for the rank's tiles (compact order, as
 * mnv_render_voxels_accel_visit_part): the frame of configs[4] -- refinement and guided sampling both on -- on one rank of several. */
int mnv_render_guided_fused_track_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, mnv_partition part,
                                       const mnv_mlp *mlp, const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out, float *split_track,
                                       float *sample_track, const int16_t *sample_counts, int32_t *visited, const int32_t *parent,
                                       unsigned long long *sample_counter, void *hip_stream);

/* A HIP stream whose kernels run on all but `reserve_cus` compute units (hipExtStreamCreateWithCUMask; the units are taken
 * evenly from the XCDs, and from their shader engines when reserve_cus is a multiple of 32).  The tuned kernel is persistent and
 * fills every wave slot of the units it may use, so kernels of other streams -- the RCCL channel workgroups of the multi-GPU
 * tile gather (about 288 VGPRs per lane: they do not fit beside more than three march workgroups) -- would otherwise wait
 * for a whole launch to drain.  Launch the march on this stream and give the accel the matching budget
 * (mnv_accel_set_cu_budget(accel, *enabled_cus)).  reserve_cus == 0: an ordinary non-blocking stream.  New: the reference
 * renders on one GPU and has no gather. */
int mnv_stream_create_reserved(int32_t reserve_cus, void **stream_out, int32_t *enabled_cus);
int mnv_stream_destroy(void *stream);

/* ------------------------------------------------ the octree grid overlay (RenderOptions::show_grid, grid_max_depth)
 * The reference draws the edges of N3Tree::gen_wireframe(grid_max_depth) (n3tree.cpp:249-329) with GL into the two attachments its march
 * then reads with offscreen == false (cuda_renderer.cpp:68-90,111-142): an RGBA8 image cleared to background_brightness with the edges in
 * black, and an R32F "Depth" image cleared to 1e9 holding the camera-space distance of the nearest edge.  Here the edge list lives on the
 * device and a line rasteriser writes that pair (mnv_frame_inputs).
 *
 * mnv_wireframe: the cubes gen_wireframe would push, built from a DEVICE tree view by a level-synchronous walk (one kernel and one wait per
 * tree level).  A voxel is a cube when child == 0 || depth >= max_depth (a negative max_depth acts like 0).  N != 2 answers
 * MNV_E_UNSUPPORTED; a child link outside [1, capacity) MNV_E_INVALID.  _update regenerates in place (after the tree or the depth changed);
 * both wait for hip_stream.  Calls that read a wireframe on other streams must have finished before it is updated or destroyed. */
typedef struct mnv_wireframe mnv_wireframe;
int mnv_wireframe_create(const mnv_tree_view *device_tree, int32_t max_depth, void *hip_stream, mnv_wireframe **out);
int mnv_wireframe_update(mnv_wireframe *w, const mnv_tree_view *device_tree, int32_t max_depth, void *hip_stream);
void mnv_wireframe_destroy(mnv_wireframe *w);
int64_t mnv_wireframe_cube_count(const mnv_wireframe *w);
/* The segments: device float [n][6] (world endpoints A xyz, B xyz), 12 per cube in _push_wireframe_bb's edge order, the corners in the
 * reference's float arithmetic; the order of the cubes is unspecified.  *n_segments receives the count (segments_out NULL and
 * cap_segments 0: the count only); a buffer of fewer than that many segments is MNV_E_INVALID. */
int mnv_wireframe_segments(const mnv_wireframe *w, float *segments_out, int64_t cap_segments, int64_t *n_segments, void *hip_stream);
/*
 * The GL pass as a kernel: writes tile [tile.h][tile.w] of both images (clear values included; either output may be NULL), the
 * mnv_frame_inputs pair of the frame.  rgba8_out must be 4-byte aligned (else MNV_E_INVALID).  Raster contract (float32, this order, no contraction):
 *   1. camera coordinates: c2w columns r, u, b, C; d = P - C; X = (r0*d0 + r1*d1) + r2*d2, Y likewise with u,
 *      z = -((b0*d0 + b1*d1) + b2*d2)
 *   2. near clip: a segment with both z < 1e-3f is dropped; if one endpoint has z < 1e-3f it moves along the camera-space segment to
 *      t = (1e-3f - z_in) / (z_out - z_in), X_in = X_in + t*(X_out - X_in) (Y alike), z_in = 1e-3f.  No far plane, no x/y clip.
 *   3. pixels: px = cx + fx*(X/z), py = cy - fy*(Y/z) (pixel (x, y) is centred at (x+0.5, y+0.5): the inverse of screen2worlddir,
 *      renderer_kernel.cu:30-38); dx = px_b - px_a, dy = py_b - py_a, dd = dx*dx + dy*dy; dd == 0 (or not finite): nothing
 *   4. line rule: x-major when |dx| >= |dy|: one fragment in every column x whose centre xc = x + 0.5f lies in [min px, max px), in
 *      row floor(py_a + ((xc - px_a) / dx) * dy); y-major alike with rows; fragments outside the tile are discarded
 *   5. fragment value: t = clamp(((xc - px_a)*dx + (yc - py_a)*dy) / dd, 0, 1) at the pixel centre (xc, yc); qa = (1 - t)/z_a,
 *      qb = t/z_b, s = qa + qb; X = (qa*X_a + qb*X_b)/s, Y alike, Z = (qa*z_a + qb*z_b)/s; dist = sqrt((X*X + Y*Y) + Z*Z);
 *      key = bits(Z) << 32 | bits(dist), the smallest key of a pixel wins
 *   6. outputs: a pixel with a fragment: tmax = dist, rgba8 = (0,0,0,255); else tmax = 1e9f, rgba8 = (c,c,c,255) with
 *      c = floor(clamp(background_brightness, 0, 1)*255 + 0.5)
 * Deliberate deviations from the GL pass: the principal point is the camera's cx, cy (the reference's K ignores them); depth ties are
 * broken by the key (GL keeps the first-drawn fragment); the fragments are this rule's, not a particular GL driver's.
 */
int mnv_render_wireframe(const mnv_wireframe *w, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, float *tmax_px_out,
                         uint8_t *rgba8_out, void *hip_stream);
/* How mnv_render_wireframe resolves depth; the images are bit-identical either way (the smallest key wins whatever the order).
 *   MNV_WIREFRAME_BINNED  (edge, 32x32 screen tile) pairs are counted, scanned and listed per tile (one wait for the pair total), then one
 *                         workgroup per tile resolves its fragments with 64-bit atomicMin in LDS
 *   MNV_WIREFRAME_GLOBAL  thread per edge, a 64-bit global atomicMin per fragment into a key image, then a resolve pass
 *   MNV_WIREFRAME_AUTO    (default) the one measured faster for the edge count
 * Scratch is kept per HIP stream; calls on one stream from several host threads are serialised by the object. */
#define MNV_WIREFRAME_AUTO 0
#define MNV_WIREFRAME_BINNED 1
#define MNV_WIREFRAME_GLOBAL 2
int mnv_wireframe_set_method(mnv_wireframe *w, int32_t method);

/* ------------------------------------------------ meshes under the volume (viewer::Mesh, include/mesh.hpp, src/mesh.cpp)
 * The reference composites its volume with meshes: Mesh::draw writes an RGBA8 image and an R32F image holding length(FragPos), and the march
 * then reads both with offscreen == false.  mnv_render_meshes is that pass for any list of meshes, without GL: it writes the
 * mnv_frame_inputs pair of a frame, alone or over the grid pass.
 *
 * mnv_mesh: the arrays Mesh::update uploads, copied to the device by mnv_mesh_create (which waits for the copies).
 *   vert       host float [n_verts][9]: position, colour, normal
 *   faces      host uint32 [n_indices], face_size per primitive, or NULL with n_indices 0 for non-indexed drawing (glDrawArrays over n_verts)
 *   face_size  1 points, 2 lines, 3 triangles
 *   unlit      the fragment shader's switch: the vertex colour alone
 * MNV_E_INVALID: another face_size, an index >= n_verts, an index count (or, non-indexed, a vertex count) that is no multiple of
 * face_size, null or empty vertices, indices without a count or a count without indices.  A new mesh is visible and has the identity as
 * its model matrix.  mnv_mesh_model_matrix takes a row-major 3 x 4 float matrix (mnv_model_matrix makes the reference's);
 * mnv_mesh_show is Mesh::visible.  Calls that draw a mesh must have finished before it is destroyed.
 */
typedef struct mnv_mesh mnv_mesh;
int mnv_mesh_create(const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size, int unlit, mnv_mesh **out);
/* new arrays for an existing handle (same checks; on an error the mesh keeps what it had); the model matrix and visibility stay */
int mnv_mesh_update(mnv_mesh *m, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size, int unlit);
void mnv_mesh_destroy(mnv_mesh *m);
int mnv_mesh_model_matrix(mnv_mesh *m, const float *matrix3x4);
int mnv_mesh_show(mnv_mesh *m, int visible);
int mnv_mesh_visible(const mnv_mesh *m);
int64_t mnv_mesh_vertex_count(const mnv_mesh *m);
int64_t mnv_mesh_face_count(const mnv_mesh *m); /* primitives: n_indices / face_size, or n_verts / face_size when non-indexed */
int32_t mnv_mesh_face_size(const mnv_mesh *m);
/* The model matrix of Mesh::draw (src/mesh.cpp:137-150) from (rotation axis-angle, translation, scale), on the host (no GPU needed):
 * identity rotation when |rotation| < 1e-3, else glm::angleAxis(|rotation|, rotation / |rotation|) as a matrix; times scale; the
 * translation in the fourth column.  Computed in double, rounded to float once.  out: row-major 3 x 4. */
int mnv_model_matrix(const float rotation[3], const float translation[3], float scale, float *matrix3x4_out);
/* viewer::Mesh::load_obj (host/mesh.hpp states what is read and how vertices are formed), on the host: the arrays mnv_mesh_create takes.
 * default_color NULL = white.  Size-query convention of mnv_n3tree_gen_wireframe: *n_floats (9 per vertex), *n_indices (0: non-indexed)
 * and *face_size are always set; vert / faces NULL with capacity 0 ask for them alone; a buffer that is too short is MNV_E_INVALID.  A
 * file that cannot be read or is malformed: MNV_E_IO, mnv_last_error names the line ("line N"). */
int mnv_obj_read(const char *path, const float *default_color, float *vert, int64_t cap_floats, int64_t *n_floats, uint32_t *faces,
                 int64_t cap_indices, int64_t *n_indices, int32_t *face_size);
/*
 * The mesh pass as kernels: writes tile [tile.h][tile.w] of both images (either output may be NULL; rgba8 images 4-byte aligned, else
 * MNV_E_INVALID).  Invisible meshes are skipped.  under == NULL: the images start cleared (tmax = 1e9f, rgba8 = the background of the
 * wireframe's step 6).  under != NULL: the pass draws over an earlier pass's images (a NULL member of `under` stands for its clear
 * value); `under` may name the outputs themselves.  Asynchronous on hip_stream but for one wait (the size of the tile lists); scratch
 * is kept per HIP stream, calls from several host threads are serialised.
 *
 * Raster contract (float32, this order, no contraction, correctly rounded division and square root).  The steps named "wireframe n" are
 * the steps of mnv_render_wireframe above, word for word.
 *   A. vertices: world position w_c = ((M[c][0]*x + M[c][1]*y) + M[c][2]*z) + M[c][3] (c = 0..2, M the model matrix; no sin / cos on the
 *      device); camera coordinates (X, Y, Z) of w by wireframe 1 (Z is its z).  Vertex normal n = t / sqrt((t0*t0 + t1*t1) + t2*t2) with
 *      t_c = (M[c][0]*a0 + M[c][1]*a1) + M[c][2]*a2 of the normal attribute a (the vertex shader's normalize(mat3(M) * aNormal)).
 *      Primitive k of a mesh takes vertices faces[k*face_size + i], or k*face_size + i when non-indexed.
 *   B. lines (face_size 2): wireframe 2-5 on the two camera-space endpoints.  Fragment weights wa = qa/s, wb = qb/s.
 *   C. points (face_size 1): dropped if Z < 1e-3f; px, py by wireframe 3; one fragment in pixel (floor(px), floor(py)) if that lies in the
 *      tile (not finite: nothing); its (X, Y, Z) are the vertex's, weight w0 = 1.
 *   D. triangles (face_size 3), no polygon clipping, no face culling (Mesh::draw enables none): dropped if all three Z < 1e-3f.
 *      Edge normals: for the vertex pairs (V1,V2), (V2,V0), (V0,V1) in this order, n = A x B = (Ay*Bz - Az*By, Az*Bx - Ax*Bz, Ax*By - Ay*Bx)
 *      of the camera-space vectors, computed with the pair in canonical order -- the vertex with the smaller X first, then the smaller Y,
 *      then the smaller Z -- and negated when the triangle names the pair the other way round: two triangles sharing an edge see exactly
 *      opposite normals.
 *      Pixels evaluated: if any Z < 1e-3f or any px, py (wireframe 3 per vertex) is not finite, every pixel of the tile; else columns
 *      floor(min px) - 1 .. floor(max px) + 1 and rows floor(min py) - 1 .. floor(max py) + 1, cut by the tile.
 *      At pixel (x, y): xc = x + 0.5f, yc = y + 0.5f; u = (xc - cx)/fx, v = (cy - yc)/fy (the ray through the centre is (u, v, 1));
 *      e_i = (n_i.x*u + n_i.y*v) + n_i.z for the three edges; s = (e0 + e1) + e2.  Covered iff (e0 >= 0, e1 >= 0, e2 >= 0, s > 0) or
 *      (e0 <= 0, e1 <= 0, e2 <= 0, s < 0): a centre exactly on an edge belongs to both triangles.  Perspective-correct barycentrics
 *      w_i = e_i / s; X = (w0*X0 + w1*X1) + w2*X2, Y and Z alike; the fragment is discarded unless Z >= 1e-3f (a vertex behind the camera
 *      needs nothing else: the part of the plane behind the eye gets Z < 0).
 *   E. depth: dist = sqrt((X*X + Y*Y) + Z*Z) (the shader's Depth = length(FragPos.xyz)); key = bits(Z) << 32 | bits(dist) (wireframe 5);
 *      the smallest key of a pixel wins; among fragments with that key the lowest draw ordinal (visible meshes in list order, then
 *      primitives in order) supplies the colour -- GL_LESS keeps the first-drawn fragment.
 *   F. colour of the winning fragment: attribute = w0*a0, + w1*a1, + w2*a2 in vertex order (as many terms as the primitive has vertices),
 *      for the colour and, lit, for the normal n of step A (not renormalised, as the shader).  Unlit: rgb = colour.  Lit, the fragment
 *      shader of src/mesh.cpp:50-72 term for term:
 *        L1 = (0.4402254521846771f, 0.17609018087387085f, 0.8804509043693542f)       (normalize(0.5, 0.2, 1))
 *        L2 = (-0.40824830532073975f, -0.8164966106414795f, -0.40824830532073975f)   (normalize(-0.5, -1, -0.5))
 *        dot(a, b) = (a0*b0 + a1*b1) + a2*b2;  max0(t) = t > 0 ? t : 0
 *        diffuse = 0.7f * max0(dot(L1, n)); diffuse2 = 0.2f * max0(dot(L2, n))
 *        view = (C0 - X, C1 - Y, C2 + Z) with C the camera centre in WORLD space and (X, Y, -Z) the shader's FragPos in CAMERA space: the
 *        reference subtracts the two as they are, and so does this; len = sqrt((view0*view0 + view1*view1) + view2*view2), vd_c = view_c / len
 *        I = -L1; dn = dot(n, I); r_c = I_c - (2*dn)*n_c                               (reflect(-L1, n))
 *        sp = max0(dot(vd, r)), squared five times (pow(., 32)); specular = 0.6f * sp
 *        k = ((0.3f + diffuse) + diffuse2) + specular; rgb = k * colour
 *      rgba8 = (floor(clamp(c, 0, 1)*255 + 0.5) per channel, 255) (wireframe 6's rule); tmax = dist.
 *   G. outputs: under == NULL: a pixel without a fragment gets tmax = 1e9f and the background of wireframe 6.  under != NULL: the winning
 *      fragment replaces the pixel iff dist < under's tmax there; otherwise both values of `under` are copied through.  So tmax is the
 *      minimum of the two passes, which is what the march needs.
 * Deliberate deviations from the GL pass: the principal point is the camera's cx, cy (the reference's K ignores them); a triangle is
 * sampled by the ray through the pixel centre in camera space (2-D homogeneous rasterisation) and lines and points by the rules above, not
 * by a particular GL driver's; depth is tested on (Z, dist) with first-drawn-wins ties instead of window z with GL_LESS; between passes
 * the test is on dist.  No pixel parity with a GL driver is claimed.
 * MNV_E_UNSUPPORTED: 2^32 - 1 or more primitives in one call.
 */
int mnv_render_meshes(const mnv_mesh *const *meshes, int32_t n_meshes, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                      const mnv_frame_inputs *under, float *tmax_px_out, uint8_t *rgba8_out, void *hip_stream);

/* ------------------------------------------------ geometry out of a tree: point queries, an iso-surface of the density, an OBJ writer
 * mnv_accel_sample_points: "what is the tree at this point" for n world-space points (device float [n][3]).  Each output is a device array
 * of n elements and may be NULL: voxel = chunk * 8 + child of the leaf, depth = its depth (the root chunk's voxels have depth 1), sigma =
 * its binary16 density as binary32.  The leaf is the one query_single_from_root (rt_core.cuh:125-150) reaches, in binary32 without
 * contraction: u_a = offset[a] + p_a * scale[a], clamped to [0, 1 - 1e-6f] (max(min(u, 1 - 1e-6f), 0)); per level u_a *= 2, the child bit is
 * floorf(u_a) (x most significant), u_a -= the bit.  A point with a non-finite coordinate gives voxel = -1, depth = 0, sigma = 0.
 * Asynchronous on hip_stream.  The descent is bounded by the accel's depth (at most 23 levels) and a child link outside [1, capacity) is not
 * followed: such points answer voxel = -1, depth = 0, sigma = 0 too, and mnv_extract_surface reports MNV_E_INVALID for such a tree.
 * MNV_E_INVALID: null accel or points with n > 0, negative n. */
int mnv_accel_sample_points(const mnv_accel *accel, const float *points, int64_t n, int32_t *voxel_out, int32_t *depth_out, float *sigma_out,
                            void *hip_stream);

/*
 * mnv_extract_surface: the iso-surface of the density as an indexed triangle mesh with a normal and a colour per vertex ("surface nets":
 * one vertex per sign-changing dual cell, no case table), built on the device in a canonical order: the same accel, level, iso and
 * colour switch give the same bytes whatever the hardware schedule.  Waits for hip_stream (it sizes the outputs).
 *
 * Contract (binary32, operations in the stated order, no contraction, correctly rounded division and square root), n = 2^level:
 *   Samples.  S(i, j, k), 0 <= i, j, k < n, is the sigma of the leaf the descent of mnv_accel_sample_points reaches from the TREE-space point
 *     ((i + 0.5) / n, (j + 0.5) / n, (k + 0.5) / n) (exact in binary32; in a tree deeper than `level` the point is a corner of finer voxels
 *     and the descent's floor rule picks the one with the larger coordinates).  Sigma bits that are not finite read as 0.  A sample is
 *     inside when S > iso.
 *   Cells.  Dual cell c = (cx, cy, cz) exists for 0 <= c_a <= n - 2 and spans the samples c + (dx, dy, dz); corner index 4 dx + 2 dy + dz.  A
 *     cell is active when its eight corners are neither all inside nor all outside.  Nothing is capped at the tree's boundary: the surface
 *     is open where the density reaches the outermost sample layer.
 *   Vertex position.  One vertex per active cell.  The 12 cell edges in the order axis a = 0, 1, 2; within an axis ascending lower corner
 *     k0; upper corner k1 = k0 with the bit of axis a set (axis 0: bit 4, axis 1: bit 2, axis 2: bit 1).  Every edge whose ends differ in
 *     side crosses at t = (iso - S[k0]) / (S[k1] - S[k0]): the point is corner k0's offset (dx, dy, dz) with component a replaced by t.
 *     local = (the sum of the crossing points in that order, per component, starting from 0) / (their count as a float);
 *     u_a = (((float)c_a + local_a) + 0.5f) * 2^-level; world position (u_a - offset[a]) / scale[a].
 *   Normal.  g_a = (((S[k] summed over the four corners with the bit of axis a set, ascending k, left to right)) - (the same over the four
 *     with it clear); w_a = -(g_a * scale[a]); len = sqrtf((w0*w0 + w1*w1) + w2*w2); normal = w / len, or (0, 0, 1) when len is 0 or not finite.
 *   Colour (MNV_EXTRACT_COLOUR; otherwise (1, 1, 1)).  The leaf of the corner with the largest S (the first in corner order on ties) seen
 *     along d = -normal, as the march colours a sample: SH rows 1.f / (1.f + expf(-tmp)) per channel with tmp over the whole basis of d
 *     (rt_core.cuh:12-68, :257-281; the exact expf of the frames); RGBA rows the three halfs as floats (rt_core.cuh:285-289).  rot_dirs and
 *     basis_minmax do not enter.  Row formats other than RGBA and SH 1 / 4 / 9 / 16 / 25: MNV_E_UNSUPPORTED.
 *   Order.  Cells are ordered by brick, then inside the brick: a brick is 8 x 8 x 8 cells, nb = n / 8 bricks per axis, brick index
 *     (bx * nb + by) * nb + bz, index inside ((cx & 7) * 8 + (cy & 7)) * 8 + (cz & 7).  A vertex's id is the rank of its cell among the
 *     active cells in that order.
 *   Faces.  For a cell p and an axis a with (b, c) the next two axes cyclically: if p_b >= 1, p_c >= 1 and the sides of the samples p and
 *     p + e_a differ, a quad over the cells q0 = p - e_b - e_c, q1 = p - e_c, q2 = p, q3 = p - e_b (all active by construction), in the order
 *     q0 q1 q2 q3 when sample p is inside and q0 q3 q2 q1 otherwise (the face normal points from inside to outside), written as the
 *     triangles (0, 1, 2) and (0, 2, 3).  Faces are ordered by owner cell p in the order above, then by axis.
 * Vertices are 9 floats (position, colour, normal: the mnv_mesh layout), indices uint32, three per triangle.
 *
 * MNV_EXTRACT_ALL_BRICKS (diagnostic) visits every brick instead of the ones an empty-space test over the top of the tree keeps; the bytes
 * are identical.  Device memory beside the outputs is proportional to the number of bricks (100 bytes each: 210 MB at level 10).
 * MNV_E_INVALID: null argument, level outside 3 .. 10, a NaN iso, unknown flag bits, a tree with a child link outside [1, capacity).
 * MNV_E_UNSUPPORTED: more than 2^31 - 1 vertices or indices. */
#define MNV_EXTRACT_COLOUR 1
#define MNV_EXTRACT_ALL_BRICKS 2
typedef struct mnv_extract_params {
    int32_t level; /* 3 .. 10: the sample lattice has 2^level points per axis */
    float iso;
    int32_t flags; /* MNV_EXTRACT_* */
} mnv_extract_params;
typedef struct mnv_surface mnv_surface;
/* what the last extraction did: bricks of the lattice, bricks the passes visited, device milliseconds per pass (HIP events on the stream) */
typedef struct mnv_surface_stats {
    int64_t bricks, candidate_bricks;
    float ms_candidates, ms_count, ms_scan, ms_emit, ms_colour, ms_total;
} mnv_surface_stats;
int mnv_extract_surface(const mnv_accel *accel, const mnv_extract_params *params, void *hip_stream, mnv_surface **out);
void mnv_surface_destroy(mnv_surface *s);
int mnv_surface_counts(const mnv_surface *s, int64_t *n_verts, int64_t *n_indices);
int mnv_surface_stats_get(const mnv_surface *s, mnv_surface_stats *out);
/* host copies: vert float [n_verts][9], faces uint32 [n_indices]; either may be NULL; a capacity (in floats / indices) below the size is
 * MNV_E_INVALID */
int mnv_surface_download(const mnv_surface *s, float *vert, int64_t cap_floats, uint32_t *faces, int64_t cap_indices);
/* the device arrays themselves (owned by the surface; NULL when it is empty) */
int mnv_surface_device(const mnv_surface *s, const float **vert, const uint32_t **faces);
/* a device-to-device copy as a triangle mesh that mnv_render_meshes and mnv_renderer_add_mesh draw; an empty surface is MNV_E_INVALID */
int mnv_surface_to_mesh(const mnv_surface *s, int unlit, mnv_mesh **out);
/* Writes a Wavefront OBJ file on the host: `v x y z r g b` and `vn x y z` per vertex, then `f a//a b//b c//c` (face_size 3), `l a b`
 * (face_size 2) per primitive; floats as %.9g, so that mnv_obj_read returns the same bits (it forms vertices in order of first use by a
 * face: a vertex no face names is not read back).  faces NULL with n_indices 0 writes the vertices alone.  MNV_E_INVALID: null path or
 * vertices with n_verts > 0, a face_size other than 2 or 3, an index count that is no multiple of it, an index >= n_verts; MNV_E_IO: the file
 * cannot be written. */
int mnv_obj_write(const char *path, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size);

/* ------------------------------------------------ levels of detail: mip the tree's rows, cut the tree at a depth
 * A tree stores a row for every interior voxel, but those rows hold whatever the voxel had before it was split (zeros in a baked PlenOctree
 * file): cutting the child links at a depth shows stale colours.  mnv_tree_mip_rows derives every interior row from the voxel's children,
 * bottom-up; mnv_tree_truncate then cuts the tree at a depth and compacts what is left into an ordinary tree that every march renders.
 * Depths as mnv_accel_sample_points has them: the root chunk's voxels have depth 1, chunk c + child[c][j] has depth(c) + 1.  N == 2, any
 * data_dim from 2 to 1024, either row format (the rule never looks at the basis); `parent` is not read.
 *
 * mnv_tree_mip_rows.  data_out: device [capacity][8][data_dim], 16-byte aligned, must not overlap tree->data (the input tree is never
 * modified).  chunk_depth_out: device int32 [capacity] or NULL; 0 = the chunk was not reached from the root.  chunks_at_depth: HOST int64
 * [24], entry d = chunks of depth d (entry 0 unused, 0).  Waits for hip_stream (it hands the counts back).
 *
 * Contract (binary32, operations in the stated order, no contraction, correctly rounded division).  h(bits) is the binary16 value as
 * binary32, bits that are not finite (infinities, NaNs) read as +0.  half() rounds a binary32 to binary16, to nearest even, once; subnormal
 * binary16 results are kept, a result of 65520 or more becomes infinity.
 *   The row of a leaf voxel (child == 0) and every row of a chunk that was not reached are copied bit for bit.
 *   The row of an interior voxel whose child chunk is k comes from the eight (already mipped) rows r_0 .. r_7 of chunk k; sigma is column
 *   data_dim - 1:
 *     w_i = h(sigma_i) > 0 ? h(sigma_i) : 0;   W = ((((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5) + w_6) + w_7.
 *     W == 0: every half of the row is 0x0000.
 *     Otherwise sigma' = half(W * 0.125f), and for every other column c: t_i = w_i * h(r_i[c]) (all eight terms, also those with w_i == 0),
 *     S = ((((((t_0 + t_1) + t_2) + t_3) + t_4) + t_5) + t_6) + t_7, the result is half(S / W).
 *   No value above is a binary32 subnormal or overflows (the inputs are binary16 values): the device's binary32 denormal mode does not
 *   enter, and no atomic operation decides an output byte.
 * MNV_E_INVALID: a null argument, a child link outside [1, capacity), a chunk reached twice, overlapping or misaligned arrays, host arrays in
 * the view.  MNV_E_UNSUPPORTED: N != 2, more than 23 levels, data_dim above 1024.
 *
 * mnv_tree_truncate.  Asynchronous on hip_stream.  tree->data holds the rows to carry (normally the mipped ones), chunk_depth is
 * mnv_tree_mip_rows' array.  The survivors are the chunks with 1 <= chunk_depth <= max_depth, kept in ascending chunk order: a survivor's
 * new index is its rank among the survivors.  new_capacity must be the number of survivors (the sum of chunks_at_depth[1 .. max_depth]);
 * nothing is written at or beyond it.  Outputs (device): child_out int32 [new_capacity][8]: rank(c + child[c][j]) - rank(c) where the voxel
 * has a child and chunk_depth[c] < max_depth, 0 otherwise; data_out [new_capacity][8][data_dim] (16-byte aligned): the survivors' rows;
 * parent_out int32 [new_capacity] or NULL: rank(parent chunk) * 8 + j of the voxel above, -1 for the root, derived from `child` (the view's
 * parent array is not read); sample_counts_out int16 [new_capacity][8] or NULL (skipped when the view has no counts): the survivors' counts.
 * A max_depth at or beyond the tree's depth gives the same topology (without the chunks that were not reached).
 * MNV_E_INVALID: a null argument, max_depth < 1, new_capacity outside [1, capacity], misaligned rows.  MNV_E_UNSUPPORTED as above. */
int mnv_tree_mip_rows(const mnv_tree_view *device_tree, uint16_t *data_out, int32_t *chunk_depth_out, int64_t chunks_at_depth[24], void *hip_stream);
int mnv_tree_truncate(const mnv_tree_view *device_tree, const int32_t *chunk_depth, int32_t max_depth, int32_t new_capacity, int32_t *child_out,
                      uint16_t *data_out, int32_t *parent_out, int16_t *sample_counts_out, void *hip_stream);

/* View-dependent levels of detail: one depth for the whole tree coarsens the voxels in front of the camera as much as those a kilometre
 * away.  mnv_tree_select_cut decides per interior voxel whether its children are worth keeping for a LIST of viewpoints -- full depth where
 * a voxel covers many pixels, coarse where several voxels share one -- and mnv_tree_cut compacts the tree along that set (rows: normally
 * mnv_tree_mip_rows').  No look direction enters: the cut serves every direction from the listed eyes.  N == 2, depths as above.
 *
 * mnv_tree_select_cut.  views: HOST array of n_views viewpoints (world-space eye, focal length in pixels).  keep_out: device uint8
 * [capacity], 1 = the chunk is kept, 0 = it is not (chunks that were not reached included).  kept_at_depth: HOST int64 [24], entry d = kept
 * chunks of depth d (entry 0 unused, 0).  Waits for hip_stream (it hands the counts back).  tree->data is not read.
 *
 * Contract (binary32, one operation at a time in the stated order, no contraction, correctly rounded division, subnormals kept).
 *   Host, once per view v:  q_k = offset[k] + scale[k] * eye[k] (the product, then the sum): the eye in tree space.  For d = 0 .. 23:
 *     e_d = max_k(2^-d / scale[k]),  r = (focal_px * e_d) / pixels,  R2[v][d] = r * r; overflow to +inf is fine and means "always refine";
 *     pixels == 0 makes every R2 +inf.
 *   The root chunk is kept.  For a kept chunk c of depth d and a voxel j of it with child[c][j] != 0 (j = 4 x + 2 y + z): the chunk
 *   c + child[c][j] is kept iff d < max_depth and (d < min_depth or D2 <= R2[v][d] for some view v), where, with (i_x, i_y, i_z) the
 *   voxel's integer corner at depth d (twice the corner of the voxel above c, plus (x, y, z); the root's is 0):
 *     lo_k = i_k * 2^-d,  hi_k = (i_k + 1) * 2^-d  (both exact),
 *     g_k = max(max(lo_k - q_k, q_k - hi_k), 0),  w_k = g_k / scale[k],  D2 = (w_x * w_x + w_y * w_y) + w_z * w_z.
 *   An eye inside the voxel has D2 == 0 and always refines.  A chunk under a chunk that is not kept is never reached, so the set is
 *   parent-closed by construction.  In words: a voxel's children are kept when, from some listed eye, the voxel could cover `pixels`
 *   pixels or more.  The walk visits kept chunks only; the order in which it does depends on the schedule and decides no output byte (every
 *   byte of keep_out is the constant the rule gives, the counts are list sizes): no atomic operation decides an output byte.
 * MNV_E_INVALID: a null argument; n_views outside [1, 4096]; an eye or focal_px that is not finite, focal_px <= 0, a q that is not finite;
 * pixels negative or not finite; a scale[k] that is not finite and positive, an offset that is not finite; min_depth < 1 or
 * max_depth < min_depth; among the links the walk FOLLOWS (those of voxels that refine): one outside [1, capacity), a chunk reached twice;
 * host arrays in the view.  MNV_E_UNSUPPORTED: N != 2, kept chunks beyond 23 levels, data_dim above 1024.
 *
 * mnv_tree_cut is mnv_tree_truncate with the survivor predicate keep[c] != 0 (keep: device uint8 [capacity]) in place of the depth test: the
 * survivors stay in ascending chunk order, a survivor's new index is its rank among them (an exclusive scan).  new_capacity must be the
 * number of survivors (the sum of kept_at_depth); nothing is written at or beyond it.  child_out [new_capacity][8]: rank(c + child[c][j]) -
 * rank(c) where the voxel has a child inside the tree that is kept, 0 otherwise; data_out (16-byte aligned), parent_out or NULL,
 * sample_counts_out or NULL as mnv_tree_truncate has them.  THE CALLER guarantees that keep is parent-closed (mnv_tree_select_cut's is): a
 * kept chunk under a parent that is not kept is compacted like the others but never linked, and its parent entry stays -1.  With keep =
 * (1 <= chunk_depth <= D) the outputs are mnv_tree_truncate's at D, byte for byte.  Asynchronous on hip_stream for everything it writes; it
 * reads keep[0] first, which waits for the work queued on hip_stream before the call.
 * MNV_E_INVALID: a null argument, keep[0] == 0, new_capacity outside [1, capacity], misaligned rows, host arrays.  MNV_E_UNSUPPORTED as above. */
typedef struct mnv_lod_view {
    float eye[3];   /* world space */
    float focal_px; /* focal length in pixels */
} mnv_lod_view;
int mnv_tree_select_cut(const mnv_tree_view *device_tree, const mnv_lod_view *views /*HOST*/, int32_t n_views, float pixels, int32_t min_depth,
                        int32_t max_depth, uint8_t *keep_out /*device [capacity]*/, int64_t kept_at_depth[24] /*HOST*/, void *hip_stream);
int mnv_tree_cut(const mnv_tree_view *device_tree, const uint8_t *keep, int32_t new_capacity, int32_t *child_out, uint16_t *data_out,
                 int32_t *parent_out, int16_t *sample_counts_out, void *hip_stream);

/* ------------------------------------------------ anti-aliased frames: jittered sub-frames in one launch, filtered resolve
 * Every march kernel sends one ray through each pixel centre.  A supersampled frame is K frames of the SAME camera whose principal point is
 * shifted by a sub-pixel offset (mnv_camera carries cx, cy per camera, and mnv_render_voxels_accel_batch marches up to MNV_MAX_BATCH cameras
 * in one launch), filtered into one frame by mnv_resolve_samples.  The reference has no counterpart: it shows point-sampled frames in a window.
 *
 * The recipe for callers that drive accel handles themselves (VolumeRenderer / mnv_renderer_set_antialiasing do the same per frame):
 *     mnv_aa_pattern(K, off);                                                  // 1. pattern
 *     for (k = 0; k < K; ++k) { cams[k] = cam; cams[k].cx = cam.cx - off[2*k]; cams[k].cy = cam.cy - off[2*k + 1]; }   // 2. shifted cameras
 *     mnv_render_voxels_accel_batch(accel, cams, K, opt, full, whole, sub, NULL, stream);   // 3. K float sub-frames, one launch
 *     mnv_aa_weights(MNV_AA_TENT, K, off, &r, w_host, cap, &n); (copy w_host to the device: w_dev)                    // 4. weights
 *     mnv_resolve_samples(sub, K, width, height, w_dev, r, rgba, rgba8, stream);            // 5. resolve
 * (sample k looks at the point (x + 0.5 + dx_k, y + 0.5 + dy_k) of pixel (x, y): px = cx + fx * X/z, so moving the principal point by
 * -d moves the image by -d under the pixel grid.)
 *
 * mnv_aa_pattern (host; no GPU needed): n_samples offsets (dx, dy), each in [-0.5, 0.5).  1 <= n_samples <= MNV_MAX_BATCH, else MNV_E_INVALID.
 * n_samples == 1 gives (0, 0).  Otherwise sample k is (H2(k + 1) - 0.5, H3(k + 1) - 0.5), Hb the radical inverse in base b (a Halton
 * sequence), computed in double exactly as
 *     f = 1; r = 0; i = k + 1; while (i > 0) { f = f / b; r = r + f * (i % b); i = i / b; }
 * then r - 0.5 rounded to float.
 */
int mnv_aa_pattern(int32_t n_samples, float *offsets_xy /* host [n_samples][2] */);
/*
 * mnv_aa_weights (host; no GPU needed): the reconstruction filter as a table weights[k][j + r][i + r] -- the weight with which sample k
 * of the pixel at window offset (i, j), i along x, both in -r .. r, enters a pixel.  Not normalised: the resolve divides by the sum it
 * accumulates.
 *   MNV_AA_BOX   r = 0, every weight 1.0f: the plain mean of a pixel's own samples
 *   MNV_AA_TENT  r = 1, max(0, 1 - |i + dx_k|) * max(0, 1 - |j + dy_k|), in double from the float offsets, rounded to float
 *                (a tent of one pixel radius centred on the pixel centre, evaluated at the sample's position)
 * Size-query convention of mnv_n3tree_gen_wireframe: *radius_out and *n_floats (= n_samples * (2r + 1)^2) are always set (either may be
 * NULL); weights NULL with cap_floats 0 asks for them alone; a buffer shorter than n_floats is MNV_E_INVALID.  Unknown filter, n_samples
 * outside 1 .. MNV_MAX_BATCH or a null offsets array: MNV_E_INVALID.
 */
#define MNV_AA_BOX 0
#define MNV_AA_TENT 1
int mnv_aa_weights(int32_t filter, int32_t n_samples, const float *offsets_xy, int32_t *radius_out, float *weights /* host */,
                   int64_t cap_floats, int64_t *n_floats);
/*
 * The resolve (a HIP kernel, asynchronous on hip_stream): n_samples sub-frames -> one frame, through a weight table of radius 0 .. 2 (the
 * tables above, or a caller's own).  sub_rgba and rgba_out are 16-byte aligned device arrays, `weights` is a DEVICE array.
 * Resolve contract (float32, this order, products and sums rounded separately -- no contraction -- and a correctly rounded division):
 *   for each pixel (x, y):  acc[0..3] = 0, wsum = 0
 *     for k = 0 .. n_samples-1, then j = -r .. r, then i = -r .. r:
 *       skip the term if (x + i, y + j) is outside the frame
 *       w = weights[k][j + r][i + r]; skip the term if w == 0
 *       acc[c] = acc[c] + w * sub[k][y + j][x + i][c]   (c = 0 .. 3)      wsum = wsum + w
 *     out[c] = wsum > 0 ? acc[c] / wsum : 0
 *   rgba_out[y][x][c] = out[c]; rgba8_out[y][x][c] = the truncating pack of the march's composite (renderer_kernel.cu:237):
 *   s = out[c] * 255; 0 unless s > 0, 255 if s >= 255, else (uint8)s.  The alpha channel is filtered and packed like the others.
 * Dividing by the accumulated wsum is what handles the frame's border (the window's terms outside the frame are missing from both sums: the
 * filter is renormalised over what exists) and tables that are not normalised.
 * MNV_E_INVALID: null sub_rgba or weights, both outputs null, n_samples outside 1 .. MNV_MAX_BATCH, radius outside 0 .. 2, non-positive
 * sizes, rgba8_out not 4-byte aligned, sub_rgba / rgba_out not 16-byte aligned.
 */
int mnv_resolve_samples(const float *sub_rgba /* device [n_samples][height][width][4] */, int32_t n_samples, int32_t width, int32_t height,
                        const float *weights /* DEVICE [n_samples][2r+1][2r+1] */, int32_t radius /* 0..2 */,
                        float *rgba_out /* device [height][width][4] or NULL */, uint8_t *rgba8_out /* or NULL */, void *hip_stream);

/* ------------------------------------------------ ray lists; orthographic and equirectangular frames
 * Every march entry point above builds its rays from a pinhole mnv_camera.  mnv_render_rays_accel marches rays the CALLER has -- the lens
 * model and pixel subset of a data set, an orthographic top-down view of a terrain (with render_depth: a height map), a 360-degree
 * panorama -- and mnv_generate_rays makes the rays of three projections.  The reference has no counterpart (svox's volume renderer takes
 * rays; the viewer does not).
 *
 * mnv_render_rays_accel: origins / dirs are DEVICE float [height][width][3] in world space; a flat list is height == 1.  Image positions
 * map to wavefronts through the ray tiles of the camera frames (8 x 8; 64 x 1 for height == 1), so neighbouring rays march together.
 * Outputs, `inputs` (tmax_px / rgba8_init, NULL or either member NULL as for mnv_render_voxels_accel_ex) are indexed like the rays.
 * Arithmetic contract, per ray, float32 in this order, no contraction (o, d: the ray's origin and direction; d need not have unit length):
 *     invnorm = 1.f / sqrtf(d0*d0 + d1*d1 + d2*d2);  dir = d * invnorm;  vdir = dir, rotated by options.rot_dirs as in every frame;
 *     cen[k] = offset[k] + scale[k] * o[k]   (the tree's offset / scale: what the frame kernels' host code computes for a camera centre);
 *     from there the set-up, march, composite and pack of mnv_render_voxels_accel_ex (with options.render_depth: of its depth image),
 *     t_max = tmax_px[ray] or 1e9f.
 * So the rays mnv_generate_rays(MNV_PROJ_PINHOLE) makes give the frame of mnv_render_voxels_accel_ex bit for bit, and a ray equals the
 * one-pixel camera (width = height = 1, cx = cy = 0.5, fx = fy = 1, c2w = [1,0,0 | 0,1,0 | -d | o]) of the oracle.
 * A DEGENERATE ray -- d0*d0 + d1*d1 + d2*d2 zero (or underflowed to zero) or not finite, or a non-finite origin component -- is a miss: its
 * pixel is what a ray that misses the bounding box gets (the background or the pixel of rgba8_init, alpha 0).
 * Every row format of the frame kernels (RGBA, SH1/4/9/16/25; anything else: MNV_E_UNSUPPORTED), on inline cell words / brick records where
 * a camera frame would be.  The ray march ALWAYS uses the exact colour math (mnv_accel_set_colour_math does not reach it), and ray lists are
 * not offered for trackers, visit marks, sample emission, partitions or batches.
 * MNV_E_INVALID, before any device call: null origins / dirs / opt / accel, both outputs null, width or height < 1, width * height > 2^28.
 */
int mnv_render_rays_accel(const mnv_accel *accel, const float *origins, const float *dirs /* device [height][width][3] */, int32_t width,
                          int32_t height, const mnv_render_options *opt,
                          const mnv_frame_inputs *inputs /* NULL, or tmax_px / rgba8_init indexed like the rays */, float *rgba_out,
                          uint8_t *rgba8_out, void *hip_stream);
/*
 * mnv_generate_rays (a HIP kernel, asynchronous on hip_stream): the rays of the rectangle `tile` (inside cam's image) into
 * origins_out / dirs_out, DEVICE float [tile.h][tile.w][3] (4-byte aligned; 16-byte aligned outputs are written with 16-byte stores).
 * With m = cam->c2w, pixel (ix, iy), u = (ix + 0.5f - cx) / fx, v = -(iy + 0.5f - cy) / fy; float32, every sum left to right, no contraction:
 *   MNV_PROJ_PINHOLE   origin = m[9..11];  dir[k] = m[k]*u + m[3+k]*v + m[6+k]*(-1.f), not normalised -- the vector the frame kernels
 *                      normalise (renderer_kernel.cu:30-38)
 *   MNV_PROJ_ORTHO     fx, fy are pixels per world unit;  origin[k] = (m[9+k] + m[k]*u) + m[3+k]*v;  dir[k] = m[6+k]*(-1.f).  Rays start ON
 *                      the camera plane: put it outside the volume
 *   MNV_PROJ_EQUIRECT  longitude [-pi, pi) left to right, latitude pi/2 .. -pi/2 top to bottom; fx, fy, cx, cy are ignored.  No sine or
 *                      cosine runs on the device: with (sl, cl) the table's entry of row iy and (so, co) of column ix,
 *                      dx = cl*so, dy = sl, dz = -(cl*co);  dir[k] = m[k]*dx + m[3+k]*dy + m[6+k]*dz;  origin = m[9..11]
 * equirect_tables: DEVICE copy of what mnv_equirect_tables(cam->width, cam->height, .) wrote (8-byte aligned); NULL unless EQUIRECT.
 * mnv_equirect_tables (host; no GPU needed): out[(width + height)][2] = (float)sin, (float)cos -- computed in double -- of
 * lon = ((x + 0.5) / width - 0.5) * 2 pi for column x = 0 .. width-1, then of lat = (0.5 - (y + 0.5) / height) * pi for row y.
 * MNV_E_INVALID, before any device call: an unknown projection, null camera / outputs / table (EQUIRECT), a rectangle with w or h < 1,
 * outside the image or of more than 2^28 pixels, misaligned arrays; mnv_equirect_tables: width or height < 1, null table.
 */
#define MNV_PROJ_PINHOLE 0
#define MNV_PROJ_ORTHO 1
#define MNV_PROJ_EQUIRECT 2
int mnv_generate_rays(int32_t projection, const mnv_camera *cam, mnv_rect tile, const float *equirect_tables /* device; NULL unless EQUIRECT */,
                      float *origins_out, float *dirs_out, void *hip_stream);
int mnv_equirect_tables(int32_t width, int32_t height, float *out /* host [(width + height)][2] */);

/* ------------------------------------------------ frame metrics: squared error (PSNR) and SSIM against a target image, on the device
 * What a user of a batch renderer does with a frame is score it -- against a photograph of the data set, the frame of the unrefined tree,
 * the frame of another build.  mnv_frame_metrics compares a float frame (what every launcher writes) with an RGBA8 target on the device and
 * leaves 40 bytes of integer sums; the frame itself never crosses the bus.  The reference has no counterpart.
 *
 * Metric contract (float32, this order, products and sums rounded separately -- no contraction -- and a correctly rounded division):
 *   per pixel and channel c = 0 .. 2, v = rgba[y][x][c]:
 *     t = (float)target8[y][x][c] / 255.f
 *     x = v > 0 ? (v < 1 ? v : 1) : 0                              (a NaN becomes 0)
 *     MNV_METRIC_QUANTISED: x = (float)pack(v) / 255.f, pack the truncating pack stated at mnv_resolve_samples (s = v * 255; 0 unless
 *       s > 0, 255 if s >= 255, else (uint8)s) -- the file `mnv_render --out` writes against the file that was read
 *   a pixel is INCLUDED unless MNV_METRIC_MASK_ALPHA is set and target8[y][x][3] == 0
 *   squared error:  e_c = x_c - t_c;  se = (e0*e0 + e1*e1) + e2*e2
 *   SSIM (MNV_METRIC_SSIM; Wang et al.: 11 x 11 Gaussian window, valid windows only, data range 1), per channel, for every window origin
 *   (x', y') with x' <= width - 11 and y' <= height - 11.  Each of the five maps v = x, t, x*x, t*t, x*t is filtered the same way,
 *     along x:  h = 0;  for i = 0 .. 10:  h = h + g[i] * v[y][x' + i]
 *     along y:  m = 0;  for j = 0 .. 10:  m = m + g[j] * h[y' + j][x']
 *   giving mx, my, exx, eyy, exy; then
 *     mxx = mx*mx;  myy = my*my;  mxy = mx*my;  sxx = exx - mxx;  syy = eyy - myy;  sxy = exy - mxy
 *     num = (2.f*mxy + C1) * (2.f*sxy + C2);  den = ((mxx + myy) + C1) * ((sxx + syy) + C2);  s = num / den      C1 = 1e-4f, C2 = 9e-4f
 *   a window is included iff all of its 121 pixels are included (counted with integers).
 *   `window`: HOST float [11], copied into the kernel's arguments; NULL = the standard window of mnv_ssim_window.
 * Sums (mnv_metric_sums, five int64 in DEVICE memory, zeroed by the call on its stream before the kernel):
 *     n_px      included pixels                      se_q32    sum over included pixels of llrint((double)se * 2^32)
 *     n_win     included windows                     ssim_q32  sum over included windows and the 3 channels of llrint((double)s * 2^32)
 *   Every term is rounded once, to nearest even, at 2^-32; from there on every addition is an integer addition, so the words do not depend
 *   on tile shape, lane mapping, reduction tree or atomic order, and a numpy restatement reproduces them exactly (tests/metrics_ref.py).
 *   Headroom: 3 * 2^32 * 2^28 < 2^62, so width * height > 2^28 is refused.
 * Optional maps (either NULL): se_map_out float [height][width], 0 where the pixel is excluded; ssim_map_out float
 * [height - 10][width - 10][3], 0 where the window is excluded.
 * MNV_METRIC_SSIM on a frame narrower or lower than 11 is no error: n_win = 0 (and ssim_map_out is not touched).
 * MNV_E_INVALID, before any device call: null rgba / target8 / sums, non-positive sizes, width * height > 2^28, rgba not 16-byte aligned,
 * target8 or a map not 4-byte aligned, sums not 8-byte aligned, unknown flag bits.
 *
 * mnv_ssim_window (host; no GPU needed): out[i] = exp(-(i - 5)^2 / 4.5) in double (sigma = 1.5), divided by the sum of the eleven taken
 * in index order, rounded to float.
 * mnv_metrics_finish (host, double): from a HOST copy of the sums, mse = se_q32 / 2^32 / (3 n_px); psnr = -10 log10(mse) (+inf for
 * mse 0, NaN for n_px 0); ssim = ssim_q32 / 2^32 / (3 n_win) (NaN for n_win 0); and the two counts.
 */
#define MNV_METRIC_QUANTISED 1
#define MNV_METRIC_MASK_ALPHA 2
#define MNV_METRIC_SSIM 4
typedef struct mnv_metric_sums {
    int64_t n_px, se_q32, n_win, ssim_q32, reserved;
} mnv_metric_sums;
typedef struct mnv_frame_metric_values {
    double mse, psnr, ssim;
    int64_t n_px, n_win;
} mnv_frame_metric_values;
int mnv_frame_metrics(const float *rgba /* device [height][width][4] */, const uint8_t *target8 /* device [height][width][4] */, int32_t width,
                      int32_t height, int32_t flags, const float *window /* HOST [11] or NULL */, mnv_metric_sums *sums /* DEVICE */,
                      float *se_map_out /* device or NULL */, float *ssim_map_out /* device or NULL */, void *hip_stream);
int mnv_ssim_window(float *out /* host [11] */);
int mnv_metrics_finish(const mnv_metric_sums *host_copy, mnv_frame_metric_values *out);
/* Binary PNM files on the host (no GPU needed): P6 (3 channels, what `mnv_render --out` writes) and P5 (1 channel), maxval 255, `#`
 * comments in the header.  Size-query convention of mnv_obj_read: *width, *height and *channels are always set once the header is read
 * (any may be NULL); data NULL with cap_bytes 0 asks for them alone; a buffer shorter than width * height * channels is MNV_E_INVALID.
 * expect_width / expect_height > 0: a file of another size is refused.  MNV_E_IO (mnv_last_error says what): a file that cannot be
 * read, another magic, a malformed or truncated header, a maxval other than 255, an unexpected size, fewer data bytes than the header
 * promises. */
int mnv_pnm_read(const char *path, int32_t expect_width, int32_t expect_height, uint8_t *data /* host */, int64_t cap_bytes, int32_t *width,
                 int32_t *height, int32_t *channels);

/* ------------------------------------------------ fitting a tree's rows to target rays: the march's gradient and a row update, on the device
 * The frame metrics above measure the gap between a tree's frames and target images; these three entry points close it.  The octree family
 * (PlenOctrees, svox) is differentiable in its row data: mnv_rays_grad marches a ray list and accumulates d(loss)/d(row) for every leaf row the
 * rays sample, mnv_rows_sgd_step applies one gradient step to a float32 master copy of the rows and writes the binary16 rows back.  The tree's
 * structure (child) never changes.  The reference has no counterpart.
 *
 * mnv_rays_grad works on the tree VIEW's own device arrays (child, binary16 data): the rows change between iterations, so it takes no accel.
 *   origins / dirs   device float [height][width][3], world space, as mnv_render_rays_accel takes them (a flat list is height == 1; 8 x 8 ray
 *                    tiles per wavefront, 64 x 1 for height == 1)
 *   target           device float [height][width][4]: the ray's target colour; alpha == 0 EXCLUDES the ray (weight 0), any other alpha
 *                    (NaN too) includes it (weight 1)
 *   tmax             device float [height][width] or NULL (1e9f), the ray limit as in mnv_frame_inputs
 *   rgba_out         device float [height][width][4] or NULL: written for every ray, excluded rays too
 *   acc              device int64 [capacity * 8][data_dim], 8-byte aligned: the kernel ADDS into it (the caller zeroes it; mnv_rows_sgd_step
 *                    clears what it consumed)
 *   sums             device mnv_fit_sums, 8-byte aligned: the kernel ADDS into it (the caller zeroes it)
 * Forward contract: mnv_render_rays_accel's, exactly.  rgba_out equals that call's float output bit for bit -- degenerate rays and misses
 * included -- for options without render_depth and without an image under the volume.
 * Names.  The ray's dense samples s = 0 .. n-1 are its march steps with sigma > sigma_thresh, in march order.  Sample s has its leaf voxel v_s
 * (chunk * 8 + child index), d_s = delta_t * delta_scale, att_s = expf(-d_s sigma) as the forward computes it, T_s the light before the sample,
 * w_s = T_s * (1.f - att_s), T_{s+1} = T_s * att_s, and the colour c_sk of channel k: for SH rows 1.f / (1.f + expf(-tmp_k)), tmp_k the
 * channel sum of the forward; for RGBA rows the row's value.  S_k are the forward's running sums BEFORE the early-stop rescale, T_end the
 * light at the end, stopped is true when T_{s+1} < stop_thresh ended the ray, scale = stopped ? 1.f / (1.f - T_end) : 1.f (the forward's own
 * factor), C_k the composited pixel (rgba_out), B_k = stopped ? C_k : background_brightness.
 * Backward contract (binary32, one operation at a time in the stated order, no contraction, then ONE rounding to fixed point):
 *   g_k = C_k - target_k                                         (the loss is 1/2 sum_k g_k^2 over the included rays)
 *   se = (g_0*g_0 + g_1*g_1) + g_2*g_2                            -> sums.se_q32
 *   gs_k = g_k * scale;   bt_k = B_k * T_end                      (once per ray)
 *   the same steps are marched again with the prefix P_k accumulated exactly as the forward accumulates S_k; at sample s, after adding it:
 *     Q_k  = S_k - P_k
 *     gc_k = gs_k * w_s
 *     RGBA rows: column k gets gc_k.
 *     SH rows:   gt_k = gc_k * (c_sk * (1.f - c_sk));  column k * basis_dim + j gets gt_k * basis_j for basis_min <= j <= basis_max -- basis_j
 *                the SH basis of the view direction after rot_dirs, as the forward multiplies it; masked coefficients get no term
 *     e_k  = (T_{s+1} * c_sk - Q_k) - bt_k
 *     column data_dim - 1 (sigma) gets (d_s * scale) * ((g_0*e_0 + g_1*e_1) + g_2*e_2)
 *   That is the derivative of the pixel with the sample set held fixed, the early-stop normalisation S_k / (1 - T_end) included (DESIGN.md
 *   5.16 derives it).  Every term x is added to acc[v_s][column] as the integer q32(x) = llrint((double)sat(x) * 2^32), sat(x) = x clamped to
 *   [-32, 32] (a NaN term: 0); se goes to sums.se_q32 the same way.  From that rounding on every addition is an integer addition, so the
 *   words do not depend on lane mapping, launch shape, ray order or atomic order, and a numpy restatement reproduces them exactly
 *   (tests/fit_ref.py).
 *   A ray with a non-finite C_k or g_k, or whose descent leaves the tree (below), contributes NOTHING and is counted in n_skipped.
 * Sums (the included rays that were not skipped): n_rays; n_stopped (early-stopped ones); n_samples (their dense samples); se_q32; and
 *   n_skipped.
 * Headroom.  One term is at most 2^5 * 2^32 = 2^37 in magnitude (terms of SH rows against targets in [0, 1] stay below 8; the clamp is the
 * guard for everything else), so a word of acc cannot wrap before it has received 2^25 terms (2^25 * 2^37 = 2^62).  A ray adds to a word
 * once per dense step it takes in that voxel (one, except where rounding keeps a step inside its leaf).  One call takes at most 2^22 rays
 * (two 1080p frames: more is MNV_E_INVALID); clear acc -- mnv_rows_sgd_step does -- before the ray total since the last clear passes 2^24.
 * se_q32: 2^24 * 2^37 < 2^62.
 * The descent is bounded and link-checked as mnv_accel_sample_points' is: at most 23 levels, a link that leaves [1, capacity) is not followed;
 * a ray that meets either is skipped.  (A tree deeper than 23 levels cannot be told from the host without a launch: its rays are skipped.)
 * MNV_E_UNSUPPORTED, before any launch: options.render_depth, N != 2, rows other than RGBA and SH 1 / 4 / 9 / 16 / 25 (what the ray march
 *   offers).  (There is no image under the volume here: the entry point takes no rgba8_init.)
 * MNV_E_INVALID, before any launch: a null tree / array / options / acc / sums, width or height < 1, width * height > 2^22, capacity < 1,
 *   a data_dim too small for the row format, acc / sums not 8-byte aligned, rgba_out / target not 16-byte aligned, and step_size not finite
 *   or <= 0 -- a march that cannot advance never reaches the device.
 *
 * mnv_rows_master_init: master[i] = (float)data[i] for n binary16 values, exact; non-finite bit patterns (inf, NaN) read as +0.
 * mnv_rows_sgd_step (elementwise): for every row r < n_rows with a non-zero word in acc[r][0 .. data_dim), per column c:
 *     g = (float)((double)acc[r][c] * 2^-32);  lr = c == data_dim - 1 ? lr_sigma : lr_colour;  m = master[r][c] - lr * g  (the product is
 *     rounded before the difference);  the sigma column: m = m < 0 ? 0 : m;  master[r][c] = m;
 *     data[r][c] = binary16(m), round to nearest even, saturating at +-65504 (no infinity is written; a NaN m writes +0)
 *   and acc[r][.] is cleared.  Rows whose words are all zero keep master and bytes untouched.
 *   MNV_E_INVALID: null arrays, n_rows < 0, data_dim < 1, a learning rate that is not finite.
 */
typedef struct mnv_fit_sums {
    int64_t n_rays, n_stopped, n_samples, n_skipped, se_q32, reserved[3];
} mnv_fit_sums;
int mnv_rays_grad(const mnv_tree_view *device_tree, const float *origins, const float *dirs /* device [height][width][3] */,
                  const float *target /* device [height][width][4] */, const float *tmax /* device [height][width] or NULL */, int32_t width,
                  int32_t height, const mnv_render_options *opt, float *rgba_out /* device or NULL */, int64_t *acc /* device */,
                  mnv_fit_sums *sums /* device */, void *hip_stream);
int mnv_rows_master_init(const uint16_t *data /* device [n] */, int64_t n, float *master_out /* device [n] */, void *hip_stream);
int mnv_rows_sgd_step(uint16_t *data, float *master, int64_t *acc /* device [n_rows][data_dim] each */, int64_t n_rows, int32_t data_dim,
                      float lr_colour, float lr_sigma, void *hip_stream);

/* ------------------------------------------------ fitting on a photo set: a normalised row step and ray mini-batches, on the device
 * mnv_rows_sgd_step takes one rate for every row, while a row's gradient grows with the rays through it; mnv_n3tree_fit is full batch and
 * stops at 2^24 pixels.  These entry points lift both limits: mnv_rows_adam_step is the row update with Adam's step (Kingma & Ba 2015), which
 * does not depend on the gradient's scale, and mnv_ray_batcher_* draws batches of rays and targets across a whole set of cameras and images,
 * so that mnv_rays_grad + one row step run per batch and the accumulators are cleared every step.
 *
 * mnv_rows_adam_step (elementwise; m1 / m2: the float32 first and second moments, zero before the first step).  The host computes
 *     omb1 = 1.f - beta1;  omb2 = 1.f - beta2                                   (binary32)
 *     c1 = (float)(1 / (1 - (double)beta1^step));  c2 likewise with beta2       (binary64 pow, rounded once)
 *   and for every row r < n_rows with a non-zero word in acc[r][0 .. data_dim) -- mnv_rows_sgd_step's rule -- per column c, in binary32, one
 *   operation at a time in this order, no contraction, division and square root correctly rounded:
 *     g   = (float)((double)acc[r][c] * 2^-32)
 *     a   = (m1 * beta1) + (g * omb1);           v = (m2 * beta2) + ((g * g) * omb2)
 *     den = sqrtf(v * c2) + eps;                 upd = (lr * (a * c1)) / den          lr = c == data_dim - 1 ? lr_sigma : lr_colour
 *     m   = master - upd;   the sigma column: m = m < 0 ? 0 : m
 *     m1 = a;  m2 = v;  master = m;  data = binary16(m) exactly as mnv_rows_sgd_step writes it (a NaN m writes +0);  acc[r][.] = 0
 *   Rows whose words are all zero keep master, moments and bytes: a lazy, sparse Adam.  Two known approximations, those of every sparse
 *   Adam: untouched rows do not decay their moments, and the bias correction uses the global step for rows first touched late.
 *   Traffic: a touched word moves 42 bytes (acc 8, master 4, m1 4, m2 4 read, the same 20 written back, 2 of data) against the SGD step's
 *   26; an untouched word reads 8 in both.  State: 22 bytes per word with Adam (2 + 4 + 4 + 4 + 8) -- about 35 GB for a tree of 1.6 G words.
 *   MNV_E_INVALID, before any launch: null arrays or parameters, n_rows < 0, data_dim < 1, step < 1, a rate that is not finite, a beta outside
 *   [0, 1), eps not finite or <= 0, misaligned arrays.
 *
 * mnv_ray_batcher_*: cameras may differ in size.  A unit is a pixel (tile 1) or an 8 x 8 pixel tile (tile 8: a camera has ceil(w/8) *
 * ceil(h/8) of them, row-major; pixels are row-major for tile 1); units are numbered camera after camera, U is their total (< 2^31).
 * create copies the cameras and a prefix table of their first units to the device; `targets` is a HOST array of n_cams DEVICE images float
 * [h][w][4] (16-byte aligned) that must outlive the handle's draws.  draw writes, for j < count, the unit perm(epoch, first + j) to rays
 * j * tile^2 .. (j + 1) * tile^2 - 1 of the outputs.  It changes nothing in the handle: any stream, any number of draws at once.
 *   The permutation is integer arithmetic only (uint32, wrapping), a 4-round Feistel network on 2k bits with cycle walking:
 *     mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     k = max(1, ceil(bitlen(U - 1) / 2));  mask = 2^k - 1;  seed_lo / seed_hi: the halves of `seed`
 *     key_r = mix32(mix32(seed_lo ^ mix32(seed_hi ^ (uint32)epoch)) + r),  r = 0 .. 3
 *     x = i;  do { L = x >> k; R = x & mask;  for r in 0 .. 3: (L, R) = (R, L ^ (mix32(R ^ key_r) & mask));  x = (L << k) | R; } while (x >= U)
 *   The Feistel map is a bijection of [0, 2^2k), so perm(epoch, .) is a bijection of [0, U), and the loop is bounded: the walk follows the
 *   orbit of i, which returns to i, and i < U -- at most 2^2k <= 4U rounds, under four on average.
 *   Rays.  Within a tile, lane l is pixel (tx * 8 + (l & 7), ty * 8 + (l >> 3)): a wavefront of mnv_rays_grad on the flat list (64 x 1 ray
 *   tiles) marches one image tile.  A pixel inside the image gets the origin and direction mnv_generate_rays(MNV_PROJ_PINHOLE) gives that
 *   pixel of that camera, bit for bit, and the 16 bytes of targets[cam][iy][ix].  A lane outside the image (edge tiles) gets the origin
 *   c2w[9 .. 11], the direction (0, 0, 0) -- a degenerate ray, a miss -- and the target (0, 0, 0, 0): alpha 0 excludes it.
 *   MNV_E_INVALID, before any launch: null arguments, n_cams outside 1 .. 4096, a tile other than 1 or 8, a camera with width or height
 *   < 1, a null or misaligned target image, U >= 2^31; draw: epoch < 0, first < 0, count < 1, first + count > U, count * tile^2 > 2^22
 *   (mnv_rays_grad's limit), origins_out / dirs_out not 4-byte aligned, target_out not 16-byte aligned.
 */
typedef struct mnv_adam_params {
    float lr_colour, lr_sigma, beta1, beta2, eps;
    int32_t reserved[3];
} mnv_adam_params;
int mnv_rows_adam_step(uint16_t *data, float *master, float *m1, float *m2, int64_t *acc /* device [n_rows][data_dim] each */, int64_t n_rows,
                       int32_t data_dim, const mnv_adam_params *p, int64_t step /* >= 1 */, void *hip_stream);
typedef struct mnv_ray_batcher mnv_ray_batcher;
int mnv_ray_batcher_create(const mnv_camera *cams /* HOST */, const float *const *targets /* HOST array of device [h][w][4] */, int32_t n_cams,
                           int32_t tile /* 1 or 8 */, uint64_t seed, mnv_ray_batcher **out);
int mnv_ray_batcher_units(const mnv_ray_batcher *b, int64_t *units, int32_t *rays_per_unit);
int mnv_ray_batcher_draw(const mnv_ray_batcher *b, int64_t epoch, int64_t first, int64_t count, float *origins_out,
                         float *dirs_out /* device [count * tile * tile][3] */, float *target_out /* device [count * tile * tile][4] */, void *hip_stream);
void mnv_ray_batcher_destroy(mnv_ray_batcher *b);

/* ------------------------------------------------ culling a tree to a pose set: the largest weight per leaf, then a bottom-up cull
 * A batch renderer knows its poses in advance.  Leaves no listed ray weights above zero -- occluded ones, those behind an early stop, the
 * inside of a thick shell -- still cost rows and accel.  The octree family's step for this (PlenOctree extraction / compression): record per
 * leaf the largest compositing weight any ray gave it, drop the leaves under a threshold, collapse the chunks that became all-empty.
 * mnv_rays_visibility is the first half, mnv_tree_cull the second; mnv_tree_cut on (child, data_out) with keep_out compacts the result.
 *
 * mnv_rays_visibility (asynchronous on hip_stream) works on the tree VIEW's own device arrays, like mnv_rays_grad; origins / dirs / tmax /
 * width / height as there.  wmax: device uint32 [capacity * 8], a word per voxel; sums: device mnv_vis_sums, 8-byte aligned.  The kernel
 * takes the MAXIMUM into wmax and ADDS into sums: calls accumulate, the caller clears both once; a word of 0 means "never weighted".
 * Contract: the rays are marched exactly as mnv_rays_grad's forward marches them, which is mnv_render_rays_accel's march: the same set-up,
 * descent, delta_t, att_s = expf(-d_s sigma), w_s = T_s * (1.f - att_s), T_{s+1} = T_s * att_s (names as above), the same early stop -- the
 * sample that ends the ray counts -- and the same skipped rays: a descent that leaves the tree (more than 23 levels, a link outside
 * [1, capacity)), more than 2^20 steps, a step that does not advance.  A skipped ray adds nothing to wmax.  For every dense sample of the
 * other rays with w_s > 0:  wmax[v_s] = max(wmax[v_s], bits(w_s)), compared as unsigned integers.  Non-negative binary32 values order as
 * their bit patterns, so the words depend on neither ray order, launch shape nor atomic order.  A NaN or non-positive w_s writes nothing.
 * No row column but sigma is read: there is no colour, no SH basis (rot_dirs and basis_minmax do not enter) and no target.
 * Sums: n_rays (the rays that were not skipped, misses included), n_stopped, n_samples (their dense samples), n_skipped.
 * MNV_E_UNSUPPORTED, before any launch: options.render_depth, N != 2, rows other than RGBA and SH 1 / 4 / 9 / 16 / 25.
 * MNV_E_INVALID, before any launch: a null tree / array / options / wmax / sums, width or height < 1, width * height > 2^22, capacity < 1, a
 *   data_dim too small for the row format, misaligned arrays, step_size not finite or <= 0.
 *
 * mnv_tree_cull.  wmax: device uint32 [capacity * 8]; weight_thresh finite and >= 0; data_out: device [capacity][8][data_dim], 16-byte
 * aligned; keep_out: device uint8 [capacity]; kept_at_depth: HOST int64 [24] as mnv_tree_select_cut's; counts: HOST.  Waits for hip_stream
 * (it hands counts back).  N == 2, any data_dim from 2 to 1024, either row format.  The input tree is never written.
 * Contract:
 *   A leaf voxel v (child == 0) of a chunk reached from the root is SEEN iff uint_as_float(wmax[v]) > weight_thresh: strictly greater; a
 *   NaN pattern is not seen, nor is a negative one.  A seen leaf's row is copied bit for bit; a leaf that is not seen gets a row of 0x0000.
 *   A chunk is DEAD iff each of its eight voxels is a leaf that is not seen or an interior voxel whose child chunk is dead.  The voxel above
 *   a dead chunk k gets a row of 0x0000 and keep_out[k] = 0; the voxel above a live chunk keeps its row bit for bit and keep_out[k] = 1.
 *   The root chunk is always kept (keep_out[0] = 1), even when everything under it died.  Chunks the walk does not reach get keep 0 and
 *   their rows are copied, as mnv_tree_mip_rows treats them.  A chunk under a dead chunk is dead: the set is parent-closed by construction.
 *   So mnv_tree_cut on a view whose data is data_out, with keep_out and new_capacity = the sum of kept_at_depth, yields the culled tree; the
 *   voxel above a dead chunk becomes an empty leaf.
 *   counts: leaves_seen; leaves_culled: the leaves not seen whose density was h(sigma) > 0 before (h as mnv_tree_mip_rows has it);
 *   dead_chunks (reached chunks with keep 0).  Level order inside the walk depends on the schedule and decides no output byte; no atomic
 *   operation decides one (the counts are sums of integers).
 * What this does to frames.  For options with sigma_thresh >= 0 and stop_thresh >= 2^-24, after mnv_rays_visibility over a ray list and
 * mnv_tree_cull at weight_thresh == 0, the arrays (child, data_out), NOT cut, give every listed ray the pixel the source tree gives it,
 * bit for bit (through mnv_render_rays_accel, mnv_rays_grad or another mnv_rays_visibility).  A culled leaf took either no dense sample or
 * only samples with w_s == 0 from every listed ray; with T_s >= stop_thresh >= 2^-24 that means 1.f - att_s == 0, att_s == 1 exactly: T was
 * unchanged by the sample and every colour term it added was w_s / den = +0 (or c * w_s = +-0 for RGBA rows, added to a sum that started at
 * +0) -- for rows of finite values; a non-finite colour coefficient in a culled leaf made a NaN term that the cull removes.  After the cull the leaf's sigma is +0, which is not above sigma_thresh: the sample is not taken, and the step sequence -- which does
 * not depend on sigma -- is the same.    After the CUT the march crosses a collapsed region in fewer, larger steps, each of
 * which adds step_size, so later sample lengths shift: frames of the cut tree are close to the source's, not equal, as on any coarser tree.
 * MNV_E_INVALID: a null argument, weight_thresh negative or not finite, a child link outside [1, capacity), a chunk reached twice,
 * overlapping or misaligned arrays, host arrays.  MNV_E_UNSUPPORTED: N != 2, more than 23 levels, data_dim above 1024. */
typedef struct mnv_vis_sums {
    int64_t n_rays, n_stopped, n_samples, n_skipped, reserved[4];
} mnv_vis_sums;
typedef struct mnv_cull_counts {
    int64_t leaves_seen, leaves_culled, dead_chunks, reserved;
} mnv_cull_counts;
int mnv_rays_visibility(const mnv_tree_view *device_tree, const float *origins, const float *dirs /* device [height][width][3] */,
                        const float *tmax /* device [height][width] or NULL */, int32_t width, int32_t height, const mnv_render_options *opt,
                        uint32_t *wmax /* device [capacity * 8] */, mnv_vis_sums *sums /* device */, void *hip_stream);
int mnv_tree_cull(const mnv_tree_view *device_tree, const uint32_t *wmax, float weight_thresh, uint16_t *data_out,
                  uint8_t *keep_out /* device [capacity] */, int64_t kept_at_depth[24] /* HOST */, mnv_cull_counts *counts /* HOST */,
                  void *hip_stream);

/* ------------------------------------------------ a tree from a coloured point cloud
 * Everything above works on a tree that exists.  mnv_point_tree_* make one from points (a photogrammetry or lidar cloud): occupancy at one
 * depth D, the chunks above it, a mean colour per occupied voxel and one density for all of them, as an ordinary tree in the reference's
 * arrays -- the start mnv_n3tree_fit refines.  N == 2; depths as above (the root chunk's voxels have depth 1).
 *
 * Use: create, add any number of times (device arrays), finish (HOST stats; their chunk counts size the outputs), write.  add after finish
 * is allowed, the next finish answers for all points so far; write before finish, or after an add that no finish followed, is
 * MNV_E_INVALID.  add and finish wait for hip_stream (they read counts back to size their lists); write is asynchronous on it.  Two handles
 * share nothing.
 *
 * Contract (binary32 where floats appear, one operation at a time in the stated order, no contraction, subnormals kept; everything after
 * the voxel of a point is integer arithmetic, so no float sum and no atomic order decides an output byte).
 *   Voxel of a point p.  q_k = offset[k] + scale[k] * p[k] (the product, then the sum: mnv_tree_select_cut's rule).  The point is DROPPED,
 *     and counted in stats.dropped, when a p[k] or q_k is not finite or a q_k lies outside [0, 1) (q_k == 1.0f is outside).  Otherwise
 *     i_k = (int)floorf(q_k * 2^D) (the product is exact) and the voxel's code is the 3 D-bit Morton word of (i_x, i_y, i_z) with x the most
 *     significant bit of each triple: the digit of level l (bits 3 (D - l) .. 3 (D - l) + 2) is j = 4 x + 2 y + z, as everywhere in the tree.
 *   Accumulation.  Per distinct code a count n and the sums S_c of the three 8-bit colour channels (64 bits each) over the accepted points
 *     of ALL add calls.  The result depends on the multiset of accepted points alone: not on their order, the split into calls, a launch
 *     shape or an atomic's turn.  More than 2^32 - 1 accepted points is MNV_E_UNSUPPORTED (the add that passes it changes nothing).
 *   Occupancy and structure.  A depth-D voxel is occupied iff n >= min_points.  A chunk of depth d exists iff it is the root or an occupied
 *     voxel lies under the depth-(d - 1) voxel above it.  Chunks are numbered breadth first: the root is 0, then depth 2, 3 .. D, within a
 *     depth ascending by the code of the voxel above.  capacity = the number of chunks = the sum of stats.chunks_at_depth.
 *     child[c][j] = index(child chunk) - c where that chunk exists, 0 otherwise (every entry of depth D is 0).  parent[c] = index(parent
 *     chunk) * 8 + j of the voxel above, -1 for the root (mnv_tree_truncate's rule).  sample_counts is 8 everywhere (the loader's value).
 *     counts[c][j] = n of every depth-D voxel of an existing chunk, those below min_points included, 0 elsewhere.
 *   Rows.  All 0x0000, except the rows of occupied depth-D voxels: column data_dim - 1 is half(sigma) (to nearest even, once); per colour
 *     channel c the mean m = (2 S_c + n) / (2 n) in integer arithmetic (round half up, 0 .. 255) picks table[m] of
 *     mnv_points_colour_table, which goes to column c (MNV_FORMAT_RGBA, data_dim 4) or to the DC coefficient c * basis_dim
 *     (MNV_FORMAT_SH, data_dim 3 * basis_dim + 1; the higher coefficients stay 0).
 *   mnv_points_colour_table (HOST, no device needed; create uploads the same table, no device transcendental is involved):
 *     RGBA: table[v] = half(v / 255.f).  SH: table[v] = half((float)(log(x / (1 - x)) / 0.28209479177387814)) computed in double, with
 *     x = clamp(v / 255, 1/512, 511/512): the inverse of the march's sigmoid of C0 * coefficient.
 *   No occupied voxel: capacity 1, the root chunk is all leaves with zero rows (with D == 1 the root's voxels are the depth-D voxels:
 *     counts holds theirs).
 * Outputs of write (device): child_out int32 [capacity][8]; data_out [capacity][8][data_dim], 16-byte aligned; parent_out int32 [capacity]
 * or NULL; sample_counts_out int16 [capacity][8] or NULL; counts_out uint32 [capacity][8] or NULL.
 * Memory.  A handle keeps 40 bytes per distinct voxel (code, count, three sums), after finish 8 bytes per chunk, and a grow-only scratch:
 * 24 bytes per element of the largest sort (keys and payloads, twice: the sort runs between the two halves), 48 per 512 elements and the
 * sort's histograms -- within 32 bytes per element --, where the elements of an add are its points (at most 2^27 at a time:
 * a longer add is sorted in pieces) and the distinct voxels held so far, which are sorted with them; while an add runs the old and the new
 * record list exist together (40 bytes per distinct voxel each).  finish holds 8 bytes per distinct voxel more while it runs.
 * MNV_E_INVALID: a null argument (rgb included); depth outside 1 .. 21; min_points == 0; a sigma that is not finite and positive; a scale
 * that is not finite and positive, an offset that is not finite; n < 0; misaligned data_out; host pointers.  MNV_E_UNSUPPORTED: a format
 * or basis_dim outside {RGBA, SH with 1, 4, 9, 16, 25}; more than 2^31 - 1 chunks, or points and distinct voxels in one sort.  Arguments
 * are checked before a device is touched; create on a machine without one is MNV_E_NO_DEVICE. */
typedef struct mnv_points_params {
    float offset[3], scale[3];   /* world -> unit cube, as mnv_tree_view has them */
    int32_t depth;               /* D: the leaf voxels' depth, 1 .. 21 */
    int32_t format, basis_dim;   /* MNV_FORMAT_RGBA, or MNV_FORMAT_SH with basis_dim in {1, 4, 9, 16, 25} */
    uint32_t min_points;         /* a depth-D voxel is occupied iff its count >= min_points; >= 1 */
    float sigma;                 /* density written to occupied voxels; finite, > 0 */
} mnv_points_params;
typedef struct mnv_points_stats {
    int64_t accepted, dropped;   /* points inside / outside the cube (or not finite), over all add calls */
    int64_t distinct_voxels;     /* depth-D voxels holding >= 1 point */
    int64_t occupied_voxels;     /* ... holding >= min_points */
    int64_t chunks_at_depth[24]; /* entry d = chunks of depth d (entry 0 unused, 0); their sum is the capacity */
} mnv_points_stats;
typedef struct mnv_point_tree mnv_point_tree;
int mnv_point_tree_create(const mnv_points_params *p, mnv_point_tree **out);
int mnv_point_tree_add(mnv_point_tree *t, const float *xyz /* device [n][3] */, const uint8_t *rgb /* device [n][3] */, int64_t n, void *hip_stream);
int mnv_point_tree_finish(mnv_point_tree *t, mnv_points_stats *stats /* HOST */, void *hip_stream);
int mnv_point_tree_write(const mnv_point_tree *t, int32_t *child_out, uint16_t *data_out, int32_t *parent_out /* or NULL */,
                         int16_t *sample_counts_out /* or NULL */, uint32_t *counts_out /* or NULL, [capacity][8] */, void *hip_stream);
void mnv_point_tree_destroy(mnv_point_tree *t);
int mnv_points_colour_table(int32_t format, int32_t basis_dim, uint16_t out[256] /* HOST */);
/* The smallest cube around the box [lo, hi] as an offset and a scale (HOST): ext_k = hi[k] - lo[k], L = max_k ext_k (1 when that is 0),
 * s = 1.f / L, scale[k] = s for the three axes, offset[k] = 0.5f - s * (0.5f * (lo[k] + hi[k])): the box's centre maps to 0.5.  A point on
 * an upper face of the box along its longest axis maps to q == 1 and would be dropped: callers that want every point inside widen the box
 * first.  MNV_E_INVALID: a null argument, a bound that is not finite, hi[k] < lo[k]. */
int mnv_points_bounds_to_cube(const float lo[3], const float hi[3], float offset[3], float scale[3]);

/* ------------------------------------------------ merging two trees: one tree placed into a voxel of another
 * A scene that arrives as tiles (one octree per spatial cell, a point cloud per survey block, a finer tree for one block of a baked scene)
 * becomes ONE tree: the union of the two structures with a stated rule for the rows, numbered in the canonical breadth-first order of
 * mnv_point_tree_write -- so merging with the one-chunk empty tree is also the call that puts an arbitrary tree into that order.  More than
 * two trees are folded, one merge after the other.  Trees whose cubes are not aligned octree voxels of each other are out of scope (that
 * would be resampling), and interior rows are not re-mipped: call mnv_tree_mip_rows on the result.
 *
 * Use: plan (HOST stats; stats.capacity sizes the outputs), write any number of times, destroy.  plan waits for hip_stream (it reads one
 * level size back per level, at most 23 times); write is asynchronous on it.  The handle keeps the two views' POINTERS: the input arrays
 * must stay alive and unchanged until the last write has finished.  Two handles share nothing.
 *
 * Inputs.  Two device trees A (the base) and B: N == 2, equal data_dim, format and basis_dim, data_dim 2 .. 1024, depths as everywhere
 * (the root chunk's voxels have depth 1); `parent` is not read; neither input is modified.  A and B may be the same tree.
 * Placement.  An integer level k in 0 .. 22 and an integer corner (x, y, z) with 0 <= x, y, z < 2^k: B's cube is the depth-k voxel of A's
 *   cube with that corner; k == 0 means the same cube.  B's offset and scale are not read: the placement is the integers
 *   (mnv_tree_voxel_cube gives the transform a tile must be built with).  The result has A's offset and scale.
 * Structure.  A union.  For a voxel (d, i) (depth, integer corner) of the merged cube a source HAS THE VOXEL EXACTLY when its own walk from
 *   its root reaches a voxel at that depth and corner -- in B's coordinates the depth is d - k and the corner is i minus the placement
 *   corner scaled by 2^(d-k); otherwise the voxel is COVERED by a shallower leaf of the source or, for B, lies outside B's cube (NONE).
 *   A merged voxel is interior iff A has it exactly with child != 0, or B has it exactly with child != 0, or d <= k and it lies on the
 *   path to B's cube: the path voxel of depth l has j_l = 4 x_l + 2 y_l + z_l with x_l = bit k - l of x; path voxels are interior even
 *   where A is a leaf.  A merged chunk exists iff it is the root or the voxel above it is interior.
 * Numbering.  Breadth first: the root is 0, then depths 2, 3 ..; within a depth ascending by the Morton code of the voxel above
 *   (equivalently by (merged index of the parent chunk, j)): mnv_point_tree_write's numbering, with child, parent and capacity as that
 *   call defines them.
 * Sources of a voxel.  a_vox is the voxel id (chunk * 8 + j) of A's exact voxel there or of A's covering leaf (it always exists: A spans
 *   the cube); b_vox the same for B, or none.
 * Rows.  h() is the binary16 value as binary32 with bits that are not finite read as +0 (the mip contract's h), pos(bits) = h(bits) > 0,
 *   sat_half() rounds a binary32 to binary16, to nearest even, once, subnormal results kept, and a result that would be infinite becomes
 *   +-65504.  sigma is column data_dim - 1.
 *     b_vox none, or !pos(sigma_b):                 A's row, bit for bit.
 *     otherwise, MNV_MERGE_OVER:                    B's row, bit for bit.
 *     otherwise, MNV_MERGE_ADD and !pos(sigma_a):   B's row, bit for bit.
 *     otherwise, MNV_MERGE_ADD and pos(sigma_a):    wa = h(sigma_a), wb = h(sigma_b), W = wa + wb; sigma' = sat_half(W); every other
 *       column c: sat_half(((wa * h(a_c)) + (wb * h(b_c))) / W).  (binary32, one operation at a time in that order, no contraction,
 *       correctly rounded division; no value there is a binary32 subnormal or overflows.)
 *   The same rule gives the rows of interior voxels from whatever the sources hold there.
 * Sample counts (sample_counts_out or NULL).  The count of the source whose row was taken verbatim; clamp(ca + cb, -32768, 32767) for a
 *   blended row; a source without a counts array counts 8.
 * Provenance (src_a_out / src_b_out or NULL): int32 [capacity][8], a_vox and b_vox (-1: none) of every merged voxel -- what a caller needs
 *   to carry float masters or counts of its own through the merge.
 * Stats (HOST).  chunks_at_depth[d], capacity (their sum); rows_from_a / rows_from_b / rows_blended: the merged voxels by the line of the
 *   row rule that applied (they sum to 8 capacity); pushed_a / pushed_b: the merged voxels whose a_vox / b_vox is a shallower covering leaf.
 * Determinism.  No atomic operation and no launch shape decides an output byte (the stats are integer sums).
 * Memory.  A handle keeps 17 bytes per chunk of capacity_a + capacity_b + k, the bound of the merged capacity (every merged chunk but the
 *   root hangs under an interior voxel of A, an interior voxel of B or a path voxel); plan holds 8 bytes more per chunk of that bound and
 *   the scan's scratch while it runs.
 * Outputs of write (device): child_out int32 [capacity][8]; data_out [capacity][8][data_dim], 16-byte aligned; parent_out int32 [capacity]
 * or NULL; sample_counts_out int16 [capacity][8] or NULL; src_a_out, src_b_out or NULL.  They must not overlap the inputs.
 * MNV_E_INVALID: a null argument; mismatched row formats; a level outside 0 .. 22, a corner outside [0, 2^k), a mode that is neither;
 * a followed link outside [1, capacity); more merged chunks than capacity_a + capacity_b + k (an input in which a chunk is reached twice);
 * misaligned rows; host arrays.  MNV_E_UNSUPPORTED: N != 2, data_dim above 1024, an input of more than 2^27 chunks, a merged depth beyond
 * 23, more than 2^31 - 1 merged chunks.  An input whose links form a cycle ends in one of the two codes (the level bound and the chunk
 * bound), never in an endless walk.  Arguments are checked before a device is touched. */
#define MNV_MERGE_OVER 0 /* where B holds density, B's row */
#define MNV_MERGE_ADD 1  /* where both hold density, the density-weighted blend */
typedef struct mnv_merge_params {
    int32_t level, corner[3]; /* the placement k : (x, y, z) */
    int32_t mode;             /* MNV_MERGE_OVER or MNV_MERGE_ADD */
    int32_t reserved;         /* 0 */
} mnv_merge_params;
typedef struct mnv_merge_stats {
    int64_t chunks_at_depth[24]; /* entry d = merged chunks of depth d (entry 0 unused, 0) */
    int64_t capacity;            /* their sum */
    int64_t rows_from_a, rows_from_b, rows_blended;
    int64_t pushed_a, pushed_b;
} mnv_merge_stats;
typedef struct mnv_tree_merge mnv_tree_merge;
int mnv_tree_merge_plan(const mnv_tree_view *a, const mnv_tree_view *b, const mnv_merge_params *p, mnv_tree_merge **out, mnv_merge_stats *stats /* HOST */,
                        void *hip_stream);
int mnv_tree_merge_write(const mnv_tree_merge *m, int32_t *child_out, uint16_t *data_out, int32_t *parent_out /* or NULL */,
                         int16_t *sample_counts_out /* or NULL */, int32_t *src_a_out /* or NULL */, int32_t *src_b_out /* or NULL */, void *hip_stream);
void mnv_tree_merge_destroy(mnv_tree_merge *m);
/* The cube of the depth-`level` voxel with integer corner `corner` of the cube (offset, scale), as an offset and a scale (HOST): the
 * transform a tile must be built with so that it merges at level : corner.  scale_out[k] = scale[k] * 2^level (exact),
 * offset_out[k] = offset[k] * 2^level - corner[k]: the product, then the difference, each rounded once (binary32).  MNV_E_INVALID: a null
 * argument, a level outside 0 .. 22, a corner outside [0, 2^level). */
int mnv_tree_voxel_cube(const float offset[3], const float scale[3], int32_t level, const int32_t corner[3], float offset_out[3], float scale_out[3]);

/* (Device times: every entry point launches on the caller's stream and records nothing itself -- bracket the call with two HIP events on that
 * stream, as bench.py does for roofline.achieved.) */

/* ------------------------------------------ host-side data model (C++ core) */

/* Opaque handle to the C++ viewer::N3Tree (host arrays + optional device copy);
 * mirrors include/n3tree/n3tree.hpp:17-69. */
typedef struct mnv_n3tree mnv_n3tree;

int mnv_n3tree_open(const char *npz_path, mnv_n3tree **out);          /* N3Tree::open, n3tree.cpp:16-205 */
int mnv_n3tree_from_arrays(const mnv_tree_view *host_view, mnv_n3tree **out); /* copies */
void mnv_n3tree_free(mnv_n3tree *t);
int mnv_n3tree_host_view(const mnv_n3tree *t, mnv_tree_view *view);
/* N3Tree::move_to_device (n3tree.cpp:207-246): allocates [max_capacity,...] device
 * arrays, copies the first `capacity` rows, builds the accel. */
int mnv_n3tree_move_to_device(mnv_n3tree *t, int64_t max_capacity, int need_parent,
                              int need_sample_counts, void *hip_stream);
int mnv_n3tree_device_view(const mnv_n3tree *t, mnv_tree_view *view);
const mnv_accel *mnv_n3tree_accel(const mnv_n3tree *t);
int mnv_n3tree_save_npz(const mnv_n3tree *t, const char *npz_path); /* svox layout, stored (no deflate) */
/* N3Tree::gen_wireframe (n3tree.cpp:249-329) on the host arrays: 24 vertices of 9 floats (position, colour 0,0,0, normal 0,0,1) per cube,
 * in the reference's order and float arithmetic.  *n_floats receives the length; out NULL with cap_floats 0 asks for it alone; a buffer
 * shorter than that is MNV_E_INVALID (and *n_floats still says what it needs). */
int mnv_n3tree_gen_wireframe(const mnv_n3tree *t, int32_t max_depth, float *out, int64_t cap_floats, int64_t *n_floats);
/* A level of detail of a tree that is on the device (mnv_n3tree_move_to_device): mnv_tree_mip_rows, then mnv_tree_truncate at max_depth, as a
 * NEW tree on the device -- data, child, parent, sample counts when `t` has them on the device, and the packed accel when `t` has one --
 * with the same offset / scale / row format; its host arrays are downloaded, so mnv_n3tree_save_npz writes it.  `t` is not changed.  Free
 * with mnv_n3tree_free.  Runs on the null stream and waits for it.  MNV_E_INVALID: max_depth < 1, a tree that is not on the device;
 * otherwise the codes of the two calls. */
int mnv_n3tree_make_lod(mnv_n3tree *t, int32_t max_depth, mnv_n3tree **out);
/* The view-dependent level of detail of a tree that is on the device: mnv_tree_mip_rows, mnv_tree_select_cut for the n_views viewpoints, then
 * mnv_tree_cut, as a NEW tree exactly as mnv_n3tree_make_lod makes one (arrays, accel, host arrays downloaded; `t` is not changed).
 * kept_at_depth: int64 [24] or NULL, the kept chunks per depth.  Runs on the null stream and waits for it.  MNV_E_INVALID: a tree that is
 * not on the device; otherwise the codes of the three calls. */
int mnv_n3tree_make_view_lod(mnv_n3tree *t, const mnv_lod_view *views, int32_t n_views, float pixels, int32_t min_depth, int32_t max_depth,
                             int64_t *kept_at_depth, mnv_n3tree **out);
/* N3Tree::make_culled: a tree that is on the device without what the pinhole frames of n_cams cameras cannot see.  wmax is cleared; per
 * camera mnv_generate_rays(MNV_PROJ_PINHOLE, the whole image) then mnv_rays_visibility; then mnv_tree_cull at weight_thresh and
 * mnv_tree_cut, as a NEW tree exactly as mnv_n3tree_make_lod makes one (arrays, accel, host arrays downloaded; `t` is not changed).
 * kept_at_depth: int64 [24] or NULL, the kept chunks per depth; counts: or NULL.  Runs on the null stream and waits for it.
 * MNV_E_INVALID: a tree that is not on the device, no camera, a camera without pixels or of more than 2^22; otherwise the codes of the calls. */
int mnv_n3tree_make_culled(mnv_n3tree *t, const mnv_camera *cams, int32_t n_cams, const mnv_render_options *opt, float weight_thresh,
                           int64_t *kept_at_depth, mnv_cull_counts *counts, mnv_n3tree **out);
/* N3Tree::fit: optimise the rows of a tree that is on the device against target frames, full batch.  Per iteration: for each camera,
 * mnv_generate_rays(MNV_PROJ_PINHOLE, the whole image) then mnv_rays_grad against targets[i] (a DEVICE float [height][width][4] frame of that
 * camera's size; alpha 0 excludes a pixel), all into one accumulator; then one mnv_rows_sgd_step.  The float32 master copy is made at the
 * start (mnv_rows_master_init).  At the end the packed accel is rebuilt (where the tree has one) and the host arrays are refreshed, so
 * mnv_n3tree_save_npz and every march see the result.  se_q32_out: HOST int64 [iterations], the se_q32 of each iteration's rays BEFORE
 * its step (exact integers; or NULL).  Runs on the null stream and waits for it.  MNV_E_INVALID: a tree that is not on the device, no camera,
 * a null target, iterations < 0, learning rates that are not finite or negative, a camera of more than 2^22 pixels, cameras whose pixels together pass 2^24 (the headroom
 * between two clears); otherwise the codes of the calls. */
typedef struct mnv_fit_params {
    int32_t iterations;
    float lr_colour, lr_sigma;
    int32_t reserved;
} mnv_fit_params;
int mnv_n3tree_fit(mnv_n3tree *t, const mnv_camera *cams, int32_t n_cams, const float *const *targets /* HOST array of n_cams device pointers */,
                   const mnv_render_options *opt, const mnv_fit_params *params, int64_t *se_q32_out);
/* N3Tree::fit_to: the targets are the teacher's frames -- mnv_render_voxels_accel of `teacher` (on the device, with its accel) at each camera,
 * float, as they are: a pixel where the teacher accumulated no opacity (alpha 0) is excluded -- then mnv_n3tree_fit.  A level of detail
 * (mnv_n3tree_make_lod of the teacher) fitted this way is the use. */
int mnv_n3tree_fit_to_tree(mnv_n3tree *t, const mnv_n3tree *teacher, const mnv_camera *cams, int32_t n_cams, const mnv_render_options *opt,
                           const mnv_fit_params *params, int64_t *se_q32_out);
/* N3Tree::fit_ex: mnv_n3tree_fit with a choice of optimizer and of batching ("fitting on a photo set" above).
 *   batch_rays == 0: full batch, mnv_n3tree_fit's loop with its 2^24 bound and the chosen row step.  optimizer == MNV_FIT_SGD with
 *     batch_rays == 0 IS mnv_n3tree_fit (steps = iterations), byte for byte: both run the same loop.
 *   batch_rays > 0: a multiple of tile^2, at most 2^22.  A mnv_ray_batcher over the cameras and targets (tile, seed) has U units;
 *     B = batch_rays / tile^2 units per step, nb = ceil(U / B) batches per epoch.  Step s = 0 .. steps - 1 draws the units
 *     [b * B, min((b + 1) * B, U)) of epoch s / nb, b = s % nb, runs ONE mnv_rays_grad on that flat list and one row step.  The accumulators
 *     are cleared by every step, so the 2^24 bound does not apply: any number of images of any size (U < 2^31, 4096 cameras).
 *   MNV_FIT_ADAM: mnv_rows_adam_step with step = s + 1; the moments are allocated (zeroed) only then.  beta1 / beta2 / eps are not read
 *     for MNV_FIT_SGD.  Adam's rates chosen on the fit scene of tests/fit_cases.py: lr_colour 0.03, lr_sigma 1, beta 0.9 / 0.999, eps 1e-8
 *     (the sweep stands in tests/fit_adam_ref.py); they do not depend on the gradient's scale, hence not on the image size.
 *   se_q32_out / n_rays_out: HOST int64 [steps] or NULL: the se_q32 and the n_rays of each step's rays BEFORE its step; their ratio
 *     (/ 2^32) is that batch's mean squared error.
 *   After the loop the accel is rebuilt and the host arrays are refreshed, as mnv_n3tree_fit does.  Runs on the null stream and waits.
 *   MNV_E_INVALID: what mnv_n3tree_fit refuses (the 2^24 bound only for batch_rays == 0), an unknown optimizer, a tile other than 1 or 8,
 *     batch_rays < 0, not a multiple of tile^2 or above 2^22, for Adam a beta outside [0, 1) or eps not finite or <= 0; otherwise the
 *     codes of the calls. */
#define MNV_FIT_SGD 0
#define MNV_FIT_ADAM 1
typedef struct mnv_fit_params_ex {
    int32_t steps, optimizer /* MNV_FIT_SGD 0, MNV_FIT_ADAM 1 */;
    float lr_colour, lr_sigma, beta1, beta2, eps;
    int32_t batch_rays /* 0: full batch */, tile /* 1 | 8 */;
    uint64_t seed;
    int32_t reserved[4];
} mnv_fit_params_ex;
int mnv_n3tree_fit_ex(mnv_n3tree *t, const mnv_camera *cams, int32_t n_cams, const float *const *targets /* HOST array of n_cams device pointers */,
                      const mnv_render_options *opt, const mnv_fit_params_ex *p, int64_t *se_q32_out /* HOST [steps] or NULL */,
                      int64_t *n_rays_out /* HOST [steps] or NULL */);
/* N3Tree::fit_to_ex: the teacher's frames first, as mnv_n3tree_fit_to_tree renders them, then mnv_n3tree_fit_ex. */
int mnv_n3tree_fit_to_tree_ex(mnv_n3tree *t, const mnv_n3tree *teacher, const mnv_camera *cams, int32_t n_cams, const mnv_render_options *opt,
                              const mnv_fit_params_ex *p, int64_t *se_q32_out, int64_t *n_rays_out);
/* N3Tree::from_points: mnv_point_tree_create, one add of the n device points, finish and write into a NEW tree on the device -- data, child,
 * parent, sample counts and the packed accel -- with the params' offset / scale / row format (basis_dim -1 for RGBA); its host arrays are
 * downloaded, so mnv_n3tree_save_npz, mnv_n3tree_make_lod, mnv_n3tree_fit and mnv_extract_surface work on it at once.  stats: HOST or NULL.
 * n == 0 gives the one-chunk empty tree.  Waits for hip_stream.  Free with mnv_n3tree_free.  The codes of the four calls. */
int mnv_n3tree_from_points(const mnv_points_params *p, const float *xyz /* device [n][3] */, const uint8_t *rgb /* device [n][3] */, int64_t n,
                           void *hip_stream, mnv_points_stats *stats, mnv_n3tree **out);
/* N3Tree::merge: mnv_tree_merge_plan and write of two trees that are on the device, `b` placed into `a` as `p` says, as a NEW tree exactly
 * as mnv_n3tree_make_lod makes one (arrays, parent, sample counts where `a` has them, the accel where `a` has one, host arrays
 * downloaded; offset, scale and row format of `a`; neither input is changed).  stats: HOST or NULL.  Runs on the null stream and waits
 * for it.  MNV_E_INVALID: a tree that is not on the device; otherwise the codes of the two calls. */
int mnv_n3tree_merge(mnv_n3tree *a, const mnv_n3tree *b, const mnv_merge_params *p, mnv_merge_stats *stats, mnv_n3tree **out);
/* DataFormat::parse / to_string (src/data_format.cpp:5-41) */
void mnv_data_format_parse(const char *str, int32_t *format, int32_t *basis_dim);
int mnv_data_format_to_string(int32_t format, int32_t basis_dim, char *buf, size_t buflen);

/* ------------------------------------------------ the VolumeRenderer role (batch / offscreen)
 * viewer::VolumeRenderer (include/renderer/renderer.hpp:9-39, src/renderer/cuda_renderer.cpp) behind the C ABI,
 * for hosts that are not C++: it owns a camera, the options and an internal stream; set() uploads the tree
 * (move_to_device(max_tree_capacity, true, true)), render() draws one frame and -- with a model loaded and
 * options.use_splitting / use_guided_sampling -- runs the reference's refinement loop
 * (cuda_renderer.cpp:98-156: trackers -> expand_voxels / get_more_samples -> prune_tree). */
typedef struct mnv_renderer mnv_renderer;
typedef struct mnv_renderer_stats {  /* what the reference prints per frame */
    int32_t track_visit, used_accel, full;
    int32_t split_candidates, added;       /* expand_voxels: "Split candidates: N", "Added: N" */
    int32_t sample_candidates, resampled;  /* get_more_samples */
    int32_t pruned;                        /* prune_tree: reclaimed chunks, -1 = nothing to prune, 0 = did not run */
    int64_t guided_samples;                /* rows sent to the networks by guided sampling */
    int64_t capacity;                      /* chunks in use after the frame */
    int32_t fused;                         /* the guided-sampling frame ran as one kernel (mnv_render_guided_fused) */
    int32_t reserved;
} mnv_renderer_stats;
int mnv_renderer_create(mnv_renderer **out);
void mnv_renderer_destroy(mnv_renderer *r);
/* VolumeRenderer::set (cuda_renderer.cpp:498-516); the tree must outlive the renderer or the next set() */
int mnv_renderer_set(mnv_renderer *r, mnv_n3tree *tree, int64_t max_tree_capacity);
/* load_model (cuda_renderer.cpp:518-539) from an .npz container: mlp_desc int32[9] (the mnv_mlp_desc integers in
 * order), mlp_center f32[3], mlp_inv_extent f32[3], mlp_params binary16, grid_dim int[2], min_position f32[3],
 * max_position f32[3] */
int mnv_renderer_load_model(mnv_renderer *r, const char *npz_path);
int mnv_renderer_set_model(mnv_renderer *r, const mnv_mlp_desc *desc, const uint16_t *params, size_t n_halfs,
                           const mnv_cluster_grid *grid);
int mnv_renderer_resize(mnv_renderer *r, int32_t width, int32_t height);
/* the renderer's RenderOptions, mutable in place (VolumeRenderer::options) */
mnv_render_options *mnv_renderer_options(mnv_renderer *r);
/* VolumeRenderer::camera pose and focal length (fx <= 0 keeps the current one; fy <= 0 means fy = fx) */
int mnv_renderer_set_camera(mnv_renderer *r, float fx, float fy, const float center[3], const float v_back[3],
                            const float v_world_up[3]);
/* seed of the sample jitter (torch::rand in the reference); accel_rebuild_after is not read: the accel follows every edit */
int mnv_renderer_set_seed(mnv_renderer *r, uint64_t seed, int32_t accel_rebuild_after);
int mnv_renderer_render(mnv_renderer *r, mnv_renderer_stats *stats /* may be NULL */);
/* wait for the frame and copy it to host buffers [height][width][4] (either may be NULL) */
int mnv_renderer_download(mnv_renderer *r, float *rgba_host, uint8_t *rgba8_host);
/*
 * Frames in flight (VolumeRenderer::frames_in_flight, default 3).  The reference issues one render_voxels call per frame on
 * one stream (src/renderer/cuda_renderer.cpp:141-142); here plain frames (no refinement, packed accel current) rotate over
 * `count` slots, each with its own HIP stream and frame buffers, so the tail of one launch overlaps the next launches.
 * mnv_renderer_render returns at once; mnv_renderer_last_slot names the slot it rendered into and
 * mnv_renderer_download_slot waits for that slot's frame only.  count = 1 restores the one-stream behaviour.
 */
int mnv_renderer_set_frames_in_flight(mnv_renderer *r, int32_t count);
/* VolumeRenderer::guided_in_flight (default off): guided-sampling frames that change nothing -- use_guided_sampling without use_splitting, a
 * network the fused kernel covers, a tree below 3/4 of its capacity -- rotate over the slots like plain frames (1.20 -> 1.09 ms per 1080p
 * frame on the cfg2 tree with three in flight).  Such a frame's sample count is not known when mnv_renderer_render returns: the stats carry
 * guided_samples = -1 and mnv_renderer_slot_guided_samples waits for the frame of `slot` and returns its count. */
int mnv_renderer_set_guided_in_flight(mnv_renderer *r, int enable);
int mnv_renderer_slot_guided_samples(mnv_renderer *r, int32_t slot, int64_t *count_out);
/* VolumeRenderer::use_fused_guided (default on): guided-sampling frames that need nothing but the picture run as one kernel;
 * off = always the four steps of cuda_renderer.cpp:107-139 (sample march, compaction, networks, composite) */
int mnv_renderer_set_fused_guided(mnv_renderer *r, int enable);
/* The reference's render loop passes offscreen == false to all three launchers (cuda_renderer.cpp:111-113,135-136,141-142): the frame is limited by
 * the GL pass's depth attachment and composited over its image.  tmax_px [height][width] float / rgba8_init [height][width][4] uint8: device
 * arrays of the caller that stay valid while frames are rendered (either may be NULL; both NULL = the offline renderer again, the default).
 * Single-rank rendering only. */
int mnv_renderer_set_frame_inputs(mnv_renderer *r, const float *tmax_px, const uint8_t *rgba8_init);
/* VolumeRenderer::set_ranks: several ranks (one process per GPU, each with its own renderer over the same scene and networks) render and
 * refine in lock step -- this rank marches its macro tiles, tracker rows and visit marks are all-gathered, the same refinement runs on
 * every replica, rank 0's frame is the whole picture.  comm NULL = back to one rank.  The communicator stays the caller's. */
int mnv_renderer_set_ranks(mnv_renderer *r, mnv_comm *comm, int32_t tile_w, int32_t tile_h);
int32_t mnv_renderer_last_slot(const mnv_renderer *r);
int mnv_renderer_download_slot(mnv_renderer *r, int32_t slot, float *rgba_host, uint8_t *rgba8_host);
/* copy the (refined) device tree back into the mnv_n3tree's host arrays */
int mnv_renderer_sync_tree(mnv_renderer *r);
/* options.show_grid: render() draws the grid of options.grid_max_depth with mnv_render_wireframe into per-slot images and passes them to
 * the frame as its mnv_frame_inputs (refused together with caller-set frame inputs or several ranks).  The wireframe of the last grid
 * frame (NULL before the first): regenerated when the depth or the tree changed.  Owned by the renderer. */
const mnv_wireframe *mnv_renderer_wireframe(const mnv_renderer *r);
/* VolumeRenderer::meshes: while any mesh of the list is visible, render() draws the grid first if options.show_grid is set, then the
 * list with mnv_render_meshes over it, into the frame slot's depth image and image on the slot's stream, and hands those to the frame as
 * its mnv_frame_inputs -- for every frame kind the grid works for (tracker and guided frames, frames in flight; with antialiasing the
 * sub-frames are issued one by one).  Refused by mnv_renderer_render (MNV_E_INVALID), like the grid, together with caller-set frame
 * inputs or several ranks.  With no visible mesh every frame is what it is without these calls, byte for byte.  The renderer does not
 * own the handles: a mesh stays the caller's and must outlive its frames (mnv_renderer_clear_meshes waits for the frames in flight). */
int mnv_renderer_add_mesh(mnv_renderer *r, const mnv_mesh *mesh);
int mnv_renderer_clear_meshes(mnv_renderer *r);
int32_t mnv_renderer_mesh_count(const mnv_renderer *r);
/* the camera (pose matrix and intrinsics) the last mnv_renderer_render used */
int mnv_renderer_camera(const mnv_renderer *r, mnv_camera *out);
/* VolumeRenderer::aa_samples / aa_filter (default 1, MNV_AA_TENT).  samples == 1: every frame is what it is without this call, byte for byte.
 * samples = K > 1: a plain frame (no refinement, packed accel) takes its frame slot as before and, on the slot's stream, marches the K
 * cameras of mnv_aa_pattern (cx - dx_k, cy - dy_k) with one mnv_render_voxels_accel_batch launch into a per-slot float sub-frame buffer
 * (K * width * height * 16 bytes, allocated at the first such frame, freed by a resize or another K) and resolves it into the slot's
 * frame with mnv_resolve_samples; frames in flight keep working.  With options.show_grid the K sub-frames are issued one by one (grid pass
 * + march per camera: the batch call takes no per-pixel inputs).  An unknown filter is refused here; mnv_renderer_render answers
 * MNV_E_INVALID while samples > 1 meets caller-set frame inputs, several ranks, a model with use_splitting / use_guided_sampling, a tree
 * without a packed accel, or samples outside 1 .. MNV_MAX_BATCH (samples = 1 renders again). */
int mnv_renderer_set_antialiasing(mnv_renderer *r, int32_t samples, int32_t filter);
/* VolumeRenderer::projection (default MNV_PROJ_PINHOLE: every frame is what it is without this call, byte for byte).  MNV_PROJ_ORTHO /
 * MNV_PROJ_EQUIRECT: a frame takes its frame slot as a plain frame does (frames in flight keep working) and, on the slot's stream,
 * generates its rays with mnv_generate_rays from the renderer's camera into per-slot buffers (width * height * 24 bytes, allocated at the
 * first such frame, freed by a resize) and marches them with mnv_render_rays_accel into the slot's frame; the equirectangular table is
 * rebuilt when the size changes.  An unknown projection is refused here; mnv_renderer_render answers MNV_E_INVALID while another projection
 * than the pinhole meets caller-set frame inputs, several ranks, options.show_grid, a visible mesh, antialiasing with more than one sample,
 * a model with use_splitting / use_guided_sampling, or a tree without a packed accel (MNV_PROJ_PINHOLE renders again). */
int mnv_renderer_set_projection(mnv_renderer *r, int32_t projection);
/* VolumeRenderer::set_target (default NULL: every frame is what it is without this call, byte for byte).  rgba8_device non-NULL: every
 * mnv_renderer_render is followed, on the frame slot's stream, by mnv_frame_metrics(`flags`, the standard window) of the slot's float
 * frame against that DEVICE array [height][width][4] into the slot's own device sums, and by a 40-byte copy of them to pinned host
 * memory -- whatever the frame kind (plain, in flight, anti-aliased, orthographic, equirectangular, grid, meshes, frame inputs,
 * refinement and guided frames).  The frames themselves do not change.  The pointer is sampled at each render: it may change per frame,
 * and an array must stay valid until its slot has been collected.  mnv_renderer_slot_metrics waits for the frame of `slot` only and
 * finishes its sums (mnv_metrics_finish); MNV_E_INVALID when the last frame of that slot was not scored.  A resize to another size clears the target,
 * and so does rgba8_device NULL (collect the frames in flight first: their scores go with it).  MNV_E_INVALID: unknown flag bits; a
 * target together with mnv_renderer_set_ranks, in either order. */
int mnv_renderer_set_target(mnv_renderer *r, const uint8_t *rgba8_device, int32_t flags);
int mnv_renderer_slot_metrics(mnv_renderer *r, int32_t slot, mnv_frame_metric_values *out);
/* VolumeRenderer::set_lod (default 0 = off: every frame is what it is without this call, byte for byte).  max_depth >= 1: the frames march
 * the tree of mnv_n3tree_make_lod(max_depth) instead of the tree that was set -- plain frames, frames in flight, anti-aliased and projected
 * frames, the grid overlay (the grid of the truncated tree) and meshes.  The renderer builds that tree at the first frame that needs it,
 * keeps one per depth and drops them all when mnv_renderer_set gets a tree (or a refinement frame edits it).  mnv_renderer_render answers
 * MNV_E_INVALID while a level of detail meets what would edit or vote on the tree: options.use_splitting, options.use_guided_sampling,
 * several ranks (level 0 renders again).  MNV_E_INVALID here: a negative depth. */
int mnv_renderer_set_lod(mnv_renderer *r, int32_t max_depth);
/* VolumeRenderer::set_view_lod (n_views == 0, the default, = off: every frame is what it is without this call, byte for byte).  With
 * n_views >= 1 the frames march the tree of mnv_n3tree_make_view_lod(views, pixels, min_depth, max_depth) instead of the tree that was set,
 * for the frame kinds of mnv_renderer_set_lod.  The caller names the viewpoints the cut must serve (an offline renderer knows its poses up
 * front); the renderer builds the tree at the first frame that needs it, keeps it until the views or parameters change, and drops it where
 * it drops the trees of mnv_renderer_set_lod.  The views are copied.  mnv_renderer_render answers MNV_E_INVALID while a view cut meets
 * options.use_splitting, options.use_guided_sampling, several ranks, or mnv_renderer_set_lod with a depth above 0.  MNV_E_INVALID here:
 * n_views outside [0, 4096], views NULL with n_views > 0, and what mnv_tree_select_cut refuses in views, pixels, min_depth, max_depth. */
int mnv_renderer_set_view_lod(mnv_renderer *r, const mnv_lod_view *views, int32_t n_views, float pixels, int32_t min_depth, int32_t max_depth);
/* Culling to a pose set.  n_cams == 0 (the default; cams may be NULL): render() is what it is without this call (byte for byte).  With
 * n_cams >= 1 the frames march the tree of mnv_n3tree_make_culled(cams, the renderer's options, weight_thresh) instead of the tree that was
 * set, in the frame kinds mnv_renderer_set_lod serves; the tree is built at the first frame that needs it, kept until the cameras, the
 * threshold or the march options (step_size, sigma_thresh, stop_thresh, render_bbox) change, and dropped where that call's trees are.
 * mnv_renderer_render refuses (MNV_E_INVALID) the combinations that call lists, and this one together with mnv_renderer_set_lod(D > 0) or
 * mnv_renderer_set_view_lod.  MNV_E_INVALID here: n_cams < 0, cams NULL with n_cams > 0, weight_thresh negative or not finite, a camera
 * without pixels or of more than 2^22. */
int mnv_renderer_set_cull(mnv_renderer *r, const mnv_camera *cams, int32_t n_cams, float weight_thresh);
/* VolumeRenderer::set_lod_fit (n_cams == 0 or params->iterations == 0, the default, = off: every frame is what it is without this call, byte
 * for byte).  Otherwise every tree mnv_renderer_set_lod / mnv_renderer_set_view_lod builds from now on is fitted, right after it is built,
 * to the frames of the tree that was set at the listed cameras (mnv_n3tree_fit_to_tree with `params`); trees built before are dropped.  The
 * cameras are copied.  Refused wherever a level of detail is (mnv_renderer_render says so).  MNV_E_INVALID here: a null argument, a negative
 * count, negative iterations, learning rates that are not finite or negative; the fit's own refusals surface at the frame that builds the tree. */
int mnv_renderer_set_lod_fit(mnv_renderer *r, const mnv_camera *cams, int32_t n_cams, const mnv_fit_params *params);
/* The same with mnv_fit_params_ex (mnv_n3tree_fit_to_tree_ex with `params`; n_cams == 0 or params->steps == 0 = off):
 * mnv_renderer_set_lod_fit is this call with MNV_FIT_SGD and batch_rays 0.  The optimizer's and the batching's refusals surface at the
 * frame that builds the tree. */
int mnv_renderer_set_lod_fit_ex(mnv_renderer *r, const mnv_camera *cams, int32_t n_cams, const mnv_fit_params_ex *params);

/* ------------------------------------------------ deterministic synthetic trees */
/* Integer-hash PRNG, IEEE-only arithmetic: bit-identical on every host. */

typedef struct mnv_synth_random_params {
    int32_t depth;          /* chunk levels; finest voxel 2^-depth */
    int32_t format;         /* MNV_FORMAT_* */
    int32_t basis_dim;      /* SH: 1,4,9,16,25; RGBA: -1 */
    float refine_prob;      /* probability a non-finest voxel is refined */
    float empty_prob;       /* probability a leaf has sigma = 0 */
    float sigma_max;        /* dense leaves: sigma ~ U(0, sigma_max) */
    float coef_sd;          /* SH-DC ~ approx N(0, coef_sd^2), higher orders decay by 1/2 per degree */
    float offset[3];
    float scale[3];         /* invradius3 */
    uint64_t seed;
} mnv_synth_random_params;

typedef struct mnv_synth_shell_params {
    int32_t depth;          /* 10 for the headline config */
    int32_t basis_dim;      /* 9 for the headline config (format SH) */
    float radius;           /* 0.35 unit-cube units */
    float half_thickness;   /* 1.5/1024 */
    float sigma_lo, sigma_hi; /* 50, 400 */
    float offset[3];
    float scale[3];
    uint64_t seed;
} mnv_synth_shell_params;

/* "Merged Mega-NeRF" stand-in (BASELINE configs[2]): anisotropic volume with a
 * terrain-like occupied layer x = h(y, z), cut into bricks_y x bricks_z sub-modules with independent seeds. */
typedef struct mnv_synth_terrain_params {
    int32_t depth;
    int32_t basis_dim;
    int32_t bricks_y, bricks_z;  /* 4 x 2 */
    int32_t noise_cells;         /* lattice cells of the value noise per unit length */
    float base, amplitude;       /* height range in unit-cube x: [base, base + amplitude] */
    float thickness;             /* half thickness of the occupied layer, unit-cube units */
    float sigma_lo, sigma_hi;
    float offset[3];
    float scale[3];              /* invradius3, e.g. (0.5, 0.125, 0.125) for a 1 : 4 : 4 world extent */
    uint64_t seed;
} mnv_synth_terrain_params;

int mnv_synth_random_tree(const mnv_synth_random_params *p, mnv_n3tree **out);
int mnv_synth_terrain_tree(const mnv_synth_terrain_params *p, mnv_n3tree **out);
int mnv_synth_shell_tree(const mnv_synth_shell_params *p, mnv_n3tree **out);

#ifdef __cplusplus
}
#endif
#endif /* MNV_H */
