// mnv_accel_capi.hip -- the frame request of the packed layout (render_accel: every argument check, once), launch planning for its kernels
// (launch_accel: ray queues, partition, launch slots), the tile assembly of rank 0, and the C-ABI entry points of include/mnv.h that render
// on an accel.  The kernels themselves: mnv_march_accel_kernel.h (instantiated by mnv_accel_march[_brick|_rays].hip), mnv_guided_fused*.h
// (mnv_accel_fused.hip).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "mnv_accel_launch.h"
#include "mnv_knobs.h"

namespace mnv {

// Per-launch parameters that live in device memory: zeroes the ray-queue heads of every frame and
// stores the camera blocks (handed over by value, so no host staging buffer or copy engine is involved).
constexpr int kStageCams = 32;
struct StageCams {
    CamBlock c[kStageCams];
};
__global__ void stage_launch_kernel(uint32_t *heads, int32_t head_words, CamBlock *dst, const StageCams cams, int32_t count) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < head_words) heads[i] = 0u;
    if (i < count * (int32_t)(sizeof(CamBlock) / 4))
        reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(cams.c)[i];
}

// Visit marks on the packed layout: the march marks the chunk that holds each leaf it steps through; the reference marks every
// chunk of every descent (query_single_from_root, rt_core.cuh:132-134), i.e. those chunks and all their ancestors.  One thread
// per marked chunk walks up the parent words until it meets a chunk that is marked already.
__global__ void close_visit_marks(int32_t *visited, const int32_t *parent, int32_t capacity) {
    const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= capacity || c == 0 || visited[c] == 0) return;
    int32_t p = parent[c] >> 3;
    while (p >= 0 && p < capacity) {
        if (__hip_atomic_load(&visited[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
        visited[p] = 1;
        if (p == 0) break;
        p = parent[p] >> 3;
    }
}

// Rank 0 after the gather: macro tile m of frame f sits at gathered[m % world][f][m / world];
// one thread per pixel, the destination is written row-major (coalesced), the source is read in tile rows.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes: one float RGBA pixel or four RGBA8 pixels
template <typename PIXEL>
__global__ void assemble_tiles_kernel(const PIXEL *__restrict__ gathered, PIXEL *__restrict__ frames, int32_t width, int32_t height,
                                      int32_t tile_w, int32_t tile_h, int32_t macros_x, int32_t j_max, int32_t world, int32_t period, int32_t n_frames) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_frame = (int64_t)width * height;
    if (idx >= per_frame * n_frames) return;
    const int32_t f = (int32_t)(idx / per_frame);
    const int32_t p = (int32_t)(idx - (int64_t)f * per_frame);
    const int32_t y = p / width, x = p - y * width;
    const int32_t mx = x / tile_w, my = y / tile_h;
    uint32_t r, j;
    part_owner_of((uint32_t)(my * macros_x + mx), world, period, r, j);
    const int64_t src = ((((int64_t)r * n_frames + f) * j_max + j) * tile_h + (y - my * tile_h)) * tile_w + (x - mx * tile_w);
    // streamed once: keep these lines from displacing the march's lookup structures in L2
    __builtin_nontemporal_store(__builtin_nontemporal_load(&gathered[src]), &frames[idx]);
}

int32_t partition_local_tiles(mnv_rect tile, mnv_partition part) {
    if (tile.w <= 0 || tile.h <= 0 || !is_partitioned(part)) return is_partitioned(part) ? 0 : 1;
    const int64_t mx = (tile.w + part.tile_w - 1) / part.tile_w, my = (tile.h + part.tile_h - 1) / part.tile_h;
    return (int32_t)part_local_count(mx * my, part.rank, part.world, root_period_of(part));
}

// Tile geometry of a launch, host arithmetic only: the ray tiles (plain frame, ray list) or this rank's macro / micro tiles (partition), the
// tile range of every ray queue and the distance between the frames of a batch.  false: this rank owns no tile of the rectangle.
static bool plan_tiles(AccelLaunch &K, mnv_rect tile, mnv_partition part, int n_frames, bool rays) {
    K.part_rank = part.rank;
    K.part_world = is_partitioned(part) ? part.world : 0;
    K.part_period = root_period_of(part);
    K.n_frames = (uint32_t)n_frames;
    static const int env_wlog = knob_int(KNOB_TILE_WLOG, 3);
    K.tile_wlog = (env_wlog >= 0 && env_wlog <= 6) ? (uint32_t)env_wlog : 3u;
    if (rays) K.tile_wlog = tile.h == 1 ? 6u : 3u;  // a flat ray list: 64 x 1 tiles
    if (!is_partitioned(part)) {
        const uint32_t tile_w = 1u << K.tile_wlog, tile_h = 64u >> K.tile_wlog;
        K.tiles_x = (uint32_t)((tile.w + tile_w - 1) / tile_w);
        const uint32_t tiles_y = (uint32_t)((tile.h + tile_h - 1) / tile_h);
        K.n_tiles = K.tiles_x * tiles_y;
        // contiguous bands of tile rows per queue
        for (int q = 0; q <= kNumQueues; ++q) K.band_begin[q] = (uint32_t)(((uint64_t)tiles_y * q) / kNumQueues) * K.tiles_x;
        // ray images with fewer tile rows than queues (a flat list has one) are split by tile count: whole rows would leave queues empty
        if (rays && tiles_y < (uint32_t)kNumQueues)
            for (int q = 0; q <= kNumQueues; ++q) K.band_begin[q] = (uint32_t)(((uint64_t)K.n_tiles * q) / kNumQueues);
        K.frame_stride_px = (uint32_t)tile.w * (uint32_t)tile.h;
    } else {
        const uint32_t local = (uint32_t)partition_local_tiles(tile, part);
        if (local == 0) return false;
        K.macro_w = (uint32_t)part.tile_w;
        K.macro_h = (uint32_t)part.tile_h;
        K.macros_x = (uint32_t)((tile.w + part.tile_w - 1) / part.tile_w);
        K.micro_x = K.macro_w / 8;
        K.micro_per_macro = K.micro_x * (K.macro_h / 8);
        K.tiles_x = K.micro_x;
        K.n_tiles = local * K.micro_per_macro;
        // contiguous runs of micro tiles (in local macro-tile order) per queue
        for (int q = 0; q <= kNumQueues; ++q) K.band_begin[q] = (uint32_t)(((uint64_t)K.n_tiles * q) / kNumQueues);
        // frames of a batch are j_max = ceil(macro tiles / world) local tiles apart on EVERY rank, so that the
        // per-rank buffers have one shape (what the gather needs) even when the tile count is ragged
        const uint32_t n_macro = K.macros_x * (uint32_t)((tile.h + part.tile_h - 1) / part.tile_h);
        K.frame_stride_px = (uint32_t)part_j_max(n_macro, part.world, root_period_of(part)) * K.macro_w * K.macro_h;
    }
    static const int env_queues = knob_int(KNOB_QUEUES, kNumQueues);
    if (env_queues >= 1 && env_queues < kNumQueues) {
        // diagnostics: fewer, larger queues (queue q of the first env_queues covers 1/env_queues of the tiles)
        const uint32_t total = K.band_begin[kNumQueues];
        for (int q = 0; q <= kNumQueues; ++q)
            K.band_begin[q] = q >= env_queues ? total : (uint32_t)(((uint64_t)total * q) / env_queues);
    }
    return true;
}

static bool march_tracked(const AccelLaunch &K) { return K.split_track || K.sample_track || K.samples || K.visited; }

// Workgroups of a launch: as many per CU as the LDS level and the kernel's register budget admit, and no more wavefronts than there
// are initial 8x8 tiles.
static int grid_blocks(const mnv_accel *accel, const AccelLaunch &K, bool rays) {
    static const int env_bpc = knob_int(KNOB_BLOCKS_PER_CU, 0);
    int blocks_per_cu = K.lds_level >= 5 ? 1 : (K.lds_level == 4 ? 6 : 8);
    if (march_tracked(K) && blocks_per_cu > MNV_TRACK_WAVES) blocks_per_cu = MNV_TRACK_WAVES;
    if (rays && blocks_per_cu > MNV_RAY_WAVES) blocks_per_cu = MNV_RAY_WAVES;
    if (env_bpc > 0) blocks_per_cu = env_bpc;
    int n_blocks = accel->num_cus * blocks_per_cu;
    const uint64_t n_waves_needed = (uint64_t)K.n_tiles * (uint64_t)K.n_frames;  // one initial 8x8 tile per wave
    if ((uint64_t)n_blocks * 4u > n_waves_needed) n_blocks = (int)((n_waves_needed + 3) / 4);
    return n_blocks < 1 ? 1 : n_blocks;
}

// The launch of a validated request: P and cams are what render_accel derived from it (a ray list's `cams` only fills the launch slot).
static int launch_accel(const AccelFrame &R, const FrameParams &P, const CamBlock *cams) {
    const mnv_accel *accel = R.accel;
    const int n_frames = R.n_cams;
    hipStream_t stream = R.stream;
    if (P.tw <= 0 || P.th <= 0 || n_frames <= 0) return 0;
    const bool rays = R.ray_origins != nullptr;
    AccelLaunch K;
    std::memset(static_cast<void *>(&K), 0, sizeof(K));
    K.P = P;
    if (R.split_track || R.sample_track || R.visited || R.samples || R.fused) {
        K.split_track = R.split_track;
        K.sample_track = R.sample_track;
        K.sample_counts = R.sample_counts;
        K.max_depth = R.opt->max_depth;
        K.max_sample_count = R.opt->max_sample_count;
        K.visited = R.visited;
    }
    if (R.samples) {
        K.num_samples = R.num_samples;
        K.samples = R.samples;
        K.cluster_indices = R.cluster_indices;
        K.max_guided_samples = R.opt->max_guided_samples;
        K.samples_dim = R.samples_dim;
        K.need_viewdir = R.opt->need_viewdir ? 1 : 0;
        K.appearance_embedding = R.opt->appearance_embedding;
        for (int i = 0; i < 2; ++i) K.grid_dim[i] = R.grid->grid_dim[i];
        for (int i = 0; i < 3; ++i) {
            K.min_position[i] = R.grid->min_position[i];
            K.range[i] = R.grid->range[i];
        }
    }
    K.fast_colour = !rays && accel->colour_math.load(std::memory_order_relaxed) > 0 ? 1 : 0;  // mnv_accel_set_colour_math: the accel's own setting (two renderers of one process may differ)
    if (!plan_tiles(K, mnv_rect{P.x0, P.y0, P.tw, P.th}, R.part, n_frames, rays)) return 0;
    static const int env_refill = knob_int(KNOB_REFILL_MIN, 0);
    K.refill_min = (env_refill > 0 && n_frames == 1) ? env_refill : 64;  // batches refill whole tiles (a grab must not straddle frames);  // sweep in DESIGN.md: 16 -> 0.606 ms, 32 -> 0.535, 48 -> 0.507, 56 -> 0.504, 64 -> 0.506
    // The per-launch slot bookkeeping is the handle's only mutable state on this path; launches from several host threads
    // (or one thread feeding several streams) serialise here from the slot's acquisition to the record of its event.
    mnv_accel *mut = const_cast<mnv_accel *>(accel);
    std::lock_guard<std::mutex> launch_lock(mut->launch_mutex);
    K.A = accel->view;  // (under the lock: a launching thread never sees a half-written view)
    const int b = (accel->view.format == MNV_FORMAT_SH && accel->view.basis_dim >= 0) ? accel->view.basis_dim : -1;
    static const int env_level = knob_int(KNOB_LDS_LEVEL, -1);
    int lds_level = accel->view.grid_level < 3 ? accel->view.grid_level : 3;  // 2 KB; level 4 (16 KB) measured equal and costs occupancy
    if (env_level >= 1 && env_level <= accel->view.grid_level) lds_level = env_level;
    K.lds_level = lds_level;
    // sample emission and the depth image read no colour rows: one instantiation (BASIS 9) serves every row format
    const bool colourless = K.samples != nullptr || (P.render_depth && !K.split_track && !K.sample_track && !K.visited);
    // Inline cell words / brick records, or the walk over the node words.  An inline cell word / a brick record calls a leaf whose sigma
    // bits are 0 "not dense" without reading it: true for every sigma_thresh >= 0, so a frame with a negative threshold walks.  SH16 / SH25
    // rows are evaluated by the cooperative pass of the march, which has no brick variant (the fused kernels read either).
    const bool brick = K.A.grid2i && !(P.sigma_thresh < 0.f) && (R.fused || b < 16 || colourless);
    if (!brick) {
        K.A.grid2i = nullptr;
        K.A.recs = nullptr;
    }
    // per-launch slot: zeroed queue heads + the camera blocks, written by stage_launch_kernel on the launch stream
    const uint32_t slot = mut->slot_counter.fetch_add(1) % kSlots;
    // a caller that runs more than kSlots launches ahead of the device waits here for the launch that last used the slot
    if (mut->slot_used[slot]) {
        hipError_t es = hipEventSynchronize(mut->slot_done[slot].get());
        if (es != hipSuccess) return (int)es;
    }
    uint8_t *ds = accel->slots_dev.get() + (size_t)slot * kSlotBytes;
    const size_t heads_bytes = (size_t)kNumQueues * 64;  // one head per queue; a queue spans the frames of the batch
    K.queue = reinterpret_cast<uint32_t *>(ds);
    CamBlock *dcams = reinterpret_cast<CamBlock *>(ds + heads_bytes);
    K.cams = dcams;
    for (int first = 0; first < n_frames; first += kStageCams) {
        StageCams sc;
        const int count = n_frames - first < kStageCams ? n_frames - first : kStageCams;
        std::memcpy(sc.c, cams + first, (size_t)count * sizeof(CamBlock));
        const int head_words = first == 0 ? (int)(heads_bytes / 4) : 0;
        const int n_threads = std::max(head_words, count * (int)(sizeof(CamBlock) / 4));
        hipLaunchKernelGGL(stage_launch_kernel, dim3((n_threads + 255) / 256), dim3(256), 0, stream, K.queue, head_words, dcams + first, sc, count);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;

    const int nb_lds = colourless ? 9 : (accel->view.format == MNV_FORMAT_SH && accel->view.basis_dim > 0) ? accel->view.basis_dim : 1;
    // (tracked frames keep one more value per ray in LDS: t_min)
    const size_t lds_bytes = 256 + (nb_lds >= 16 ? 1024 : 0) + (size_t)(nb_lds + 2 + (march_tracked(K) ? 1 : 0)) * 256 * 4 + ((size_t)4 << (3 * lds_level));
    const int n_blocks = grid_blocks(accel, K, rays);
    int rc = attach_diagnostics(mut, K, rays, R.fused != nullptr, n_blocks, stream);
    if (rc) return rc;
    if (rays)
        rc = launch_march_rays(K, R.ray_origins, R.ray_dirs, b, colourless, brick, n_blocks, lds_bytes, stream);
    else if (R.fused)
        rc = launch_fused(accel, K, *R.fused, b, lds_level, (uint64_t)K.n_tiles * (uint64_t)n_frames, stream);
    else
        rc = brick ? launch_march_brick(K, b, colourless, n_blocks, lds_bytes, stream) : launch_march(K, b, colourless, n_blocks, lds_bytes, stream);
    if (rc == 0 && K.visited && R.parent) {
        hipLaunchKernelGGL(close_visit_marks, dim3((unsigned)((accel->view.capacity + 255) / 256)), dim3(256), 0, stream, K.visited, R.parent,
                           accel->view.capacity);
        rc = (int)hipGetLastError();
    }
    if (rc == 0 && R.fused)  // the fault word's pinned mirror follows the frame on its stream (render_accel, mnv_accel_fused_faults)
        rc = (int)hipMemcpyAsync(mut->fault.host.get(), mut->fault.dev.get(), 4, hipMemcpyDeviceToHost, stream);
    if (rc == 0) {
        rc = (int)hipEventRecord(mut->slot_done[slot].get(), stream);
        mut->slot_used[slot] = true;
    }
    return rc;
}

// A spin-wait that the watchdog of guided_fused2_kernel abandoned leaves wrong pixels behind.  The launches are asynchronous, so the
// frame itself cannot answer for it: the NEXT fused call on this accel does, once per fault, and mnv_accel_fused_faults reads the count.
static int report_fused_fault(const mnv_accel *accel) {
    mnv_accel *mut = const_cast<mnv_accel *>(accel);
    std::lock_guard<std::mutex> g(mut->launch_mutex);
    const uint32_t seen = *static_cast<volatile uint32_t *>(mut->fault.host.get());
    if (seen == mut->fault_reported) return MNV_OK;
    const uint32_t n = seen - mut->fault_reported;
    mut->fault_reported = seen;
    fprintf(stderr, "libmnv: %u wavefront(s) of an earlier fused guided-sampling frame on this accel abandoned a spin-wait (watchdog): that frame is wrong\n", n);
    return set_error(MNV_E_FAULT, "an earlier fused guided-sampling frame on this accel ran into the kernel's watchdog and is wrong; mnv_accel_set_fused_kernel(accel, 1) selects the kernel without spin-waits");
}

// Validates a request -- every check of every entry point, before any device call -- and launches it.
static int render_accel(const AccelFrame &request) {
    AccelFrame R = request;
    const mnv_accel *accel = R.accel;
    const mnv_render_options *opt = R.opt;
    const bool samples = R.entry == AccelFrame::kSamples, fused = R.entry == AccelFrame::kFused, rays = R.entry == AccelFrame::kRays;
    if (rays) {
        if (!R.ray_origins || !R.ray_dirs) return set_error(MNV_E_INVALID, "ray origins / directions are null");
        if (!R.rgba && !R.rgba8) return set_error(MNV_E_INVALID, "both outputs are null");
        if (R.ray_width < 1 || R.ray_height < 1) return set_error(MNV_E_INVALID, "a ray image needs width >= 1 and height >= 1");
        if ((int64_t)R.ray_width * (int64_t)R.ray_height > ((int64_t)1 << 28)) return set_error(MNV_E_INVALID, "more than 2^28 rays in one call");
    }
    if (fused && (!accel || !R.cams || !opt || !R.mlp || !R.grid)) return set_error(MNV_E_INVALID, "null argument");
    if (samples && (!opt || !R.num_samples || !R.samples || !R.cluster_indices || !R.grid)) return set_error(MNV_E_INVALID, "null argument");
    if (!opt && R.entry != AccelFrame::kPlain) return set_error(MNV_E_INVALID, "options are null");  // (kPlain: fill_params answers for camera and options)
    if (!accel) return set_error(MNV_E_INVALID, "accel is null");
    if (fused) {
        const int rc = report_fused_fault(accel);
        if (rc) return rc;
    }
    if (R.visited && !R.parent) return set_error(MNV_E_INVALID, "visit marks on the packed layout need the parent array (the ancestors of the marked chunks)");
    const int b = (accel->view.format == MNV_FORMAT_SH && accel->view.basis_dim >= 0) ? accel->view.basis_dim : -1;
    if (samples && R.samples_dim != 4 + (opt->need_viewdir ? 3 : 0) + (opt->appearance_embedding != -1 ? 1 : 0))
        return set_error(MNV_E_INVALID, "samples_dim must be 4 + 3 * need_viewdir + (appearance_embedding != -1)");
    if (fused && opt->render_depth) return set_error(MNV_E_UNSUPPORTED, "the fused guided-sampling frame has no depth mode; use the four-step path");
    if ((samples || fused) && opt->max_guided_samples < 1) return set_error(MNV_E_INVALID, "max_guided_samples must be positive");
    FusedGuided F;
    if (fused) {
        const MlpShape &S = R.mlp->shape;
        if (S.hidden_width != 64 || S.nkk0 > 2)
            return set_error(MNV_E_UNSUPPORTED, "the fused guided-sampling frame runs 64-wide networks with at most 64 encoded inputs; use the four-step path");
        if (S.out_dim != accel->view.data_dim + 1) return set_error(MNV_E_INVALID, "the model's out_dim must be the tree's data_dim + 1 (cuda_renderer.cpp:255-257)");
        if ((S.need_viewdir != 0) != (opt->need_viewdir != 0)) return set_error(MNV_E_INVALID, "options.need_viewdir does not match the model");
        if (S.n_embeddings > 0 && opt->appearance_embedding == -1) return set_error(MNV_E_INVALID, "the model needs an appearance embedding");
        if (!(b == -1 || b == 1 || b == 4 || b == 9 || b == 16))
            return set_error(MNV_E_UNSUPPORTED, "the fused guided-sampling frame supports RGBA and SH1/4/9/16 trees; use the four-step path");
        std::memset(static_cast<void *>(&F), 0, sizeof(F));
        F.S = S;
        F.frags = R.mlp->frags.get();
        F.biases = R.mlp->biases.get();
        F.embeddings = R.mlp->embeddings.get();
        for (int i = 0; i < 2; ++i) F.grid_dim[i] = R.grid->grid_dim[i];
        for (int i = 0; i < 3; ++i) {
            F.min_position[i] = R.grid->min_position[i];
            F.range[i] = R.grid->range[i];
        }
        F.max_guided_samples = opt->max_guided_samples;
        F.appearance_embedding = opt->appearance_embedding;
        static const int env_batch = knob_int(KNOB_FUSED_BATCH_MIN, kFW);
        F.batch_min = env_batch < 1 ? 1 : (env_batch > kFW ? kFW : env_batch);
        F.sample_counter = R.sample_counter;
        F.diag = accel->fused_diag.load(std::memory_order_relaxed);
        static const int env_switch = knob_int(KNOB_F2_SWITCH_MIN, 32);
        F.switch_min = env_switch;
        R.fused = &F;
    }
    // Sample emission writes no image, and in the fused frame the composite of the network's results adds the image under the volume with
    // weight 1 - out[3] = 0 (render_nerf_results_kernel leaves out[3] at 1, renderer_kernel.cu:316, composite_and_write :224-234): both stop
    // at the pixel's t_max (get_samples_from_voxels_kernel, :354-357) and neither reads rgba8_init
    if (samples || fused) R.inputs.rgba8_init = nullptr;
    mnv_camera shape = {};
    if (rays) {
        if (!(b == -1 || b == 1 || b == 4 || b == 9 || b == 16 || b == 25))
            return set_error(MNV_E_UNSUPPORTED, "the ray march serves RGBA and SH1/4/9/16/25 rows");
        shape.width = R.ray_width;  // (fill_params wants an image size; the march reads no camera)
        shape.height = R.ray_height;
        shape.fx = shape.fy = 1.f;
        R.cams = &shape;
        R.n_cams = 1;
        R.tile = mnv_rect{0, 0, R.ray_width, R.ray_height};
    }
    if (!R.cams || R.n_cams < 1 || R.n_cams > MNV_MAX_BATCH) return set_error(MNV_E_INVALID, "need 1 .. MNV_MAX_BATCH cameras");
    const mnv_partition &part = R.part;
    if (is_partitioned(part) && (part.rank < 0 || part.rank >= part.world || part.tile_w < 8 || part.tile_h < 8 ||
                           part.tile_w % 8 || part.tile_h % 8 || part.root_period < 0 || part.root_period == 1))
        return set_error(MNV_E_INVALID, "partition needs 0 <= rank < world, macro tiles that are multiples of 8 pixels and root_period 0 or >= 2");
    for (int i = 1; i < R.n_cams; ++i)
        if (R.cams[i].width != R.cams[0].width || R.cams[i].height != R.cams[0].height)
            return set_error(MNV_E_INVALID, "all cameras of a batch must have the same image size");
    FrameParams P;
    std::memset(&P, 0, sizeof(P));
    int rc = fill_params(P, &R.cams[0], opt, R.tile);
    if (rc) return rc;
    // pixel indices of a launch are 32 bits wide (frame f starts at f * pixels per frame)
    if ((uint64_t)(R.tile.w > 0 ? R.tile.w : 0) * (uint64_t)(R.tile.h > 0 ? R.tile.h : 0) * (uint64_t)R.n_cams > 0xffffffffull)
        return set_error(MNV_E_UNSUPPORTED, "more than 2^32 pixels in one launch: render fewer frames per call");
    std::memcpy(P.offset, R.xform ? R.xform : accel->view.offset, sizeof(P.offset));
    std::memcpy(P.scale, R.xform ? R.xform + 3 : accel->view.scale, sizeof(P.scale));
    P.rgba = R.rgba;
    P.rgba8 = R.rgba8;
    P.tmax_px = R.inputs.tmax_px;
    P.rgba8_init = R.inputs.rgba8_init;
    CamBlock blocks[MNV_MAX_BATCH];
    std::memset(&blocks[0], 0, sizeof(blocks[0]));
    for (int i = 0; i < R.n_cams && !rays; ++i) {
        fill_camera(blocks[i], &R.cams[i]);
        fill_origin(blocks[i], P.offset, P.scale);
    }
    rc = launch_accel(R, P, blocks);
    if (rc == kUnsupportedBasis) return set_error(MNV_E_UNSUPPORTED, "unsupported basis_dim for the accel path");
    return check_hip((hipError_t)rc, rays ? "march_accel_kernel (rays)" : "march_accel_kernel");
}

// a one-camera request of `entry`'s family (inputs NULL: offscreen)
static AccelFrame frame_on(AccelFrame::Entry entry, const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                           const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, void *hip_stream) {
    AccelFrame R;
    R.entry = entry;
    R.accel = accel;
    R.cams = cam;
    R.opt = opt;
    R.tile = tile;
    if (inputs) R.inputs = *inputs;
    R.rgba = rgba_out;
    R.rgba8 = rgba8_out;
    R.stream = (hipStream_t)hip_stream;
    return R;
}

static AccelFrame &with_trackers(AccelFrame &R, float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited = nullptr,
                                 const int32_t *parent = nullptr) {
    R.split_track = split_track;
    R.sample_track = sample_track;
    R.sample_counts = sample_counts;
    R.visited = visited;
    R.parent = parent;
    return R;
}

static void with_samples(AccelFrame &R, int16_t *num_samples, float *samples, int32_t samples_dim, int16_t *cluster_indices, const mnv_cluster_grid *grid) {
    R.num_samples = num_samples;
    R.samples = samples;
    R.samples_dim = samples_dim;
    R.cluster_indices = cluster_indices;
    R.grid = grid;
}

static AccelFrame &with_network(AccelFrame &R, const mnv_mlp *mlp, const mnv_cluster_grid *grid, unsigned long long *sample_counter) {
    R.mlp = mlp;
    R.grid = grid;
    R.sample_counter = sample_counter;
    return R;
}

int render_accel_for_tree(const mnv_accel *accel, const mnv_tree_view *tree, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                          const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track,
                          hipStream_t stream) {
    float xform[6];
    std::memcpy(xform, tree->offset, sizeof(tree->offset));
    std::memcpy(xform + 3, tree->scale, sizeof(tree->scale));
    AccelFrame R = frame_on(AccelFrame::kPlain, accel, cam, opt, tile, inputs, rgba_out, rgba8_out, (void *)stream);
    R.xform = xform;
    // the refinement trackers (the reference passes them with every call, cuda_renderer.cpp:141-142) take the voxels' sample counts from the CALL's view
    return render_accel(with_trackers(R, split_track, sample_track, tree->sample_counts));
}

}  // namespace mnv

using namespace mnv;

extern "C" {

int32_t mnv_partition_local_tiles(mnv_rect tile, mnv_partition part) { return partition_local_tiles(tile, part); }

int mnv_accel_set_colour_math(mnv_accel *accel, int mode) {
    if (!accel) return set_error(MNV_E_INVALID, "accel is null");
    accel->colour_math.store(mode > 0 ? 1 : 0, std::memory_order_relaxed);
    return MNV_OK;
}

int mnv_accel_set_fused_kernel(mnv_accel *accel, int version) {
    if (!accel) return set_error(MNV_E_INVALID, "accel is null");
    accel->fused_kernel.store(version == 1 || version == 2 ? version : 0, std::memory_order_relaxed);
    return MNV_OK;
}

int mnv_accel_set_fused_diag(mnv_accel *accel, unsigned long long *words32) {
    if (!accel) return set_error(MNV_E_INVALID, "accel is null");
    accel->fused_diag.store(words32, std::memory_order_relaxed);
    return MNV_OK;
}

int mnv_accel_fused_faults(const mnv_accel *accel, uint32_t *count_out) {
    if (!accel || !count_out) return set_error(MNV_E_INVALID, "null argument");
    uint32_t v = 0;
    const int rc = check_hip(hipMemcpy(&v, accel->fault.dev.get(), 4, hipMemcpyDeviceToHost), "read fault word");  // waits for the device
    if (rc) return rc;
    *count_out = v;
    return MNV_OK;
}

int mnv_assemble_tiles(const void *gathered, void *frames, int32_t width, int32_t height, mnv_partition part, int32_t n_frames,
                       int32_t bytes_per_pixel, void *hip_stream) {
    if (!gathered || !frames || width < 1 || height < 1 || n_frames < 1 || part.world < 1 || part.tile_w < 8 || part.tile_h < 8 ||
        part.tile_w % 8 || part.tile_h % 8)
        return set_error(MNV_E_INVALID, "invalid tile-assembly arguments");
    if (bytes_per_pixel != 4 && bytes_per_pixel != 16) return set_error(MNV_E_UNSUPPORTED, "pixels are RGBA8 (4 bytes) or float RGBA (16 bytes)");
    const int32_t macros_x = (width + part.tile_w - 1) / part.tile_w, macros_y = (height + part.tile_h - 1) / part.tile_h;
    if (part.root_period < 0) return set_error(MNV_E_INVALID, "root_period must be 0 or >= 2");
    const int32_t period = root_period_of(part);
    const int32_t j_max = (int32_t)part_j_max((int64_t)macros_x * macros_y, part.world, period);
    hipStream_t stream = (hipStream_t)hip_stream;
    static const bool env_narrow = knob_set(KNOB_ASSEMBLE_NARROW);  // diagnostics: one RGBA8 pixel per thread
    if (bytes_per_pixel == 4 && width % 4 == 0 && !env_narrow) {
        // RGBA8: tile rows and frame rows are contiguous runs of pixels and tile_w is a multiple of 8, so the same index arithmetic
        // holds in units of four pixels: 16 bytes per thread instead of 4 (rank 0 runs this beside its march on the few compute
        // units the march leaves free)
        const int64_t n4 = (int64_t)(width / 4) * height * n_frames;
        hipLaunchKernelGGL(assemble_tiles_kernel<u32x4>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, static_cast<const u32x4 *>(gathered),
                           static_cast<u32x4 *>(frames), width / 4, height, part.tile_w / 4, part.tile_h, macros_x, j_max, part.world, period, n_frames);
        return check_hip(hipGetLastError(), "assemble_tiles_kernel");
    }
    const int64_t n = (int64_t)width * height * n_frames;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (bytes_per_pixel == 4)
        hipLaunchKernelGGL(assemble_tiles_kernel<uint32_t>, grid, block, 0, stream, static_cast<const uint32_t *>(gathered), static_cast<uint32_t *>(frames),
                           width, height, part.tile_w, part.tile_h, macros_x, j_max, part.world, period, n_frames);
    else
        hipLaunchKernelGGL(assemble_tiles_kernel<u32x4>, grid, block, 0, stream, static_cast<const u32x4 *>(gathered), static_cast<u32x4 *>(frames), width,
                           height, part.tile_w, part.tile_h, macros_x, j_max, part.world, period, n_frames);
    return check_hip(hipGetLastError(), "assemble_tiles_kernel");
}

int mnv_render_voxels_accel(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt,
                            mnv_rect tile, float *rgba_out, uint8_t *rgba8_out, void *hip_stream) {
    return render_accel(frame_on(AccelFrame::kPlain, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream));
}

int mnv_render_voxels_accel_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt,
                                 mnv_rect tile, mnv_partition part, float *rgba_out, uint8_t *rgba8_out,
                                 void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kPlain, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    R.part = part;
    return render_accel(R);
}

int mnv_render_voxels_accel_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                               const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, void *hip_stream) {
    return render_accel(frame_on(AccelFrame::kPlain, accel, cam, opt, tile, inputs, rgba_out, rgba8_out, hip_stream));
}

int mnv_render_rays_accel(const mnv_accel *accel, const float *origins, const float *dirs, int32_t width, int32_t height,
                          const mnv_render_options *opt, const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kRays, accel, nullptr, opt, mnv_rect{}, inputs, rgba_out, rgba8_out, hip_stream);
    R.ray_origins = origins;
    R.ray_dirs = dirs;
    R.ray_width = width;
    R.ray_height = height;
    return render_accel(R);
}

int mnv_render_voxels_accel_batch(const mnv_accel *accel, const mnv_camera *cams, int32_t n_cams,
                                  const mnv_render_options *opt, mnv_rect tile, mnv_partition part, float *rgba_out,
                                  uint8_t *rgba8_out, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kPlain, accel, cams, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    R.n_cams = n_cams;
    R.part = part;
    return render_accel(R);
}

int mnv_render_voxels_accel_track(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt,
                                  mnv_rect tile, float *rgba_out, uint8_t *rgba8_out, float *split_track,
                                  float *sample_track, const int16_t *sample_counts, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kTracked, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts));
}

int mnv_render_voxels_accel_visit(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, float *rgba_out,
                                  uint8_t *rgba8_out, float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited,
                                  const int32_t *parent, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kTracked, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts, visited, parent));
}

int mnv_render_voxels_accel_visit_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                     const mnv_frame_inputs *inputs, float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track,
                                     const int16_t *sample_counts, int32_t *visited, const int32_t *parent, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kTracked, accel, cam, opt, tile, inputs, rgba_out, rgba8_out, hip_stream);
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts, visited, parent));
}

int mnv_render_voxels_accel_visit_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, mnv_partition part,
                                       float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track, const int16_t *sample_counts,
                                       int32_t *visited, const int32_t *parent, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kTracked, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    R.part = part;
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts, visited, parent));
}

int mnv_get_samples_from_voxels_accel_visit_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                               const mnv_frame_inputs *inputs, float *split_track, float *sample_track, const int16_t *sample_counts,
                                               int32_t *visited, const int32_t *parent, int16_t *num_samples, float *samples, int32_t samples_dim,
                                               int16_t *cluster_indices, const mnv_cluster_grid *grid, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kSamples, accel, cam, opt, tile, inputs, nullptr, nullptr, hip_stream);
    with_samples(R, num_samples, samples, samples_dim, cluster_indices, grid);
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts, visited, parent));
}

int mnv_get_samples_from_voxels_accel_visit(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                            float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited,
                                            const int32_t *parent, int16_t *num_samples, float *samples, int32_t samples_dim,
                                            int16_t *cluster_indices, const mnv_cluster_grid *grid, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kSamples, accel, cam, opt, tile, nullptr, nullptr, nullptr, hip_stream);
    with_samples(R, num_samples, samples, samples_dim, cluster_indices, grid);
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts, visited, parent));
}

int mnv_get_samples_from_voxels_accel(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                      float *split_track, float *sample_track, const int16_t *sample_counts, int16_t *num_samples,
                                      float *samples, int32_t samples_dim, int16_t *cluster_indices, const mnv_cluster_grid *grid,
                                      void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kSamples, accel, cam, opt, tile, nullptr, nullptr, nullptr, hip_stream);
    with_samples(R, num_samples, samples, samples_dim, cluster_indices, grid);
    return render_accel(with_trackers(R, split_track, sample_track, sample_counts));
}

int mnv_render_guided_fused(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, const mnv_mlp *mlp,
                            const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out, unsigned long long *sample_counter,
                            void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kFused, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    return render_accel(with_network(R, mlp, grid, sample_counter));
}

int mnv_render_guided_fused_track_ex(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                                     const mnv_frame_inputs *inputs, const mnv_mlp *mlp, const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out,
                                     float *split_track, float *sample_track, const int16_t *sample_counts, int32_t *visited, const int32_t *parent,
                                     unsigned long long *sample_counter, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kFused, accel, cam, opt, tile, inputs, rgba_out, rgba8_out, hip_stream);
    with_trackers(R, split_track, sample_track, sample_counts, visited, parent);
    return render_accel(with_network(R, mlp, grid, sample_counter));
}

int mnv_render_guided_fused_track(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, const mnv_mlp *mlp,
                                  const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out, float *split_track, float *sample_track,
                                  const int16_t *sample_counts, int32_t *visited, const int32_t *parent, unsigned long long *sample_counter,
                                  void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kFused, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    with_trackers(R, split_track, sample_track, sample_counts, visited, parent);
    return render_accel(with_network(R, mlp, grid, sample_counter));
}

int mnv_render_guided_fused_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, mnv_partition part,
                                 const mnv_mlp *mlp, const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out,
                                 unsigned long long *sample_counter, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kFused, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    R.part = part;
    return render_accel(with_network(R, mlp, grid, sample_counter));
}

int mnv_render_guided_fused_track_part(const mnv_accel *accel, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, mnv_partition part,
                                       const mnv_mlp *mlp, const mnv_cluster_grid *grid, float *rgba_out, uint8_t *rgba8_out, float *split_track,
                                       float *sample_track, const int16_t *sample_counts, int32_t *visited, const int32_t *parent,
                                       unsigned long long *sample_counter, void *hip_stream) {
    AccelFrame R = frame_on(AccelFrame::kFused, accel, cam, opt, tile, nullptr, rgba_out, rgba8_out, hip_stream);
    R.part = part;
    with_trackers(R, split_track, sample_track, sample_counts, visited, parent);
    return render_accel(with_network(R, mlp, grid, sample_counter));
}

}  // extern "C"
