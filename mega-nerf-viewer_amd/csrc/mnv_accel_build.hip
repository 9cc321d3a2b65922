// mnv_accel_build.hip -- the packed layout ("accel", mnv_accel.h) is derived from the reference's arrays here: chunk depths, node words,
// colour rows, the two lookup grids; mnv_accel_create / _rebuild / _destroy.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "mnv_accel_launch.h"
#include "mnv_knobs.h"

namespace mnv {

// ------------------------------------------------------------------ accel build kernels

// Level-synchronous depth propagation: depth[child chunk] = depth[chunk] + 1.
__global__ void accel_depth_pass(const int32_t *child, int32_t *depth, int32_t capacity, int32_t level,
                                 int32_t *changed) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (int64_t)capacity * 8) return;
    const int32_t c = (int32_t)(v >> 3);
    if (depth[c] != level) return;
    const int32_t skip = child[v];
    if (skip != 0) {
        const int64_t t = (int64_t)c + skip;
        if (t >= 0 && t < capacity) {
            depth[t] = level + 1;
            *changed = 1;
        }
    }
}

__global__ void accel_pack_nodes(const int32_t *child, const uint16_t *data, const int32_t *depth,
                                 uint32_t *nodes, int32_t capacity, int32_t data_dim) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (int64_t)capacity * 8) return;
    const int32_t c = (int32_t)(v >> 3);
    const int32_t skip = child[v];
    if (skip != 0) {
        nodes[v] = (uint32_t)(c + skip);
    } else {
        const uint32_t d = (uint32_t)depth[c] & 0x7fu;
        nodes[v] = kLeafBit | (d << 16) | (uint32_t)data[v * data_dim + data_dim - 1];
    }
}

// rows[v] = 3 channel blocks of chan_halfs binary16 each (the basis_dim coefficients of the channel,
// zero padded to a multiple of 8 B); one thread per (voxel, channel)
__global__ void accel_pack_rows(const uint16_t *data, uint16_t *rows, int64_t nvox, int32_t data_dim,
                                int32_t per_chan, int32_t chan_halfs, int32_t row_halfs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox * 3) return;
    const int64_t v = i / 3;
    const int32_t c = (int32_t)(i % 3);
    const uint16_t *src = data + v * data_dim + c * per_chan;
    uint16_t *dst = rows + v * row_halfs + c * chan_halfs;
    for (int32_t k = 0; k < chan_halfs; ++k) dst[k] = k < per_chan ? src[k] : (uint16_t)0;
    if (c == 2) {
        // the half behind the three channel blocks carries the voxel's sigma (every format has it spare): a dense sample found through a
        // brick record reads it with its colours instead of a node word
        rows[v * row_halfs + 3 * chan_halfs] = data[v * data_dim + data_dim - 1];
        for (int32_t k = 3 * chan_halfs + 1; k < row_halfs; ++k) rows[v * row_halfs + k] = 0;
    }
}

// grid[(ix*G + iy)*G + iz] = word of the voxel of depth <= L that covers cell (ix,iy,iz)
__global__ void accel_build_grid(const uint32_t *nodes, uint32_t *grid, uint32_t *grid_vox, int32_t L) {
    const int32_t G = 1 << L;
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * G * G) return;
    const int32_t iz = i & (G - 1), iy = (i >> L) & (G - 1), ix = i >> (2 * L);
    uint32_t chunk = 0, word = 0, vox = 0;
    for (int32_t l = 1; l <= L; ++l) {
        const int32_t s = L - l;
        const int32_t cidx = (((ix >> s) & 1) << 2) | (((iy >> s) & 1) << 1) | ((iz >> s) & 1);
        vox = chunk * 8u + (uint32_t)cidx;
        word = nodes[vox];
        if (word & kLeafBit) break;
        chunk = word;
    }
    grid[i] = word;
    grid_vox[i] = vox;  // voxel index of the covering leaf (meaningful when `word` is a leaf)
}

// grid2[grid2_index(c)] = word of the voxel of depth <= L2 covering cell c, grid2_vox = its voxel index
__global__ void accel_build_grid2(const uint32_t *nodes, uint32_t *grid2, uint32_t *grid2_vox, int32_t L2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // natural (x-major) cell number
    const uint32_t G = 1u << L2;
    if (i >= (uint64_t)G * G * G) return;
    const uint32_t iz = i & (G - 1), iy = (i >> L2) & (G - 1), ix = i >> (2 * L2);
    uint32_t chunk = 0, word = 0, vox = 0;
    for (int32_t l = 1; l <= L2; ++l) {
        const int32_t s = L2 - l;
        const uint32_t cidx = (((ix >> s) & 1u) << 2) | (((iy >> s) & 1u) << 1) | ((iz >> s) & 1u);
        vox = chunk * 8u + cidx;
        word = nodes[vox];
        if (word & kLeafBit) break;
        chunk = word;
    }
    const uint32_t o = grid2_index(ix, iy, iz, L2);
    grid2[o] = word;
    grid2_vox[o] = vox;
}

// grid2i = grid2 with the last level folded into the words of the cells whose chunk holds eight leaves (mnv_accel.h); one thread per cell
__global__ void accel_build_grid2i(const uint32_t *nodes, const uint32_t *grid2, uint32_t *grid2i, int64_t cells, uint32_t inline_base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    grid2i[i] = inline_cell_word(nodes, grid2[i], inline_base);
}

__global__ void accel_min_chunk_of_depth(const int32_t *depth, int32_t capacity, int32_t d, int32_t *out) {
    const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < capacity && depth[c] == d) atomicMin(out, c);
}

int min_chunk_of_depth(const int32_t *depth, int32_t capacity, int32_t d, int32_t *scratch, hipStream_t stream, uint32_t *out) {
    int rc;
    int32_t h = capacity;
    if ((rc = check_hip(hipMemcpyAsync(scratch, &h, 4, hipMemcpyHostToDevice, stream), "seed min chunk"))) return rc;
    hipLaunchKernelGGL(accel_min_chunk_of_depth, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, stream, depth, capacity, d, scratch);
    if ((rc = check_hip(hipMemcpyAsync(&h, scratch, 4, hipMemcpyDeviceToHost, stream), "read min chunk"))) return rc;
    if ((rc = check_hip(hipStreamSynchronize(stream), "min chunk of depth"))) return rc;
    *out = (uint32_t)h;
    return MNV_OK;
}

// what the inline words and records cover (mnv_accel_lookup_coverage): [0] non-leaf cells of the second grid, [1] of them inline, [2] of them NOT
// inline although their chunk holds eight leaves (its number lies outside the 22-bit field), [3] chunks of depth L2 + 1 (= brick records in use)
__global__ void accel_count_coverage(const uint32_t *nodes, const uint32_t *grid2, const uint32_t *grid2i, int64_t cells, unsigned long long *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const uint32_t w = grid2[i];
    if (w & kLeafBit) return;
    // (a chunk is named by exactly one cell of level L2: [0] also counts the chunks of depth L2 + 1)
    atomicAdd(&out[0], 1ull);
    if (grid2i && (grid2i[i] & kInlineBit)) {
        atomicAdd(&out[1], 1ull);
    } else {
        bool leaves = true;
        for (int s = 0; s < 8; ++s) leaves = leaves && (nodes[(int64_t)w * 8 + s] & kLeafBit) != 0u;
        if (leaves) atomicAdd(&out[2], 1ull);
    }
}

// brick record of every chunk c of depth L2 + 1 (layout: mnv_accel.h); one thread per (chunk, voxel s1)
__global__ void accel_build_recs(const uint32_t *nodes, const int32_t *depth, uint2 *recs, int32_t capacity, int32_t L2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)capacity * 8) return;
    if (depth[i >> 3] != L2 + 1) return;
    recs[i] = brick_record_entry(nodes, i);
}

void launch_build_recs(const uint32_t *nodes, const int32_t *depth, uint2 *recs, int32_t capacity, int32_t L2, hipStream_t stream) {
    const int64_t n = (int64_t)capacity * 8;
    hipLaunchKernelGGL(accel_build_recs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, nodes, depth, recs, capacity, L2);
}

void launch_build_grid2i(const uint32_t *nodes, const uint32_t *grid2, uint32_t *grid2i, int32_t L2, uint32_t inline_base, hipStream_t stream) {
    const int64_t cells = (int64_t)1 << (3 * L2);
    hipLaunchKernelGGL(accel_build_grid2i, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, nodes, grid2, grid2i, cells, inline_base);
}

void launch_pack_rows(const uint16_t *data, uint16_t *rows, int64_t nvox, int32_t data_dim, int32_t per_chan, int32_t chan_halfs, int32_t row_halfs,
                      hipStream_t stream) {
    hipLaunchKernelGGL(accel_pack_rows, dim3((unsigned)((nvox * 3 + 255) / 256)), dim3(256), 0, stream, data, rows, nvox, data_dim, per_chan, chan_halfs, row_halfs);
}
void launch_build_grid(const uint32_t *nodes, uint32_t *grid, uint32_t *grid_vox, int32_t L, hipStream_t stream) {
    const int64_t cells = (int64_t)1 << (3 * L);
    hipLaunchKernelGGL(accel_build_grid, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, nodes, grid, grid_vox, L);
}
void launch_build_grid2(const uint32_t *nodes, uint32_t *grid2, uint32_t *grid2_vox, int32_t L2, hipStream_t stream) {
    const int64_t cells = (int64_t)1 << (3 * L2);
    hipLaunchKernelGGL(accel_build_grid2, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, nodes, grid2, grid2_vox, L2);
}

// (Re)build every derived array of `a` from the tree: chunk depths, node words, colour rows, lookup grids.  The big arrays
// (nodes, rows, depth) are sized for a->reserved chunks and kept; the grids are reallocated only when their level changes.
int accel_build(mnv_accel *a, const mnv_tree_view *t, hipStream_t stream) {
    int rc = MNV_OK;
    const int b = (t->format == MNV_FORMAT_SH && t->basis_dim >= 0) ? t->basis_dim : -1;
    const int64_t cap = t->capacity, nvox = cap * 8, max_capacity = a->reserved;
    const int row_bytes = row_bytes_for(b);
    int32_t *depth = a->depth.get(), *changed = a->flags.get();
    // chunk depths: root chunk holds depth-1 voxels
    if ((rc = check_hip(hipMemsetAsync(depth, 0, max_capacity * 4, stream), "memset depth"))) return rc;
    const int32_t one = 1;
    if ((rc = check_hip(hipMemcpyAsync(depth, &one, 4, hipMemcpyHostToDevice, stream), "seed depth"))) return rc;
    const unsigned nb = (unsigned)((nvox + 255) / 256);
    int max_depth = 1;
    for (int level = 1; level < 25; ++level) {
        int32_t flag = 0;
        if ((rc = check_hip(hipMemsetAsync(changed, 0, 4, stream), "memset flag"))) return rc;
        hipLaunchKernelGGL(accel_depth_pass, dim3(nb), dim3(256), 0, stream, t->child, depth, t->capacity, level, changed);
        if ((rc = check_hip(hipMemcpyAsync(&flag, changed, 4, hipMemcpyDeviceToHost, stream), "read flag"))) return rc;
        if ((rc = check_hip(hipStreamSynchronize(stream), "accel_depth_pass"))) return rc;
        if (!flag) break;
        max_depth = level + 1;
    }
    if (max_depth > 23) return set_error(MNV_E_UNSUPPORTED, "accel supports trees up to depth 23; use mnv_render_voxels");
    hipLaunchKernelGGL(accel_pack_nodes, dim3(nb), dim3(256), 0, stream, t->child, t->data, depth, a->nodes.get(), t->capacity, t->data_dim);
    hipLaunchKernelGGL(accel_pack_rows, dim3((unsigned)((nvox * 3 + 255) / 256)), dim3(256), 0, stream, t->data,
                       reinterpret_cast<uint16_t *>(a->rows.get()), nvox, t->data_dim, b > 0 ? b : 1, chan_bytes_for(b) / 2,
                       row_bytes / 2);
    int L = max_depth < kMaxGridLevel ? max_depth : kMaxGridLevel;
    const int64_t gcells = (int64_t)1 << (3 * L);
    if (!a->grid || a->view.grid_level != L) {
        a->grid.reset();
        a->grid_vox.reset();
        if ((rc = check_hip(a->grid.alloc(gcells), "hipMalloc(grid)"))) return rc;
        if ((rc = check_hip(a->grid_vox.alloc(gcells), "hipMalloc(grid_vox)"))) return rc;
    }
    hipLaunchKernelGGL(accel_build_grid, dim3((unsigned)((gcells + 255) / 256)), dim3(256), 0, stream, a->nodes.get(), a->grid.get(), a->grid_vox.get(), L);
    // second lookup grid at level L2 <= min(max_depth - 1, 9): 8^L2 words per array (64 MiB at level 8,
    // 512 MiB at level 9).  Pick the deepest level whose two arrays stay below max(128 MiB, 2 x the packed
    // tree): HBM is 288 GB, and every level moved into the grid removes a dependent load from deep steps
    // (cfg2: level 8 -> 0.506 ms/frame, level 9 -> 0.471 ms/frame).
    int L2 = max_depth - 1 < kMaxGrid2Level ? max_depth - 1 : kMaxGrid2Level;
    const int64_t budget = std::max<int64_t>((int64_t)128 << 20, 2 * (nvox * 4 + nvox * row_bytes));
    while (L2 > L && ((int64_t)8 << (3 * L2)) > budget) --L2;
    static const int env_l2 = knob_int(KNOB_GRID2_LEVEL, -1);
    if (env_l2 >= 0 && env_l2 <= kMaxGrid2Level && env_l2 < max_depth) L2 = env_l2;
    if (L2 <= L || L2 < 2) L2 = 0;
    int64_t g2cells = 0;
    if (a->grid2 && a->view.grid2_level != L2) {
        a->grid2.reset();
        a->grid2_vox.reset();
        a->grid2i.reset();
    }
    if (L2 > 0) {
        g2cells = (int64_t)1 << (3 * L2);
        if (!a->grid2) {
            if ((rc = check_hip(a->grid2.alloc(g2cells), "hipMalloc(grid2)"))) return rc;
            if ((rc = check_hip(a->grid2_vox.alloc(g2cells), "hipMalloc(grid2_vox)"))) return rc;
        }
        hipLaunchKernelGGL(accel_build_grid2, dim3((unsigned)((g2cells + 255) / 256)), dim3(256), 0, stream, a->nodes.get(), a->grid2.get(), a->grid2_vox.get(), L2);
    }
    // What frames read instead of node words (mnv_accel_refresh patches both with the tree edit, a prune derives them again):
    //  * grid2i: grid2 with the last level folded into the words of the cells whose chunk holds eight leaves -- a depth-10 tree (cfg2, L2 = 9)
    //    then never reads a node word: LDS grid -> grid2i [-> row];
    //  * brick records: the two levels below the grid from one 64-byte record per depth-(L2 + 1) chunk, for trees that have two such levels
    //    (depth >= L2 + 2; cfg3): LDS grid -> grid2i -> record [-> row] instead of LDS grid -> grid2 -> node -> node [-> row].
    static const int env_bricks = knob_int(KNOB_BRICK_LEVELS, 3);  // bit 0: inline cell words, bit 1: records
    const bool want_inline = (env_bricks & 1) && L2 > 0, want_recs = (env_bricks & 2) && want_inline && max_depth >= L2 + 2;
    if (want_inline) {
        if (!a->grid2i && (rc = check_hip(a->grid2i.alloc(g2cells), "hipMalloc(grid2i)"))) return rc;
        uint32_t base = 0;
        if ((rc = min_chunk_of_depth(depth, t->capacity, L2 + 1, a->flags.get() + 6, stream, &base))) return rc;
        a->view.inline_base = base;
        launch_build_grid2i(a->nodes.get(), a->grid2.get(), a->grid2i.get(), L2, base, stream);
    } else {
        a->grid2i.reset();
    }
    if (want_recs) {
        if (!a->recs && (rc = check_hip(a->recs.alloc((size_t)max_capacity * 8), "hipMalloc(brick records)"))) return rc;
        launch_build_recs(a->nodes.get(), depth, a->recs.get(), t->capacity, L2, stream);
    } else {
        a->recs.reset();
    }
    if ((rc = check_hip(hipGetLastError(), "accel build launch"))) return rc;
    if ((rc = check_hip(hipStreamSynchronize(stream), "accel build"))) return rc;
    a->publish_view(want_inline, want_recs);
    a->view.grid_level = L;
    a->view.grid2_level = L2;
    a->view.max_depth = max_depth;
    a->view.row_bytes = row_bytes;
    a->view.sigma_off = 3 * chan_bytes_for(b);
    for (int i = 0; i < 3; ++i) {
        a->view.offset[i] = t->offset[i];
        a->view.scale[i] = t->scale[i];
    }
    a->view.data_dim = t->data_dim;
    a->view.basis_dim = t->basis_dim;
    a->view.format = t->format;
    a->view.capacity = t->capacity;
    a->built_capacity = cap;
    a->bytes = a->frame_bytes();
    return MNV_OK;
}

}  // namespace mnv

using namespace mnv;

extern "C" {

int mnv_accel_create(const mnv_tree_view *t, void *hip_stream, mnv_accel **out) {
    return mnv_accel_create_reserved(t, t ? t->capacity : 0, hip_stream, out);
}

int mnv_accel_create_reserved(const mnv_tree_view *t, int64_t max_capacity, void *hip_stream, mnv_accel **out) {
    if (!t || !out) return set_error(MNV_E_INVALID, "null argument");
    if (max_capacity < t->capacity) return set_error(MNV_E_INVALID, "max_capacity is smaller than the tree");
    if (t->N != 2) return set_error(MNV_E_UNSUPPORTED, "accel needs N == 2");
    if (!t->data || !t->child || t->capacity < 1 || t->data_dim < 1) return set_error(MNV_E_INVALID, "invalid device tree view");
    const int b = (t->format == MNV_FORMAT_SH && t->basis_dim >= 0) ? t->basis_dim : -1;
    if (!(b == -1 || b == 1 || b == 4 || b == 9 || b == 16 || b == 25))
        return set_error(MNV_E_UNSUPPORTED, "accel supports RGBA and SH1/4/9/16/25 rows; use mnv_render_voxels for others");
    if (b >= 0 && t->data_dim != 3 * b + 1) return set_error(MNV_E_UNSUPPORTED, "accel needs data_dim == 3 * basis_dim + 1");
    if (b < 0 && t->data_dim != 4) return set_error(MNV_E_UNSUPPORTED, "accel needs data_dim == 4 for RGBA rows");
    hipStream_t stream = (hipStream_t)hip_stream;
    std::unique_ptr<mnv_accel> a(new mnv_accel());
    int rc = MNV_OK;
    if ((rc = check_hip(hipGetDevice(&a->device), "hipGetDevice"))) return rc;
    hipDeviceProp_t prop;
    if ((rc = check_hip(hipGetDeviceProperties(&prop, a->device), "hipGetDeviceProperties"))) return rc;
    a->num_cus = a->device_cus = prop.multiProcessorCount;

    const int row_bytes = row_bytes_for(b);
    a->reserved = max_capacity;
    if ((rc = check_hip(a->nodes.alloc((size_t)max_capacity * 8), "hipMalloc(nodes)"))) return rc;
    if ((rc = check_hip(a->rows.alloc((size_t)max_capacity * 8 * row_bytes), "hipMalloc(rows)"))) return rc;
    if ((rc = check_hip(a->depth.alloc((size_t)max_capacity), "hipMalloc(depth)"))) return rc;
    if ((rc = check_hip(a->flags.alloc(8), "hipMalloc(flag)"))) return rc;
    if ((rc = alloc_pair(a->fault, 1, "hipMalloc(fault)", "hipHostMalloc(fault)"))) return rc;
    if ((rc = check_hip(hipMemsetAsync(a->fault.dev.get(), 0, 4, stream), "memset fault"))) return rc;
    *a->fault.host.get() = 0u;
    if ((rc = check_hip(a->slots_dev.alloc((size_t)kSlots * kSlotBytes), "hipMalloc(slots)"))) return rc;
    for (int i = 0; i < kSlots; ++i)
        if ((rc = check_hip(a->slot_done[i].create(hipEventDisableTiming), "hipEventCreate(slot)"))) return rc;

    if ((rc = accel_build(a.get(), t, stream))) return rc;
    *out = a.release();
    return MNV_OK;
}

int mnv_accel_rebuild(mnv_accel *a, const mnv_tree_view *t, void *hip_stream) {
    if (!a || !t) return set_error(MNV_E_INVALID, "null argument");
    if (!t->data || !t->child || t->capacity < 1 || t->capacity > a->reserved)
        return set_error(MNV_E_INVALID, "invalid tree view, or the tree outgrew the reserved capacity");
    if (t->data_dim != a->view.data_dim || t->format != a->view.format || t->basis_dim != a->view.basis_dim)
        return set_error(MNV_E_INVALID, "tree view does not match the accel");
    std::lock_guard<std::mutex> view_lock(a->launch_mutex);  // launch_accel copies the view under the same lock
    return accel_build(a, t, (hipStream_t)hip_stream);
}

void mnv_accel_destroy(mnv_accel *a) {
    if (!a) return;
    report_diagnostics(a);
    delete a;
}

size_t mnv_accel_device_bytes(const mnv_accel *a) { return a ? a->bytes : 0; }
int32_t mnv_accel_grid2_level(const mnv_accel *a) { return a ? a->view.grid2_level : -1; }
int32_t mnv_accel_brick_levels(const mnv_accel *a) { return a ? (a->view.recs ? 2 : a->view.grid2i ? 1 : 0) : -1; }

int mnv_accel_lookup_coverage(const mnv_accel *a, int64_t out4[4]) {
    if (!a || !out4) return set_error(MNV_E_INVALID, "null argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (a->view.grid2_level <= 0) return MNV_OK;
    mnv_accel *mut = const_cast<mnv_accel *>(a);
    std::lock_guard<std::mutex> view_lock(mut->launch_mutex);
    Buffer<unsigned long long> dev;
    unsigned long long h[4] = {};
    int rc;
    if ((rc = check_hip(dev.alloc(4), "hipMalloc(coverage)"))) return rc;
    rc = check_hip(hipMemset(dev.get(), 0, sizeof(h)), "memset coverage");
    const int64_t cells = (int64_t)1 << (3 * a->view.grid2_level);
    if (!rc) {
        hipLaunchKernelGGL(accel_count_coverage, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, nullptr, a->nodes.get(), a->grid2.get(), a->view.grid2i, cells, dev.get());
        rc = check_hip(hipMemcpy(h, dev.get(), sizeof(h), hipMemcpyDeviceToHost), "read coverage");  // (the null stream: behind every launch of the device)
    }
    if (rc) return rc;
    out4[0] = (int64_t)h[0];
    out4[1] = (int64_t)h[1];
    out4[2] = (int64_t)h[2];
    out4[3] = a->view.recs ? (int64_t)h[0] : 0;
    return MNV_OK;
}

int mnv_accel_set_cu_budget(mnv_accel *a, int32_t num_cus) {
    if (!a) return set_error(MNV_E_INVALID, "accel is null");
    if (num_cus > a->device_cus) return set_error(MNV_E_INVALID, "the device has fewer compute units");
    a->num_cus = num_cus <= 0 ? a->device_cus : num_cus;
    return MNV_OK;
}

}  // extern "C"
