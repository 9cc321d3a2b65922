// mnv_lod.hip -- levels of detail of a tree: mnv_tree_mip_rows derives every interior voxel's row from its children, bottom-up (the mip
// contract of include/mnv.h), mnv_tree_truncate cuts the tree at a depth and compacts the survivors.  The result is an ordinary N3Tree in the
// reference's array layout: every march kernel renders it unchanged.
//
// Depths: the level walk of mnv_tree_walk.h, whose lists hold (chunk, flat index of the voxel above it).
//
// Rows: one launch per depth, deepest first, a group of 8 .. 64 lanes per chunk of that depth (32 for SH9: two chunks per wavefront).  A
// chunk's eight rows are data_dim aligned 16-byte segments (448 B for SH9).  The group stages them into LDS with 16-byte loads -- the
// halfs of leaf voxels from the input tree, the halfs of interior voxels from data_out, where the launch of the level below left them --
// stores the merged segments to data_out, and then computes the row of the voxel ABOVE the chunk, one column per lane with the eight
// weights and W read from LDS, into data_out.  So every row of the tree is read once and written once; the input tree is never written.
//
// Truncation: the compaction of mnv_tree_walk.h with the depth word as the survivor predicate.
//
// binary16 <-> binary32 as mnv_tree_walk.h has it.  Build flags as everywhere: -ffp-contract=off, correctly rounded division.
#include <hip/hip_runtime.h>

#include <mutex>

#include "mnv_tree_walk.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kWavesPerBlock = 4;

// ---------------------------------------------------------------------------------------------------- rows

// A group of G lanes (a power of two, 8 .. 64, at least data_dim where that is below 64) per list entry (chunk k, voxel above it), 64 / G
// entries per wavefront: rows of k into LDS and data_out, then the row of the voxel above
__global__ void __launch_bounds__(64 * kWavesPerBlock) lod_mip_kernel(const uint16_t *__restrict__ data_in, uint16_t *__restrict__ data_out,
                                                                       const int32_t *__restrict__ child, const int2 *__restrict__ list, int64_t n,
                                                                       int32_t dd, int32_t log2_g) {
    extern __shared__ uint4 lod_lds[];  // [kWavesPerBlock][64 / G][dd] segments
    const int G = 1 << log2_g, per_wave = 64 >> log2_g;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> log2_g, gl = lane & (G - 1);
    const int64_t idx = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * per_wave + grp;
    const bool active = idx < n;
    uint4 *seg = lod_lds + ((size_t)wave * per_wave + grp) * dd;
    const int2 e = active ? list[idx] : make_int2(0, -1);
    const int64_t k = e.x;
    // interior voxels of k: the group's first eight lanes look, the group's byte of the ballot says
    const bool interior = active && gl < 8 && child[k * 8 + gl] != 0;
    const unsigned mask = (unsigned)((__ballot(interior) >> (grp << log2_g)) & 0xffull);
    if (active) {
        const uint4 *in4 = reinterpret_cast<const uint4 *>(data_in) + k * dd;
        uint4 *out4 = reinterpret_cast<uint4 *>(data_out) + k * dd;
        for (int s = gl; s < dd; s += G) {
            mnv::Seg16 a;
            a.v = in4[s];
            if (mask) {
                const int j0 = (8 * s) / dd, j1 = (8 * s + 7) / dd;  // the rows segment s holds halfs of
                unsigned span = 0;
                for (int j = j0; j <= j1; ++j) span |= 1u << j;
                if (mask & span) {
                    mnv::Seg16 b;
                    b.v = out4[s];
                    for (int i = 0; i < 8; ++i)
                        if ((mask >> ((8 * s + i) / dd)) & 1u) a.h[i] = b.h[i];
                }
            }
            seg[s] = a.v;
            out4[s] = a.v;
        }
    }
    __syncthreads();
    if (!active || e.y < 0) return;
    const uint16_t *rows = reinterpret_cast<const uint16_t *>(seg);
    float w[8];
    for (int i = 0; i < 8; ++i) {
        const float sg = mnv::h(rows[i * dd + dd - 1]);
        w[i] = sg > 0.f ? sg : 0.f;
    }
    const float W = ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) + w[7];
    uint16_t *above = data_out + (int64_t)e.y * dd;
    for (int c = gl; c < dd; c += G) {
        uint16_t r = 0;
        if (W != 0.f) {
            if (c == dd - 1) {
                r = mnv::half(W * 0.125f);
            } else {
                float S = w[0] * mnv::h(rows[c]);
                for (int i = 1; i < 8; ++i) S = S + w[i] * mnv::h(rows[i * dd + c]);
                r = mnv::half(S / W);
            }
        }
        above[c] = r;
    }
}

}  // namespace

extern "C" {

int mnv_tree_mip_rows(const mnv_tree_view *tree, uint16_t *data_out, int32_t *chunk_depth_out, int64_t chunks_at_depth[24], void *hip_stream) {
    int rc;
    if (!data_out || !chunks_at_depth) return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: null output");
    if ((rc = mnv::check_view(tree, "mnv_tree_mip_rows"))) return rc;
    const int32_t cap = tree->capacity, dd = tree->data_dim;
    const size_t data_bytes = (size_t)cap * 16 * dd;
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: data_out must be 16-byte aligned");
    if (mnv::overlap(data_out, data_bytes, tree->data, data_bytes))
        return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: data_out must not alias the tree's data (the input tree is never modified)");
    hipStream_t stream = (hipStream_t)hip_stream;
    for (int d = 0; d < 24; ++d) chunks_at_depth[d] = 0;

    mnv::WalkGuard guard;
    mnv::LevelLists L;
    if ((rc = guard.begin(stream))) return rc;
    rc = mnv::walk_levels(tree->child, cap, chunk_depth_out, "mnv_tree_mip_rows", guard, L);
    for (int d = 1; d <= L.levels; ++d) chunks_at_depth[d] = L.size(d);
    if (rc) return rc;
    int log2_g = 3;  // lanes per chunk: 8, 16, 32 or 64, at least data_dim where that is below 64
    while ((1 << log2_g) < dd && log2_g < 6) ++log2_g;
    const int per_block = kWavesPerBlock * (64 >> log2_g);
    const size_t lds = (size_t)per_block * dd * 16;
    for (int d = L.levels; d >= 1; --d) {
        hipLaunchKernelGGL(lod_mip_kernel, dim3(mnv::blocks_for(L.size(d), per_block)), dim3(64 * kWavesPerBlock), lds, stream, tree->data, data_out, tree->child,
                           L.order + L.offset[d], L.size(d), dd, log2_g);
        if ((rc = check_hip(hipGetLastError(), "lod_mip_kernel"))) return rc;
    }
    if (L.offset[L.levels + 1] < cap && (rc = mnv::copy_unreached(tree->data, data_out, L.depth, cap, dd, stream))) return rc;
    return check_hip(hipStreamSynchronize(stream), "mnv_tree_mip_rows");
}

int mnv_tree_truncate(const mnv_tree_view *tree, const int32_t *chunk_depth, int32_t max_depth, int32_t new_capacity, int32_t *child_out, uint16_t *data_out,
                      int32_t *parent_out, int16_t *sample_counts_out, void *hip_stream) {
    int rc;
    if (!chunk_depth || !child_out || !data_out) return set_error(MNV_E_INVALID, "mnv_tree_truncate: null chunk depths / output");
    if ((rc = mnv::check_view(tree, "mnv_tree_truncate"))) return rc;
    if (max_depth < 1) return set_error(MNV_E_INVALID, "mnv_tree_truncate: max_depth must be at least 1");
    if (new_capacity < 1 || new_capacity > tree->capacity) return set_error(MNV_E_INVALID, "mnv_tree_truncate: new_capacity outside [1, capacity]");
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_tree_truncate: data_out must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    int dev = -1;
    if ((rc = mnv::current_device(&dev))) return rc;
    std::lock_guard<std::mutex> lock(mnv::stream_scratch_mutex());
    return mnv::compact_tree(tree, mnv::DepthKeep{chunk_depth, max_depth}, new_capacity, child_out, data_out, parent_out, sample_counts_out, "truncation",
                             mnv::stream_scratch(dev, stream), stream);
}

}  // extern "C"
