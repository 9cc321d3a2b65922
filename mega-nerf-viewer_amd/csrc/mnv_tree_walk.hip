// mnv_tree_walk.hip -- the kernels and host code behind mnv_tree_walk.h: the plain level walk that mnv_tree_mip_rows and mnv_tree_cull start
// from, the compaction that mnv_tree_truncate and mnv_tree_cut end with, and the scratch both keep between calls.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <vector>

#include "mnv_tree_walk.h"

namespace mnv {

namespace {

constexpr int kMaxDataDim = 1024;  // four wavefronts' chunks of data_dim 16-byte segments per workgroup in LDS: 64 KB (the mip pass)

// ---------------------------------------------------------------------------------------------------- the level walk

// thread t: child (t & 7) of list entry t >> 3.  ctr[0]: size of the next level, ctr[1]: fault bits (1 link outside the tree, 2 a chunk reached twice)
__global__ void __launch_bounds__(256) walk_level_kernel(const int32_t *__restrict__ child, int32_t capacity, const int2 *__restrict__ front, int64_t n_front,
                                                          int32_t depth, int2 *__restrict__ next, int64_t cap_next, int32_t *__restrict__ chunk_depth,
                                                          unsigned long long *__restrict__ ctr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool push = false;
    int32_t nid = 0, above = 0;
    if (t < n_front * 8) {
        const int32_t c = front[t >> 3].x;
        const int j = (int)(t & 7);
        const int32_t ch = child[(int64_t)c * 8 + j];
        if (ch != 0) {
            const int64_t n = (int64_t)c + ch;
            if (n < 1 || n >= capacity) {
                atomicOr(&ctr[1], 1ull);
            } else if (atomicCAS(&chunk_depth[n], 0, depth + 1) != 0) {
                atomicOr(&ctr[1], 2ull);
            } else {
                nid = (int32_t)n;
                above = c * 8 + j;
                push = true;
            }
        }
    }
    wave_append(push, &ctr[0], [=](unsigned long long slot) {
        if ((int64_t)slot < cap_next)
            next[slot] = make_int2(nid, above);
        else
            atomicOr(&ctr[1], 2ull);  // more arrivals than chunks left
    });
}

// thread per 16-byte segment
__global__ void __launch_bounds__(256) copy_unreached_kernel(const uint4 *__restrict__ in4, uint4 *__restrict__ out4, const int32_t *__restrict__ chunk_depth,
                                                              int64_t n_seg, int32_t dd) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_seg) return;
    if (chunk_depth[t / dd] == 0) out4[t] = in4[t];
}

struct WalkScratch {
    Buffer<int2> order;     // the level lists, [capacity]
    Buffer<int32_t> depth;  // chunk depths when the caller wants none
    Mirrored<unsigned long long> ctr;
};
std::mutex g_walk_mutex;
WalkScratch *const g_walk = new WalkScratch[kMaxWalkDevices];  // (lives as long as the process: no hipFree after the runtime went)

// ---------------------------------------------------------------------------------------------------- compaction

// thread per (chunk, voxel) of the input: links, parents and sample counts of the survivors
template <typename Keep>
__global__ void __launch_bounds__(256) compact_topology_kernel(const int32_t *__restrict__ child, const int16_t *__restrict__ counts, const Keep keep,
                                                                const int32_t *__restrict__ rank, int32_t capacity, int32_t new_capacity,
                                                                int32_t *__restrict__ child_out, int32_t *__restrict__ parent_out, int16_t *__restrict__ counts_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)capacity * 8) return;
    const int32_t c = (int32_t)(t >> 3);
    const int j = (int)(t & 7);
    if (!keep.survives(c)) return;
    const int32_t nc = rank[c];
    if (nc < 0 || nc >= new_capacity) return;
    const int64_t o = (int64_t)nc * 8 + j;
    const int32_t ch = child[t];
    int32_t link = 0;
    if (ch != 0 && keep.carries(c)) {
        const int64_t k = (int64_t)c + ch;
        if (k >= 1 && k < capacity && keep.survives(k)) {
            const int32_t nk = rank[k];
            if (nk >= 0 && nk < new_capacity) {
                link = nk - nc;
                if (parent_out) parent_out[nk] = (int32_t)o;
            }
        }
    }
    child_out[o] = link;
    if (counts_out) counts_out[o] = counts[t];
    if (parent_out && c == 0 && j == 0) parent_out[nc] = -1;
}

// thread per 16-byte segment of the input rows: the survivors' rows to their new place
template <typename Keep>
__global__ void __launch_bounds__(256) compact_rows_kernel(const uint4 *__restrict__ in4, const Keep keep, const int32_t *__restrict__ rank, int64_t n_seg, int32_t dd,
                                                            int32_t new_capacity, uint4 *__restrict__ out4) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_seg) return;
    const int64_t c = t / dd;
    if (!keep.survives(c)) return;
    const int32_t nc = rank[c];
    if (nc < 0 || nc >= new_capacity) return;
    out4[(int64_t)nc * dd + (t - c * dd)] = in4[t];
}

struct ScratchEntry {
    int device;
    hipStream_t stream;
    StreamScratch *scratch;
};
std::mutex g_stream_mutex;
std::vector<ScratchEntry> *const g_stream = new std::vector<ScratchEntry>();

}  // namespace

int check_view(const mnv_tree_view *t, const char *who) {
    if (!t || !t->data || !t->child) return set_error(MNV_E_INVALID, std::string(who) + ": null tree view / arrays");
    if (t->N != 2) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": only N == 2 trees");
    if (t->capacity < 1) return set_error(MNV_E_INVALID, std::string(who) + ": a tree has at least its root chunk");
    if (t->data_dim < 2) return set_error(MNV_E_INVALID, std::string(who) + ": data_dim must be at least 2");
    if (t->data_dim > kMaxDataDim) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": data_dim above 1024");
    if (((uintptr_t)t->data & 15u) != 0) return set_error(MNV_E_INVALID, std::string(who) + ": the data array must be 16-byte aligned");
    if (!on_device(t->child) || !on_device(t->data)) return set_error(MNV_E_INVALID, std::string(who) + ": the tree view must hold device arrays");
    return MNV_OK;
}

int WalkGuard::begin(hipStream_t stream) {
    int rc;
    if ((rc = current_device(&device_))) return rc;
    if (device_ >= kMaxWalkDevices) return set_error(MNV_E_NO_DEVICE, "no current HIP device");
    lock_ = std::unique_lock<std::mutex>(g_walk_mutex);
    stream_ = stream;
    return MNV_OK;
}

int walk_levels(const int32_t *child, int32_t capacity, int32_t *chunk_depth, const char *who, const WalkGuard &guard, LevelLists &out) {
    int rc;
    const size_t cap = (size_t)capacity;
    hipStream_t stream = guard.stream();
    WalkScratch &S = g_walk[guard.device()];
    int32_t *depth = chunk_depth;
    if (!depth) {
        if ((rc = check_hip(grow(S.depth, cap, cap + cap / 4, stream, false), "hipMalloc(chunk depths)"))) return rc;
        depth = S.depth.get();
    }
    if ((rc = check_hip(grow(S.order, cap, cap + cap / 4, stream, false), "hipMalloc(level lists)"))) return rc;
    if (!S.ctr && (rc = alloc_pair(S.ctr, 2, "hipMalloc(level counters)", "hipHostMalloc(level counters)"))) return rc;
    int2 *order = S.order.get();
    const int2 root = make_int2(0, -1);
    const int32_t one = 1;
    if ((rc = check_hip(hipMemsetAsync(depth, 0, cap * 4, stream), "clear chunk depths")) ||
        (rc = check_hip(hipMemcpyAsync(depth, &one, 4, hipMemcpyHostToDevice, stream), "root depth")) ||
        (rc = check_hip(hipMemcpyAsync(order, &root, sizeof(root), hipMemcpyHostToDevice, stream), "root entry")) ||
        (rc = check_hip(hipMemsetAsync(S.ctr.dev.get(), 0, 16, stream), "level counters")))
        return rc;
    out.order = order;
    out.depth = depth;
    unsigned long long *ctr = S.ctr.dev.get();
    return walk_loop(out, capacity, INT_MAX, S.ctr, who, "walk_level_kernel", stream, [=](int d, int64_t front, int64_t n_front, int64_t next, int64_t cap_next) {
        hipLaunchKernelGGL(walk_level_kernel, dim3(blocks_for(n_front * 8)), dim3(256), 0, stream, child, capacity, order + front, n_front, d, order + next, cap_next,
                           depth, ctr);
    });
}

int copy_unreached(const uint16_t *data_in, uint16_t *data_out, const int32_t *chunk_depth, int32_t capacity, int32_t data_dim, hipStream_t stream) {
    const int64_t n_seg = (int64_t)capacity * data_dim;
    hipLaunchKernelGGL(copy_unreached_kernel, dim3(blocks_for(n_seg)), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(data_in), reinterpret_cast<uint4 *>(data_out),
                       chunk_depth, n_seg, data_dim);
    return check_hip(hipGetLastError(), "copy_unreached_kernel");
}

std::mutex &stream_scratch_mutex() { return g_stream_mutex; }

StreamScratch &stream_scratch(int device, hipStream_t stream) {
    for (const ScratchEntry &e : *g_stream)
        if (e.device == device && e.stream == stream) return *e.scratch;
    g_stream->push_back(ScratchEntry{device, stream, new StreamScratch()});
    return *g_stream->back().scratch;
}

template <typename Keep>
int compact_tree(const mnv_tree_view *tree, Keep keep, int32_t new_capacity, int32_t *child_out, uint16_t *data_out, int32_t *parent_out,
                 int16_t *sample_counts_out, const char *what, StreamScratch &S, hipStream_t stream) {
    int rc;
    const int32_t cap = tree->capacity, dd = tree->data_dim;
    auto flags = rocprim::make_transform_iterator(keep.words(), keep.flag());
    size_t tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp_bytes, flags, (int32_t *)nullptr, 0, (size_t)cap, rocprim::plus<int32_t>(), stream);
    const size_t rank_bytes = ((size_t)cap * 4 + 255) & ~(size_t)255, need = rank_bytes + tmp_bytes + 256;
    if ((rc = check_hip(grow(S.bytes, need, need + need / 4, stream, true), (std::string("hipMalloc(") + what + " scratch)").c_str()))) return rc;
    int32_t *rank = reinterpret_cast<int32_t *>(S.bytes.get());
    if ((rc = check_hip(rocprim::exclusive_scan(S.bytes.get() + rank_bytes, tmp_bytes, flags, rank, 0, (size_t)cap, rocprim::plus<int32_t>(), stream), "exclusive_scan")))
        return rc;
    if (parent_out && (rc = check_hip(hipMemsetAsync(parent_out, 0xff, (size_t)new_capacity * 4, stream), "clear parents"))) return rc;
    const int16_t *counts = sample_counts_out ? tree->sample_counts : nullptr;
    hipLaunchKernelGGL(compact_topology_kernel<Keep>, dim3(blocks_for((int64_t)cap * 8)), dim3(256), 0, stream, tree->child, counts, keep, rank, cap, new_capacity, child_out,
                       parent_out, counts ? sample_counts_out : nullptr);
    if ((rc = check_hip(hipGetLastError(), "compact_topology_kernel"))) return rc;
    const int64_t n_seg = (int64_t)cap * dd;
    hipLaunchKernelGGL(compact_rows_kernel<Keep>, dim3(blocks_for(n_seg)), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(tree->data), keep, rank, n_seg, dd,
                       new_capacity, reinterpret_cast<uint4 *>(data_out));
    return check_hip(hipGetLastError(), "compact_rows_kernel");
}

template int compact_tree<DepthKeep>(const mnv_tree_view *, DepthKeep, int32_t, int32_t *, uint16_t *, int32_t *, int16_t *, const char *, StreamScratch &, hipStream_t);
template int compact_tree<ByteKeep>(const mnv_tree_view *, ByteKeep, int32_t, int32_t *, uint16_t *, int32_t *, int16_t *, const char *, StreamScratch &, hipStream_t);

}  // namespace mnv
