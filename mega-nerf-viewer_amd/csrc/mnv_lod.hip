// mnv_lod.hip -- levels of detail of a tree: mnv_tree_mip_rows derives every interior voxel's row from its children, bottom-up (the mip
// contract of include/mnv.h), mnv_tree_truncate cuts the tree at a depth and compacts the survivors.  The result is an ordinary N3Tree in the
// reference's array layout: every march kernel renders it unchanged.
//
// Depths: one top-down, level-synchronous walk of `child` from the root, as the grid overlay does (mnv_wireframe.hip).  Level d holds the
// list of (chunk, flat index of the voxel above it); a chunk enters the next list when it is reached for the first time (a 32-bit
// compare-and-swap on its depth word: the word it stores is the level, whoever stores it), a second arrival or a link outside
// [1, capacity) raises a flag the host reads with the level's size.  The lists of all levels share one array of `capacity` entries.  The
// order inside a level depends on the schedule; it only decides which wavefront handles a chunk, no output byte.
//
// Rows: one launch per depth, deepest first, a group of 8 .. 64 lanes per chunk of that depth (32 for SH9: two chunks per wavefront).  A
// chunk's eight rows are data_dim aligned 16-byte segments (448 B for SH9).  The group stages them into LDS with 16-byte loads -- the
// halfs of leaf voxels from the input tree, the halfs of interior voxels from data_out, where the launch of the level below left them --
// stores the merged segments to data_out, and then computes the row of the voxel ABOVE the chunk, one column per lane with the eight
// weights and W read from LDS, into data_out.  So every row of the tree is read once and written once; the input tree is never written.
//
// binary16 <-> binary32 is done with integer arithmetic (and one exact binary32 add for subnormal results): no conversion instruction's
// denormal mode enters.  Build flags as everywhere: -ffp-contract=off, correctly rounded division.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cstring>
#include <mutex>
#include <vector>

#include "mnv_internal.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kMaxLodDepth = 23;  // as the packed accel
constexpr int kMaxDataDim = 1024;  // four wavefronts' chunks of data_dim 16-byte segments per workgroup in LDS: 64 KB
constexpr int kWavesPerBlock = 4;

unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------------------------------------------- depths

// thread t: child (t & 7) of list entry t >> 3.  ctr[0]: size of the next level, ctr[1]: fault bits (1 link outside the tree, 2 a chunk reached twice)
__global__ void __launch_bounds__(256) lod_level_kernel(const int32_t *__restrict__ child, int32_t capacity, const int2 *__restrict__ front, int64_t n_front,
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
    const unsigned lane = __lane_id();
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const unsigned long long m = __ballot(push);
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if ((int)lane == leader) base = atomicAdd(&ctr[0], (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (push) {
            const unsigned long long slot = base + (unsigned long long)__popcll(m & below);
            if ((int64_t)slot < cap_next)
                next[slot] = make_int2(nid, above);
            else
                atomicOr(&ctr[1], 2ull);  // more arrivals than chunks left
        }
    }
}

// ---------------------------------------------------------------------------------------------------- rows

// h(bits): the binary16 value as binary32; bits that are not finite read as +0
__device__ __forceinline__ float lod_h(uint32_t b) {
    const uint32_t e = (b >> 10) & 31u, m = b & 0x3ffu, s = (b & 0x8000u) << 16;
    if (e == 31u) return 0.f;
    if (e == 0u) return __uint_as_float(s | __float_as_uint((float)m * 0x1p-24f));  // (a subnormal half is a normal float)
    return __uint_as_float(s | ((e + 112u) << 23) | (m << 13));
}

// half(): binary32 -> binary16 bits, round to nearest even, once; subnormal results kept, overflow to infinity
__device__ __forceinline__ uint16_t lod_half(float f) {
    uint32_t x = __float_as_uint(f);
    const uint32_t s = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(s | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (x < 0x38800000u) {  // below 2^-14: the sum with 0.5 has the spacing of binary16 subnormals (2^-24) and is rounded by the add
        const float r = __uint_as_float(x) + 0.5f;
        return (uint16_t)(s | (__float_as_uint(r) - 0x3f000000u));
    }
    x += 0xfffu + ((x >> 13) & 1u);
    x = (x - 0x38000000u) >> 13;
    return (uint16_t)(s | (x > 0x7c00u ? 0x7c00u : x));
}

union Seg16 {
    uint4 v;
    uint16_t h[8];
};

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
            Seg16 a;
            a.v = in4[s];
            if (mask) {
                const int j0 = (8 * s) / dd, j1 = (8 * s + 7) / dd;  // the rows segment s holds halfs of
                unsigned span = 0;
                for (int j = j0; j <= j1; ++j) span |= 1u << j;
                if (mask & span) {
                    Seg16 b;
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
        const float sg = lod_h(rows[i * dd + dd - 1]);
        w[i] = sg > 0.f ? sg : 0.f;
    }
    const float W = ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) + w[7];
    uint16_t *above = data_out + (int64_t)e.y * dd;
    for (int c = gl; c < dd; c += G) {
        uint16_t r = 0;
        if (W != 0.f) {
            if (c == dd - 1) {
                r = lod_half(W * 0.125f);
            } else {
                float S = w[0] * lod_h(rows[c]);
                for (int i = 1; i < 8; ++i) S = S + w[i] * lod_h(rows[i * dd + c]);
                r = lod_half(S / W);
            }
        }
        above[c] = r;
    }
}

// rows of the chunks the walk did not reach, bit for bit; thread per 16-byte segment
__global__ void __launch_bounds__(256) lod_copy_unreached_kernel(const uint4 *__restrict__ in4, uint4 *__restrict__ out4, const int32_t *__restrict__ chunk_depth,
                                                                  int64_t n_seg, int32_t dd) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_seg) return;
    if (chunk_depth[t / dd] == 0) out4[t] = in4[t];
}

// ---------------------------------------------------------------------------------------------------- truncation

struct SurvivorFlag {
    int32_t max_depth;
    __host__ __device__ int32_t operator()(int32_t d) const { return d >= 1 && d <= max_depth ? 1 : 0; }
};

// thread per (chunk, voxel) of the input: links, parents and sample counts of the survivors
__global__ void __launch_bounds__(256) lod_truncate_topology_kernel(const int32_t *__restrict__ child, const int16_t *__restrict__ counts,
                                                                     const int32_t *__restrict__ chunk_depth, const int32_t *__restrict__ rank, int32_t capacity,
                                                                     int32_t max_depth, int32_t new_capacity, int32_t *__restrict__ child_out,
                                                                     int32_t *__restrict__ parent_out, int16_t *__restrict__ counts_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)capacity * 8) return;
    const int32_t c = (int32_t)(t >> 3);
    const int j = (int)(t & 7);
    const int32_t d = chunk_depth[c];
    if (d < 1 || d > max_depth) return;
    const int32_t nc = rank[c];
    if (nc < 0 || nc >= new_capacity) return;
    const int64_t o = (int64_t)nc * 8 + j;
    const int32_t ch = child[t];
    int32_t link = 0;
    if (ch != 0 && d < max_depth) {
        const int64_t k = (int64_t)c + ch;
        if (k >= 1 && k < capacity) {
            const int32_t nk = rank[k], dk = chunk_depth[k];
            if (dk >= 1 && dk <= max_depth && nk >= 0 && nk < new_capacity) {
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
__global__ void __launch_bounds__(256) lod_truncate_rows_kernel(const uint4 *__restrict__ in4, const int32_t *__restrict__ chunk_depth, const int32_t *__restrict__ rank,
                                                                 int64_t n_seg, int32_t dd, int32_t max_depth, int32_t new_capacity, uint4 *__restrict__ out4) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_seg) return;
    const int64_t c = t / dd;
    const int32_t d = chunk_depth[c];
    if (d < 1 || d > max_depth) return;
    const int32_t nc = rank[c];
    if (nc < 0 || nc >= new_capacity) return;
    out4[(int64_t)nc * dd + (t - c * dd)] = in4[t];
}

// scratch of the asynchronous truncation (ranks and the scan's temporary), one per HIP stream: calls on a stream are ordered, so the next
// call may reuse what the previous one still reads.  Heap objects that live as long as the process (no hipFree after the runtime went).
struct StreamScratch {
    int device = -1;
    hipStream_t stream = nullptr;
    mnv::Buffer<uint8_t> bytes;
};
std::mutex g_scratch_mutex;
std::vector<StreamScratch> *const g_scratch = new std::vector<StreamScratch>();

// scratch of the level walk (mnv_tree_mip_rows waits for its stream: one call at a time per process uses it), per device, kept as above
constexpr int kMaxDevices = 16;
struct MipScratch {
    mnv::Buffer<int2> order;     // the level lists, [capacity]
    mnv::Buffer<int32_t> depth;  // chunk depths when the caller wants none
    mnv::Mirrored<unsigned long long> ctr;
};
std::mutex g_mip_mutex;
MipScratch *const g_mip = new MipScratch[kMaxDevices];

bool on_device(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

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

}  // namespace

extern "C" {

int mnv_tree_mip_rows(const mnv_tree_view *tree, uint16_t *data_out, int32_t *chunk_depth_out, int64_t chunks_at_depth[24], void *hip_stream) {
    int rc;
    if (!data_out || !chunks_at_depth) return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: null output");
    if ((rc = check_view(tree, "mnv_tree_mip_rows"))) return rc;
    const int32_t cap = tree->capacity, dd = tree->data_dim;
    const size_t data_bytes = (size_t)cap * 16 * dd;
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: data_out must be 16-byte aligned");
    if ((const uint8_t *)data_out < (const uint8_t *)tree->data + data_bytes && (const uint8_t *)tree->data < (const uint8_t *)data_out + data_bytes)
        return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: data_out must not alias the tree's data (the input tree is never modified)");
    hipStream_t stream = (hipStream_t)hip_stream;
    for (int d = 0; d < 24; ++d) chunks_at_depth[d] = 0;

    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        (void)hipGetLastError();
        return set_error(MNV_E_NO_DEVICE, "no current HIP device");
    }
    // the walk's scratch is kept between calls (grow-only, per device): the call holds the lock until it has waited for the stream
    std::lock_guard<std::mutex> lock(g_mip_mutex);
    MipScratch &M = g_mip[dev];
    struct Drain {  // ... also when an error leaves this function early: queued work may still use the scratch
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{stream};
    mnv::Mirrored<unsigned long long> &ctr = M.ctr;
    int32_t *depth = chunk_depth_out;
    if (!depth) {
        if ((rc = check_hip(mnv::grow(M.depth, (size_t)cap, (size_t)cap + cap / 4, stream, false), "hipMalloc(chunk depths)"))) return rc;
        depth = M.depth.get();
    }
    if ((rc = check_hip(mnv::grow(M.order, (size_t)cap, (size_t)cap + cap / 4, stream, false), "hipMalloc(level lists)"))) return rc;
    if (!ctr && (rc = mnv::alloc_pair(ctr, 2, "hipMalloc(level counters)", "hipHostMalloc(level counters)"))) return rc;
    int2 *order = M.order.get();

    const int2 root = make_int2(0, -1);
    const int32_t one = 1;
    if ((rc = check_hip(hipMemsetAsync(depth, 0, (size_t)cap * 4, stream), "clear chunk depths")) ||
        (rc = check_hip(hipMemcpyAsync(depth, &one, 4, hipMemcpyHostToDevice, stream), "root depth")) ||
        (rc = check_hip(hipMemcpyAsync(order, &root, sizeof(root), hipMemcpyHostToDevice, stream), "root entry")) ||
        (rc = check_hip(hipMemsetAsync(ctr.dev.get(), 0, 16, stream), "level counters")))
        return rc;
    int64_t offset[26] = {0};  // level d's entries: order[offset[d] .. offset[d + 1])
    offset[1] = 0;
    offset[2] = 1;
    chunks_at_depth[1] = 1;
    int levels = 1;
    for (int d = 1;; ++d) {
        const int64_t n_front = offset[d + 1] - offset[d], cap_next = (int64_t)cap - offset[d + 1];
        hipLaunchKernelGGL(lod_level_kernel, dim3(blocks_for(n_front * 8)), dim3(256), 0, stream, tree->child, cap, order + offset[d], n_front, d,
                           order + offset[d + 1], cap_next, depth, ctr.dev.get());
        if ((rc = check_hip(hipGetLastError(), "lod_level_kernel")) ||
            (rc = check_hip(hipMemcpyAsync(ctr.host.get(), ctr.dev.get(), 16, hipMemcpyDeviceToHost, stream), "level counters")) ||
            (rc = check_hip(hipMemsetAsync(ctr.dev.get(), 0, 8, stream), "level counters")) || (rc = check_hip(hipStreamSynchronize(stream), "lod_level_kernel")))
            return rc;
        const unsigned long long fault = ctr.host.get()[1];
        if (fault & 1ull) return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: a child link leaves the tree (outside [1, capacity))");
        if (fault & 2ull) return set_error(MNV_E_INVALID, "mnv_tree_mip_rows: a chunk is reached twice (not a tree)");
        const int64_t n_next = (int64_t)ctr.host.get()[0];
        if (n_next == 0) break;
        if (d + 1 > kMaxLodDepth) return set_error(MNV_E_UNSUPPORTED, "mnv_tree_mip_rows: tree deeper than 23 levels");
        offset[d + 2] = offset[d + 1] + n_next;
        chunks_at_depth[d + 1] = n_next;
        levels = d + 1;
    }
    int log2_g = 3;  // lanes per chunk: 8, 16, 32 or 64, at least data_dim where that is below 64
    while ((1 << log2_g) < dd && log2_g < 6) ++log2_g;
    const int per_block = kWavesPerBlock * (64 >> log2_g);
    const size_t lds = (size_t)per_block * dd * 16;
    for (int d = levels; d >= 1; --d) {
        const int64_t n = offset[d + 1] - offset[d];
        hipLaunchKernelGGL(lod_mip_kernel, dim3(blocks_for(n, per_block)), dim3(64 * kWavesPerBlock), lds, stream, tree->data, data_out, tree->child,
                           order + offset[d], n, dd, log2_g);
        if ((rc = check_hip(hipGetLastError(), "lod_mip_kernel"))) return rc;
    }
    if (offset[levels + 1] < cap) {
        const int64_t n_seg = (int64_t)cap * dd;
        hipLaunchKernelGGL(lod_copy_unreached_kernel, dim3(blocks_for(n_seg)), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(tree->data),
                           reinterpret_cast<uint4 *>(data_out), depth, n_seg, dd);
        if ((rc = check_hip(hipGetLastError(), "lod_copy_unreached_kernel"))) return rc;
    }
    return check_hip(hipStreamSynchronize(stream), "mnv_tree_mip_rows");
}

int mnv_tree_truncate(const mnv_tree_view *tree, const int32_t *chunk_depth, int32_t max_depth, int32_t new_capacity, int32_t *child_out, uint16_t *data_out,
                      int32_t *parent_out, int16_t *sample_counts_out, void *hip_stream) {
    int rc;
    if (!chunk_depth || !child_out || !data_out) return set_error(MNV_E_INVALID, "mnv_tree_truncate: null chunk depths / output");
    if ((rc = check_view(tree, "mnv_tree_truncate"))) return rc;
    if (max_depth < 1) return set_error(MNV_E_INVALID, "mnv_tree_truncate: max_depth must be at least 1");
    if (new_capacity < 1 || new_capacity > tree->capacity) return set_error(MNV_E_INVALID, "mnv_tree_truncate: new_capacity outside [1, capacity]");
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_tree_truncate: data_out must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int32_t cap = tree->capacity, dd = tree->data_dim;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return set_error(MNV_E_NO_DEVICE, "no current HIP device");
    }
    auto flags = rocprim::make_transform_iterator(chunk_depth, SurvivorFlag{max_depth});
    size_t tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp_bytes, flags, (int32_t *)nullptr, 0, (size_t)cap, rocprim::plus<int32_t>(), stream);
    const size_t rank_bytes = ((size_t)cap * 4 + 255) & ~(size_t)255, need = rank_bytes + tmp_bytes + 256;

    std::lock_guard<std::mutex> lock(g_scratch_mutex);
    StreamScratch *S = nullptr;
    for (auto &e : *g_scratch)
        if (e.device == dev && e.stream == stream) S = &e;
    if (!S) {
        g_scratch->emplace_back();
        S = &g_scratch->back();
        S->device = dev;
        S->stream = stream;
    }
    if ((rc = check_hip(mnv::grow(S->bytes, need, need + need / 4, stream, true), "hipMalloc(truncation scratch)"))) return rc;
    int32_t *rank = reinterpret_cast<int32_t *>(S->bytes.get());
    if ((rc = check_hip(rocprim::exclusive_scan(S->bytes.get() + rank_bytes, tmp_bytes, flags, rank, 0, (size_t)cap, rocprim::plus<int32_t>(), stream), "exclusive_scan")))
        return rc;
    if (parent_out && (rc = check_hip(hipMemsetAsync(parent_out, 0xff, (size_t)new_capacity * 4, stream), "clear parents"))) return rc;
    const int16_t *counts = sample_counts_out ? tree->sample_counts : nullptr;
    hipLaunchKernelGGL(lod_truncate_topology_kernel, dim3(blocks_for((int64_t)cap * 8)), dim3(256), 0, stream, tree->child, counts, chunk_depth, rank, cap, max_depth,
                       new_capacity, child_out, parent_out, counts ? sample_counts_out : nullptr);
    if ((rc = check_hip(hipGetLastError(), "lod_truncate_topology_kernel"))) return rc;
    const int64_t n_seg = (int64_t)cap * dd;
    hipLaunchKernelGGL(lod_truncate_rows_kernel, dim3(blocks_for(n_seg)), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(tree->data), chunk_depth, rank, n_seg, dd,
                       max_depth, new_capacity, reinterpret_cast<uint4 *>(data_out));
    return check_hip(hipGetLastError(), "lod_truncate_rows_kernel");
}

}  // extern "C"
