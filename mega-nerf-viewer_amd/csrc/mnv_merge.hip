// mnv_merge.hip -- merging two trees (the merge contract of include/mnv.h): mnv_tree_merge_plan / write / destroy.  Tree B is placed into
// a voxel of tree A (the integer placement level : corner); the result is the union of the two structures in canonical breadth-first
// order, every row taken from A, from B, or blended.  The result is an ordinary N3Tree: every march kernel renders it unchanged.
//
// plan: a top-down, level-synchronous dual walk.  Level d is the list of the merged chunks of depth d IN FINAL ORDER; an entry is a pair of
// references (a_ref, b_ref): the source's chunk at this place (>= 0), the voxel of a shallower leaf that covers it (~voxel id), and for B
// also "none" (outside B's cube) and "on the path" (the chunk holds a voxel above B's cube).  A thread per merged voxel, eight lanes a chunk,
// a wavefront eight chunks:
//   level   follows both references one voxel down and decides whether the merged voxel is interior; the chunk's interior mask is one byte
//           of the wavefront's ballot, its bit count the chunk's number of child chunks
//   scan    rocprim::exclusive_scan over the counts: where a chunk's children start in the next level
//   emit    the voxel's child chunk goes to next level's slot scan[chunk] + popcount(mask below j): ascending by (parent, j), which is the
//           canonical order -- no append, no atomic
// One read-back per level sizes the next list (at most 23 waits).  The handle keeps 17 bytes per chunk: the two references, the index of
// the first child chunk, the mask and the parent; links and sources are recomputed from them by write.  The counters of mnv_merge_stats
// are sums of ballot popcounts (integers: the order of the adds cannot change them).
//
// write: one launch, a group of 8 .. 64 lanes per merged chunk.  The group's first eight lanes find their voxel's sources, read the two
// sigma halfs, classify the row (A's, B's, blended) and store the link, the sample count and the provenance.  A chunk whose eight rows are
// the eight rows of ONE source chunk -- the common case -- is moved as data_dim 16-byte segments; any other chunk builds its data_dim
// segments half by half (rows of odd data_dim are 2-byte aligned in the sources) and still stores 16 bytes at a time.
//
// Build flags as everywhere: -ffp-contract=off, correctly rounded division; binary32 subnormals are kept (the default of the target).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <algorithm>
#include <cstring>
#include <memory>

#include "mnv_tree_walk.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kMaxMergeDepth = 23;      // as the packed accel
constexpr int kMaxMergeLevel = 22;      // B's root chunk then has depth 23
constexpr int kMaxDataDim = 1024;       // as mnv_tree_truncate
constexpr int32_t kMaxChunks = 1 << 27;  // of an input: a voxel id (chunk * 8 + j) is an int32, and eight times a level's size a uint32
constexpr int32_t kNone = INT32_MIN, kPath = INT32_MIN + 1;  // b_ref: outside B's cube / the chunk holds a voxel above B's cube

// ---------------------------------------------------------------------------------------------------- the walk

// one source, one voxel down.  ref >= 0: the source's chunk here; ref < 0: ~(voxel id of the leaf that covers this place)
struct Step {
    int32_t vox, next;  // the voxel that supplies the row; the reference of the chunk below
    bool exact, interior, fault;
};

__device__ __forceinline__ Step merge_step(int32_t ref, const int32_t *__restrict__ child, int32_t cap, int j) {
    Step s;
    s.fault = false, s.interior = false;
    if (ref < 0) {
        s.vox = ~ref, s.next = ref, s.exact = false;
        return s;
    }
    s.vox = ref * 8 + j, s.exact = true, s.next = ~s.vox;
    const int32_t link = child[s.vox];
    if (link != 0) {
        const int64_t k = (int64_t)ref + link;
        if (k < 1 || k >= cap) {
            s.fault = true;
        } else {
            s.next = (int32_t)k, s.interior = true;
        }
    }
    return s;
}

// pos(bits) = h(bits) > 0: positive, finite, not zero
__device__ __forceinline__ bool merge_pos(uint32_t b) { return b != 0u && b < 0x7c00u; }

// 0: A's row, 1: B's row, 2: blended
__device__ __forceinline__ int merge_kind(bool has_b, uint32_t sigma_a, uint32_t sigma_b, int mode) {
    if (!has_b || !merge_pos(sigma_b)) return 0;
    return mode == MNV_MERGE_ADD && merge_pos(sigma_a) ? 2 : 1;
}

struct Inputs {
    const int32_t *a_child, *b_child;
    const uint16_t *a_data, *b_data;
    const int16_t *a_counts, *b_counts;
    int32_t a_cap, b_cap, dd, mode;
};

struct LevelArgs {
    const int32_t *a_ref, *b_ref;  // this level's entries
    int64_t n, first;              // how many; the merged index of the first
    int32_t digit, last;           // j of the path voxel at this depth (-1 below the placement level); last: its child chunk is B's root
    int64_t first_next;
    uint8_t *mask;                 // [n]
    uint32_t *count;               // [n]: level; the scanned offsets: emit
    int32_t *first_child;          // [n]
    int32_t *a_next, *b_next, *parent_next;  // the next level's entries
    unsigned long long *ctr;       // [0] fault bits (1: a link outside the tree), [1] rows from A, [2] from B, [3] blended, [4] pushed A, [5] pushed B
};

struct Voxel {
    Step a, b;
    bool has_b, interior;
};

__device__ __forceinline__ Voxel merge_voxel(const Inputs &I, int32_t a_ref, int32_t b_ref, int j, int digit, int last) {
    Voxel v;
    v.a = merge_step(a_ref, I.a_child, I.a_cap, j);
    v.has_b = b_ref > kPath;
    bool on_path = false;
    if (v.has_b) {
        v.b = merge_step(b_ref, I.b_child, I.b_cap, j);
    } else {
        on_path = b_ref == kPath && j == digit;
        v.b.vox = -1, v.b.exact = false, v.b.interior = false, v.b.fault = false;
        v.b.next = on_path ? (last ? 0 : kPath) : kNone;
    }
    v.interior = v.a.interior || v.b.interior || on_path;
    return v;
}

// thread t: voxel t & 7 of entry t >> 3, over a fixed grid with its stride.  The chunk's mask and count; the fault bit and the counters
// of the stats are kept per wavefront (popcounts of ballots: wave-uniform) and added once at the end -- one atomic per 64 voxels on one
// address was served one after the other (16 of the 24 ms of a plan over 7.2 M chunks)
constexpr int kLevelGrid = 2048;
__global__ void __launch_bounds__(256) merge_level_kernel(Inputs I, LevelArgs L) {
    const unsigned lane = threadIdx.x & 63u;
    const int64_t total = L.n * 8, stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long from_a = 0, from_b = 0, blended = 0, pushed_a = 0, pushed_b = 0;
    bool fault = false;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t - lane < total; t += stride) {  // (wave-uniform bounds)
        const int64_t e = t >> 3;
        const int j = (int)(t & 7);
        const bool valid = t < total;
        Voxel v;
        v.interior = false, v.has_b = false, v.a.fault = v.b.fault = false, v.a.exact = v.b.exact = true, v.a.vox = 0, v.b.vox = -1;
        if (valid) v = merge_voxel(I, L.a_ref[e], L.b_ref[e], j, L.digit, L.last);
        const unsigned long long m = __ballot(valid && v.interior);
        const uint32_t byte = (uint32_t)(m >> (8u * (lane >> 3))) & 0xffu;
        if (valid && j == 0) {
            L.mask[e] = (uint8_t)byte;
            L.count[e] = (uint32_t)__popc(byte);
        }
        fault = fault || __ballot(valid && (v.a.fault || v.b.fault)) != 0ull;
        int kind = -1;
        if (valid) {
            const uint32_t sa = I.a_data[(int64_t)v.a.vox * I.dd + (I.dd - 1)];
            const uint32_t sb = v.has_b ? I.b_data[(int64_t)v.b.vox * I.dd + (I.dd - 1)] : 0u;
            kind = merge_kind(v.has_b, sa, sb, I.mode);
        }
        from_a += (unsigned long long)__popcll(__ballot(kind == 0));
        from_b += (unsigned long long)__popcll(__ballot(kind == 1));
        blended += (unsigned long long)__popcll(__ballot(kind == 2));
        pushed_a += (unsigned long long)__popcll(__ballot(valid && !v.a.exact));
        pushed_b += (unsigned long long)__popcll(__ballot(valid && v.has_b && !v.b.exact));
    }
    if (lane == 0) {
        if (fault) atomicOr(&L.ctr[0], 1ull);
        if (from_a) atomicAdd(&L.ctr[1], from_a);
        if (from_b) atomicAdd(&L.ctr[2], from_b);
        if (blended) atomicAdd(&L.ctr[3], blended);
        if (pushed_a) atomicAdd(&L.ctr[4], pushed_a);
        if (pushed_b) atomicAdd(&L.ctr[5], pushed_b);
    }
}

// the same thread shape: the child chunk of an interior voxel becomes entry count[e] (scanned) + popcount(mask below j) of the next level
__global__ void __launch_bounds__(256) merge_emit_kernel(Inputs I, LevelArgs L, int64_t n_next) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, e = t >> 3;
    const int j = (int)(t & 7);
    if (e >= L.n) return;
    const uint32_t byte = L.mask[e];
    const int64_t at = (int64_t)L.count[e];
    if (j == 0) L.first_child[e] = (int32_t)(L.first_next + at);
    if (!((byte >> j) & 1u)) return;
    const int64_t slot = at + __popc(byte & ((1u << j) - 1u));
    if (slot >= n_next) return;  // (the scan's total is n_next)
    const Voxel v = merge_voxel(I, L.a_ref[e], L.b_ref[e], j, L.digit, L.last);
    L.a_next[slot] = v.a.next;
    L.b_next[slot] = v.b.next;
    L.parent_next[slot] = (int32_t)((L.first + e) * 8 + j);
}

// ---------------------------------------------------------------------------------------------------- rows

struct WriteArgs {
    const int32_t *a_ref, *b_ref, *first_child, *parent;
    const uint8_t *mask;
    int64_t n_chunks;
    int32_t log2_g;
    int32_t *child_out;
    uint16_t *data_out;
    int32_t *parent_out;
    int16_t *counts_out;
    int32_t *src_a_out, *src_b_out;
};

__global__ void __launch_bounds__(256) merge_write_kernel(Inputs I, WriteArgs P) {
    __shared__ int4 voxel_info[32][8];  // per group and voxel: a_vox, b_vox, kind, sigma_a | sigma_b << 16
    const int G = 1 << P.log2_g, grp = threadIdx.x >> P.log2_g, gl = threadIdx.x & (G - 1);
    const int64_t c = (int64_t)blockIdx.x * (256 >> P.log2_g) + grp;
    const bool active = c < P.n_chunks;
    const int dd = I.dd;
    int32_t a_ref = 0, b_ref = kNone;
    if (active) a_ref = P.a_ref[c], b_ref = P.b_ref[c];
    if (active && gl < 8) {
        const int j = gl;
        const int32_t a_vox = a_ref < 0 ? ~a_ref : a_ref * 8 + j;
        const int32_t b_vox = b_ref >= 0 ? b_ref * 8 + j : (b_ref > kPath ? ~b_ref : -1);
        const uint32_t sa = I.a_data[(int64_t)a_vox * dd + (dd - 1)];
        const uint32_t sb = b_vox >= 0 ? I.b_data[(int64_t)b_vox * dd + (dd - 1)] : 0u;
        const int kind = merge_kind(b_vox >= 0, sa, sb, I.mode);
        voxel_info[grp][j] = make_int4(a_vox, b_vox, kind, (int)(sa | (sb << 16)));
        const uint32_t m = P.mask[c];
        const int64_t o = c * 8 + j;
        P.child_out[o] = (m >> j) & 1u ? (int32_t)((int64_t)P.first_child[c] + __popc(m & ((1u << j) - 1u)) - c) : 0;
        if (P.parent_out && j == 0) P.parent_out[c] = P.parent[c];
        if (P.counts_out) {
            const int32_t ca = I.a_counts ? I.a_counts[a_vox] : 8, cb = (I.b_counts && b_vox >= 0) ? I.b_counts[b_vox] : 8;
            const int32_t sum = ca + cb;
            P.counts_out[o] = (int16_t)(kind == 0 ? ca : kind == 1 ? cb : (sum > 32767 ? 32767 : sum < -32768 ? -32768 : sum));
        }
        if (P.src_a_out) P.src_a_out[o] = a_vox;
        if (P.src_b_out) P.src_b_out[o] = b_vox;
    }
    __syncthreads();
    if (!active) return;
    int kinds = 0;  // bit k: some voxel of the chunk has kind k
    for (int j = 0; j < 8; ++j) kinds |= 1 << voxel_info[grp][j].z;
    uint4 *out4 = reinterpret_cast<uint4 *>(P.data_out) + c * dd;
    const uint4 *whole = nullptr;  // the source chunk whose eight rows are this chunk's
    if (kinds == 1 && a_ref >= 0) whole = reinterpret_cast<const uint4 *>(I.a_data) + (int64_t)a_ref * dd;
    if (kinds == 2 && b_ref >= 0) whole = reinterpret_cast<const uint4 *>(I.b_data) + (int64_t)b_ref * dd;
    if (whole) {
        for (int s = gl; s < dd; s += G) out4[s] = whole[s];
        return;
    }
    for (int s = gl; s < dd; s += G) {
        mnv::Seg16 o;
        for (int i = 0; i < 8; ++i) {
            const int at = 8 * s + i, j = at / dd, col = at - j * dd;
            const int4 vi = voxel_info[grp][j];
            if (vi.z == 0) {
                o.h[i] = I.a_data[(int64_t)vi.x * dd + col];
            } else if (vi.z == 1) {
                o.h[i] = I.b_data[(int64_t)vi.y * dd + col];
            } else {
                const float wa = mnv::h((uint32_t)vi.w & 0xffffu), wb = mnv::h((uint32_t)vi.w >> 16), W = wa + wb;
                if (col == dd - 1) {
                    o.h[i] = mnv::sat_half(W);
                } else {
                    const float ta = wa * mnv::h(I.a_data[(int64_t)vi.x * dd + col]), tb = wb * mnv::h(I.b_data[(int64_t)vi.y * dd + col]);
                    o.h[i] = mnv::sat_half((ta + tb) / W);
                }
            }
        }
        out4[s] = o.v;
    }
}

// ---------------------------------------------------------------------------------------------------- host

// what can be said about a view before a device is touched
int check_view_host(const mnv_tree_view *t, const char *who, const char *which) {
    const std::string w = std::string(who) + ": tree " + which;
    if (!t->data || !t->child) return set_error(MNV_E_INVALID, w + ": null arrays");
    if (t->N != 2) return set_error(MNV_E_UNSUPPORTED, w + ": only N == 2 trees");
    if (t->capacity < 1) return set_error(MNV_E_INVALID, w + ": a tree has at least its root chunk");
    if (t->capacity > kMaxChunks) return set_error(MNV_E_UNSUPPORTED, w + ": more than 2^27 chunks");
    if (t->data_dim < 2) return set_error(MNV_E_INVALID, w + ": data_dim must be at least 2");
    if (t->data_dim > kMaxDataDim) return set_error(MNV_E_UNSUPPORTED, w + ": data_dim above 1024");
    if (((uintptr_t)t->data & 15u) != 0) return set_error(MNV_E_INVALID, w + ": the data array must be 16-byte aligned");
    return MNV_OK;
}

}  // namespace

struct mnv_tree_merge {
    Inputs in;
    int64_t capacity = 0;
    mnv::Buffer<int32_t> a_ref, b_ref, first_child, parent;  // [capacity] (allocated for the bound)
    mnv::Buffer<uint8_t> mask;
};

extern "C" {

int mnv_tree_merge_plan(const mnv_tree_view *a, const mnv_tree_view *b, const mnv_merge_params *p, mnv_tree_merge **out, mnv_merge_stats *stats, void *hip_stream) {
    const char *who = "mnv_tree_merge_plan";
    int rc;
    if (out) *out = nullptr;
    if (!a || !b || !p || !out || !stats) return set_error(MNV_E_INVALID, std::string(who) + ": null argument");
    std::memset(stats, 0, sizeof(*stats));
    if ((rc = check_view_host(a, who, "A")) || (rc = check_view_host(b, who, "B"))) return rc;
    if (a->data_dim != b->data_dim || a->format != b->format || a->basis_dim != b->basis_dim)
        return set_error(MNV_E_INVALID, std::string(who) + ": the two trees must have the same data_dim, format and basis_dim");
    if (p->level < 0 || p->level > kMaxMergeLevel) return set_error(MNV_E_INVALID, std::string(who) + ": level outside 0 .. 22");
    for (int k = 0; k < 3; ++k)
        if (p->corner[k] < 0 || (int64_t)p->corner[k] >= ((int64_t)1 << p->level))
            return set_error(MNV_E_INVALID, std::string(who) + ": a corner outside [0, 2^level)");
    if (p->mode != MNV_MERGE_OVER && p->mode != MNV_MERGE_ADD) return set_error(MNV_E_INVALID, std::string(who) + ": mode must be over (0) or add (1)");
    for (const mnv_tree_view *t : {a, b})
        if (!mnv::on_device(t->child) || !mnv::on_device(t->data) || (t->sample_counts && !mnv::on_device(t->sample_counts)))
            return set_error(MNV_E_INVALID, std::string(who) + ": the tree views must hold device arrays");
    int dev = -1;
    if ((rc = mnv::current_device(&dev))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    // every merged chunk but the root lies under an interior voxel of A, an interior voxel of B or a path voxel
    const int64_t bound = (int64_t)a->capacity + b->capacity + p->level;
    std::unique_ptr<mnv_tree_merge> m(new mnv_tree_merge());
    m->in = Inputs{a->child, b->child, a->data, b->data, a->sample_counts, b->sample_counts, a->capacity, b->capacity, a->data_dim, p->mode};
    size_t tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)bound, rocprim::plus<uint32_t>(), stream);
    mnv::Buffer<uint32_t> count, scanned;
    mnv::Buffer<uint8_t> tmp;
    mnv::Mirrored<unsigned long long> ctr;  // the kernels' six words, then the last count and the last offset of a level
    if ((rc = check_hip(m->a_ref.alloc((size_t)bound), "hipMalloc(merge references)")) || (rc = check_hip(m->b_ref.alloc((size_t)bound), "hipMalloc(merge references)")) ||
        (rc = check_hip(m->first_child.alloc((size_t)bound), "hipMalloc(merge first children)")) || (rc = check_hip(m->parent.alloc((size_t)bound), "hipMalloc(merge parents)")) ||
        (rc = check_hip(m->mask.alloc((size_t)bound), "hipMalloc(merge masks)")) || (rc = check_hip(count.alloc((size_t)bound), "hipMalloc(merge counts)")) ||
        (rc = check_hip(scanned.alloc((size_t)bound), "hipMalloc(merge offsets)")) || (rc = check_hip(tmp.alloc(tmp_bytes + 256), "hipMalloc(scan scratch)")) ||
        (rc = mnv::alloc_pair(ctr, 8, "hipMalloc(merge counters)", "hipHostMalloc(merge counters)")))
        return rc;
    struct Drain {  // also when an error leaves this function early: queued work may still use the scratch
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{stream};
    const int32_t root[3] = {0, p->level == 0 ? 0 : kPath, -1};
    if ((rc = check_hip(hipMemsetAsync(ctr.dev.get(), 0, 64, stream), "clear the merge counters")) ||
        (rc = check_hip(hipMemcpyAsync(m->a_ref.get(), &root[0], 4, hipMemcpyHostToDevice, stream), "root entry")) ||
        (rc = check_hip(hipMemcpyAsync(m->b_ref.get(), &root[1], 4, hipMemcpyHostToDevice, stream), "root entry")) ||
        (rc = check_hip(hipMemcpyAsync(m->parent.get(), &root[2], 4, hipMemcpyHostToDevice, stream), "root entry")))
        return rc;
    uint32_t *tail = reinterpret_cast<uint32_t *>(ctr.host.get() + 6);  // [0] the last count, [1] the last offset
    int64_t first = 0, n = 1;
    stats->chunks_at_depth[1] = 1;
    for (int d = 1;; ++d) {
        LevelArgs L;
        L.a_ref = m->a_ref.get() + first, L.b_ref = m->b_ref.get() + first;
        L.n = n, L.first = first, L.first_next = first + n;
        L.digit = -1, L.last = d == p->level ? 1 : 0;
        if (d <= p->level) {
            const int s = p->level - d;
            L.digit = 4 * ((p->corner[0] >> s) & 1) + 2 * ((p->corner[1] >> s) & 1) + ((p->corner[2] >> s) & 1);
        }
        L.mask = m->mask.get() + first, L.count = count.get(), L.first_child = m->first_child.get() + first;
        L.a_next = m->a_ref.get() + first + n, L.b_next = m->b_ref.get() + first + n, L.parent_next = m->parent.get() + first + n;
        L.ctr = ctr.dev.get();
        hipLaunchKernelGGL(merge_level_kernel, dim3(std::min(mnv::blocks_for(n * 8), (unsigned)kLevelGrid)), dim3(256), 0, stream, m->in, L);
        if ((rc = check_hip(hipGetLastError(), "merge_level_kernel"))) return rc;
        size_t tb = tmp_bytes;
        if ((rc = check_hip(rocprim::exclusive_scan(tmp.get(), tb, count.get(), scanned.get(), 0u, (size_t)n, rocprim::plus<uint32_t>(), stream), "exclusive_scan")) ||
            (rc = check_hip(hipMemcpyAsync(ctr.host.get(), ctr.dev.get(), 48, hipMemcpyDeviceToHost, stream), "merge counters")) ||
            (rc = check_hip(hipMemcpyAsync(&tail[0], count.get() + (n - 1), 4, hipMemcpyDeviceToHost, stream), "copy a level size")) ||
            (rc = check_hip(hipMemcpyAsync(&tail[1], scanned.get() + (n - 1), 4, hipMemcpyDeviceToHost, stream), "copy a level size")) ||
            (rc = check_hip(hipStreamSynchronize(stream), who)))
            return rc;
        if (ctr.host.get()[0] & 1ull) return set_error(MNV_E_INVALID, std::string(who) + ": a child link leaves its tree (outside [1, capacity))");
        const int64_t n_next = (int64_t)tail[0] + tail[1];
        if (n_next == 0) {
            L.count = scanned.get();  // (first_child of the deepest level: never followed, but defined)
            hipLaunchKernelGGL(merge_emit_kernel, dim3(mnv::blocks_for(n * 8)), dim3(256), 0, stream, m->in, L, n_next);
            if ((rc = check_hip(hipGetLastError(), "merge_emit_kernel"))) return rc;
            first += n;
            break;
        }
        if (d + 1 > kMaxMergeDepth) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": the merged tree is deeper than 23 levels");
        if (first + n + n_next > 0x7fffffffll) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 merged chunks");
        if (first + n + n_next > bound)
            return set_error(MNV_E_INVALID, std::string(who) + ": more merged chunks than the inputs hold (a chunk of an input is reached twice)");
        L.count = scanned.get();
        hipLaunchKernelGGL(merge_emit_kernel, dim3(mnv::blocks_for(n * 8)), dim3(256), 0, stream, m->in, L, n_next);
        if ((rc = check_hip(hipGetLastError(), "merge_emit_kernel"))) return rc;
        stats->chunks_at_depth[d + 1] = n_next;
        first += n;
        n = n_next;
    }
    if ((rc = check_hip(hipStreamSynchronize(stream), who))) return rc;  // the scratch goes
    m->capacity = first;
    stats->capacity = first;
    const unsigned long long *c = ctr.host.get();
    stats->rows_from_a = (int64_t)c[1], stats->rows_from_b = (int64_t)c[2], stats->rows_blended = (int64_t)c[3];
    stats->pushed_a = (int64_t)c[4], stats->pushed_b = (int64_t)c[5];
    *out = m.release();
    return MNV_OK;
}

int mnv_tree_merge_write(const mnv_tree_merge *m, int32_t *child_out, uint16_t *data_out, int32_t *parent_out, int16_t *sample_counts_out, int32_t *src_a_out,
                         int32_t *src_b_out, void *hip_stream) {
    const char *who = "mnv_tree_merge_write";
    if (!m || !child_out || !data_out) return set_error(MNV_E_INVALID, std::string(who) + ": null argument");
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, std::string(who) + ": data_out must be 16-byte aligned");
    if (!mnv::on_device(child_out) || !mnv::on_device(data_out) || (parent_out && !mnv::on_device(parent_out)) || (sample_counts_out && !mnv::on_device(sample_counts_out)) ||
        (src_a_out && !mnv::on_device(src_a_out)) || (src_b_out && !mnv::on_device(src_b_out)))
        return set_error(MNV_E_INVALID, std::string(who) + ": the outputs must be device arrays");
    WriteArgs P;
    P.a_ref = m->a_ref.get(), P.b_ref = m->b_ref.get(), P.first_child = m->first_child.get(), P.parent = m->parent.get(), P.mask = m->mask.get();
    P.n_chunks = m->capacity;
    P.log2_g = 3;  // lanes per chunk: 8, 16, 32 or 64, at least data_dim where that is below 64
    while ((1 << P.log2_g) < m->in.dd && P.log2_g < 6) ++P.log2_g;
    P.child_out = child_out, P.data_out = data_out, P.parent_out = parent_out, P.counts_out = sample_counts_out, P.src_a_out = src_a_out, P.src_b_out = src_b_out;
    hipLaunchKernelGGL(merge_write_kernel, dim3(mnv::blocks_for(m->capacity, 256 >> P.log2_g)), dim3(256), 0, (hipStream_t)hip_stream, m->in, P);
    return check_hip(hipGetLastError(), "merge_write_kernel");
}

void mnv_tree_merge_destroy(mnv_tree_merge *m) { delete m; }

}  // extern "C"
