// mnv_tree_walk.h -- what the passes over a tree's arrays share ("Walking and compacting a tree"): the wave-aggregated append and
// the binary16 helpers as device code each includer instantiates; the plain level walk, the compaction along a survivor predicate and the
// per-stream scratch as host functions of mnv_tree_walk.hip, which owns their kernels (the library has no relocatable device code).
#pragma once

#include <climits>
#include <mutex>

#include "mnv_internal.h"

namespace mnv {

// ---------------------------------------------------------------------------------------------------- device

// The lanes of a wavefront that push take consecutive slots of a list whose size is *counter, with one atomic per wavefront; store(slot)
// runs in each of them.  The bound of the list and what an overflow raises are the caller's, in `store`.  (A callback and not a returned
// slot: the store then sits under the test for an empty ballot, and every caller compiles to what it was with the idiom written out.)
template <typename Store>
__device__ __forceinline__ void wave_append(bool push, unsigned long long *counter, Store store) {
    const unsigned lane = __lane_id();
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const unsigned long long m = __ballot(push);
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if ((int)lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (push) store(base + (unsigned long long)__popcll(m & below));
    }
}

union Seg16 {  // eight halfs of a row array, moved as one 16-byte segment
    uint4 v;
    uint16_t h[8];
};

// binary16 <-> binary32 with integer arithmetic (and one exact binary32 add for subnormal results): no conversion instruction's denormal
// mode enters.  Not the march's half_bits_to_float (mnv_device.h), which answers non-finite bits differently.

__host__ __device__ __forceinline__ uint32_t f32_bits(float f) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}
__host__ __device__ __forceinline__ float bits_f32(uint32_t b) {
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// h(bits): the binary16 value as binary32; bits that are not finite read as +0
__host__ __device__ __forceinline__ float h(uint32_t b) {
    const uint32_t e = (b >> 10) & 31u, m = b & 0x3ffu, s = (b & 0x8000u) << 16;
    if (e == 31u) return 0.f;
    if (e == 0u) return bits_f32(s | f32_bits((float)m * 0x1p-24f));  // (a subnormal half is a normal float)
    return bits_f32(s | ((e + 112u) << 23) | (m << 13));
}

// binary32 -> binary16 bits, round to nearest even, once; subnormal results kept.  kSaturate: a result that would be infinite is 65504 (no
// NaN arrives); otherwise overflow goes to infinity and a NaN stays one
template <bool kSaturate>
__host__ __device__ __forceinline__ uint16_t round_half(float f) {
    uint32_t x = f32_bits(f);
    const uint32_t s = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (kSaturate && x >= 0x47800000u) return (uint16_t)(s | 0x7bffu);  // 65536 and more
    if (!kSaturate && x >= 0x7f800000u) return (uint16_t)(s | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (x < 0x38800000u) {  // below 2^-14: the sum with 0.5 has the spacing of binary16 subnormals (2^-24) and is rounded by the add
        const float r = bits_f32(x) + 0.5f;
        return (uint16_t)(s | (f32_bits(r) - 0x3f000000u));
    }
    x += 0xfffu + ((x >> 13) & 1u);
    x = (x - 0x38000000u) >> 13;
    return (uint16_t)(s | (kSaturate ? (x >= 0x7c00u ? 0x7bffu : x) : (x > 0x7c00u ? 0x7c00u : x)));
}
__host__ __device__ __forceinline__ uint16_t half(float f) { return round_half<false>(f); }
__host__ __device__ __forceinline__ uint16_t sat_half(float f) { return round_half<true>(f); }

// ---------------------------------------------------------------------------------------------------- the level walk

constexpr int kMaxWalkDepth = 23;    // as the packed accel
constexpr int kMaxWalkDevices = 16;  // devices that have walk scratch

// the arguments every pass checks first, in this order
int check_view(const mnv_tree_view *t, const char *who);

// A level-synchronous, top-down walk of `child` from the root: level d holds a list of the chunks of depth d.  A chunk enters the next list
// when it is reached for the first time (a 32-bit compare-and-swap on its word: the word it stores is the same, whoever stores it); a
// second arrival or a link outside [1, capacity) raises a fault bit that the host reads with the level's size.  The lists of all levels
// share one array of `capacity` entries.  The order inside a level depends on the schedule; it only decides which wavefront handles a
// chunk, no output byte.
struct LevelLists {
    int64_t offset[26] = {0};  // level d's entries: order[offset[d] .. offset[d + 1])
    int levels = 0;            // the deepest level that holds a chunk
    int64_t size(int d) const { return offset[d + 1] - offset[d]; }
    // walk_levels only: (chunk, flat index of the voxel above it), and the chunks' depths (0 = not reached)
    const int2 *order = nullptr;
    int32_t *depth = nullptr;
};

// The host half of such a walk.  launch(d, front, n_front, next, cap_next) queues the kernel of level d < max_depth: its front is the
// entries [front, front + n_front) of the lists, its arrivals go to [next, next + cap_next).  ctr: [0] the size of the next level, [1]
// the fault bits (1 a link outside the tree, 2 a chunk reached twice); both are zero before the first level.  One wait per level.  The
// levels found so far are in L after a refusal too.
template <typename Launch>
int walk_loop(LevelLists &L, int64_t capacity, int max_depth, Mirrored<unsigned long long> &ctr, const char *who, const char *kernel, hipStream_t stream, Launch launch) {
    int rc;
    L.offset[1] = 0;
    L.offset[2] = 1;
    L.levels = 1;
    for (int d = 1; d < max_depth; ++d) {
        launch(d, L.offset[d], L.size(d), L.offset[d + 1], capacity - L.offset[d + 1]);
        if ((rc = check_hip(hipGetLastError(), kernel)) ||
            (rc = check_hip(hipMemcpyAsync(ctr.host.get(), ctr.dev.get(), 16, hipMemcpyDeviceToHost, stream), "level counters")) ||
            (rc = check_hip(hipMemsetAsync(ctr.dev.get(), 0, 8, stream), "level counters")) || (rc = check_hip(hipStreamSynchronize(stream), kernel)))
            return rc;
        const unsigned long long fault = ctr.host.get()[1];
        if (fault & 1ull) return set_error(MNV_E_INVALID, std::string(who) + ": a child link leaves the tree (outside [1, capacity))");
        if (fault & 2ull) return set_error(MNV_E_INVALID, std::string(who) + ": a chunk is reached twice (not a tree)");
        const int64_t n_next = (int64_t)ctr.host.get()[0];
        if (n_next == 0) break;
        if (d + 1 > kMaxWalkDepth) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": tree deeper than 23 levels");
        L.offset[d + 2] = L.offset[d + 1] + n_next;
        L.levels = d + 1;
    }
    return MNV_OK;
}

// The plain walk keeps its lists, depth words and counters per device between calls (grow-only), so one call at a time per process uses
// them.  The guard is that turn: begin() takes it, and it ends only after the stream has been waited for -- also when an error leaves the
// caller early, since queued work may still use the scratch.  The caller keeps the guard on its stack until its last launch is queued.
class WalkGuard {
   public:
    WalkGuard() = default;
    WalkGuard(const WalkGuard &) = delete;
    WalkGuard &operator=(const WalkGuard &) = delete;
    ~WalkGuard() {
        if (lock_.owns_lock()) (void)hipStreamSynchronize(stream_);
    }
    int begin(hipStream_t stream);  // refuses when there is no current device (or one past kMaxWalkDevices)
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }

   private:
    std::unique_lock<std::mutex> lock_;
    hipStream_t stream_ = nullptr;
    int device_ = -1;
};

// All levels of the tree.  chunk_depth: device [capacity] or null (then the scratch's own words).  Waits for the guard's stream per level.
int walk_levels(const int32_t *child, int32_t capacity, int32_t *chunk_depth, const char *who, const WalkGuard &guard, LevelLists &out);

// rows of the chunks the walk did not reach (depth word 0), bit for bit from data_in to data_out
int copy_unreached(const uint16_t *data_in, uint16_t *data_out, const int32_t *chunk_depth, int32_t capacity, int32_t data_dim, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------- compaction

// Scratch of the asynchronous passes, one per (device, HIP stream): calls on a stream are ordered, so the next call may reuse what the
// previous one still reads.  Heap objects that live as long as the process (no hipFree after the runtime went) and never move.
struct StreamScratch {
    mnv::Buffer<uint8_t> bytes;  // compaction: ranks and the scan's temporary
    mnv::Buffer<int4> order;     // selection: the level lists, [capacity]
    mnv::Buffer<int32_t> mark;   // ... a word per chunk: reached
    mnv::Buffer<float> views;    // ... q [n_views][4], then R2 [n_views][24]
    mnv::Mirrored<unsigned long long> ctr;
};
std::mutex &stream_scratch_mutex();
StreamScratch &stream_scratch(int device, hipStream_t stream);  // (under stream_scratch_mutex())

// Which chunks a compaction keeps.  survives(c): chunk c stays; carries(c): the links out of a surviving c are followed at all; word() of
// words(): the survivor flag the rank scan sums.  The arrays are the caller's and may disagree with the tree.
struct DepthKeep {  // mnv_tree_truncate: the depth word in [1, max_depth], links cut at max_depth
    const int32_t *depth;
    int32_t max_depth;
    struct Flag {
        int32_t max_depth;
        __host__ __device__ int32_t operator()(int32_t d) const { return d >= 1 && d <= max_depth ? 1 : 0; }
    };
    const int32_t *words() const { return depth; }
    __host__ __device__ Flag flag() const { return Flag{max_depth}; }
    __device__ bool survives(int64_t c) const { return flag()(depth[c]) != 0; }
    __device__ bool carries(int64_t c) const { return depth[c] < max_depth; }
};
struct ByteKeep {  // mnv_tree_cut: the keep byte
    const uint8_t *keep;
    struct Flag {
        __host__ __device__ int32_t operator()(uint8_t k) const { return k != 0 ? 1 : 0; }
    };
    const uint8_t *words() const { return keep; }
    Flag flag() const { return Flag{}; }
    __device__ bool survives(int64_t c) const { return keep[c] != 0; }
    __device__ bool carries(int64_t) const { return true; }
};

// The survivors of `tree` in their old order in arrays of new_capacity chunks: ranks from an exclusive rocPRIM scan, a thread per (chunk,
// voxel) for links / parents / sample counts, a thread per 16-byte segment for the rows.  A link is carried when its target lies in
// [1, capacity), survives and has a rank below new_capacity.  Asynchronous on `stream`; `what` names the pass in the text of a failed
// allocation.  Instantiated for DepthKeep and ByteKeep.
template <typename Keep>
int compact_tree(const mnv_tree_view *tree, Keep keep, int32_t new_capacity, int32_t *child_out, uint16_t *data_out, int32_t *parent_out,
                 int16_t *sample_counts_out, const char *what, StreamScratch &S, hipStream_t stream);

}  // namespace mnv
