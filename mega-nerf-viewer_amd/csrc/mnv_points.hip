// mnv_points.hip -- a tree from a coloured point cloud (the points contract of include/mnv.h): mnv_point_tree_create / add / finish / write.
// The result is an ordinary N3Tree in the reference's array layout: every march kernel renders it unchanged.
//
// Every number that decides an output byte is an integer: a point's voxel is one binary32 product, one sum and a floor per axis, a voxel's
// record is a count and three 64-bit sums of 8-bit channels, a colour is a table entry picked by an integer mean.  So the order of the
// points, the split into calls, the launch shape and the order in which any atomic lands cannot change a byte (the one atomic counts
// dropped points).
//
// add, per batch of at most kMaxBatch points:
//   keys     one thread per point: 64-bit Morton code (all-ones for a dropped point) and the packed colour; the handle's records so far join
//            the batch as elements of their own (code, index | bit 31), so one sort and one reduction serve a first add and a merge alike
//   sort     rocprim::radix_sort_pairs over the 3 D significant bits
//   count    heads (an element whose code differs from its left neighbour's) per wavefront tile of kTile elements; an exclusive scan of the
//            tile counts gives every head its record index; the host reads the total once and sizes the new record list
//   reduce   per wavefront: a segmented inclusive scan of (count, three sums) over 64 elements (heads by ballot, six shuffle steps), runs
//            that end inside the 64 written by their last lane, the open run carried in wave-uniform registers to the next 64.  A run whose
//            head lies in the tile is written by that tile (complete, or the part inside the tile); what a tile holds of a run that began
//            in an earlier tile goes to the tile's `pre` slot
//   fix-up   one thread per tile whose last run goes on: adds the `pre` slots of the tiles after it, up to the first that holds a head.
//            Every record has one writer per kernel: no atomics
// A dropped point sorts with the largest code (only the low 3 D bits are sorted) and adds nothing to the run it lands in; it can leave a
// record of count 0 there, which nothing counts.
//
// finish: occupied records (count >= min_points) compacted to a sorted code list; for d = D .. 2 the chunk list of depth d is the list below
// shifted right by three bits with duplicates removed (flags, inclusive scan, scatter: the lists are sorted already).  One read-back per
// level sizes the next list.  write: one launch per depth, a group of 8 .. 64 lanes per chunk; the group's first eight lanes find their
// voxel's child chunk (binary search in the next level's list) or record (binary search in the records), the group then stores the chunk's
// rows as data_dim 16-byte segments, as mnv_lod.hip does.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mnv_tree_walk.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kMaxPointDepth = 21;             // 3 * 21 = 63 bits of code; the all-ones key is no code
constexpr int64_t kMaxBatch = (int64_t)1 << 27;  // points sorted at a time: bounds the scratch of one add
constexpr int kSteps = 8, kTile = 64 * kSteps;   // elements per wavefront tile
constexpr int kWaves = 4;                        // wavefronts per workgroup
constexpr uint32_t kRecordBit = 0x80000000u;     // an element's payload: a packed colour, or the index of a record with this bit
constexpr uint64_t kDropped = ~0ull;

struct Rec {  // one distinct voxel: 40 bytes
    uint64_t code, n, r, g, b;
};

struct Acc {
    uint64_t n, r, g, b;
};

// ---------------------------------------------------------------------------------------------------- keys

struct KeyParams {
    float offset[3], scale[3];
    float cells;  // 2^D
};

// bit i of v (i < 21) to bit 3 i
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__device__ __forceinline__ bool finite_f(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(256) points_key_kernel(const float *__restrict__ xyz, const uint8_t *__restrict__ rgb, int64_t n, KeyParams P,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, unsigned long long *__restrict__ dropped) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    bool ok = valid;
    uint64_t key = kDropped;
    uint32_t val = 0;
    if (valid) {
        uint32_t cell[3];
        for (int k = 0; k < 3; ++k) {
            const float p = xyz[i * 3 + k];
            const float m = P.scale[k] * p;
            const float q = P.offset[k] + m;
            ok = ok && finite_f(p) && finite_f(q) && q >= 0.f && q < 1.f;
            cell[k] = ok ? (uint32_t)(int)floorf(q * P.cells) : 0u;
        }
        if (ok) key = (spread3(cell[0]) << 2) | (spread3(cell[1]) << 1) | spread3(cell[2]);
        val = (uint32_t)rgb[i * 3 + 0] | ((uint32_t)rgb[i * 3 + 1] << 8) | ((uint32_t)rgb[i * 3 + 2] << 16);
        keys[i] = key;
        vals[i] = val;
    }
    const unsigned long long m = __ballot(valid && !ok);
    if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(dropped, (unsigned long long)__popcll(m));
}

// the handle's records as elements behind the batch's points
__global__ void __launch_bounds__(256) points_record_keys_kernel(const Rec *__restrict__ recs, int64_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = recs[i].code;
    vals[i] = kRecordBit | (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------------- runs of equal codes

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int delta) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, delta), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), delta);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ Acc acc_add(Acc a, Acc b) { return Acc{a.n + b.n, a.r + b.r, a.g + b.g, a.b + b.b}; }
__device__ __forceinline__ Acc acc_from(Acc a, int src) { return Acc{shfl64(a.n, src), shfl64(a.r, src), shfl64(a.g, src), shfl64(a.b, src)}; }

// 64 sorted elements from `at`: this lane's code, and whether it starts a run.  left: the code before `at` (ignored when at == 0).
__device__ __forceinline__ bool run_head(const uint64_t *__restrict__ keys, int64_t at, int64_t end, uint64_t mask, int lane, uint64_t left, uint64_t *code_out,
                                         uint64_t *key_out) {
    const int64_t i = at + lane;
    const bool valid = i < end;
    const uint64_t key = valid ? keys[i] : 0ull, code = key & mask;
    uint64_t prev = shfl_up64(code, 1);
    if (lane == 0) prev = left;
    *code_out = code;
    *key_out = key;
    return valid && (i == 0 || code != prev);
}

// heads per tile
__global__ void __launch_bounds__(64 * kWaves) points_count_kernel(const uint64_t *__restrict__ keys, int64_t n, uint64_t mask, uint32_t *__restrict__ tile_heads) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), base = w * kTile;
    if (base >= n) return;  // (the whole wavefront)
    uint64_t left = base > 0 ? keys[base - 1] & mask : 0ull;
    uint32_t heads = 0;
    for (int s = 0; s < kSteps; ++s) {
        const int64_t at = base + s * 64;
        if (at >= n) break;
        uint64_t code, key;
        const bool head = run_head(keys, at, n, mask, lane, left, &code, &key);
        heads += (uint32_t)__popcll(__ballot(head));
        left = shfl64(code, 63);
    }
    if (lane == 0) tile_heads[w] = heads;
}

struct TileInfo {
    uint32_t flags;      // 1: the tile's first element goes on a run of an earlier tile (pre holds that part), 2: the tile holds a head
    uint32_t last_rank;  // record of the tile's last head
};

__global__ void __launch_bounds__(64 * kWaves) points_reduce_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n, uint64_t mask,
                                                                     const Rec *__restrict__ old_recs, const uint32_t *__restrict__ tile_base,
                                                                     Rec *__restrict__ recs, Acc *__restrict__ pre, TileInfo *__restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), base = w * kTile;
    if (base >= n) return;  // (the whole wavefront)
    uint64_t left = base > 0 ? keys[base - 1] & mask : 0ull;
    uint32_t rank = tile_base[w];  // heads before the ones of this step
    Acc carry{0, 0, 0, 0};         // the open run: wave-uniform
    uint64_t carry_code = 0;
    uint32_t carry_rank = 0;
    bool carry_owned = false;  // its head lies in this tile
    bool has_pre = false;
    for (int s = 0; s < kSteps; ++s) {
        const int64_t at = base + s * 64;
        if (at >= n) break;
        const int nvalid = (int)(n - at < 64 ? n - at : 64);
        uint64_t code, key;
        const bool head = run_head(keys, at, n, mask, lane, left, &code, &key);
        left = shfl64(code, 63);
        if (s == 0) has_pre = __shfl((int)head, 0) == 0;
        Acc a{0, 0, 0, 0};
        if (lane < nvalid && key != kDropped) {
            const uint32_t v = vals[at + lane];
            if (v & kRecordBit) {
                const Rec o = old_recs[v & ~kRecordBit];
                a = Acc{o.n, o.r, o.g, o.b};
            } else {
                a = Acc{1ull, v & 255u, (v >> 8) & 255u, (v >> 16) & 255u};
            }
        }
        const unsigned long long hm = __ballot(head);
        for (int off = 1; off < 64; off <<= 1) {  // segmented inclusive scan: add the lane `off` to the left unless a head lies in (lane - off, lane]
            const Acc t{shfl_up64(a.n, off), shfl_up64(a.r, off), shfl_up64(a.g, off), shfl_up64(a.b, off)};
            if (lane >= off && ((hm >> (lane - off + 1)) & ((1ull << off) - 1ull)) == 0ull) a = acc_add(a, t);
        }
        if (hm == 0ull) {
            carry = acc_add(carry, acc_from(a, nvalid - 1));
            continue;
        }
        const int first = __ffsll((long long)hm) - 1, last = 63 - __clzll((long long)hm);
        if (first > 0) carry = acc_add(carry, acc_from(a, first - 1));
        if (s > 0 || first > 0 || has_pre) {  // the open run ends before `first`
            if (lane == 0) {
                if (carry_owned)
                    recs[carry_rank] = Rec{carry_code, carry.n, carry.r, carry.g, carry.b};
                else
                    pre[w] = carry;
            }
        }
        // runs that begin and end inside these 64: their last lane writes them
        if (lane >= first && lane + 1 < nvalid && ((hm >> (lane + 1)) & 1ull)) {
            const unsigned long long upto = hm & (~0ull >> (63 - lane));
            const int h = 63 - __clzll((long long)upto);
            recs[rank + (uint32_t)__popcll(hm & ((1ull << h) - 1ull))] = Rec{code, a.n, a.r, a.g, a.b};
        }
        carry = acc_from(a, nvalid - 1);
        carry_code = shfl64(code, last);
        carry_rank = rank + (uint32_t)__popcll(hm) - 1u;
        carry_owned = true;
        rank += (uint32_t)__popcll(hm);
    }
    if (lane == 0) {
        if (carry_owned)
            recs[carry_rank] = Rec{carry_code, carry.n, carry.r, carry.g, carry.b};
        else
            pre[w] = carry;
        info[w] = TileInfo{(has_pre ? 1u : 0u) | (carry_owned ? 2u : 0u), carry_rank};
    }
}

// a tile whose last run goes on into the next tiles collects what they hold of it
__global__ void __launch_bounds__(256) points_fixup_kernel(const Acc *__restrict__ pre, const TileInfo *__restrict__ info, int64_t n_tiles, Rec *__restrict__ recs) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w + 1 >= n_tiles) return;
    const TileInfo me = info[w];
    if (!(me.flags & 2u) || !(info[w + 1].flags & 1u)) return;
    Rec r = recs[me.last_rank];
    for (int64_t k = w + 1; k < n_tiles; ++k) {
        const TileInfo t = info[k];
        if (!(t.flags & 1u)) break;
        const Acc p = pre[k];
        r.n += p.n, r.r += p.r, r.g += p.g, r.b += p.b;
        if (t.flags & 2u) break;
    }
    recs[me.last_rank] = r;
}

// ---------------------------------------------------------------------------------------------------- structure

// flag[i]: record i is occupied; *distinct += records with at least one point.  A fixed grid walks the records with its stride and every
// wavefront adds its count once: one atomic per 64 records on one address was served one after the other (1.37 ms for 7.3 M records)
constexpr int kOccupiedGrid = 1024;
__global__ void __launch_bounds__(256) points_occupied_kernel(const Rec *__restrict__ recs, int64_t n, uint64_t min_points, uint32_t *__restrict__ flag,
                                                               unsigned long long *__restrict__ distinct) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long total = 0;
    for (int64_t at = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); at < n; at += stride) {  // (wave-uniform bounds)
        const int64_t i = at + lane;
        uint64_t c = 0;
        if (i < n) {
            c = recs[i].n;
            flag[i] = c >= min_points ? 1u : 0u;
        }
        total += (unsigned long long)__popcll(__ballot(c > 0));
    }
    if (lane == 0 && total) atomicAdd(distinct, total);
}

// flag[i]: in[i] >> 3 differs from its left neighbour's
__global__ void __launch_bounds__(256) points_parent_flags_kernel(const uint64_t *__restrict__ in, int64_t n, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || (in[i] >> 3) != (in[i - 1] >> 3)) ? 1u : 0u;
}

// pos: the inclusive scan of the flags; a flagged element goes to pos - 1
template <bool FROM_RECORDS>
__global__ void __launch_bounds__(256) points_scatter_kernel(const void *__restrict__ in, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t n,
                                                              uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    out[pos[i] - 1u] = FROM_RECORDS ? static_cast<const Rec *>(in)[i].code : static_cast<const uint64_t *>(in)[i] >> 3;
}

// ---------------------------------------------------------------------------------------------------- arrays

struct WriteParams {
    const uint64_t *level;  // this depth's chunks: the code of the voxel above each (null: the root)
    int64_t n_chunks, first;  // ... and the index of the first of them
    bool leaf_level;        // depth D: the voxels are looked up in the records
    const uint64_t *next;   // otherwise in the next depth's list
    int64_t n_next, first_next;
    const Rec *recs;  // depth D: the records
    int64_t n_recs;
    uint64_t min_points;
    const uint16_t *table;
    int32_t dd, colour_stride, log2_g;  // colour channel c sits in column c * colour_stride
    uint16_t sigma;
    int32_t *child;
    uint16_t *data;
    int32_t *parent;
    int16_t *sample_counts;
    uint32_t *counts;
};

// index of `v` in a sorted list read through `at`, or -1
template <typename At>
__device__ __forceinline__ int64_t find_code(At at, int64_t n, uint64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (at(mid) < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && at(lo) == v ? lo : -1;
}

__global__ void __launch_bounds__(256) points_write_kernel(WriteParams P) {
    __shared__ uint2 voxel_info[32][8];  // per group and voxel: the three colour halfs and the occupied bit
    const int G = 1 << P.log2_g, grp = threadIdx.x >> P.log2_g, gl = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 >> P.log2_g) + grp;
    const bool active = k < P.n_chunks;
    const int64_t c = P.first + k;
    if (active && gl < 8) {
        const uint64_t v = (P.level ? P.level[k] : 0ull) * 8ull + (uint64_t)gl;
        int32_t link = 0;
        uint32_t count = 0;
        uint2 vi = make_uint2(0u, 0u);
        if (!P.leaf_level) {
            const uint64_t *next = P.next;
            const int64_t m = find_code([next](int64_t i) { return next[i]; }, P.n_next, v);
            if (m >= 0) {
                link = (int32_t)(P.first_next + m - c);
                if (P.parent) P.parent[P.first_next + m] = (int32_t)(c * 8 + gl);
            }
        } else {
            const Rec *recs = P.recs;
            const int64_t m = find_code([recs](int64_t i) { return recs[i].code; }, P.n_recs, v);
            if (m >= 0) {
                const Rec r = recs[m];
                count = (uint32_t)r.n;
                if (r.n >= P.min_points) {
                    const uint64_t d2 = 2ull * r.n;
                    const uint32_t mr = (uint32_t)((2ull * r.r + r.n) / d2), mg = (uint32_t)((2ull * r.g + r.n) / d2), mb = (uint32_t)((2ull * r.b + r.n) / d2);
                    vi = make_uint2((uint32_t)P.table[mr] | ((uint32_t)P.table[mg] << 16), (uint32_t)P.table[mb] | 0x10000u);
                }
            }
        }
        voxel_info[grp][gl] = vi;
        P.child[c * 8 + gl] = link;
        if (P.sample_counts) P.sample_counts[c * 8 + gl] = 8;
        if (P.counts) P.counts[c * 8 + gl] = count;
        if (P.parent && c == 0 && gl == 0) P.parent[0] = -1;
    }
    __syncthreads();
    if (!active) return;
    uint4 *out4 = reinterpret_cast<uint4 *>(P.data) + c * P.dd;
    for (int s = gl; s < P.dd; s += G) {
        mnv::Seg16 a;
        a.v = make_uint4(0u, 0u, 0u, 0u);
        if (P.leaf_level) {
            for (int i = 0; i < 8; ++i) {
                const int at = 8 * s + i, j = at / P.dd, col = at - j * P.dd;
                const uint2 vi = voxel_info[grp][j];
                if (!(vi.y & 0x10000u)) continue;
                if (col == P.dd - 1)
                    a.h[i] = P.sigma;
                else if (col == 0)
                    a.h[i] = (uint16_t)(vi.x & 0xffffu);
                else if (col == P.colour_stride)
                    a.h[i] = (uint16_t)(vi.x >> 16);
                else if (col == 2 * P.colour_stride)
                    a.h[i] = (uint16_t)(vi.y & 0xffffu);
            }
        }
        out4[s] = a.v;
    }
}

// ---------------------------------------------------------------------------------------------------- host

int check_format(int32_t format, int32_t basis_dim, const char *who) {
    if (format == MNV_FORMAT_RGBA) return MNV_OK;
    if (format == MNV_FORMAT_SH && (basis_dim == 1 || basis_dim == 4 || basis_dim == 9 || basis_dim == 16 || basis_dim == 25)) return MNV_OK;
    return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": the format must be RGBA, or SH with basis_dim 1, 4, 9, 16 or 25");
}

void colour_table(int32_t format, uint16_t out[256]) {
    for (int v = 0; v < 256; ++v) {
        if (format == MNV_FORMAT_RGBA) {
            out[v] = mnv::half((float)v / 255.f);
        } else {
            double x = (double)v / 255.0;
            x = x < 1.0 / 512.0 ? 1.0 / 512.0 : x > 511.0 / 512.0 ? 511.0 / 512.0 : x;
            out[v] = mnv::half((float)(std::log(x / (1.0 - x)) / 0.28209479177387814));
        }
    }
}

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

}  // namespace

struct mnv_point_tree {
    mnv_points_params p;
    int dd = 0, colour_stride = 1;
    uint64_t mask = 0;
    uint16_t sigma_half = 0;
    mnv::Buffer<uint16_t> table;
    mnv::Mirrored<unsigned long long> ctr;  // [0] dropped points of the batch in flight, [1] records that hold a point
    mnv::Buffer<Rec> recs;                  // sorted by code
    int64_t n_recs = 0;
    mnv::Buffer<uint8_t> scratch;  // grow-only: the sort's arrays and the tiles' slots
    int64_t accepted = 0, dropped = 0;
    bool finished = false;
    mnv::Buffer<uint64_t> level[kMaxPointDepth + 2];  // [d], d = 2 .. D: the code of the voxel above every chunk of depth d
    mnv_points_stats stats;
};

namespace {

// one batch of at most kMaxBatch points: sorted with the records so far and reduced to the new record list
int add_batch(mnv_point_tree *t, const float *xyz, const uint8_t *rgb, int64_t n, hipStream_t stream) {
    int rc;
    const int64_t n_old = t->n_recs, n_elem = n + n_old;
    if (n_elem > 0x7fffffffll) return set_error(MNV_E_UNSUPPORTED, "mnv_point_tree_add: more than 2^31 - 1 points and distinct voxels in one batch");
    const int key_bits = 3 * t->p.depth;
    const int64_t n_tiles = (n_elem + kTile - 1) / kTile;
    size_t tmp_sort = 0, tmp_scan = 0;
    {  // (the two halves of a double buffer: the sort keeps no copy of its own, its temporary is histograms)
        rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
        rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
        (void)rocprim::radix_sort_pairs(nullptr, tmp_sort, k, v, (size_t)n_elem, 0, key_bits, stream);
    }
    (void)rocprim::exclusive_scan(nullptr, tmp_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n_tiles, rocprim::plus<uint32_t>(), stream);
    Carver c;
    const size_t o_keys = c.take((size_t)n_elem * 8), o_keys2 = c.take((size_t)n_elem * 8), o_vals = c.take((size_t)n_elem * 4), o_vals2 = c.take((size_t)n_elem * 4);
    const size_t o_heads = c.take((size_t)n_tiles * 4), o_base = c.take((size_t)n_tiles * 4), o_pre = c.take((size_t)n_tiles * sizeof(Acc));
    const size_t o_info = c.take((size_t)n_tiles * sizeof(TileInfo)), o_tmp = c.take(std::max(tmp_sort, tmp_scan));
    if ((rc = check_hip(mnv::grow(t->scratch, c.off, c.off + c.off / 8, stream, true), "hipMalloc(point scratch)"))) return rc;
    uint8_t *ws = t->scratch.get();
    uint64_t *keys = reinterpret_cast<uint64_t *>(ws + o_keys);
    uint32_t *vals = reinterpret_cast<uint32_t *>(ws + o_vals);
    uint32_t *heads = reinterpret_cast<uint32_t *>(ws + o_heads), *base = reinterpret_cast<uint32_t *>(ws + o_base);
    Acc *pre = reinterpret_cast<Acc *>(ws + o_pre);
    TileInfo *info = reinterpret_cast<TileInfo *>(ws + o_info);

    KeyParams K;
    for (int k = 0; k < 3; ++k) K.offset[k] = t->p.offset[k], K.scale[k] = t->p.scale[k];
    K.cells = (float)((int64_t)1 << t->p.depth);
    if ((rc = check_hip(hipMemsetAsync(t->ctr.dev.get(), 0, 8, stream), "clear the drop counter"))) return rc;
    hipLaunchKernelGGL(points_key_kernel, dim3(mnv::blocks_for(n)), dim3(256), 0, stream, xyz, rgb, n, K, keys, vals, t->ctr.dev.get());
    if ((rc = check_hip(hipGetLastError(), "points_key_kernel"))) return rc;
    if (n_old > 0) {
        hipLaunchKernelGGL(points_record_keys_kernel, dim3(mnv::blocks_for(n_old)), dim3(256), 0, stream, t->recs.get(), n_old, keys + n, vals + n);
        if ((rc = check_hip(hipGetLastError(), "points_record_keys_kernel"))) return rc;
    }
    size_t tmp = tmp_sort;
    rocprim::double_buffer<uint64_t> key_pair(keys, reinterpret_cast<uint64_t *>(ws + o_keys2));
    rocprim::double_buffer<uint32_t> val_pair(vals, reinterpret_cast<uint32_t *>(ws + o_vals2));
    if ((rc = check_hip(rocprim::radix_sort_pairs(ws + o_tmp, tmp, key_pair, val_pair, (size_t)n_elem, 0, key_bits, stream), "radix_sort_pairs"))) return rc;
    const uint64_t *sorted = key_pair.current();  // (whichever half the last pass wrote)
    const uint32_t *svals = val_pair.current();
    hipLaunchKernelGGL(points_count_kernel, dim3(mnv::blocks_for(n_tiles, kWaves)), dim3(64 * kWaves), 0, stream, sorted, n_elem, t->mask, heads);
    if ((rc = check_hip(hipGetLastError(), "points_count_kernel"))) return rc;
    tmp = tmp_scan;
    if ((rc = check_hip(rocprim::exclusive_scan(ws + o_tmp, tmp, heads, base, 0u, (size_t)n_tiles, rocprim::plus<uint32_t>(), stream), "exclusive_scan"))) return rc;
    uint32_t last[2] = {0, 0};
    if ((rc = check_hip(hipMemcpyAsync(&last[0], base + (n_tiles - 1), 4, hipMemcpyDeviceToHost, stream), "copy the record count")) ||
        (rc = check_hip(hipMemcpyAsync(&last[1], heads + (n_tiles - 1), 4, hipMemcpyDeviceToHost, stream), "copy the record count")) ||
        (rc = check_hip(hipMemcpyAsync(t->ctr.host.get(), t->ctr.dev.get(), 8, hipMemcpyDeviceToHost, stream), "copy the drop counter")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "mnv_point_tree_add")))
        return rc;
    const int64_t n_new = (int64_t)last[0] + last[1], n_dropped = (int64_t)t->ctr.host.get()[0];
    if (t->accepted + (n - n_dropped) > 0xffffffffll) return set_error(MNV_E_UNSUPPORTED, "mnv_point_tree_add: more than 2^32 - 1 accepted points");
    mnv::Buffer<Rec> recs;
    if ((rc = check_hip(recs.alloc((size_t)n_new), "hipMalloc(point records)"))) return rc;
    hipLaunchKernelGGL(points_reduce_kernel, dim3(mnv::blocks_for(n_tiles, kWaves)), dim3(64 * kWaves), 0, stream, sorted, svals, n_elem, t->mask, t->recs.get(), base,
                       recs.get(), pre, info);
    if ((rc = check_hip(hipGetLastError(), "points_reduce_kernel"))) return rc;
    if (n_tiles > 1) {
        hipLaunchKernelGGL(points_fixup_kernel, dim3(mnv::blocks_for(n_tiles)), dim3(256), 0, stream, pre, info, n_tiles, recs.get());
        if ((rc = check_hip(hipGetLastError(), "points_fixup_kernel"))) return rc;
    }
    if ((rc = check_hip(hipStreamSynchronize(stream), "mnv_point_tree_add"))) return rc;  // the old records go
    t->recs = std::move(recs);
    t->n_recs = n_new;
    t->accepted += n - n_dropped;
    t->dropped += n_dropped;
    return MNV_OK;
}

// the flagged elements of `in` (records, or a code list shifted right by three bits) compacted into `out`; *n_out: how many
template <bool FROM_RECORDS>
int compact(const void *in, int64_t n, uint32_t *flag, uint32_t *pos, void *tmp, size_t tmp_bytes, mnv::Buffer<uint64_t> &out, int64_t *n_out, hipStream_t stream) {
    int rc;
    *n_out = 0;
    out.reset();
    if (n == 0) return MNV_OK;
    if ((rc = check_hip(rocprim::inclusive_scan(tmp, tmp_bytes, flag, pos, (size_t)n, rocprim::plus<uint32_t>(), stream), "inclusive_scan"))) return rc;
    uint32_t total = 0;
    if ((rc = check_hip(hipMemcpyAsync(&total, pos + (n - 1), 4, hipMemcpyDeviceToHost, stream), "copy a list size")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "mnv_point_tree_finish")))
        return rc;
    *n_out = total;
    if (total == 0) return MNV_OK;
    if ((rc = check_hip(out.alloc(total), "hipMalloc(chunk list)"))) return rc;
    hipLaunchKernelGGL(points_scatter_kernel<FROM_RECORDS>, dim3(mnv::blocks_for(n)), dim3(256), 0, stream, in, flag, pos, n, out.get());
    return check_hip(hipGetLastError(), "points_scatter_kernel");
}

}  // namespace

extern "C" {

int mnv_points_colour_table(int32_t format, int32_t basis_dim, uint16_t out[256]) {
    if (!out) return set_error(MNV_E_INVALID, "mnv_points_colour_table: null output");
    int rc;
    if ((rc = check_format(format, basis_dim, "mnv_points_colour_table"))) return rc;
    colour_table(format, out);
    return MNV_OK;
}

int mnv_point_tree_create(const mnv_points_params *p, mnv_point_tree **out) {
    if (!p || !out) return set_error(MNV_E_INVALID, "mnv_point_tree_create: null argument");
    *out = nullptr;
    if (p->depth < 1 || p->depth > kMaxPointDepth) return set_error(MNV_E_INVALID, "mnv_point_tree_create: depth outside 1 .. 21");
    if (p->min_points == 0) return set_error(MNV_E_INVALID, "mnv_point_tree_create: min_points must be at least 1");
    if (!std::isfinite(p->sigma) || !(p->sigma > 0.f)) return set_error(MNV_E_INVALID, "mnv_point_tree_create: sigma must be finite and positive");
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(p->scale[k]) || !(p->scale[k] > 0.f)) return set_error(MNV_E_INVALID, "mnv_point_tree_create: a scale that is not finite and positive");
        if (!std::isfinite(p->offset[k])) return set_error(MNV_E_INVALID, "mnv_point_tree_create: an offset that is not finite");
    }
    int rc;
    if ((rc = check_format(p->format, p->basis_dim, "mnv_point_tree_create"))) return rc;
    int dev = -1;
    if ((rc = mnv::current_device(&dev))) return rc;
    auto *t = new mnv_point_tree();
    t->p = *p;
    t->dd = p->format == MNV_FORMAT_RGBA ? 4 : 3 * p->basis_dim + 1;
    t->colour_stride = p->format == MNV_FORMAT_RGBA ? 1 : p->basis_dim;
    t->mask = (1ull << (3 * p->depth)) - 1ull;
    t->sigma_half = mnv::half(p->sigma);
    std::memset(&t->stats, 0, sizeof(t->stats));
    uint16_t table[256];
    colour_table(p->format, table);
    if ((rc = check_hip(t->table.alloc(256), "hipMalloc(colour table)")) ||
        (rc = check_hip(hipMemcpy(t->table.get(), table, sizeof(table), hipMemcpyHostToDevice), "upload the colour table")) ||
        (rc = mnv::alloc_pair(t->ctr, 2, "hipMalloc(point counters)", "hipHostMalloc(point counters)"))) {
        delete t;
        return rc;
    }
    *out = t;
    return MNV_OK;
}

void mnv_point_tree_destroy(mnv_point_tree *t) { delete t; }

int mnv_point_tree_add(mnv_point_tree *t, const float *xyz, const uint8_t *rgb, int64_t n, void *hip_stream) {
    if (!t) return set_error(MNV_E_INVALID, "mnv_point_tree_add: null handle");
    if (n < 0) return set_error(MNV_E_INVALID, "mnv_point_tree_add: n < 0");
    if (n == 0) return MNV_OK;
    if (!xyz || !rgb) return set_error(MNV_E_INVALID, "mnv_point_tree_add: null points / colours");
    if (!mnv::on_device(xyz) || !mnv::on_device(rgb)) return set_error(MNV_E_INVALID, "mnv_point_tree_add: the points and colours must be device arrays");
    t->finished = false;
    for (int64_t at = 0; at < n; at += kMaxBatch) {
        const int rc = add_batch(t, xyz + at * 3, rgb + at * 3, std::min(kMaxBatch, n - at), (hipStream_t)hip_stream);
        if (rc) return rc;
    }
    return MNV_OK;
}

int mnv_point_tree_finish(mnv_point_tree *t, mnv_points_stats *stats, void *hip_stream) {
    if (!t || !stats) return set_error(MNV_E_INVALID, "mnv_point_tree_finish: null argument");
    int rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int D = t->p.depth;
    const int64_t n = t->n_recs;
    mnv_points_stats S;
    std::memset(&S, 0, sizeof(S));
    S.accepted = t->accepted;
    S.dropped = t->dropped;
    S.chunks_at_depth[1] = 1;
    for (auto &l : t->level) l.reset();
    t->finished = false;
    if (n > 0) {
        size_t tmp_bytes = 0;
        (void)rocprim::inclusive_scan(nullptr, tmp_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, rocprim::plus<uint32_t>(), stream);
        mnv::Buffer<uint32_t> flag, pos;
        mnv::Buffer<uint8_t> tmp;
        mnv::Buffer<uint64_t> occupied;
        if ((rc = check_hip(flag.alloc((size_t)n), "hipMalloc(flags)")) || (rc = check_hip(pos.alloc((size_t)n), "hipMalloc(ranks)")) ||
            (rc = check_hip(tmp.alloc(tmp_bytes + 256), "hipMalloc(scan scratch)")) ||
            (rc = check_hip(hipMemsetAsync(t->ctr.dev.get() + 1, 0, 8, stream), "clear the voxel counter")))
            return rc;
        hipLaunchKernelGGL(points_occupied_kernel, dim3(std::min(mnv::blocks_for(n), (unsigned)kOccupiedGrid)), dim3(256), 0, stream, t->recs.get(), n, (uint64_t)t->p.min_points, flag.get(),
                           t->ctr.dev.get() + 1);
        if ((rc = check_hip(hipGetLastError(), "points_occupied_kernel")) ||
            (rc = check_hip(hipMemcpyAsync(t->ctr.host.get() + 1, t->ctr.dev.get() + 1, 8, hipMemcpyDeviceToHost, stream), "copy the voxel counter")))
            return rc;
        int64_t m = 0;
        if ((rc = compact<true>(t->recs.get(), n, flag.get(), pos.get(), tmp.get(), tmp_bytes, occupied, &m, stream))) return rc;  // (waits: the counter is here)
        S.distinct_voxels = (int64_t)t->ctr.host.get()[1];
        S.occupied_voxels = m;
        const uint64_t *below = occupied.get();
        for (int d = D; d >= 2 && m > 0; --d) {
            hipLaunchKernelGGL(points_parent_flags_kernel, dim3(mnv::blocks_for(m)), dim3(256), 0, stream, below, m, flag.get());
            if ((rc = check_hip(hipGetLastError(), "points_parent_flags_kernel"))) return rc;
            int64_t m_up = 0;
            if ((rc = compact<false>(below, m, flag.get(), pos.get(), tmp.get(), tmp_bytes, t->level[d], &m_up, stream))) return rc;
            S.chunks_at_depth[d] = m_up;
            below = t->level[d].get();
            m = m_up;
        }
        if ((rc = check_hip(hipStreamSynchronize(stream), "mnv_point_tree_finish"))) return rc;  // the lists above go
    }
    int64_t capacity = 0;
    for (int d = 1; d < 24; ++d) capacity += S.chunks_at_depth[d];
    if (capacity > 0x7fffffffll) return set_error(MNV_E_UNSUPPORTED, "mnv_point_tree_finish: more than 2^31 - 1 chunks");
    t->stats = S;
    t->finished = true;
    *stats = S;
    return MNV_OK;
}

int mnv_point_tree_write(const mnv_point_tree *t, int32_t *child_out, uint16_t *data_out, int32_t *parent_out, int16_t *sample_counts_out, uint32_t *counts_out,
                         void *hip_stream) {
    if (!t || !child_out || !data_out) return set_error(MNV_E_INVALID, "mnv_point_tree_write: null argument");
    if (!t->finished) return set_error(MNV_E_INVALID, "mnv_point_tree_write: call mnv_point_tree_finish first (also after a later add)");
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_point_tree_write: data_out must be 16-byte aligned");
    if (!mnv::on_device(child_out) || !mnv::on_device(data_out) || (parent_out && !mnv::on_device(parent_out)) || (sample_counts_out && !mnv::on_device(sample_counts_out)) ||
        (counts_out && !mnv::on_device(counts_out)))
        return set_error(MNV_E_INVALID, "mnv_point_tree_write: the outputs must be device arrays");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int D = t->p.depth;
    int log2_g = 3;  // lanes per chunk: 8, 16, 32 or 64, at least data_dim where that is below 64
    while ((1 << log2_g) < t->dd && log2_g < 6) ++log2_g;
    int64_t first = 0;
    for (int d = 1; d <= D; ++d) {
        const int64_t n_chunks = t->stats.chunks_at_depth[d];
        if (n_chunks == 0) break;
        WriteParams P;
        P.level = d == 1 ? nullptr : t->level[d].get();
        P.n_chunks = n_chunks;
        P.first = first;
        P.leaf_level = d == D;
        P.next = d < D ? t->level[d + 1].get() : nullptr;
        P.n_next = d < D ? t->stats.chunks_at_depth[d + 1] : 0;
        P.first_next = first + n_chunks;
        P.recs = t->recs.get();
        P.n_recs = t->n_recs;
        P.min_points = t->p.min_points;
        P.table = t->table.get();
        P.dd = t->dd;
        P.colour_stride = t->colour_stride;
        P.log2_g = log2_g;
        P.sigma = t->sigma_half;
        P.child = child_out;
        P.data = data_out;
        P.parent = parent_out;
        P.sample_counts = sample_counts_out;
        P.counts = counts_out;
        hipLaunchKernelGGL(points_write_kernel, dim3(mnv::blocks_for(n_chunks, 256 >> log2_g)), dim3(256), 0, stream, P);
        const int rc = check_hip(hipGetLastError(), "points_write_kernel");
        if (rc) return rc;
        first += n_chunks;
    }
    return MNV_OK;
}

}  // extern "C"
