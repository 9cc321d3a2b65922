// mnv_extract.hip -- geometry out of a tree: point queries (mnv_accel_sample_points) and the iso-surface of the density as an indexed,
// coloured triangle mesh (mnv_extract_surface; table-free "surface nets").  The contract both follow is in include/mnv.h; this file is
// its device form, binary32 in the stated order under the Makefile's -ffp-contract=off and correctly rounded divide / sqrt.
//
// Everything reads the accel's node words (mnv_accel.h: one word per voxel, internal = the child chunk, leaf = depth and sigma bits) by a
// plain descent from the root.  A lattice sample ((i + 0.5) / n, ..) with n = 2^level descends by the bits of 2 i + 1 (level + 1 of them,
// zeros below): x * 2, floorf and x - floorf(x) are exact in binary32 on [0, 2), so this is query_single_from_root's float descent.
//
// Passes of an extraction (a brick is 8 x 8 x 8 dual cells and the 9 x 9 x 9 samples they span):
//   (a) candidates   one thread per brick: eight descents truncated at the brick's depth (level - 3) over {b, b + 1}^3; a brick whose
//                    eight bricks are single leaves on one side of iso has no active cell.  Flags are scanned (rocPRIM) into a list in
//                    ascending brick order.
//   (b) count        one workgroup per candidate: the samples staged in LDS, then per brick a 512-bit mask of active cells (one wave64
//                    ballot per word) and the vertex and quad counts.
//   (c) scans        exclusive, over all bricks: a brick's first vertex and first quad.
//   (d) emit         the same staging; a vertex's id is its brick's first vertex plus a popcount over the mask below its cell, a quad's
//                    slot its brick's first quad plus ballot popcounts over the owner cells below: no atomic decides an index, so the
//                    output order is the contract's whatever the schedule.
//   (e) colour       one thread per vertex (emit leaves the leaf's voxel index in the colour slot): the march's colour arithmetic
//                    (mnv_device.h) along d = -normal.
// Scratch is per brick: flag 4, list position 4, list 4, mask 64, counts 8, offsets 16 bytes.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mnv_accel_launch.h"

using mnv::Buffer;
using mnv::check_hip;
using mnv::Event;
using mnv::set_error;

namespace {

constexpr int kMaxDescent = 23;  // the accel refuses deeper trees (mnv_accel_build.hip)
constexpr int kBrick = 8, kStage = kBrick + 1, kStageN = kStage * kStage * kStage;

struct TreeRef {
    const uint32_t *nodes;
    const uint8_t *rows;
    int32_t capacity, max_depth, row_bytes, chan_halfs;
    float offset[3], scale[3];
};

enum { kLeaf = 0, kInner = 1, kFault = 2 };

// Root descent by lattice bits: q = coordinates on a lattice of 2^bits points per axis (zeros below), at most `limit` levels.
// kLeaf: `word` / `vox` describe the leaf.  kInner: `limit` levels down the voxel is still divided.  kFault: a link outside the tree.
__device__ __forceinline__ int descend_lattice(const TreeRef &T, uint32_t qx, uint32_t qy, uint32_t qz, int bits, int limit, uint32_t &word,
                                               int32_t &vox) {
    int32_t chunk = 0;
    for (int d = 1; d <= limit; ++d) {
        const int sh = bits - d;
        const uint32_t c = sh >= 0 ? ((((qx >> sh) & 1u) << 2) | (((qy >> sh) & 1u) << 1) | ((qz >> sh) & 1u)) : 0u;
        const int64_t v = (int64_t)chunk * 8 + (int64_t)c;
        const uint32_t w = T.nodes[v];
        if (w & mnv::kLeafBit) {
            word = w;
            vox = (int32_t)v;
            return kLeaf;
        }
        if (w < 1u || w >= (uint32_t)T.capacity) return kFault;  // report, do not follow
        chunk = (int32_t)w;
    }
    return kInner;
}

// sigma of a leaf word as the extraction reads it: bits that are not finite read as 0
__device__ __forceinline__ float leaf_sigma(uint32_t word) {
    const uint16_t h = (uint16_t)(word & 0xffffu);
    return (h & 0x7c00u) == 0x7c00u ? 0.f : mnv::half_bits_to_float(h);
}

// S(i, j, k) of the level-`level` lattice and the voxel it came from; a fault reads as an empty sample
__device__ __forceinline__ float lattice_sample(const TreeRef &T, int level, uint32_t i, uint32_t j, uint32_t k, int32_t &vox, uint32_t *fault) {
    uint32_t word = 0;
    const int limit = T.max_depth < kMaxDescent ? T.max_depth : kMaxDescent;
    const int st = descend_lattice(T, 2u * i + 1u, 2u * j + 1u, 2u * k + 1u, level + 1, limit, word, vox);
    if (st != kLeaf) {
        atomicOr(fault, 1u);
        vox = 0;
        return 0.f;
    }
    return leaf_sigma(word);
}

// ---------------------------------------------------------------------------------------------------- point queries

__global__ void __launch_bounds__(256) sample_points_kernel(TreeRef T, const float *__restrict__ points, int64_t n, int32_t *__restrict__ voxel,
                                                             int32_t *__restrict__ depth, float *__restrict__ sigma) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    int32_t vox = -1, dep = 0;
    float sg = 0.f;
    const uint32_t inf = 0x7f800000u;
    const bool finite = (__float_as_uint(p[0]) & inf) != inf && (__float_as_uint(p[1]) & inf) != inf && (__float_as_uint(p[2]) & inf) != inf;
    if (finite) {
        float u[3];
        for (int a = 0; a < 3; ++a) {
            u[a] = T.offset[a] + p[a] * T.scale[a];
            u[a] = fmaxf(fminf(u[a], 1.f - 1e-6f), 0.f);  // rt_core.cuh:125-127
        }
        int32_t chunk = 0;
        const int limit = T.max_depth < kMaxDescent ? T.max_depth : kMaxDescent;
        for (int d = 1; d <= limit; ++d) {
            int32_t c = 0;
            for (int a = 0; a < 3; ++a) {  // rt_core.cuh:138-143
                u[a] *= 2.f;
                const float f = floorf(u[a]);
                c = c * 2 + (int32_t)f;
                u[a] -= f;
            }
            const int64_t v = (int64_t)chunk * 8 + c;
            const uint32_t w = T.nodes[v];
            if (w & mnv::kLeafBit) {
                vox = (int32_t)v;
                dep = d;
                sg = mnv::half_bits_to_float((uint16_t)(w & 0xffffu));
                break;
            }
            if (w < 1u || w >= (uint32_t)T.capacity) break;  // a link outside the tree: not followed
            chunk = (int32_t)w;
        }
    }
    if (voxel) voxel[i] = vox;
    if (depth) depth[i] = dep;
    if (sigma) sigma[i] = sg;
}

// ---------------------------------------------------------------------------------------------------- (a) candidate bricks

__global__ void __launch_bounds__(256) candidate_kernel(TreeRef T, int level, float iso, int all, int64_t n_bricks, uint32_t *__restrict__ flag,
                                                         uint32_t *__restrict__ fault) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bricks) return;
    if (all) {
        flag[b] = 1u;
        return;
    }
    const int D = level - 3;
    const uint32_t nb = 1u << D;
    const uint32_t bz = (uint32_t)b & (nb - 1u), by = ((uint32_t)b >> D) & (nb - 1u), bx = (uint32_t)b >> (2 * D);
    bool cand = false;
    int side = -1;
    for (int k = 0; k < 8; ++k) {
        const uint32_t x = min(bx + (uint32_t)(k >> 2), nb - 1u), y = min(by + (uint32_t)((k >> 1) & 1), nb - 1u), z = min(bz + (uint32_t)(k & 1), nb - 1u);
        uint32_t word = 0;
        int32_t vox = 0;
        const int st = descend_lattice(T, x, y, z, D, D, word, vox);
        if (st == kFault) atomicOr(fault, 1u);
        if (st != kLeaf) {
            cand = true;
        } else {
            const int s = leaf_sigma(word) > iso ? 1 : 0;
            if (side >= 0 && s != side) cand = true;
            side = s;
        }
    }
    flag[b] = cand ? 1u : 0u;
}

// list[pos[b]] = b for the flagged bricks; the last thread leaves the list's length in totals[0]
__global__ void __launch_bounds__(256) candidate_list_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t n_bricks,
                                                              uint32_t *__restrict__ list, unsigned long long *__restrict__ totals) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bricks) return;
    if (flag[b]) list[pos[b]] = (uint32_t)b;
    if (b == n_bricks - 1) totals[0] = (unsigned long long)pos[b] + flag[b];
}

// ---------------------------------------------------------------------------------------------------- (b), (d): one workgroup per brick

struct BrickCoords {
    uint32_t bx, by, bz;
};

__device__ __forceinline__ BrickCoords brick_coords(uint32_t b, int level) {
    const int D = level - 3;
    const uint32_t nb = 1u << D;
    return {b >> (2 * D), (b >> D) & (nb - 1u), b & (nb - 1u)};
}

// the 9^3 samples of a brick into LDS (sample (x, y, z) of the stage at (x * 9 + y) * 9 + z); a sample beyond the lattice reads 0 and is
// never part of an existing cell
__device__ __forceinline__ void stage_brick(const TreeRef &T, int level, BrickCoords B, float *S, int32_t *V, uint32_t *fault) {
    const uint32_t n = 1u << level;
    for (int s = threadIdx.x; s < kStageN; s += blockDim.x) {
        const uint32_t x = B.bx * kBrick + (uint32_t)(s / (kStage * kStage)), y = B.by * kBrick + (uint32_t)((s / kStage) % kStage),
                       z = B.bz * kBrick + (uint32_t)(s % kStage);
        int32_t vox = 0;
        float v = 0.f;
        if (x < n && y < n && z < n) v = lattice_sample(T, level, x, y, z, vox, fault);
        S[s] = v;
        if (V) V[s] = vox;
    }
    __syncthreads();
}

// cell `cell` (index inside the brick) of brick B: does it exist, its inside bits by corner, and which of its three faces it owns
struct CellState {
    uint32_t cx, cy, cz;  // global cell coordinates
    int lx, ly, lz;
    bool valid, active;
    uint32_t inside;  // bit k: corner k is inside
    bool face[3];
};

__device__ __forceinline__ int stage_index(int x, int y, int z) { return (x * kStage + y) * kStage + z; }

__device__ __forceinline__ CellState cell_state(const float *S, BrickCoords B, int level, int cell, float iso) {
    CellState c;
    const uint32_t n = 1u << level;
    c.lx = cell >> 6, c.ly = (cell >> 3) & 7, c.lz = cell & 7;
    c.cx = B.bx * kBrick + (uint32_t)c.lx, c.cy = B.by * kBrick + (uint32_t)c.ly, c.cz = B.bz * kBrick + (uint32_t)c.lz;
    c.valid = c.cx + 1u < n && c.cy + 1u < n && c.cz + 1u < n;
    c.inside = 0u;
    for (int k = 0; k < 8; ++k)
        if (S[stage_index(c.lx + (k >> 2), c.ly + ((k >> 1) & 1), c.lz + (k & 1))] > iso) c.inside |= 1u << k;
    c.active = c.valid && c.inside != 0u && c.inside != 0xffu;
    const bool in0 = c.inside & 1u;
    // axis a's neighbour sample p + e_a is corner 4 >> a; the quad needs p_b >= 1 and p_c >= 1 for the next two axes
    c.face[0] = c.valid && c.cy >= 1u && c.cz >= 1u && in0 != (bool)((c.inside >> 4) & 1u);
    c.face[1] = c.valid && c.cz >= 1u && c.cx >= 1u && in0 != (bool)((c.inside >> 2) & 1u);
    c.face[2] = c.valid && c.cx >= 1u && c.cy >= 1u && in0 != (bool)((c.inside >> 1) & 1u);
    return c;
}

__global__ void __launch_bounds__(256) count_kernel(TreeRef T, int level, float iso, const uint32_t *__restrict__ list,
                                                     unsigned long long *__restrict__ mask, uint32_t *__restrict__ vcnt, uint32_t *__restrict__ qcnt,
                                                     uint32_t *__restrict__ fault) {
    __shared__ float S[kStageN];
    __shared__ uint32_t tot[2];
    const uint32_t b = list[blockIdx.x];
    const BrickCoords B = brick_coords(b, level);
    if (threadIdx.x < 2) tot[threadIdx.x] = 0u;
    stage_brick(T, level, B, S, nullptr, fault);
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
    for (int it = 0; it < 2; ++it) {
        const CellState c = cell_state(S, B, level, it * 256 + (int)threadIdx.x, iso);
        const unsigned long long ma = __ballot(c.active);
        const unsigned long long m0 = __ballot(c.face[0]), m1 = __ballot(c.face[1]), m2 = __ballot(c.face[2]);
        if (lead) {
            mask[(int64_t)b * 8 + it * 4 + wave] = ma;
            atomicAdd(&tot[0], (uint32_t)__popcll(ma));
            atomicAdd(&tot[1], (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2)));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        vcnt[b] = tot[0];
        qcnt[b] = tot[1];
    }
}

// totals[1] = vertices, totals[2] = quads (the exclusive scans' last element plus the last count)
__global__ void totals_kernel(const unsigned long long *__restrict__ voff, const uint32_t *__restrict__ vcnt, const unsigned long long *__restrict__ qoff,
                              const uint32_t *__restrict__ qcnt, int64_t n_bricks, unsigned long long *__restrict__ totals) {
    totals[1] = voff[n_bricks - 1] + vcnt[n_bricks - 1];
    totals[2] = qoff[n_bricks - 1] + qcnt[n_bricks - 1];
}

// id of the vertex of (active) cell (cx, cy, cz): its brick's first vertex plus the active cells below it in the brick
__device__ __forceinline__ uint32_t vertex_id(const unsigned long long *__restrict__ mask, const unsigned long long *__restrict__ voff, int level,
                                              uint32_t cx, uint32_t cy, uint32_t cz) {
    const int D = level - 3;
    const int64_t b = ((((int64_t)(cx >> 3) << D) + (cy >> 3)) << D) + (cz >> 3);
    const uint32_t idx = ((cx & 7u) << 6) | ((cy & 7u) << 3) | (cz & 7u), w = idx >> 6, l = idx & 63u;
    unsigned long long r = voff[b];
    for (uint32_t j = 0; j < w; ++j) r += (unsigned long long)__popcll(mask[b * 8 + j]);
    r += (unsigned long long)__popcll(mask[b * 8 + w] & (l ? (~0ull >> (64u - l)) : 0ull));
    return (uint32_t)r;
}

struct EmitParams {
    int level;
    float iso, inv_n;  // 2^-level
    int colour;
};

__global__ void __launch_bounds__(256) emit_kernel(TreeRef T, EmitParams P, const uint32_t *__restrict__ list,
                                                    const unsigned long long *__restrict__ mask, const unsigned long long *__restrict__ voff,
                                                    const unsigned long long *__restrict__ qoff, float *__restrict__ vert, int64_t n_verts,
                                                    uint32_t *__restrict__ faces, int64_t n_quads, uint32_t *__restrict__ fault) {
    __shared__ float S[kStageN];
    __shared__ int32_t V[kStageN];
    __shared__ uint32_t wave_quads[8];
    const uint32_t b = list[blockIdx.x];
    const BrickCoords B = brick_coords(b, P.level);
    stage_brick(T, P.level, B, S, V, fault);
    const int wave = threadIdx.x >> 6;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long below = lane ? (~0ull >> (64u - lane)) : 0ull;
    CellState cs[2];
    uint32_t qpre[2];  // quads of the owner cells below this one in its wave
    for (int it = 0; it < 2; ++it) {
        cs[it] = cell_state(S, B, P.level, it * 256 + (int)threadIdx.x, P.iso);
        const unsigned long long m0 = __ballot(cs[it].face[0]), m1 = __ballot(cs[it].face[1]), m2 = __ballot(cs[it].face[2]);
        qpre[it] = (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below));
        if (lane == 0) wave_quads[it * 4 + wave] = (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2));
    }
    __syncthreads();
    for (int it = 0; it < 2; ++it) {
        const CellState &c = cs[it];
        if (c.active) {
            float Sc[8];
            int best = 0;
            for (int k = 0; k < 8; ++k) {
                Sc[k] = S[stage_index(c.lx + (k >> 2), c.ly + ((k >> 1) & 1), c.lz + (k & 1))];
                if (Sc[k] > Sc[best]) best = k;
            }
            float sum[3] = {0.f, 0.f, 0.f};
            int cnt = 0;
            for (int a = 0; a < 3; ++a) {
                const int bit = 4 >> a;
                for (int k0 = 0; k0 < 8; ++k0) {
                    if (k0 & bit) continue;
                    const int k1 = k0 | bit;
                    if ((Sc[k0] > P.iso) == (Sc[k1] > P.iso)) continue;
                    const float t = (P.iso - Sc[k0]) / (Sc[k1] - Sc[k0]);
                    float p[3] = {(float)(k0 >> 2), (float)((k0 >> 1) & 1), (float)(k0 & 1)};
                    p[a] = t;
                    sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
                    ++cnt;
                }
            }
            const uint32_t cc[3] = {c.cx, c.cy, c.cz};
            float pos[3], w[3];
            for (int a = 0; a < 3; ++a) {
                const float local = sum[a] / (float)cnt;
                const float u = (((float)cc[a] + local) + 0.5f) * P.inv_n;
                pos[a] = (u - T.offset[a]) / T.scale[a];
            }
            const float g0 = (((Sc[4] + Sc[5]) + Sc[6]) + Sc[7]) - (((Sc[0] + Sc[1]) + Sc[2]) + Sc[3]);
            const float g1 = (((Sc[2] + Sc[3]) + Sc[6]) + Sc[7]) - (((Sc[0] + Sc[1]) + Sc[4]) + Sc[5]);
            const float g2 = (((Sc[1] + Sc[3]) + Sc[5]) + Sc[7]) - (((Sc[0] + Sc[2]) + Sc[4]) + Sc[6]);
            w[0] = -(g0 * T.scale[0]), w[1] = -(g1 * T.scale[1]), w[2] = -(g2 * T.scale[2]);
            const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            float nrm[3] = {0.f, 0.f, 1.f};
            if (len != 0.f && (__float_as_uint(len) & 0x7f800000u) != 0x7f800000u) nrm[0] = w[0] / len, nrm[1] = w[1] / len, nrm[2] = w[2] / len;
            const uint32_t id = vertex_id(mask, voff, P.level, c.cx, c.cy, c.cz);
            if ((int64_t)id < n_verts) {
                float *o = vert + (int64_t)id * 9;
                o[0] = pos[0], o[1] = pos[1], o[2] = pos[2];
                if (P.colour) {  // the colour pass reads the voxel from here
                    o[3] = __int_as_float(V[stage_index(c.lx + (best >> 2), c.ly + ((best >> 1) & 1), c.lz + (best & 1))]);
                    o[4] = 0.f, o[5] = 0.f;
                } else {
                    o[3] = 1.f, o[4] = 1.f, o[5] = 1.f;
                }
                o[6] = nrm[0], o[7] = nrm[1], o[8] = nrm[2];
            } else {
                atomicOr(fault, 2u);
            }
        }
        if (c.face[0] || c.face[1] || c.face[2]) {
            unsigned long long q = qoff[b] + qpre[it];
            for (int j = 0; j < it * 4 + wave; ++j) q += wave_quads[j];
            const uint32_t cc[3] = {c.cx, c.cy, c.cz};
            const bool in0 = c.inside & 1u;
            for (int a = 0; a < 3; ++a) {
                if (!c.face[a]) continue;
                const int ab = (a + 1) % 3, ac = (a + 2) % 3;
                uint32_t q0[3] = {cc[0], cc[1], cc[2]}, q1[3] = {cc[0], cc[1], cc[2]}, q3[3] = {cc[0], cc[1], cc[2]};
                q0[ab] -= 1u, q0[ac] -= 1u;
                q1[ac] -= 1u;
                q3[ab] -= 1u;
                const uint32_t i0 = vertex_id(mask, voff, P.level, q0[0], q0[1], q0[2]), i1 = vertex_id(mask, voff, P.level, q1[0], q1[1], q1[2]),
                               i2 = vertex_id(mask, voff, P.level, cc[0], cc[1], cc[2]), i3 = vertex_id(mask, voff, P.level, q3[0], q3[1], q3[2]);
                const uint32_t ia = in0 ? i1 : i3, ic = in0 ? i3 : i1;  // q0 q1 q2 q3 when sample p is inside, q0 q3 q2 q1 otherwise
                if ((int64_t)q < n_quads) {
                    uint32_t *f = faces + (int64_t)q * 6;
                    f[0] = i0, f[1] = ia, f[2] = i2, f[3] = i0, f[4] = i2, f[5] = ic;
                } else {
                    atomicOr(fault, 2u);
                }
                ++q;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- (e) colour

// BASIS 0: RGBA rows
template <int BASIS>
__global__ void __launch_bounds__(256) colour_kernel(TreeRef T, float *__restrict__ vert, int64_t n_verts) {
    __shared__ uint64_t tab[32];
    mnv::load_exp_table(tab);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_verts) return;
    float *v = vert + i * 9;
    const uint32_t vox = __float_as_uint(v[3]);
    if (vox >= (uint32_t)T.capacity * 8u) {
        v[3] = 0.f;
        return;
    }
    const uint16_t *row = reinterpret_cast<const uint16_t *>(T.rows + (int64_t)vox * T.row_bytes);
    float rgb[3];
    if constexpr (BASIS == 0) {
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = mnv::half_bits_to_float(row[ch]);  // rt_core.cuh:285-289
    } else {
        const float d[3] = {-v[6], -v[7], -v[8]};
        float basis[BASIS];
        mnv::sh_basis<BASIS>(d, basis);
        auto coef = [&](int k) { return mnv::half_bits_to_float(row[k]); };
        for (int ch = 0; ch < 3; ++ch) {
            const float tmp = mnv::sh_channel<BASIS>(basis, coef, ch * T.chan_halfs);
            rgb[ch] = 1.f / (1.f + mnv::exact_expf(-tmp, tab));  // rt_core.cuh:281 with weight 1
        }
    }
    v[3] = rgb[0], v[4] = rgb[1], v[5] = rgb[2];
}

struct U32ToU64 {
    __host__ __device__ unsigned long long operator()(uint32_t x) const { return (unsigned long long)x; }
};

// row format of the accel as the march sees it: -1 RGBA, 1 / 4 / 9 / 16 / 25 SH, anything else unsupported (-2)
int row_basis(const mnv::AccelView &A) {
    if (A.format == MNV_FORMAT_SH && A.basis_dim >= 0) {
        const int b = A.basis_dim;
        return (b == 1 || b == 4 || b == 9 || b == 16 || b == 25) ? b : -2;
    }
    return A.format == MNV_FORMAT_RGBA ? -1 : -2;
}

TreeRef tree_ref(const mnv_accel *a) {
    const mnv::AccelView &A = a->view;
    TreeRef T{};
    T.nodes = A.nodes;
    T.rows = A.rows;
    T.capacity = A.capacity;
    T.max_depth = A.max_depth;
    T.row_bytes = A.row_bytes;
    const int b = row_basis(A);
    T.chan_halfs = mnv::chan_bytes_for(b > 0 ? b : -1) / 2;
    for (int i = 0; i < 3; ++i) T.offset[i] = A.offset[i], T.scale[i] = A.scale[i];
    return T;
}

int require_device() {
    int dev = -1;
    return mnv::current_device(&dev);
}

}  // namespace

struct mnv_surface {
    Buffer<float> vert;      // device [n_verts][9]
    Buffer<uint32_t> faces;  // device [n_indices]
    int64_t n_verts = 0, n_indices = 0;
    mnv_surface_stats stats{};

    ~mnv_surface() {
        if (vert || faces) (void)hipDeviceSynchronize();
    }
};

namespace {

// the per-call scratch and the events that time the passes; freed whatever way extract() leaves
struct Scratch {
    Buffer<uint32_t> flag, pos, list, vcnt, qcnt, fault;
    Buffer<unsigned long long> mask, voff, qoff, totals;
    Buffer<uint8_t> tmp;
    Event ev[6];
};

int extract(const mnv_accel *accel, const mnv_extract_params *prm, hipStream_t stream, mnv_surface *out) {
    const TreeRef T = tree_ref(accel);
    const int level = prm->level;
    const bool colour = (prm->flags & MNV_EXTRACT_COLOUR) != 0, all = (prm->flags & MNV_EXTRACT_ALL_BRICKS) != 0;
    const int basis = row_basis(accel->view);
    const int64_t n_bricks = (int64_t)1 << (3 * (level - 3));
    Scratch W;
    int rc;
    for (Event &e : W.ev)
        if ((rc = check_hip(e.create(hipEventDefault), "hipEventCreate"))) return rc;
    size_t tmp32 = 0, tmp64 = 0;
    auto in64 = rocprim::make_transform_iterator((const uint32_t *)nullptr, U32ToU64());
    (void)rocprim::exclusive_scan(nullptr, tmp32, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n_bricks, rocprim::plus<uint32_t>(), stream);
    (void)rocprim::exclusive_scan(nullptr, tmp64, in64, (unsigned long long *)nullptr, 0ull, (size_t)n_bricks, rocprim::plus<unsigned long long>(), stream);
    const size_t tmp_bytes = std::max(tmp32, tmp64) + 256;
    if ((rc = check_hip(W.flag.alloc((size_t)n_bricks), "hipMalloc(extract flags)")) ||
        (rc = check_hip(W.pos.alloc((size_t)n_bricks), "hipMalloc(extract positions)")) ||
        (rc = check_hip(W.list.alloc((size_t)n_bricks), "hipMalloc(extract list)")) ||
        (rc = check_hip(W.vcnt.alloc((size_t)n_bricks), "hipMalloc(extract counts)")) ||
        (rc = check_hip(W.qcnt.alloc((size_t)n_bricks), "hipMalloc(extract counts)")) ||
        (rc = check_hip(W.mask.alloc((size_t)n_bricks * 8), "hipMalloc(extract masks)")) ||
        (rc = check_hip(W.voff.alloc((size_t)n_bricks), "hipMalloc(extract offsets)")) ||
        (rc = check_hip(W.qoff.alloc((size_t)n_bricks), "hipMalloc(extract offsets)")) ||
        (rc = check_hip(W.totals.alloc(3), "hipMalloc(extract totals)")) ||
        (rc = check_hip(W.fault.alloc(1), "hipMalloc(extract fault)")) ||
        (rc = check_hip(W.tmp.alloc(tmp_bytes), "hipMalloc(extract scan scratch)")))
        return rc;
    if ((rc = check_hip(hipMemsetAsync(W.fault.get(), 0, 4, stream), "extract memset")) ||
        (rc = check_hip(hipMemsetAsync(W.vcnt.get(), 0, (size_t)n_bricks * 4, stream), "extract memset")) ||
        (rc = check_hip(hipMemsetAsync(W.qcnt.get(), 0, (size_t)n_bricks * 4, stream), "extract memset")) ||
        (rc = check_hip(hipMemsetAsync(W.mask.get(), 0, (size_t)n_bricks * 64, stream), "extract memset")))
        return rc;
    // (a) candidates, compacted in ascending brick order
    (void)hipEventRecord(W.ev[0].get(), stream);
    hipLaunchKernelGGL(candidate_kernel, dim3(mnv::blocks_for(n_bricks)), dim3(256), 0, stream, T, level, prm->iso, all ? 1 : 0, n_bricks, W.flag.get(), W.fault.get());
    size_t t = tmp_bytes;
    if ((rc = check_hip(rocprim::exclusive_scan(W.tmp.get(), t, (const uint32_t *)W.flag.get(), W.pos.get(), 0u, (size_t)n_bricks, rocprim::plus<uint32_t>(), stream),
                        "exclusive_scan(candidates)")))
        return rc;
    hipLaunchKernelGGL(candidate_list_kernel, dim3(mnv::blocks_for(n_bricks)), dim3(256), 0, stream, W.flag.get(), W.pos.get(), n_bricks, W.list.get(), W.totals.get());
    (void)hipEventRecord(W.ev[1].get(), stream);
    unsigned long long totals[3] = {0, 0, 0};
    uint32_t fault = 0;
    if ((rc = check_hip(hipGetLastError(), "extract candidate pass")) ||
        (rc = check_hip(hipMemcpyAsync(totals, W.totals.get(), 8, hipMemcpyDeviceToHost, stream), "read candidate count")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "extract candidate pass")))
        return rc;
    const int64_t n_cand = (int64_t)totals[0];
    if (n_cand < 0 || n_cand > n_bricks) return set_error(MNV_E_INVALID, "mnv_extract_surface: candidate count out of range");
    // (b) count, (c) scans
    if (n_cand > 0) hipLaunchKernelGGL(count_kernel, dim3((unsigned)n_cand), dim3(256), 0, stream, T, level, prm->iso, W.list.get(), W.mask.get(), W.vcnt.get(), W.qcnt.get(), W.fault.get());
    (void)hipEventRecord(W.ev[2].get(), stream);
    t = tmp_bytes;
    if ((rc = check_hip(rocprim::exclusive_scan(W.tmp.get(), t, rocprim::make_transform_iterator((const uint32_t *)W.vcnt.get(), U32ToU64()), W.voff.get(), 0ull, (size_t)n_bricks,
                                                rocprim::plus<unsigned long long>(), stream),
                        "exclusive_scan(vertices)")))
        return rc;
    t = tmp_bytes;
    if ((rc = check_hip(rocprim::exclusive_scan(W.tmp.get(), t, rocprim::make_transform_iterator((const uint32_t *)W.qcnt.get(), U32ToU64()), W.qoff.get(), 0ull, (size_t)n_bricks,
                                                rocprim::plus<unsigned long long>(), stream),
                        "exclusive_scan(quads)")))
        return rc;
    hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(1), 0, stream, W.voff.get(), W.vcnt.get(), W.qoff.get(), W.qcnt.get(), n_bricks, W.totals.get());
    (void)hipEventRecord(W.ev[3].get(), stream);
    if ((rc = check_hip(hipGetLastError(), "extract count pass")) ||
        (rc = check_hip(hipMemcpyAsync(totals, W.totals.get(), 3 * 8, hipMemcpyDeviceToHost, stream), "read extract totals")) ||
        (rc = check_hip(hipMemcpyAsync(&fault, W.fault.get(), 4, hipMemcpyDeviceToHost, stream), "read extract fault")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "extract count pass")))
        return rc;
    if (fault) return set_error(MNV_E_INVALID, "mnv_extract_surface: a child link leaves the tree (not a valid N3Tree)");
    const unsigned long long n_verts = totals[1], n_quads = totals[2];
    if (n_verts > (unsigned long long)INT32_MAX || n_quads * 6ull > (unsigned long long)INT32_MAX)
        return set_error(MNV_E_UNSUPPORTED, "mnv_extract_surface: more than 2^31 - 1 vertices or indices (lower the level)");
    // (d) emit, (e) colour
    if (n_verts > 0 && (rc = check_hip(out->vert.alloc((size_t)n_verts * 9), "hipMalloc(surface vertices)"))) return rc;
    if (n_quads > 0 && (rc = check_hip(out->faces.alloc((size_t)n_quads * 6), "hipMalloc(surface indices)"))) return rc;
    float *vert = out->vert.get();
    uint32_t *faces = out->faces.get();
    out->n_verts = (int64_t)n_verts, out->n_indices = (int64_t)n_quads * 6;
    if (n_verts > 0) {
        const EmitParams P = {level, prm->iso, std::ldexp(1.f, -level), colour ? 1 : 0};
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)n_cand), dim3(256), 0, stream, T, P, W.list.get(), W.mask.get(), W.voff.get(), W.qoff.get(), vert, (int64_t)n_verts, faces,
                           (int64_t)n_quads, W.fault.get());
    }
    (void)hipEventRecord(W.ev[4].get(), stream);
    if (n_verts > 0 && colour) {
        const dim3 grid(mnv::blocks_for((int64_t)n_verts)), block(256);
        switch (basis) {
            case -1: hipLaunchKernelGGL(colour_kernel<0>, grid, block, 0, stream, T, vert, (int64_t)n_verts); break;
            case 1: hipLaunchKernelGGL(colour_kernel<1>, grid, block, 0, stream, T, vert, (int64_t)n_verts); break;
            case 4: hipLaunchKernelGGL(colour_kernel<4>, grid, block, 0, stream, T, vert, (int64_t)n_verts); break;
            case 9: hipLaunchKernelGGL(colour_kernel<9>, grid, block, 0, stream, T, vert, (int64_t)n_verts); break;
            case 16: hipLaunchKernelGGL(colour_kernel<16>, grid, block, 0, stream, T, vert, (int64_t)n_verts); break;
            default: hipLaunchKernelGGL(colour_kernel<25>, grid, block, 0, stream, T, vert, (int64_t)n_verts); break;
        }
    }
    (void)hipEventRecord(W.ev[5].get(), stream);
    if ((rc = check_hip(hipGetLastError(), "extract emit pass")) ||
        (rc = check_hip(hipMemcpyAsync(&fault, W.fault.get(), 4, hipMemcpyDeviceToHost, stream), "read extract fault")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "extract emit pass")))
        return rc;
    if (fault) return set_error(MNV_E_INVALID, "mnv_extract_surface: the tree changed during the call (the passes disagree)");
    mnv_surface_stats &st = out->stats;
    st.bricks = n_bricks, st.candidate_bricks = n_cand;
    (void)hipEventElapsedTime(&st.ms_candidates, W.ev[0].get(), W.ev[1].get());
    (void)hipEventElapsedTime(&st.ms_count, W.ev[1].get(), W.ev[2].get());
    (void)hipEventElapsedTime(&st.ms_scan, W.ev[2].get(), W.ev[3].get());
    (void)hipEventElapsedTime(&st.ms_emit, W.ev[3].get(), W.ev[4].get());
    (void)hipEventElapsedTime(&st.ms_colour, W.ev[4].get(), W.ev[5].get());
    (void)hipEventElapsedTime(&st.ms_total, W.ev[0].get(), W.ev[5].get());
    return MNV_OK;
}

}  // namespace

extern "C" {

int mnv_accel_sample_points(const mnv_accel *accel, const float *points, int64_t n, int32_t *voxel_out, int32_t *depth_out, float *sigma_out,
                            void *hip_stream) {
    if (n < 0) return set_error(MNV_E_INVALID, "mnv_accel_sample_points: negative point count");
    if (!accel || (n > 0 && !points)) return set_error(MNV_E_INVALID, "mnv_accel_sample_points: null accel / points");
    int rc = require_device();
    if (rc) return rc;
    if (accel->view.capacity < 1 || !accel->view.nodes) return set_error(MNV_E_INVALID, "mnv_accel_sample_points: the accel holds no tree");
    if (n == 0 || (!voxel_out && !depth_out && !sigma_out)) return MNV_OK;
    hipLaunchKernelGGL(sample_points_kernel, dim3(mnv::blocks_for(n)), dim3(256), 0, (hipStream_t)hip_stream, tree_ref(accel), points, n, voxel_out, depth_out,
                       sigma_out);
    return check_hip(hipGetLastError(), "sample_points_kernel");
}

int mnv_extract_surface(const mnv_accel *accel, const mnv_extract_params *params, void *hip_stream, mnv_surface **out) {
    if (!out) return set_error(MNV_E_INVALID, "null output");
    *out = nullptr;
    if (!accel || !params) return set_error(MNV_E_INVALID, "mnv_extract_surface: null accel / params");
    if (params->level < 3 || params->level > 10) return set_error(MNV_E_INVALID, "mnv_extract_surface: level must be 3 .. 10");
    if (params->iso != params->iso) return set_error(MNV_E_INVALID, "mnv_extract_surface: iso is NaN");
    if (params->flags & ~(MNV_EXTRACT_COLOUR | MNV_EXTRACT_ALL_BRICKS)) return set_error(MNV_E_INVALID, "mnv_extract_surface: unknown flag bits");
    int rc = require_device();
    if (rc) return rc;
    if (accel->view.capacity < 1 || !accel->view.nodes) return set_error(MNV_E_INVALID, "mnv_extract_surface: the accel holds no tree");
    if ((params->flags & MNV_EXTRACT_COLOUR) && row_basis(accel->view) == -2)
        return set_error(MNV_E_UNSUPPORTED, "mnv_extract_surface: colours need RGBA or SH 1 / 4 / 9 / 16 / 25 rows");
    mnv_surface *s = new mnv_surface();
    rc = extract(accel, params, (hipStream_t)hip_stream, s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return MNV_OK;
}

void mnv_surface_destroy(mnv_surface *s) { delete s; }

int mnv_surface_counts(const mnv_surface *s, int64_t *n_verts, int64_t *n_indices) {
    if (!s) return set_error(MNV_E_INVALID, "null surface");
    if (n_verts) *n_verts = s->n_verts;
    if (n_indices) *n_indices = s->n_indices;
    return MNV_OK;
}

int mnv_surface_stats_get(const mnv_surface *s, mnv_surface_stats *out) {
    if (!s || !out) return set_error(MNV_E_INVALID, "null surface / output");
    *out = s->stats;
    return MNV_OK;
}

int mnv_surface_download(const mnv_surface *s, float *vert, int64_t cap_floats, uint32_t *faces, int64_t cap_indices) {
    if (!s) return set_error(MNV_E_INVALID, "null surface");
    if ((vert && cap_floats < s->n_verts * 9) || (faces && cap_indices < s->n_indices))
        return set_error(MNV_E_INVALID, "mnv_surface_download: buffer too small (mnv_surface_counts holds the sizes)");
    int rc;
    if (vert && s->n_verts > 0 && (rc = check_hip(hipMemcpy(vert, s->vert.get(), (size_t)s->n_verts * 9 * sizeof(float), hipMemcpyDeviceToHost), "download vertices")))
        return rc;
    if (faces && s->n_indices > 0 && (rc = check_hip(hipMemcpy(faces, s->faces.get(), (size_t)s->n_indices * sizeof(uint32_t), hipMemcpyDeviceToHost), "download indices")))
        return rc;
    return MNV_OK;
}

int mnv_surface_device(const mnv_surface *s, const float **vert, const uint32_t **faces) {
    if (!s) return set_error(MNV_E_INVALID, "null surface");
    if (vert) *vert = s->vert.get();
    if (faces) *faces = s->faces.get();
    return MNV_OK;
}

int mnv_surface_to_mesh(const mnv_surface *s, int unlit, mnv_mesh **out) {
    if (!out) return set_error(MNV_E_INVALID, "null output");
    *out = nullptr;
    if (!s) return set_error(MNV_E_INVALID, "null surface");
    if (s->n_verts == 0 || s->n_indices == 0) return set_error(MNV_E_INVALID, "mnv_surface_to_mesh: the surface is empty");
    Buffer<float> dv;
    Buffer<uint32_t> df;
    int rc;
    if ((rc = check_hip(dv.alloc((size_t)s->n_verts * 9), "hipMalloc(mesh vertices)")) ||
        (rc = check_hip(df.alloc((size_t)s->n_indices), "hipMalloc(mesh indices)")) ||
        (rc = check_hip(hipMemcpy(dv.get(), s->vert.get(), dv.bytes(), hipMemcpyDeviceToDevice), "copy mesh vertices")) ||
        (rc = check_hip(hipMemcpy(df.get(), s->faces.get(), df.bytes(), hipMemcpyDeviceToDevice), "copy mesh indices")) ||
        (rc = mnv::mesh_adopt_device(dv.get(), s->n_verts, df.get(), s->n_indices, 3, unlit, out)))
        return rc;
    (void)dv.release(), (void)df.release();  // (the mesh owns them now)
    return MNV_OK;
}

}  // extern "C"
