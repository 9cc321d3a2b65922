// mnv_visibility.hip -- culling a tree to what a set of rays can see: mnv_rays_visibility (the largest compositing weight any listed ray gave
// each leaf) and mnv_tree_cull (zero the rows of what was not seen, find the chunks that died).  The contract is include/mnv.h's ("culling a
// tree to a pose set"); DESIGN.md 5.17 has the argument why threshold 0 leaves the listed rays' pixels unchanged.  tests/visibility_ref.py
// restates both in numpy.  With mnv_tree_cut (mnv_lod_view.hip) behind them the result is an ordinary, smaller N3Tree.
//
// mnv_rays_visibility: one ray per lane, one wavefront per workgroup, 8 x 8 ray tiles (64 x 1 for a flat list), a workgroup walks tiles with
// the grid's stride -- the launch shape of mnv_rays_grad, whose forward march (set-up, bounded link-checked descent, delta_t, exact expf,
// early stop) is restated here statement for statement without its colour block: no row column but sigma is read.  Two marches per ray, as
// there: the first finds out whether the ray is skipped (a skipped ray must add nothing) and how many dense samples it has, the second
// repeats the same steps and writes.  The words are maxima of non-negative binary32 bit patterns, so they depend on no order.
//
// mnv_tree_cull: the level walk of mnv_tree_walk.h (a list of (chunk, voxel above) per depth), then one launch per depth, deepest
// first, a group of 8 .. 64 lanes per chunk as the mip pass has them.  The group's first eight lanes decide the chunk's eight voxels -- a
// leaf by its word of wmax, an interior voxel by the keep byte the launch of the level below wrote for its child chunk -- a ballot hands
// the eight bits to the whole group, which then moves the chunk's rows in 16-byte segments and zeroes the halves of dead voxels on the way.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mnv_tree_walk.h"

#pragma clang fp contract(off)

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kMaxDescent = 23;     // levels, as mnv_rays_grad
constexpr int kMaxSteps = 1 << 20;  // march steps of one ray; a ray that needs more is skipped
constexpr int kVisGrid = 4096;      // workgroups of one wavefront: 16 per CU
constexpr int64_t kMaxRays = (int64_t)1 << 22;
constexpr int kMaxDataDim = 1024;
constexpr int kWavesPerBlock = 4;
constexpr int kCullGrid = 8192;     // workgroups of four wavefronts: 32 per CU

// ---------------------------------------------------------------------------------------------------- visibility

struct VisArgs {
    mnv::FrameParams P;  // options, offset / scale, tw x th, tmax_px
    const uint16_t *data;
    const int32_t *child;
    const float *origins, *dirs;
    uint32_t *wmax;
    unsigned long long *sums;
    int32_t data_dim, capacity;
    int32_t tiles_x, n_tiles, flat;
};

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;  // (lane 0 holds the sum)
}

// One march step at t (mnv_fit.hip's march_step, rt_core.cuh:220-231): the leaf under the ray, delta_t and sigma.  false: the descent left the tree.
__device__ __forceinline__ bool march_step(const VisArgs &K, const float (&cen)[3], const float (&dir)[3], const float (&invdir)[3], float t, int32_t &vox,
                                           float &delta_t, float &sigma) {
    float pos[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pos[i] = cen[i] + t * dir[i];
        pos[i] = fmaxf(fminf(pos[i], 1.f - 1e-6f), 0.f);
    }
    int32_t chunk = 0, cidx = 0;
    int depth = 1;
    bool leaf = false;
    for (; depth <= kMaxDescent; ++depth) {
        cidx = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            pos[i] *= 2.f;
            const float f = floorf(pos[i]);
            cidx = cidx * 2 + (int)f;
            pos[i] -= f;
        }
        const int32_t skip = K.child[(int64_t)chunk * 8 + cidx];
        if (skip == 0) {
            leaf = true;
            break;
        }
        const int64_t next = (int64_t)chunk + skip;
        if (next < 1 || next >= K.capacity) break;  // a link outside the tree: not followed
        chunk = (int32_t)next;
    }
    if (!leaf) return false;
    float tu = 1e4f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t1 = -pos[i] * invdir[i];
        const float t2 = t1 + invdir[i];
        tu = fminf(tu, fmaxf(t1, t2));
    }
    const float cube = __uint_as_float((uint32_t)(127 + depth) << 23);  // 2^depth
    delta_t = tu / cube + K.P.step_size;
    vox = chunk * 8 + cidx;
    sigma = mnv::half_bits_to_float(K.data[(int64_t)vox * K.data_dim + K.data_dim - 1]);
    return true;
}

__global__ __launch_bounds__(64) void rays_visibility_kernel(const VisArgs K) {
    __shared__ uint64_t s_exp[32];
    mnv::load_exp_table(s_exp);
    const mnv::FrameParams &P = K.P;
    const int lane = threadIdx.x;
    long long sum[4] = {0, 0, 0, 0};  // n_rays, n_stopped, n_samples, n_skipped

    for (int tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
        const int bx = K.flat ? tile * 64 + lane : (tile % K.tiles_x) * 8 + (lane & 7);
        const int by = K.flat ? 0 : (tile / K.tiles_x) * 8 + (lane >> 3);
        const bool has_ray = bx < P.tw && by < P.th;
        const int64_t pix = has_ray ? (int64_t)by * P.tw + bx : 0;

        // ---- the ray (rays_grad_kernel, statement for statement; no SH basis is kept)
        mnv::RaySetup<1> r;
        float cen[3] = {0.f, 0.f, 0.f};
        r.in_bbox = false;
        if (has_ray) {
            const float *__restrict__ ro = K.origins + pix * 3, *__restrict__ rd = K.dirs + pix * 3;
            const float w0 = ro[0], w1 = ro[1], w2 = ro[2];
            float d[3] = {rd[0], rd[1], rd[2]};
            const float len2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            const bool valid = len2 > 0.f && len2 < __builtin_inff() && (w0 - w0) + (w1 - w1) + (w2 - w2) == 0.f;
            const float p0 = P.scale[0] * w0, p1 = P.scale[1] * w1, p2 = P.scale[2] * w2;
            cen[0] = P.offset[0] + p0;
            cen[1] = P.offset[1] + p1;
            cen[2] = P.offset[2] + p2;
            mnv::setup_ray_dir<0>(P, cen, d, r, mnv::frame_tmax(P, pix));
            r.in_bbox = r.in_bbox && valid;
        }

        // ---- first march: is the ray skipped, how many dense samples does it take
        float T = 1.f;
        bool stopped = false, broken = false;
        int n_dense = 0;
        if (r.in_bbox) {
            float t = r.tmin;
            int steps = 0;
            while (t < r.tmax) {
                int32_t vox;
                float delta_t, sigma;
                if (++steps > kMaxSteps || !march_step(K, cen, r.dir, r.invdir, t, vox, delta_t, sigma)) {
                    broken = true;
                    break;
                }
                if (sigma > P.sigma_thresh) {
                    const float att = mnv::exact_expf(-delta_t * r.delta_scale * sigma, s_exp);
                    ++n_dense;
                    T *= att;
                    if (T < P.stop_thresh) {
                        stopped = true;
                        break;
                    }
                }
                const float tn = t + delta_t;
                if (!(tn > t)) {  // a step that does not advance: the ray is skipped, the march ends
                    broken = true;
                    break;
                }
                t = tn;
            }
        }
        if (has_ray) {
            if (broken) {
                sum[3] += 1;
            } else {
                sum[0] += 1;
                sum[1] += stopped ? 1 : 0;
                sum[2] += n_dense;
            }
        }

        // ---- second march: the same steps; every dense sample's weight goes to its leaf's word
        if (!has_ray || broken) continue;
        float t = r.tmin;
        T = 1.f;
        for (int left = n_dense; left > 0 && t < r.tmax;) {
            int32_t vox;
            float delta_t, sigma;
            if (!march_step(K, cen, r.dir, r.invdir, t, vox, delta_t, sigma)) break;  // (cannot happen: the first march took this very step)
            if (sigma > P.sigma_thresh) {
                const float att = mnv::exact_expf(-delta_t * r.delta_scale * sigma, s_exp);
                const uint32_t w = __float_as_uint(T * (1.f - att));
                // w > 0 and not NaN, on the bits: 0 < w <= +inf's pattern (a negative or NaN weight writes nothing)
                if (w - 1u < 0x7f800000u) {
                    // A plain load first: neighbouring rays and earlier views hit the same leaves, so most samples find a word that is
                    // already >= theirs.  The load may be stale; words only grow, so a stale value is <= the current one and can only
                    // let a redundant atomicMax through, never keep a needed one back.
                    if (K.wmax[vox] < w) atomicMax(K.wmax + vox, w);
                }
                T *= att;
                --left;
            }
            t = t + delta_t;
        }
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long s = wave_sum(sum[k]);
        if (lane == 0 && s != 0) atomicAdd(K.sums + k, (unsigned long long)s);
    }
}

// ---------------------------------------------------------------------------------------------------- cull

// the counters of cull_rows_kernel (words 0 and 1 are not used: the walk's counters were there once, and the kernel's offsets stay)
enum { kCtrSeen = 2, kCtrCulled = 3, kCtrDead = 4, kCtrKept = 5, kCtrWords = kCtrKept + 24 };

// A group of G lanes (a power of two, 8 .. 64) per list entry of one depth, 64 / G entries per wavefront.  thresh_bits: the pattern of the
// (finite, non-negative) threshold.  A word of wmax is seen iff it is a non-negative, non-NaN pattern above thresh_bits: such patterns order
// as their values, so the comparison is the contract's uint_as_float(wmax) > weight_thresh without a float compare.
__global__ void __launch_bounds__(64 * kWavesPerBlock) cull_rows_kernel(const uint16_t *__restrict__ data_in, uint16_t *__restrict__ data_out,
                                                                         const int32_t *__restrict__ child, const uint32_t *__restrict__ wmax,
                                                                         uint32_t thresh_bits, const int2 *__restrict__ list, int64_t n, int32_t dd,
                                                                         int32_t log2_g, int32_t depth, uint8_t *__restrict__ keep,
                                                                         unsigned long long *__restrict__ ctr) {
    const int G = 1 << log2_g, per_wave = 64 >> log2_g;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> log2_g, gl = lane & (G - 1);
    const int64_t per_block = (int64_t)kWavesPerBlock * per_wave, n_blocks = (n + per_block - 1) / per_block;
    int n_seen = 0, n_culled = 0, n_kept = 0, n_dead = 0;  // (wave-uniform)
    // a workgroup walks the list with the grid's stride, so the four counts cost one atomic each per wavefront and not per chunk: with an
    // atomic per wavefront and chunk pair the pass ran at the rate of same-address atomics (10 ms for cfg2's 1.5 M chunks)
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t idx = (blk * kWavesPerBlock + wave) * per_wave + grp;
        const bool active = idx < n;
        const int64_t k = active ? list[idx].x : 0;
        bool live = false, seen_leaf = false, culled_full = false;
        if (active && gl < 8) {
            const int64_t v = k * 8 + gl;
            const int32_t ch = child[v];
            if (ch == 0) {
                const uint32_t w = wmax[v];
                live = seen_leaf = w <= 0x7f800000u && w > thresh_bits;
                if (!live) {  // was there anything to lose: h(sigma) > 0, non-finite patterns read +0
                    const uint32_t s = data_in[v * dd + dd - 1];
                    culled_full = (s & 0x8000u) == 0 && (s & 0x7fffu) != 0 && (s & 0x7c00u) != 0x7c00u;
                }
            } else {
                live = keep[k + ch] != 0;  // (the walk checked the link; the launch of the level below wrote the byte)
            }
        }
        const unsigned long long b_live = __ballot(live);
        const unsigned mask = (unsigned)((b_live >> (grp << log2_g)) & 0xffull);
        const bool stays = mask != 0 || k == 0;  // the root chunk always stays
        if (active) {
            const uint4 *in4 = reinterpret_cast<const uint4 *>(data_in) + k * dd;
            uint4 *out4 = reinterpret_cast<uint4 *>(data_out) + k * dd;
            for (int s = gl; s < dd; s += G) {
                mnv::Seg16 a;
                a.v = in4[s];
                if (mask != 0xffu) {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (!((mask >> ((8 * s + i) / dd)) & 1u)) a.h[i] = 0;
                }
                out4[s] = a.v;
            }
            if (gl == 0) keep[k] = stays ? 1 : 0;
        }
        n_seen += __popcll(__ballot(seen_leaf));
        n_culled += __popcll(__ballot(culled_full));
        n_kept += __popcll(__ballot(active && gl == 0 && stays));
        n_dead += __popcll(__ballot(active && gl == 0 && !stays));
    }
    // the counts: sums of integers, in any order
    if (lane == 0) {
        if (n_seen) atomicAdd(&ctr[kCtrSeen], (unsigned long long)n_seen);
        if (n_culled) atomicAdd(&ctr[kCtrCulled], (unsigned long long)n_culled);
        if (n_dead) atomicAdd(&ctr[kCtrDead], (unsigned long long)n_dead);
        if (n_kept) atomicAdd(&ctr[kCtrKept + depth], (unsigned long long)n_kept);
    }
}

// the counters of mnv_tree_cull, per device; used under the walk's guard and kept as long as the process (no hipFree after the runtime went)
mnv::Mirrored<unsigned long long> *const g_cull_ctr = new mnv::Mirrored<unsigned long long>[mnv::kMaxWalkDevices];

}  // namespace

extern "C" {

int mnv_rays_visibility(const mnv_tree_view *tree, const float *origins, const float *dirs, const float *tmax, int32_t width, int32_t height,
                        const mnv_render_options *opt, uint32_t *wmax, mnv_vis_sums *sums, void *hip_stream) {
    // every argument before any device call
    if (!tree || !origins || !dirs || !opt || !wmax || !sums) return set_error(MNV_E_INVALID, "mnv_rays_visibility: null tree / rays / options / wmax / sums");
    if (width < 1 || height < 1) return set_error(MNV_E_INVALID, "mnv_rays_visibility: a ray image needs width >= 1 and height >= 1");
    if ((int64_t)width * (int64_t)height > kMaxRays) return set_error(MNV_E_INVALID, "mnv_rays_visibility: more than 2^22 rays in one call");
    if (tree->N != 2) return set_error(MNV_E_UNSUPPORTED, "mnv_rays_visibility: N != 2");
    if (opt->render_depth) return set_error(MNV_E_UNSUPPORTED, "mnv_rays_visibility: render_depth has no compositing weights");
    if (!tree->data || !tree->child || tree->capacity < 1) return set_error(MNV_E_INVALID, "mnv_rays_visibility: the view holds no tree");
    const int b = (tree->format == MNV_FORMAT_SH && tree->basis_dim >= 0) ? tree->basis_dim : -1;
    if (!(b == -1 || b == 1 || b == 4 || b == 9 || b == 16 || b == 25))
        return set_error(MNV_E_UNSUPPORTED, "mnv_rays_visibility: RGBA and SH1/4/9/16/25 rows (what the ray march serves)");
    if (tree->data_dim < (b > 0 ? 3 * b + 1 : 4)) return set_error(MNV_E_INVALID, "mnv_rays_visibility: data_dim too small for the row format");
    if (!std::isfinite(opt->step_size) || !(opt->step_size > 0.f))
        return set_error(MNV_E_INVALID, "mnv_rays_visibility: step_size must be finite and positive (the march must advance)");
    if (((uintptr_t)sums & 7u) != 0) return set_error(MNV_E_INVALID, "mnv_rays_visibility: sums must be 8-byte aligned");
    if ((((uintptr_t)origins | (uintptr_t)dirs | (uintptr_t)tmax | (uintptr_t)wmax) & 3u) != 0)
        return set_error(MNV_E_INVALID, "mnv_rays_visibility: rays, tmax and wmax must be 4-byte aligned");
    VisArgs K;
    std::memset(static_cast<void *>(&K), 0, sizeof(K));
    mnv_camera shape = {};  // (fill_params wants an image size; the march reads no camera)
    shape.width = width;
    shape.height = height;
    shape.fx = shape.fy = 1.f;
    const int rc = mnv::fill_params(K.P, &shape, opt, mnv_rect{0, 0, width, height});
    if (rc) return rc;
    std::memcpy(K.P.offset, tree->offset, sizeof(K.P.offset));
    std::memcpy(K.P.scale, tree->scale, sizeof(K.P.scale));
    K.P.tmax_px = tmax;
    K.data = tree->data;
    K.child = tree->child;
    K.origins = origins;
    K.dirs = dirs;
    K.wmax = wmax;
    K.sums = reinterpret_cast<unsigned long long *>(sums);
    K.data_dim = tree->data_dim;
    K.capacity = tree->capacity;
    K.flat = height == 1 ? 1 : 0;
    K.tiles_x = K.flat ? (width + 63) / 64 : (width + 7) / 8;
    K.n_tiles = K.flat ? K.tiles_x : K.tiles_x * ((height + 7) / 8);
    hipLaunchKernelGGL(rays_visibility_kernel, dim3((unsigned)std::min(K.n_tiles, kVisGrid)), dim3(64), 0, (hipStream_t)hip_stream, K);
    return check_hip(hipGetLastError(), "rays_visibility_kernel");
}

int mnv_tree_cull(const mnv_tree_view *tree, const uint32_t *wmax, float weight_thresh, uint16_t *data_out, uint8_t *keep_out, int64_t kept_at_depth[24],
                  mnv_cull_counts *counts, void *hip_stream) {
    const char *who = "mnv_tree_cull";
    int rc;
    if (!tree || !tree->data || !tree->child || !wmax || !data_out || !keep_out || !kept_at_depth || !counts)
        return set_error(MNV_E_INVALID, std::string(who) + ": null tree view / arrays / output");
    for (int d = 0; d < 24; ++d) kept_at_depth[d] = 0;
    std::memset(counts, 0, sizeof(*counts));
    if (tree->N != 2) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": only N == 2 trees");
    if (tree->capacity < 1) return set_error(MNV_E_INVALID, std::string(who) + ": a tree has at least its root chunk");
    if (tree->data_dim < 2) return set_error(MNV_E_INVALID, std::string(who) + ": data_dim must be at least 2");
    if (tree->data_dim > kMaxDataDim) return set_error(MNV_E_UNSUPPORTED, std::string(who) + ": data_dim above 1024");
    if (!std::isfinite(weight_thresh) || weight_thresh < 0.f) return set_error(MNV_E_INVALID, std::string(who) + ": weight_thresh must be finite and not negative");
    const int32_t cap = tree->capacity, dd = tree->data_dim;
    const size_t data_bytes = (size_t)cap * 16 * dd;
    if ((((uintptr_t)tree->data | (uintptr_t)data_out) & 15u) != 0) return set_error(MNV_E_INVALID, std::string(who) + ": the data arrays must be 16-byte aligned");
    if (((uintptr_t)wmax & 3u) != 0) return set_error(MNV_E_INVALID, std::string(who) + ": wmax must be 4-byte aligned");
    if (!mnv::on_device(tree->child) || !mnv::on_device(tree->data) || !mnv::on_device(wmax) || !mnv::on_device(data_out) || !mnv::on_device(keep_out))
        return set_error(MNV_E_INVALID, std::string(who) + ": the tree view, wmax, data_out and keep_out must be device arrays");
    if (mnv::overlap(data_out, data_bytes, tree->data, data_bytes) || mnv::overlap(data_out, data_bytes, tree->child, (size_t)cap * 32) ||
        mnv::overlap(data_out, data_bytes, wmax, (size_t)cap * 32) || mnv::overlap(data_out, data_bytes, keep_out, (size_t)cap) ||
        mnv::overlap(keep_out, (size_t)cap, tree->data, data_bytes) || mnv::overlap(keep_out, (size_t)cap, tree->child, (size_t)cap * 32) ||
        mnv::overlap(keep_out, (size_t)cap, wmax, (size_t)cap * 32))
        return set_error(MNV_E_INVALID, std::string(who) + ": the outputs must overlap neither each other nor the inputs (the input tree is never modified)");
    hipStream_t stream = (hipStream_t)hip_stream;
    const float thresh = weight_thresh + 0.f;  // (-0 becomes +0)
    uint32_t thresh_bits;
    std::memcpy(&thresh_bits, &thresh, 4);

    // the call holds the walk's scratch, and with it its own counters, until it has waited for the stream
    mnv::WalkGuard guard;
    mnv::LevelLists L;
    if ((rc = guard.begin(stream))) return rc;
    mnv::Mirrored<unsigned long long> &ctr = g_cull_ctr[guard.device()];
    if (!ctr && (rc = mnv::alloc_pair(ctr, kCtrWords, "hipMalloc(level counters)", "hipHostMalloc(level counters)"))) return rc;
    if ((rc = check_hip(hipMemsetAsync(ctr.dev.get(), 0, kCtrWords * 8, stream), "level counters")) ||
        (rc = check_hip(hipMemsetAsync(keep_out, 0, (size_t)cap, stream), "clear keep")) ||
        (rc = mnv::walk_levels(tree->child, cap, nullptr, who, guard, L)))
        return rc;
    int log2_g = 3;  // lanes per chunk: 8, 16, 32 or 64, at least data_dim where that is below 64
    while ((1 << log2_g) < dd && log2_g < 6) ++log2_g;
    const int per_block = kWavesPerBlock * (64 >> log2_g);
    for (int d = L.levels; d >= 1; --d) {
        hipLaunchKernelGGL(cull_rows_kernel, dim3(std::min(mnv::blocks_for(L.size(d), per_block), (unsigned)kCullGrid)), dim3(64 * kWavesPerBlock), 0, stream, tree->data, data_out,
                           tree->child, wmax, thresh_bits, L.order + L.offset[d], L.size(d), dd, log2_g, d, keep_out, ctr.dev.get());
        if ((rc = check_hip(hipGetLastError(), "cull_rows_kernel"))) return rc;
    }
    if (L.offset[L.levels + 1] < cap && (rc = mnv::copy_unreached(tree->data, data_out, L.depth, cap, dd, stream))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(ctr.host.get(), ctr.dev.get(), kCtrWords * 8, hipMemcpyDeviceToHost, stream), "cull counters")) ||
        (rc = check_hip(hipStreamSynchronize(stream), who)))
        return rc;
    const unsigned long long *c = ctr.host.get();
    counts->leaves_seen = (int64_t)c[kCtrSeen];
    counts->leaves_culled = (int64_t)c[kCtrCulled];
    counts->dead_chunks = (int64_t)c[kCtrDead];
    for (int d = 1; d < 24; ++d) kept_at_depth[d] = (int64_t)c[kCtrKept + d];
    return MNV_OK;
}

}  // extern "C"
