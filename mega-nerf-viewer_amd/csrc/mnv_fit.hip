// mnv_fit.hip -- fitting a tree's rows to target rays: mnv_rays_grad (the march of a ray list and its gradient in one launch),
// mnv_rows_master_init and mnv_rows_sgd_step (the float32 master copy of the rows and one gradient step on it).  The contract is
// include/mnv.h's ("fitting a tree's rows"); DESIGN.md 5.16 derives the density term.  tests/fit_ref.py restates all three in numpy.
//
// mnv_rays_grad: one ray per lane, one wavefront per workgroup, 8 x 8 ray tiles (64 x 1 for a flat list) as the other ray kernels; a
// workgroup walks tiles with the grid's stride, so the five sums cost one atomic each per workgroup and not per tile.  Two marches per ray
// instead of a per-ray sample store: the first is the forward march (on the view's own child / data arrays: the rows change between two
// calls, so there is no accel to read) and gives the pixel, S_k, T_end and with them g_k, scale and B_k; the second repeats the same steps
// -- the same instructions on the same inputs -- with the prefix P_k and emits every dense sample's terms.
// The scatter: a row's data_dim accumulators are contiguous (224 bytes for SH9).  The lanes that took a dense sample in this step write
// (voxel, gc / gt, density term, lane) to a compact list in LDS; then the wavefront walks the list, 64 / G samples at a time (G the power of
// two >= data_dim), and lane c of a group adds column c of that sample's row: one 64-bit integer atomic per lane, consecutive lanes on
// consecutive words, result unused.  Every term is rounded to fixed point BEFORE it leaves its lane, so nothing depends on who adds what
// when.  Lanes that hit the same voxel are not merged (integer addition would allow it; no measurement asked for it yet).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mnv_internal.h"

#pragma clang fp contract(off)

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kMaxDescent = 23;       // levels, as the packed accel and mnv_accel_sample_points
constexpr int kMaxSteps = 1 << 20;    // march steps of one ray; a ray that needs more is skipped
constexpr int kGradGrid = 4096;       // workgroups of one wavefront: 16 per CU
constexpr int64_t kMaxRays = (int64_t)1 << 22;

struct FitArgs {
    mnv::FrameParams P;  // options, offset / scale, rot_dirs constants, tw x th, tmax_px, rgba
    const uint16_t *data;
    const int32_t *child;
    const float *origins, *dirs;
    const float4 *target;
    unsigned long long *acc;
    unsigned long long *sums;
    int32_t data_dim, capacity;
    int32_t tiles_x, n_tiles, flat;
    int32_t group_log2;  // G = 1 << group_log2 lanes add one sample's row
};

// llrint((double)sat(x) * 2^32): the product is exact in double, the rounding is to nearest even
__device__ __forceinline__ long long q32(float x) {
    const float s = x != x ? 0.f : fminf(fmaxf(x, -32.f), 32.f);
    return (long long)rint((double)s * 4294967296.0);
}

__device__ __forceinline__ bool finite3(float a, float b, float c) { return (a - a) + (b - b) + (c - c) == 0.f; }

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;  // (lane 0 holds the sum)
}

// One march step at t (rt_core.cuh:220-231): the leaf under the ray, delta_t and sigma.  false: the descent left the tree.
__device__ __forceinline__ bool march_step(const FitArgs &K, const float (&cen)[3], const float (&dir)[3], const float (&invdir)[3], float t, int32_t &vox,
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

// The colour of a dense sample: the forward's three terms (what S_k / P_k accumulate) and c_sk.
template <int BASIS>
__device__ __forceinline__ void sample_colour(const FitArgs &K, const uint16_t *__restrict__ row, const float *basis, float weight, const uint64_t *s_exp,
                                              float (&term)[3], float (&c)[3]) {
    if constexpr (BASIS > 0) {
        auto coef = [&](int k) { return mnv::half_bits_to_float(row[k]); };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float tmp = mnv::sh_channel<BASIS>(basis, coef, k * BASIS);
            const float den = 1.f + mnv::exact_expf(-tmp, s_exp);
            term[k] = weight / den;  // colour_sigmoid<false>
            c[k] = 1.f / den;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = mnv::half_bits_to_float(row[k]);
            term[k] = c[k] * weight;
        }
    }
}

template <int BASIS /* -1 RGBA; 1 / 4 / 9 / 16 / 25 */>
__global__ __launch_bounds__(64) void rays_grad_kernel(const FitArgs K) {
    constexpr int NB = BASIS > 0 ? BASIS : 1, NBP = NB | 1;  // (an odd pitch: lane l's basis at l * NBP, conflict-free either way)
    __shared__ uint64_t s_exp[32];
    __shared__ float s_basis[64 * NBP];
    __shared__ uint32_t s_stage[64 * 8];  // the step's dense samples, compact: vox, x0, x1, x2, density term, lane
    mnv::load_exp_table(s_exp);
    const mnv::FrameParams &P = K.P;
    const int lane = threadIdx.x;
    const int G = 1 << K.group_log2, n_groups = 64 >> K.group_log2;
    long long sum[5] = {0, 0, 0, 0, 0};  // n_rays, n_stopped, n_samples, n_skipped, se_q32

    for (int tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
        const int bx = K.flat ? tile * 64 + lane : (tile % K.tiles_x) * 8 + (lane & 7);
        const int by = K.flat ? 0 : (tile / K.tiles_x) * 8 + (lane >> 3);
        const bool has_ray = bx < P.tw && by < P.th;
        const int64_t pix = has_ray ? (int64_t)by * P.tw + bx : 0;

        // ---- the ray (march_accel_kernel<.., RAYS>, statement for statement)
        mnv::RaySetup<NB> r;
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
            mnv::setup_ray_dir<(BASIS > 0 ? BASIS : 0)>(P, cen, d, r, mnv::frame_tmax(P, pix));
            r.in_bbox = r.in_bbox && valid;
        }

        // ---- first march: the forward (rt_core.cuh:220-331)
        float S[3] = {0.f, 0.f, 0.f}, T = 1.f;
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
                    const float weight = T * (1.f - att);
                    float term[3], c[3];
                    sample_colour<BASIS>(K, K.data + (int64_t)vox * K.data_dim, r.basis, weight, s_exp, term, c);
                    S[0] += term[0];
                    S[1] += term[1];
                    S[2] += term[2];
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
        const float scale = stopped ? 1.f / (1.f - T) : 1.f;
        float C[3] = {S[0], S[1], S[2]};
        float o3 = 0.f;
        if (stopped) {
            C[0] *= scale;
            C[1] *= scale;
            C[2] *= scale;
            o3 = 1.f;
        } else if (r.in_bbox) {
            o3 = 1.f - T;
        }
        const float remain = P.background_brightness * (1.f - o3);  // composite_and_write, the offscreen branch
        C[0] += remain;
        C[1] += remain;
        C[2] += remain;
        if (has_ray && P.rgba) reinterpret_cast<float4 *>(P.rgba)[pix] = make_float4(C[0], C[1], C[2], o3);

        // ---- the loss of this ray
        float4 tg = make_float4(0.f, 0.f, 0.f, 0.f);
        if (has_ray) tg = K.target[pix];
        const bool included = has_ray && tg.w != 0.f;
        const float g[3] = {C[0] - tg.x, C[1] - tg.y, C[2] - tg.z};
        const bool skipped = included && (broken || !finite3(C[0], C[1], C[2]) || !finite3(g[0], g[1], g[2]));
        const bool counts = included && !skipped;
        if (counts) {
            sum[0] += 1;
            sum[1] += stopped ? 1 : 0;
            sum[2] += n_dense;
            sum[4] += q32((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        }
        if (skipped) sum[3] += 1;

        // ---- second march: the same steps with the prefix sums; the wavefront scatters each step's dense samples together
        bool alive = counts && n_dense > 0;
        if (__ballot(alive) == 0) continue;  // (wave-uniform)
        const float gs[3] = {g[0] * scale, g[1] * scale, g[2] * scale};
        const float T_end = T;
        float bt[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) bt[k] = (stopped ? C[k] : P.background_brightness) * T_end;
        if constexpr (BASIS > 0) {
#pragma unroll
            for (int j = 0; j < NB; ++j) s_basis[lane * NBP + j] = r.basis[j];
        }
        float Pk[3] = {0.f, 0.f, 0.f}, t = r.tmin;
        T = 1.f;
        int left = n_dense;
        while (__ballot(alive) != 0) {
            bool dense = false;
            int32_t vox = 0;
            float x[3] = {0.f, 0.f, 0.f}, dens = 0.f;
            if (alive) {
                float delta_t, sigma;
                (void)march_step(K, cen, r.dir, r.invdir, t, vox, delta_t, sigma);  // (the first march took this very step)
                if (sigma > P.sigma_thresh) {
                    const float att = mnv::exact_expf(-delta_t * r.delta_scale * sigma, s_exp);
                    const float weight = T * (1.f - att);
                    float term[3], c[3];
                    sample_colour<BASIS>(K, K.data + (int64_t)vox * K.data_dim, r.basis, weight, s_exp, term, c);
                    const float Tn = T * att;
                    float e[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        Pk[k] += term[k];
                        const float Q = S[k] - Pk[k];
                        const float gc = gs[k] * weight;
                        if constexpr (BASIS > 0) x[k] = gc * (c[k] * (1.f - c[k]));
                        else x[k] = gc;
                        e[k] = (Tn * c[k] - Q) - bt[k];
                    }
                    const float ds = (delta_t * r.delta_scale) * scale;
                    dens = ds * ((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2]);
                    dense = true;
                    T = Tn;
                    --left;
                }
                t = t + delta_t;
                alive = left > 0 && t < r.tmax;  // (the samples behind the last dense one are the forward's business alone)
            }
            const uint64_t mask = __ballot(dense);
            if (mask == 0) continue;
            if (dense) {
                const int slot = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                uint32_t *st = s_stage + slot * 8;
                st[0] = (uint32_t)vox;
                st[1] = __float_as_uint(x[0]);
                st[2] = __float_as_uint(x[1]);
                st[3] = __float_as_uint(x[2]);
                st[4] = __float_as_uint(dens);
                st[5] = (uint32_t)lane;
            }
            __syncthreads();  // (one wavefront: the list is written)
            const int n_list = __builtin_popcountll(mask);
            const int grp = lane >> K.group_log2, col0 = lane & (G - 1);
            for (int base = 0; base < n_list; base += n_groups) {
                const int slot = base + grp;
                if (slot >= n_list) continue;
                const uint32_t *st = s_stage + slot * 8;
                unsigned long long *row = K.acc + (int64_t)st[0] * K.data_dim;
                for (int col = col0; col < K.data_dim; col += G) {
                    float v;
                    if (col == K.data_dim - 1) {
                        v = __uint_as_float(st[4]);
                    } else if constexpr (BASIS > 0) {
                        if (col >= 3 * BASIS) continue;
                        const int k = col / BASIS, j = col - k * BASIS;
                        if (j < P.basis_min || j > P.basis_max) continue;  // a masked coefficient gets no term
                        v = __uint_as_float(st[1 + k]) * s_basis[(int)st[5] * NBP + j];
                    } else {
                        if (col >= 3) continue;
                        v = __uint_as_float(st[1 + col]);
                    }
                    const long long q = q32(v);
                    if (q != 0) atomicAdd(row + col, (unsigned long long)q);
                }
            }
            __syncthreads();  // (the list is read before the next step rewrites it)
        }
    }

#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const long long s = wave_sum(sum[k]);
        if (lane == 0 && s != 0) atomicAdd(K.sums + k, (unsigned long long)s);
    }
}

__global__ __launch_bounds__(256) void master_init_kernel(const uint16_t *__restrict__ data, int64_t n, float *__restrict__ master) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint16_t h = data[i];
        master[i] = (h & 0x7c00u) == 0x7c00u ? 0.f : mnv::half_bits_to_float(h);
    }
}

// binary16(m), round to nearest even, saturating at +-65504; NaN: +0
__device__ __forceinline__ uint16_t half_sat(float m) {
    const float s = m != m ? 0.f : fminf(fmaxf(m, -65504.f), 65504.f);
    const _Float16 h = (_Float16)s;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

// A workgroup owns 256 consecutive rows = 256 * data_dim consecutive words of each array, and walks them twice with consecutive lanes on
// consecutive words: the first pass marks the rows that have a word set (in LDS), the second updates the words of marked rows -- the
// accumulators are read again from cache.  (One row per lane read 64 lines per instruction: 0.30 TB/s on cfg2's 2.7 GB.)
constexpr int kSgdRows = 256;
__global__ __launch_bounds__(256) void sgd_step_kernel(uint16_t *__restrict__ data, float *__restrict__ master, long long *__restrict__ acc, int64_t n_rows,
                                                       int data_dim, float lr_colour, float lr_sigma) {
    __shared__ int touched[kSgdRows];
    for (int64_t r0 = (int64_t)blockIdx.x * kSgdRows; r0 < n_rows; r0 += (int64_t)gridDim.x * kSgdRows) {
        const int rows = (int)(n_rows - r0 < kSgdRows ? n_rows - r0 : kSgdRows);
        const int words = rows * data_dim;
        const int64_t base = r0 * data_dim;
        touched[threadIdx.x] = 0;
        __syncthreads();
        for (int e = threadIdx.x; e < words; e += 256)
            if (acc[base + e] != 0) touched[e / data_dim] = 1;  // (every writer stores the same value)
        __syncthreads();
        for (int e = threadIdx.x; e < words; e += 256) {
            const int row = e / data_dim, c = e - row * data_dim;
            if (!touched[row]) continue;
            const float g = (float)((double)acc[base + e] * (1.0 / 4294967296.0));
            const float step = (c == data_dim - 1 ? lr_sigma : lr_colour) * g;
            float v = master[base + e] - step;
            if (c == data_dim - 1) v = v < 0.f ? 0.f : v;
            master[base + e] = v;
            data[base + e] = half_sat(v);
            acc[base + e] = 0;
        }
        __syncthreads();  // (the marks are read before the next tile clears them)
    }
}

template <int B>
int launch_grad(const FitArgs &K, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(rays_grad_kernel<B>, dim3((unsigned)grid), dim3(64), 0, stream, K);
    return check_hip(hipGetLastError(), "rays_grad_kernel");
}

}  // namespace

extern "C" {

int mnv_rays_grad(const mnv_tree_view *tree, const float *origins, const float *dirs, const float *target, const float *tmax, int32_t width, int32_t height,
                  const mnv_render_options *opt, float *rgba_out, int64_t *acc, mnv_fit_sums *sums, void *hip_stream) {
    // every argument before any device call
    if (!tree || !origins || !dirs || !target || !opt || !acc || !sums) return set_error(MNV_E_INVALID, "mnv_rays_grad: null tree / rays / target / options / acc / sums");
    if (width < 1 || height < 1) return set_error(MNV_E_INVALID, "mnv_rays_grad: a ray image needs width >= 1 and height >= 1");
    if ((int64_t)width * (int64_t)height > kMaxRays) return set_error(MNV_E_INVALID, "mnv_rays_grad: more than 2^22 rays in one call (the accumulators' headroom)");
    if (tree->N != 2) return set_error(MNV_E_UNSUPPORTED, "mnv_rays_grad: N != 2");
    if (opt->render_depth) return set_error(MNV_E_UNSUPPORTED, "mnv_rays_grad: render_depth has no gradient here");
    if (!tree->data || !tree->child || tree->capacity < 1) return set_error(MNV_E_INVALID, "mnv_rays_grad: the view holds no tree");
    const int b = (tree->format == MNV_FORMAT_SH && tree->basis_dim >= 0) ? tree->basis_dim : -1;
    if (!(b == -1 || b == 1 || b == 4 || b == 9 || b == 16 || b == 25)) return set_error(MNV_E_UNSUPPORTED, "mnv_rays_grad: RGBA and SH1/4/9/16/25 rows (what the ray march serves)");
    if (tree->data_dim < (b > 0 ? 3 * b + 1 : 4)) return set_error(MNV_E_INVALID, "mnv_rays_grad: data_dim too small for the row format");
    if (!std::isfinite(opt->step_size) || !(opt->step_size > 0.f)) return set_error(MNV_E_INVALID, "mnv_rays_grad: step_size must be finite and positive (the march must advance)");
    if ((((uintptr_t)acc | (uintptr_t)sums) & 7u) != 0) return set_error(MNV_E_INVALID, "mnv_rays_grad: acc and sums must be 8-byte aligned");
    if ((((uintptr_t)target | (uintptr_t)rgba_out) & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_rays_grad: target and rgba_out must be 16-byte aligned");
    if ((((uintptr_t)origins | (uintptr_t)dirs | (uintptr_t)tmax) & 3u) != 0) return set_error(MNV_E_INVALID, "mnv_rays_grad: rays and tmax must be 4-byte aligned");
    FitArgs K;
    std::memset(static_cast<void *>(&K), 0, sizeof(K));
    mnv_camera shape = {};  // (fill_params wants an image size; the march reads no camera)
    shape.width = width;
    shape.height = height;
    shape.fx = shape.fy = 1.f;
    const int rc = mnv::fill_params(K.P, &shape, opt, mnv_rect{0, 0, width, height});
    if (rc) return rc;
    std::memcpy(K.P.offset, tree->offset, sizeof(K.P.offset));
    std::memcpy(K.P.scale, tree->scale, sizeof(K.P.scale));
    K.P.rgba = rgba_out;
    K.P.tmax_px = tmax;
    K.data = tree->data;
    K.child = tree->child;
    K.origins = origins;
    K.dirs = dirs;
    K.target = reinterpret_cast<const float4 *>(target);
    K.acc = reinterpret_cast<unsigned long long *>(acc);
    K.sums = reinterpret_cast<unsigned long long *>(sums);
    K.data_dim = tree->data_dim;
    K.capacity = tree->capacity;
    K.flat = height == 1 ? 1 : 0;
    K.tiles_x = K.flat ? (width + 63) / 64 : (width + 7) / 8;
    K.n_tiles = K.flat ? K.tiles_x : K.tiles_x * ((height + 7) / 8);
    int gl = 2;
    while (gl < 6 && (1 << gl) < tree->data_dim) ++gl;
    K.group_log2 = gl;
    const int grid = std::min(K.n_tiles, kGradGrid);
    hipStream_t stream = (hipStream_t)hip_stream;
    switch (b) {
        case -1: return launch_grad<-1>(K, grid, stream);
        case 1: return launch_grad<1>(K, grid, stream);
        case 4: return launch_grad<4>(K, grid, stream);
        case 9: return launch_grad<9>(K, grid, stream);
        case 16: return launch_grad<16>(K, grid, stream);
        default: return launch_grad<25>(K, grid, stream);
    }
}

int mnv_rows_master_init(const uint16_t *data, int64_t n, float *master_out, void *hip_stream) {
    if (!data || !master_out || n < 0) return set_error(MNV_E_INVALID, "mnv_rows_master_init: null array or negative count");
    if (n == 0) return MNV_OK;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(master_init_kernel, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, (hipStream_t)hip_stream, data, n, master_out);
    return check_hip(hipGetLastError(), "master_init_kernel");
}

int mnv_rows_sgd_step(uint16_t *data, float *master, int64_t *acc, int64_t n_rows, int32_t data_dim, float lr_colour, float lr_sigma, void *hip_stream) {
    if (!data || !master || !acc || n_rows < 0 || data_dim < 1) return set_error(MNV_E_INVALID, "mnv_rows_sgd_step: null array, negative row count or data_dim < 1");
    if (!std::isfinite(lr_colour) || !std::isfinite(lr_sigma)) return set_error(MNV_E_INVALID, "mnv_rows_sgd_step: the learning rates must be finite");
    if (((uintptr_t)acc & 7u) != 0 || ((uintptr_t)master & 3u) != 0 || ((uintptr_t)data & 1u) != 0) return set_error(MNV_E_INVALID, "mnv_rows_sgd_step: misaligned array");
    if (n_rows == 0) return MNV_OK;
    const int64_t blocks = (n_rows + 255) / 256;
    hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, (hipStream_t)hip_stream, data, master,
                       reinterpret_cast<long long *>(acc), n_rows, (int)data_dim, lr_colour, lr_sigma);
    return check_hip(hipGetLastError(), "sgd_step_kernel");
}

}  // extern "C"
