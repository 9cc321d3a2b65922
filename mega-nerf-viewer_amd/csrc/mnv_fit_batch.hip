// mnv_fit_batch.hip -- what a fit on a photo set needs beside mnv_fit.hip: mnv_rows_adam_step (the row update with Adam's normalised step)
// and mnv_ray_batcher_* (mini-batches of rays and targets drawn across a set of cameras and images, on the device).  The contracts are
// include/mnv.h's ("fitting on a photo set"); tests/fit_adam_ref.py restates both in numpy.
//
// adam_step_kernel has sgd_step_kernel's shape (mnv_fit.hip): a workgroup owns 256 consecutive rows, marks the touched ones in LDS and walks
// the words of all four arrays with consecutive lanes on consecutive words -- one 8-byte and three 4-byte loads per touched word, the same
// back plus the 2-byte row word.  Every operation of the update is one binary32 instruction: no contraction (the pragma below and the
// Makefile's flag), division and square root correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).
//
// The batcher's permutation is integer arithmetic only (a 4-round Feistel network with cycle walking), so a draw is a pure function of
// (handle, epoch, first, count): no atomics, no state on the device that a draw changes, any stream.  tile 8: one wavefront per unit -- the
// unit number, the camera search and the camera block are wave-uniform (scalar loads), the 64 lanes are the 8 x 8 pixels; origins and
// directions go through LDS so that a unit's 768 bytes leave as 48 aligned 16-byte stores.  tile 1: one lane per unit, the prefix table in
// LDS, outputs staged as mnv_generate_rays stages them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mnv_internal.h"

#pragma clang fp contract(off)

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kRows = 256;             // rows of one workgroup, as sgd_step_kernel
constexpr int kMaxCams = 4096;         // the prefix table of the tile-1 kernel sits in LDS
constexpr int64_t kMaxRays = (int64_t)1 << 22;  // mnv_rays_grad's limit

// binary16(m), round to nearest even, saturating at +-65504; NaN: +0 -- sgd_step_kernel's (mnv_fit.hip), statement for statement
__device__ __forceinline__ uint16_t half_sat(float m) {
    const float s = m != m ? 0.f : fminf(fmaxf(m, -65504.f), 65504.f);
    const _Float16 h = (_Float16)s;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

struct AdamArgs {
    float lr_colour, lr_sigma, beta1, beta2, omb1, omb2, c1, c2, eps;
};

__global__ __launch_bounds__(256) void adam_step_kernel(uint16_t *__restrict__ data, float *__restrict__ master, float *__restrict__ m1, float *__restrict__ m2,
                                                        long long *__restrict__ acc, int64_t n_rows, int data_dim, const AdamArgs A) {
    __shared__ int touched[kRows];
    for (int64_t r0 = (int64_t)blockIdx.x * kRows; r0 < n_rows; r0 += (int64_t)gridDim.x * kRows) {
        const int rows = (int)(n_rows - r0 < kRows ? n_rows - r0 : kRows);
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
            const float a = (m1[base + e] * A.beta1) + (g * A.omb1);
            const float v = (m2[base + e] * A.beta2) + ((g * g) * A.omb2);
            const float den = sqrtf(v * A.c2) + A.eps;
            const float upd = ((c == data_dim - 1 ? A.lr_sigma : A.lr_colour) * (a * A.c1)) / den;
            float m = master[base + e] - upd;
            if (c == data_dim - 1) m = m < 0.f ? 0.f : m;
            m1[base + e] = a;
            m2[base + e] = v;
            master[base + e] = m;
            data[base + e] = half_sat(m);
            acc[base + e] = 0;
        }
        __syncthreads();  // (the marks are read before the next tile clears them)
    }
}

// ---- the batcher
struct DevCam {  // 96 bytes: the pinhole constants of mnv_generate_rays, the image and where its target is
    float fx, fy, cx, cy;
    float m[12];
    int32_t w, h, tiles_x, pad;
    const float4 *target;
    uint64_t pad2;
};

struct Perm {
    uint32_t key[4];
    uint32_t k, mask, units;
};

struct DrawArgs {
    Perm P;
    const DevCam *cams;
    const uint32_t *prefix;  // [n_cams + 1]: the first unit of every camera, then U
    int32_t n_cams;
    int64_t first, count;
    float *origins, *dirs;
    float4 *target;
    int32_t vector_stores;  // origins and dirs are 16-byte aligned
};

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The unit at place i < U of the epoch's order.  The Feistel map is a bijection of [0, 2^2k); the walk follows i's orbit under it, which
// comes back to i < U, so it meets a value below U after at most 2^2k <= 4U applications (on average under four).
__host__ __device__ __forceinline__ uint32_t perm(const Perm &P, uint32_t i) {
    uint32_t x = i;
    do {
        uint32_t L = x >> P.k, R = x & P.mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t t = L ^ (mix32(R ^ P.key[r]) & P.mask);
            L = R;
            R = t;
        }
        x = (L << P.k) | R;
    } while (x >= P.units);
    return x;
}

// the camera of unit u: the last c with prefix[c] <= u (prefix[0] == 0, u < prefix[n_cams])
template <typename Table>
__device__ __forceinline__ int camera_of(const Table prefix, int n_cams, uint32_t u) {
    int lo = 0, hi = n_cams;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

// mnv_generate_rays' pinhole ray of pixel (ix, iy), statement for statement
__device__ __forceinline__ void pinhole_ray(const DevCam &cam, int ix, int iy, float (&o)[3], float (&d)[3]) {
    const float u = (ix + 0.5f - cam.cx) / cam.fx, v = -(iy + 0.5f - cam.cy) / cam.fy;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = cam.m[9 + k];
        d[k] = cam.m[k] * u + cam.m[3 + k] * v + cam.m[6 + k] * -1.f;
    }
}

// 256 staged rays (3 floats each) of one output leave as aligned 16-byte vectors; `floats` of them are valid
__device__ __forceinline__ void store_staged(float *__restrict__ out, const float *s, int floats, bool vector_stores) {
    const int t = threadIdx.x;
    if (vector_stores && 4 * t + 4 <= floats) {
        reinterpret_cast<float4 *>(out)[t] = reinterpret_cast<const float4 *>(s)[t];
    } else if (vector_stores) {
        for (int f = 4 * t; f < floats; ++f) out[f] = s[f];
    } else {
        for (int f = t; f < floats; f += 256) out[f] = s[f];
    }
}

// tile 8: wavefront w of workgroup b writes unit j = 4 b + w, lane l its pixel (tx * 8 + (l & 7), ty * 8 + (l >> 3))
__global__ __launch_bounds__(256) void draw_tiles_kernel(const DrawArgs A) {
    __shared__ __attribute__((aligned(16))) float s_o[256 * 3];
    __shared__ __attribute__((aligned(16))) float s_d[256 * 3];
    const int lane = threadIdx.x & 63;
    const int64_t j0 = (int64_t)blockIdx.x * 4;
    const int64_t j = j0 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (j < A.count) {
        const uint32_t u = perm(A.P, (uint32_t)(A.first + j));
        const int c = camera_of(A.prefix, A.n_cams, u);
        const DevCam &cam = A.cams[c];
        const uint32_t local = u - A.prefix[c];
        const int ty = (int)(local / (uint32_t)cam.tiles_x), tx = (int)(local - (uint32_t)ty * (uint32_t)cam.tiles_x);
        const int ix = tx * 8 + (lane & 7), iy = ty * 8 + (lane >> 3);
        float4 tg = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ix < cam.w && iy < cam.h) {
            pinhole_ray(cam, ix, iy, o, d);
            tg = cam.target[(int64_t)iy * cam.w + ix];
        } else {  // a lane outside the image: a degenerate ray (a miss) with an excluded target
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = cam.m[9 + k];
        }
        A.target[j * 64 + lane] = tg;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s_o[threadIdx.x * 3 + k] = o[k];
        s_d[threadIdx.x * 3 + k] = d[k];
    }
    __syncthreads();
    const int64_t left = A.count - j0;  // units of this workgroup and behind it (>= 1)
    const int floats = (int)(left < 4 ? left : 4) * 192;
    store_staged(A.origins + j0 * 192, s_o, floats, A.vector_stores != 0);
    store_staged(A.dirs + j0 * 192, s_d, floats, A.vector_stores != 0);
}

// tile 1: lane t of workgroup b writes unit j = 256 b + t, a pixel
__global__ __launch_bounds__(256) void draw_pixels_kernel(const DrawArgs A) {
    __shared__ uint32_t s_prefix[kMaxCams + 1];
    __shared__ __attribute__((aligned(16))) float s_o[256 * 3];
    __shared__ __attribute__((aligned(16))) float s_d[256 * 3];
    for (int i = threadIdx.x; i <= A.n_cams; i += 256) s_prefix[i] = A.prefix[i];
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (j < A.count) {
        const uint32_t u = perm(A.P, (uint32_t)(A.first + j));
        const int c = camera_of(s_prefix, A.n_cams, u);
        const DevCam &cam = A.cams[c];
        const uint32_t local = u - s_prefix[c];
        const int iy = (int)(local / (uint32_t)cam.w), ix = (int)(local - (uint32_t)iy * (uint32_t)cam.w);
        pinhole_ray(cam, ix, iy, o, d);
        A.target[j] = cam.target[local];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s_o[threadIdx.x * 3 + k] = o[k];
        s_d[threadIdx.x * 3 + k] = d[k];
    }
    __syncthreads();
    const int64_t left = A.count - j0;
    const int floats = (int)(left < 256 ? left : 256) * 3;
    store_staged(A.origins + j0 * 3, s_o, floats, A.vector_stores != 0);
    store_staged(A.dirs + j0 * 3, s_d, floats, A.vector_stores != 0);
}

}  // namespace

struct mnv_ray_batcher {
    mnv::Buffer<DevCam> cams;
    mnv::Buffer<uint32_t> prefix;
    int32_t n_cams = 0, tile = 8;
    uint64_t seed = 0;
    int64_t units = 0;
};

extern "C" {

int mnv_rows_adam_step(uint16_t *data, float *master, float *m1, float *m2, int64_t *acc, int64_t n_rows, int32_t data_dim, const mnv_adam_params *p,
                       int64_t step, void *hip_stream) {
    if (!data || !master || !m1 || !m2 || !acc || !p || n_rows < 0 || data_dim < 1)
        return set_error(MNV_E_INVALID, "mnv_rows_adam_step: null array or parameters, negative row count or data_dim < 1");
    if (step < 1) return set_error(MNV_E_INVALID, "mnv_rows_adam_step: steps are counted from 1");
    if (!std::isfinite(p->lr_colour) || !std::isfinite(p->lr_sigma)) return set_error(MNV_E_INVALID, "mnv_rows_adam_step: the learning rates must be finite");
    if (!(p->beta1 >= 0.f && p->beta1 < 1.f) || !(p->beta2 >= 0.f && p->beta2 < 1.f)) return set_error(MNV_E_INVALID, "mnv_rows_adam_step: beta1 and beta2 must lie in [0, 1)");
    if (!std::isfinite(p->eps) || !(p->eps > 0.f)) return set_error(MNV_E_INVALID, "mnv_rows_adam_step: eps must be finite and positive");
    if (((uintptr_t)acc & 7u) != 0 || (((uintptr_t)master | (uintptr_t)m1 | (uintptr_t)m2) & 3u) != 0 || ((uintptr_t)data & 1u) != 0)
        return set_error(MNV_E_INVALID, "mnv_rows_adam_step: misaligned array");
    if (n_rows == 0) return MNV_OK;
    AdamArgs A;
    A.lr_colour = p->lr_colour;
    A.lr_sigma = p->lr_sigma;
    A.beta1 = p->beta1;
    A.beta2 = p->beta2;
    A.omb1 = 1.f - p->beta1;
    A.omb2 = 1.f - p->beta2;
    A.c1 = (float)(1.0 / (1.0 - std::pow((double)p->beta1, (double)step)));
    A.c2 = (float)(1.0 / (1.0 - std::pow((double)p->beta2, (double)step)));
    A.eps = p->eps;
    const int64_t blocks = (n_rows + kRows - 1) / kRows;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, (hipStream_t)hip_stream, data, master, m1, m2,
                       reinterpret_cast<long long *>(acc), n_rows, (int)data_dim, A);
    return check_hip(hipGetLastError(), "adam_step_kernel");
}

int mnv_ray_batcher_create(const mnv_camera *cams, const float *const *targets, int32_t n_cams, int32_t tile, uint64_t seed, mnv_ray_batcher **out) {
    if (!cams || !targets || !out) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: null cameras / targets / handle");
    if (n_cams < 1 || n_cams > kMaxCams) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: 1 .. 4096 cameras");
    if (tile != 1 && tile != 8) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: a unit is a pixel (tile 1) or an 8 x 8 tile (tile 8)");
    std::vector<DevCam> dc((size_t)n_cams);
    std::vector<uint32_t> prefix((size_t)n_cams + 1, 0u);
    int64_t units = 0;
    for (int32_t i = 0; i < n_cams; ++i) {
        const mnv_camera &c = cams[i];
        if (!targets[i]) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: a target image is null");
        if (((uintptr_t)targets[i] & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: a target image is not 16-byte aligned");
        if (c.width < 1 || c.height < 1) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: a camera has no pixels");
        DevCam &d = dc[(size_t)i];
        std::memset(static_cast<void *>(&d), 0, sizeof(d));
        d.fx = c.fx, d.fy = c.fy, d.cx = c.cx, d.cy = c.cy;
        std::memcpy(d.m, c.c2w, sizeof(d.m));
        d.w = c.width, d.h = c.height;
        d.tiles_x = (c.width + 7) / 8;
        d.target = reinterpret_cast<const float4 *>(targets[i]);
        prefix[(size_t)i] = (uint32_t)units;
        units += tile == 8 ? (int64_t)d.tiles_x * ((c.height + 7) / 8) : (int64_t)c.width * c.height;
        if (units >= ((int64_t)1 << 31)) return set_error(MNV_E_INVALID, "mnv_ray_batcher_create: 2^31 units or more");
    }
    prefix[(size_t)n_cams] = (uint32_t)units;
    mnv_ray_batcher *b = new mnv_ray_batcher;
    int rc = check_hip(b->cams.alloc(dc.size()), "hipMalloc(batcher cameras)");
    if (!rc) rc = check_hip(b->prefix.alloc(prefix.size()), "hipMalloc(batcher prefix table)");
    if (!rc) rc = check_hip(hipMemcpy(b->cams.get(), dc.data(), dc.size() * sizeof(DevCam), hipMemcpyHostToDevice), "upload batcher cameras");
    if (!rc) rc = check_hip(hipMemcpy(b->prefix.get(), prefix.data(), prefix.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "upload batcher prefix table");
    if (rc) {
        delete b;
        return rc;
    }
    b->n_cams = n_cams;
    b->tile = tile;
    b->seed = seed;
    b->units = units;
    *out = b;
    return MNV_OK;
}

int mnv_ray_batcher_units(const mnv_ray_batcher *b, int64_t *units, int32_t *rays_per_unit) {
    if (!b) return set_error(MNV_E_INVALID, "mnv_ray_batcher_units: null handle");
    if (units) *units = b->units;
    if (rays_per_unit) *rays_per_unit = b->tile * b->tile;
    return MNV_OK;
}

int mnv_ray_batcher_draw(const mnv_ray_batcher *b, int64_t epoch, int64_t first, int64_t count, float *origins_out, float *dirs_out, float *target_out,
                         void *hip_stream) {
    // every argument before any device call
    if (!b || !origins_out || !dirs_out || !target_out) return set_error(MNV_E_INVALID, "mnv_ray_batcher_draw: null handle or output");
    if (epoch < 0) return set_error(MNV_E_INVALID, "mnv_ray_batcher_draw: negative epoch");
    if (first < 0 || count < 1 || first > b->units || count > b->units - first) return set_error(MNV_E_INVALID, "mnv_ray_batcher_draw: the window leaves [0, units)");
    const int64_t per = (int64_t)b->tile * b->tile;
    if (count > kMaxRays / per) return set_error(MNV_E_INVALID, "mnv_ray_batcher_draw: more than 2^22 rays in one draw (mnv_rays_grad's limit)");
    if ((((uintptr_t)origins_out | (uintptr_t)dirs_out) & 3u) != 0 || ((uintptr_t)target_out & 15u) != 0)
        return set_error(MNV_E_INVALID, "mnv_ray_batcher_draw: origins / dirs must be 4-byte aligned, the targets 16-byte aligned");
    DrawArgs A;
    std::memset(static_cast<void *>(&A), 0, sizeof(A));
    const uint32_t lo = (uint32_t)b->seed, hi = (uint32_t)(b->seed >> 32);
    const uint32_t base = mix32(lo ^ mix32(hi ^ (uint32_t)epoch));
    for (uint32_t r = 0; r < 4; ++r) A.P.key[r] = mix32(base + r);
    uint32_t bitlen = 0;
    for (uint64_t v = (uint64_t)b->units - 1; v != 0; v >>= 1) ++bitlen;
    A.P.k = std::max<uint32_t>(1u, (bitlen + 1) / 2);
    A.P.mask = (1u << A.P.k) - 1u;
    A.P.units = (uint32_t)b->units;
    A.cams = b->cams.get();
    A.prefix = b->prefix.get();
    A.n_cams = b->n_cams;
    A.first = first;
    A.count = count;
    A.origins = origins_out;
    A.dirs = dirs_out;
    A.target = reinterpret_cast<float4 *>(target_out);
    A.vector_stores = (((uintptr_t)origins_out | (uintptr_t)dirs_out) & 15u) == 0 ? 1 : 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (b->tile == 8) {
        hipLaunchKernelGGL(draw_tiles_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, A);
        return check_hip(hipGetLastError(), "draw_tiles_kernel");
    }
    hipLaunchKernelGGL(draw_pixels_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, A);
    return check_hip(hipGetLastError(), "draw_pixels_kernel");
}

void mnv_ray_batcher_destroy(mnv_ray_batcher *b) { delete b; }

}  // extern "C"
