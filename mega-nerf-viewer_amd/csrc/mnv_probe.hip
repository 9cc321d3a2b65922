// mnv_probe.hip -- element-wise probes of the device functions of mnv_device.h, for tests/test_primitives_gpu.py.  Linked into
// testhooks/libmnv.so only: the shipped library exports no mnv_hook_ symbol (tests/test_capi_symbols.py).
//
// Every kernel calls the very function the march kernels call -- nothing is restated here -- under the same compiler flags (the Makefile's csrc/%.o rule).  One thread per element, bounds-checked, 256-thread blocks; the
// expf table sits in LDS through load_exp_table as in the real kernels.  All array arguments are device pointers, `frame` / `cam` of
// mnv_hook_probe_setup_ray are host pointers to the argument blocks that the kernels take by value.  Every entry point returns MNV_OK or
// an MNV_E_* / HIP code and is asynchronous on `hip_stream`.
#include <hip/hip_runtime.h>

#include "mnv_internal.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;                         // consecutive-pattern kernels: patterns per thread ...
constexpr int kChunk = kThreads * kPerThread;          // ... and per workgroup (4096)
constexpr uint32_t kDigestBlock = 1u << 20;            // patterns per digest block
constexpr uint32_t kChunksPerBlock = kDigestBlock / kChunk;
constexpr int kSetupRow = 41;                          // floats per mnv_hook_probe_setup_ray row

unsigned grid_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// which 0 exact_expf, 1 exact_expf_select, 2 exact_expf_core (meaningful only where 3 says so), 3 the range test the march kernel puts in
// front of exact_expf_core, on the argument's magnitude bits: 1.0 in range, 0.0 out of it
__device__ __forceinline__ float expf_variant(float x, int which, const uint64_t *tab) {
    if (which == 3) return mnv::exact_expf_core_in_range(__float_as_uint(x) & 0x7fffffffu) ? 1.f : 0.f;
    if (which == 2) return mnv::exact_expf_core(x, tab);
    return which ? mnv::exact_expf_select(x, tab) : mnv::exact_expf(x, tab);
}

// result bits with every NaN replaced by the one quiet NaN (the digests and the variant comparison do not see NaN payloads)
__device__ __forceinline__ uint32_t canonical_bits(float v) { return v != v ? 0x7fc00000u : __float_as_uint(v); }

__global__ void __launch_bounds__(kThreads) probe_expf_kernel(const float *__restrict__ x, int64_t n, int which, float *__restrict__ out) {
    __shared__ uint64_t s_exp[32];
    mnv::load_exp_table(s_exp);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    out[i] = expf_variant(x[i], which, s_exp);
}

// Workgroup g covers the patterns [g * 4096, (g + 1) * 4096) of the range that starts at first_block * 2^20; it adds its share of
// sum(bits) and sum(bits * (i + 1)) (i: index in the 2^20 block, both mod 2^64) to the block's two words with one atomic each.
__global__ void __launch_bounds__(kThreads) probe_expf_digest_kernel(uint32_t first_block, uint32_t n_blocks, int which,
                                                                     unsigned long long *__restrict__ digests) {
    __shared__ uint64_t s_exp[32];
    __shared__ unsigned long long s_sum[2][kThreads];
    mnv::load_exp_table(s_exp);
    const uint32_t blk = blockIdx.x / kChunksPerBlock, chunk = blockIdx.x % kChunksPerBlock;
    unsigned long long a = 0, b = 0;
    if (blk < n_blocks) {
        const uint32_t base = (first_block + blk) * kDigestBlock;
#pragma unroll 4
        for (int k = 0; k < kPerThread; ++k) {
            const uint32_t i = chunk * kChunk + k * kThreads + threadIdx.x;
            const unsigned long long bits = canonical_bits(expf_variant(__uint_as_float(base + i), which, s_exp));
            a += bits;
            b += bits * (unsigned long long)(i + 1u);
        }
    }
    s_sum[0][threadIdx.x] = a;
    s_sum[1][threadIdx.x] = b;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_sum[0][threadIdx.x] += s_sum[0][threadIdx.x + w];
            s_sum[1][threadIdx.x] += s_sum[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2 && blk < n_blocks) atomicAdd(&digests[2 * (int64_t)blk + threadIdx.x], s_sum[threadIdx.x][0]);
}

__global__ void __launch_bounds__(kThreads) probe_expf_variants_differ_kernel(uint32_t first_bits, uint64_t n, unsigned long long *__restrict__ count,
                                                                              uint32_t *__restrict__ first16) {
    __shared__ uint64_t s_exp[32];
    mnv::load_exp_table(s_exp);
#pragma unroll 4
    for (int k = 0; k < kPerThread; ++k) {
        const uint64_t i = (uint64_t)blockIdx.x * kChunk + (uint64_t)k * kThreads + threadIdx.x;
        if (i >= n) break;
        const uint32_t bits = first_bits + (uint32_t)i;
        const float x = __uint_as_float(bits);
        if (canonical_bits(mnv::exact_expf(x, s_exp)) != canonical_bits(mnv::exact_expf_select(x, s_exp))) {
            const unsigned long long slot = atomicAdd(count, 1ull);
            if (slot < 16) first16[slot] = bits;
        }
    }
}

__global__ void __launch_bounds__(kThreads) probe_half_kernel(const uint16_t *__restrict__ bits, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    out[i] = mnv::half_bits_to_float(bits[i]);
}

__global__ void __launch_bounds__(kThreads) probe_sigmoid_kernel(const float *__restrict__ w, const float *__restrict__ t, int64_t n, int mode,
                                                                 float *__restrict__ out) {
    __shared__ uint64_t s_exp[32];
    mnv::load_exp_table(s_exp);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    out[i] = mode ? mnv::colour_sigmoid<true>(w[i], t[i], s_exp) : mnv::colour_sigmoid<false>(w[i], t[i], s_exp);
}

// dirs [n][3], coefs [n][3 * B] binary16 bits (channel c at c * B, as a voxel row) -> basis_out [n][B], channel_out [n][3]
template <int B>
__global__ void __launch_bounds__(kThreads) probe_sh_kernel(const float *__restrict__ dirs, const uint16_t *__restrict__ coefs, int64_t n,
                                                            float *__restrict__ basis_out, float *__restrict__ channel_out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    float b[B];
    mnv::sh_basis<B>(d, b);
#pragma unroll
    for (int k = 0; k < B; ++k) basis_out[i * B + k] = b[k];
    const uint16_t *row = coefs + i * 3 * B;
    auto coef = [&](int k) -> float { return mnv::half_bits_to_float(row[k]); };
#pragma unroll
    for (int c = 0; c < 3; ++c) channel_out[3 * i + c] = mnv::sh_channel<B>(b, coef, c * B);
}

// half_mul on every pair (word w, multiplier m): out[0][m][w] from the low half of words[w], out[1][m][w] from its high half -- every
// thread, so every lane position, runs both forms of the instruction
__global__ void __launch_bounds__(kThreads) probe_half_product_kernel(const uint32_t *__restrict__ words, int64_t n_words, const float *__restrict__ mult,
                                                                      int64_t n_mult, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_words * n_mult) return;
    const uint32_t w = words[i % n_words];
    const float b = mult[i / n_words];
    out[i] = mnv::half_mul(w, false, b);
    out[n_words * n_mult + i] = mnv::half_mul(w, true, b);
}

// basis [n][B], coefs [n][3 * B] binary16 bits (channel c at c * B, as a voxel row) -> channel_out [n][3] through sh_channel_mix on the
// row's 32-bit words, as the march kernels' per-lane colour block calls it (channel offsets 0, B, 2 B: odd ones for odd B)
template <int B>
__global__ void __launch_bounds__(kThreads) probe_sh_mix_kernel(const float *__restrict__ basis, const uint16_t *__restrict__ coefs, int64_t n,
                                                                float *__restrict__ channel_out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float b[B];
#pragma unroll
    for (int k = 0; k < B; ++k) b[k] = basis[i * B + k];
    constexpr int NW = (3 * B + 1) / 2;
    const uint16_t *row = coefs + i * 3 * B;
    uint32_t rw[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) rw[j] = (uint32_t)row[2 * j] | (2 * j + 1 < 3 * B ? (uint32_t)row[2 * j + 1] << 16 : 0u);
#pragma unroll
    for (int c = 0; c < 3; ++c) channel_out[3 * i + c] = mnv::sh_channel_mix<B>(b, [&](int j) -> uint32_t { return rw[j]; }, c * B);
}

// one row of kSetupRow floats per element: dir[3] invdir[3] delta_scale tmin tmax in_bbox basis[25] true_dir[3] vdir[3]
template <int B>
__global__ void __launch_bounds__(kThreads) probe_setup_ray_kernel(const mnv::FrameParams P, const mnv::CamBlock cam, const int32_t *__restrict__ ix,
                                                                   const int32_t *__restrict__ iy, const float *__restrict__ tmax, int64_t n,
                                                                   float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    mnv::RaySetup<B> r;
    mnv::setup_ray<B>(P, cam, ix[i], iy[i], r, tmax[i]);
    float true_dir[3], vdir[3];
    mnv::world_ray_dirs(P, cam, ix[i], iy[i], true_dir, vdir);
    float *o = out + i * kSetupRow;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = r.dir[k];
        o[3 + k] = r.invdir[k];
        o[35 + k] = true_dir[k];
        o[38 + k] = vdir[k];
    }
    o[6] = r.delta_scale;
    o[7] = r.tmin;
    o[8] = r.tmax;
    o[9] = r.in_bbox ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < 25; ++k) o[10 + k] = k < B ? r.basis[k] : 0.f;
}

// P.rgba / P.rgba8 / P.rgba8_init / P.background_brightness are set by the entry point; o [n] float4
__global__ void __launch_bounds__(kThreads) probe_composite_kernel(const mnv::FrameParams P, const float4 *__restrict__ o, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 v = o[i];
    mnv::composite_and_write(P, i, v.x, v.y, v.z, v.w);
}

}  // namespace

extern "C" {

// sizeof the two by-value argument blocks of mnv_hook_probe_setup_ray (the binding checks its mirrors against them)
int mnv_hook_probe_frame_size(void) { return (int)sizeof(mnv::FrameParams); }
int mnv_hook_probe_cam_size(void) { return (int)sizeof(mnv::CamBlock); }

// bytes the library's owners hold right now (csrc/mnv_devmem.h): which 0 device memory, 1 pinned host memory
int64_t mnv_hook_live_bytes(int which) {
    return which == 1 ? mnv::live_bytes<mnv::Mem::pinned>().load(std::memory_order_relaxed) : mnv::live_bytes<mnv::Mem::device>().load(std::memory_order_relaxed);
}

int mnv_hook_probe_expf(const float *x, int64_t n, int which, float *out, void *hip_stream) {
    if (n < 0 || (n > 0 && (!x || !out)) || which < 0 || which > 3) return set_error(MNV_E_INVALID, "mnv_hook_probe_expf: bad arguments");
    if (n == 0) return MNV_OK;
    hipLaunchKernelGGL(probe_expf_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)hip_stream, x, n, which, out);
    return check_hip(hipGetLastError(), "probe_expf_kernel");
}

// digests [n_blocks][2] uint64: block first_block + b covers the bit patterns [(first_block + b) << 20, (first_block + b + 1) << 20)
int mnv_hook_probe_expf_digest(uint32_t first_block, uint32_t n_blocks, int which, uint64_t *digests, void *hip_stream) {
    if (!digests || which < 0 || which > 3 || n_blocks > 4096u || first_block > 4096u - n_blocks)
        return set_error(MNV_E_INVALID, "mnv_hook_probe_expf_digest: bad arguments");
    if (n_blocks == 0) return MNV_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int rc = check_hip(hipMemsetAsync(digests, 0, (size_t)n_blocks * 16, stream), "mnv_hook_probe_expf_digest: memset");
    if (rc != MNV_OK) return rc;
    hipLaunchKernelGGL(probe_expf_digest_kernel, dim3(n_blocks * kChunksPerBlock), dim3(kThreads), 0, stream, first_block, n_blocks, which,
                       reinterpret_cast<unsigned long long *>(digests));
    return check_hip(hipGetLastError(), "probe_expf_digest_kernel");
}

// both variants on the n consecutive bit patterns from first_bits (n <= 2^32, wrapping): *count = inputs whose results differ (two NaNs
// are equal), first16[0 .. min(count, 16)) = some of them
int mnv_hook_probe_expf_variants_differ(uint32_t first_bits, uint64_t n, uint64_t *count, uint32_t *first16, void *hip_stream) {
    if (!count || !first16 || n > (1ull << 32)) return set_error(MNV_E_INVALID, "mnv_hook_probe_expf_variants_differ: bad arguments");
    hipStream_t stream = (hipStream_t)hip_stream;
    int rc = check_hip(hipMemsetAsync(count, 0, 8, stream), "mnv_hook_probe_expf_variants_differ: memset");
    if (rc == MNV_OK) rc = check_hip(hipMemsetAsync(first16, 0, 64, stream), "mnv_hook_probe_expf_variants_differ: memset");
    if (rc != MNV_OK || n == 0) return rc;
    hipLaunchKernelGGL(probe_expf_variants_differ_kernel, dim3((unsigned)((n + kChunk - 1) / kChunk)), dim3(kThreads), 0, stream, first_bits, n,
                       reinterpret_cast<unsigned long long *>(count), first16);
    return check_hip(hipGetLastError(), "probe_expf_variants_differ_kernel");
}

int mnv_hook_probe_half(const uint16_t *bits, int64_t n, float *out, void *hip_stream) {
    if (n < 0 || (n > 0 && (!bits || !out))) return set_error(MNV_E_INVALID, "mnv_hook_probe_half: bad arguments");
    if (n == 0) return MNV_OK;
    hipLaunchKernelGGL(probe_half_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)hip_stream, bits, n, out);
    return check_hip(hipGetLastError(), "probe_half_kernel");
}

// mode 0: colour_sigmoid<false> (exact), 1: colour_sigmoid<true> (hardware exp2 / rcp)
int mnv_hook_probe_sigmoid(const float *w, const float *t, int64_t n, int mode, float *out, void *hip_stream) {
    if (n < 0 || (n > 0 && (!w || !t || !out)) || mode < 0 || mode > 1) return set_error(MNV_E_INVALID, "mnv_hook_probe_sigmoid: bad arguments");
    if (n == 0) return MNV_OK;
    hipLaunchKernelGGL(probe_sigmoid_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)hip_stream, w, t, n, mode, out);
    return check_hip(hipGetLastError(), "probe_sigmoid_kernel");
}

int mnv_hook_probe_sh(int basis_dim, const float *dirs, const uint16_t *coefs, int64_t n, float *basis_out, float *channel_out, void *hip_stream) {
    if (n < 0 || (n > 0 && (!dirs || !coefs || !basis_out || !channel_out))) return set_error(MNV_E_INVALID, "mnv_hook_probe_sh: bad arguments");
    if (n == 0) return MNV_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    const dim3 grid(grid_for(n)), block(kThreads);
    switch (basis_dim) {
    case 1: hipLaunchKernelGGL(probe_sh_kernel<1>, grid, block, 0, stream, dirs, coefs, n, basis_out, channel_out); break;
    case 4: hipLaunchKernelGGL(probe_sh_kernel<4>, grid, block, 0, stream, dirs, coefs, n, basis_out, channel_out); break;
    case 9: hipLaunchKernelGGL(probe_sh_kernel<9>, grid, block, 0, stream, dirs, coefs, n, basis_out, channel_out); break;
    case 16: hipLaunchKernelGGL(probe_sh_kernel<16>, grid, block, 0, stream, dirs, coefs, n, basis_out, channel_out); break;
    case 25: hipLaunchKernelGGL(probe_sh_kernel<25>, grid, block, 0, stream, dirs, coefs, n, basis_out, channel_out); break;
    default: return set_error(MNV_E_INVALID, "mnv_hook_probe_sh: basis_dim must be 1, 4, 9, 16 or 25");
    }
    return check_hip(hipGetLastError(), "probe_sh_kernel");
}

// words [n_words] uint32, mult [n_mult] float -> out [2][n_mult][n_words] float: half_mul of the low (out[0]) and the high (out[1]) half
// of every word with every multiplier
int mnv_hook_probe_half_product(const uint32_t *words, int64_t n_words, const float *mult, int64_t n_mult, float *out, void *hip_stream) {
    if (n_words < 0 || n_mult < 0 || n_words > (1 << 24) || n_mult > (1 << 10) || (n_words > 0 && n_mult > 0 && (!words || !mult || !out)))
        return set_error(MNV_E_INVALID, "mnv_hook_probe_half_product: bad arguments");
    if (n_words == 0 || n_mult == 0) return MNV_OK;
    hipLaunchKernelGGL(probe_half_product_kernel, dim3(grid_for(n_words * n_mult)), dim3(kThreads), 0, (hipStream_t)hip_stream, words, n_words, mult,
                       n_mult, out);
    return check_hip(hipGetLastError(), "probe_half_product_kernel");
}

// sh_channel_mix (the march kernels' channel sum on raw row words): basis [n][basis_dim] float, coefs [n][3 * basis_dim] binary16 bits
// -> channel_out [n][3]
int mnv_hook_probe_sh_mix(int basis_dim, const float *basis, const uint16_t *coefs, int64_t n, float *channel_out, void *hip_stream) {
    if (n < 0 || (n > 0 && (!basis || !coefs || !channel_out))) return set_error(MNV_E_INVALID, "mnv_hook_probe_sh_mix: bad arguments");
    if (n == 0) return MNV_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    const dim3 grid(grid_for(n)), block(kThreads);
    switch (basis_dim) {
    case 1: hipLaunchKernelGGL(probe_sh_mix_kernel<1>, grid, block, 0, stream, basis, coefs, n, channel_out); break;
    case 4: hipLaunchKernelGGL(probe_sh_mix_kernel<4>, grid, block, 0, stream, basis, coefs, n, channel_out); break;
    case 9: hipLaunchKernelGGL(probe_sh_mix_kernel<9>, grid, block, 0, stream, basis, coefs, n, channel_out); break;
    case 16: hipLaunchKernelGGL(probe_sh_mix_kernel<16>, grid, block, 0, stream, basis, coefs, n, channel_out); break;
    case 25: hipLaunchKernelGGL(probe_sh_mix_kernel<25>, grid, block, 0, stream, basis, coefs, n, channel_out); break;
    default: return set_error(MNV_E_INVALID, "mnv_hook_probe_sh_mix: basis_dim must be 1, 4, 9, 16 or 25");
    }
    return check_hip(hipGetLastError(), "probe_sh_mix_kernel");
}

// frame: host pointer to a FrameParams; cam: host pointer to a CamBlock, or NULL for frame->cam (the kernels take the camera apart from
// the frame block).  out [n][41] float: dir[3] invdir[3] delta_scale tmin tmax in_bbox(0/1) basis[25] (zero beyond basis_dim) and
// world_ray_dirs' true_dir[3] vdir[3].
int mnv_hook_probe_setup_ray(const void *frame, const void *cam, const int32_t *ix, const int32_t *iy, const float *tmax, int64_t n, int basis_dim,
                             float *out, void *hip_stream) {
    if (!frame || n < 0 || (n > 0 && (!ix || !iy || !tmax || !out))) return set_error(MNV_E_INVALID, "mnv_hook_probe_setup_ray: bad arguments");
    if (n == 0) return MNV_OK;
    mnv::FrameParams P = *static_cast<const mnv::FrameParams *>(frame);
    P.rgba = nullptr;
    P.rgba8 = nullptr;
    P.tmax_px = nullptr;
    P.rgba8_init = nullptr;
    const mnv::CamBlock C = cam ? *static_cast<const mnv::CamBlock *>(cam) : P.cam;
    hipStream_t stream = (hipStream_t)hip_stream;
    const dim3 grid(grid_for(n)), block(kThreads);
    switch (basis_dim) {
    case 1: hipLaunchKernelGGL(probe_setup_ray_kernel<1>, grid, block, 0, stream, P, C, ix, iy, tmax, n, out); break;
    case 4: hipLaunchKernelGGL(probe_setup_ray_kernel<4>, grid, block, 0, stream, P, C, ix, iy, tmax, n, out); break;
    case 9: hipLaunchKernelGGL(probe_setup_ray_kernel<9>, grid, block, 0, stream, P, C, ix, iy, tmax, n, out); break;
    case 16: hipLaunchKernelGGL(probe_setup_ray_kernel<16>, grid, block, 0, stream, P, C, ix, iy, tmax, n, out); break;
    case 25: hipLaunchKernelGGL(probe_setup_ray_kernel<25>, grid, block, 0, stream, P, C, ix, iy, tmax, n, out); break;
    default: return set_error(MNV_E_INVALID, "mnv_hook_probe_setup_ray: basis_dim must be 1, 4, 9, 16 or 25");
    }
    return check_hip(hipGetLastError(), "probe_setup_ray_kernel");
}

// o [n][4] float (16-byte aligned); init_px: [n][4] bytes of the image under the volume, or NULL for the background_brightness branch;
// rgba [n][4] float and / or rgba8 [n][4] bytes
int mnv_hook_probe_composite(const float *o, const uint8_t *init_px, float background, int64_t n, float *rgba, uint8_t *rgba8, void *hip_stream) {
    if (n < 0 || (n > 0 && (!o || (!rgba && !rgba8)))) return set_error(MNV_E_INVALID, "mnv_hook_probe_composite: bad arguments");
    if (((uintptr_t)o & 15u) || ((uintptr_t)rgba & 15u) || ((uintptr_t)rgba8 & 3u) || ((uintptr_t)init_px & 3u))
        return set_error(MNV_E_INVALID, "mnv_hook_probe_composite: misaligned buffer");
    if (n == 0) return MNV_OK;
    mnv::FrameParams P = {};
    P.background_brightness = background;
    P.rgba = rgba;
    P.rgba8 = rgba8;
    P.rgba8_init = init_px;
    hipLaunchKernelGGL(probe_composite_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)hip_stream, P, reinterpret_cast<const float4 *>(o), n);
    return check_hip(hipGetLastError(), "probe_composite_kernel");
}

}  // extern "C"
