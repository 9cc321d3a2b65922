// mnv_resolve.hip -- the reconstruction-filter resolve of anti-aliased frames: n jittered sub-frames (float RGBA, the output of one
// mnv_render_voxels_accel_batch launch) -> one frame, through a weight table of radius 0 .. 2.  The arithmetic is the resolve contract of
// include/mnv.h (mnv_resolve_samples), float32 in a fixed order under the Makefile's -ffp-contract=off and correctly rounded division; the
// sample pattern and the filter tables are host code (host/host_capi.cpp: mnv_aa_pattern, mnv_aa_weights).
//
// One output pixel per lane; the sum over (k, j, i) runs in the contract's order inside the lane, nothing is reduced across lanes.  The
// weight table (at most 64 x 25 floats) is staged once per workgroup in LDS; its reads are wave-uniform (broadcast), and so is the
// branch on w == 0.
//   r == 0  no neighbour is read: every lane streams its own pixel of the n sub-frames (16-byte loads, coalesced), no tile, no halo.
//   r  > 0  a workgroup owns a 32 x 8 pixel tile; per sub-frame the tile with its halo ((32 + 2r) x (8 + 2r) float4, at most 2 per lane)
//           goes global -> registers -> LDS with 16-byte loads and stores, two LDS buffers, one barrier per sub-frame; the loads of
//           sub-frame k + 1 are in flight while sub-frame k is accumulated from LDS.  A wavefront is two tile rows of 32 lanes and a
//           16-byte LDS read is served in four groups of 16 lanes that each lie inside one half of the wavefront, i.e. inside one tile
//           row: the 16 lanes of a group read 16 distinct 16-byte slots of one contiguous 512-byte stretch, which are 16 distinct slots
//           of the 256-byte bank row whatever the row pitch and whatever the window shift i.  So the pitch is 32 + 2r float4, unpadded.
//           The staging stores run over the tile image linearly (lane t -> float4 t): 8 consecutive lanes write 128 contiguous bytes.
#include <hip/hip_runtime.h>

#include "mnv_internal.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;
constexpr int kMaxWeights = MNV_MAX_BATCH * 25;

__device__ __forceinline__ void write_pixel(float4 acc, float wsum, int64_t p, float *__restrict__ rgba_out, uint32_t *__restrict__ rgba8_out) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (wsum > 0.f) o = make_float4(acc.x / wsum, acc.y / wsum, acc.z / wsum, acc.w / wsum);
    if (rgba_out) reinterpret_cast<float4 *>(rgba_out)[p] = o;
    if (rgba8_out) rgba8_out[p] = mnv::pack_u8(o.x) | (mnv::pack_u8(o.y) << 8) | (mnv::pack_u8(o.z) << 16) | (mnv::pack_u8(o.w) << 24);
}

// r == 0: weights[k] is the one weight of sub-frame k
__global__ void __launch_bounds__(kThreads) resolve_point_kernel(const float4 *__restrict__ sub, int n, int64_t n_px, const float *__restrict__ weights,
                                                                 float *__restrict__ rgba_out, uint32_t *__restrict__ rgba8_out) {
    __shared__ float w_lds[MNV_MAX_BATCH];
    for (int t = threadIdx.x; t < n; t += kThreads) w_lds[t] = weights[t];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_px) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float wsum = 0.f;
    const float4 *s = sub + p;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
        const float4 v = s[(int64_t)k * n_px];
        const float w = w_lds[k];
        if (w == 0.f) continue;
        acc.x = acc.x + w * v.x;
        acc.y = acc.y + w * v.y;
        acc.z = acc.z + w * v.z;
        acc.w = acc.w + w * v.w;
        wsum = wsum + w;
    }
    write_pixel(acc, wsum, p, rgba_out, rgba8_out);
}

template <int R>
__global__ void __launch_bounds__(kThreads) resolve_window_kernel(const float4 *__restrict__ sub, int n, int width, int height,
                                                                  const float *__restrict__ weights, float *__restrict__ rgba_out,
                                                                  uint32_t *__restrict__ rgba8_out) {
    constexpr int D = 2 * R + 1, PW = kTileW + 2 * R, PH = kTileH + 2 * R, IMG = PW * PH;  // the tile image with its halo
    constexpr int PER = (IMG + kThreads - 1) / kThreads;                                  // float4 per lane and sub-frame (2)
    __shared__ float4 tile[2][IMG];
    __shared__ float w_lds[kMaxWeights];
    const int tid = threadIdx.x, tx = tid & (kTileW - 1), ty = tid / kTileW;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int64_t n_px = (int64_t)width * height;
    for (int t = tid; t < n * D * D; t += kThreads) w_lds[t] = weights[t];
    // this lane's share of the tile image: LDS slot, and the pixel it comes from (-1: outside the frame, never read back)
    int slot[PER];
    int64_t src[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int t = tid + q * kThreads;
        slot[q] = t < IMG ? t : -1;
        const int gx = x0 - R + t % PW, gy = y0 - R + t / PW;
        src[q] = (t < IMG && gx >= 0 && gx < width && gy >= 0 && gy < height) ? (int64_t)gy * width + gx : -1;
    }
    float4 pre[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) pre[q] = src[q] >= 0 ? sub[src[q]] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int x = x0 + tx, y = y0 + ty;
    // which window terms exist for this pixel (contract: a term outside the frame is skipped)
    bool in_x[D], in_y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        in_x[d] = x + d - R >= 0 && x + d - R < width;
        in_y[d] = y + d - R >= 0 && y + d - R < height;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float wsum = 0.f;
    for (int k = 0; k < n; ++k) {
        float4 *buf = tile[k & 1];
#pragma unroll
        for (int q = 0; q < PER; ++q)
            if (slot[q] >= 0) buf[slot[q]] = pre[q];
        __syncthreads();  // (also: every lane has finished reading this buffer two sub-frames ago, and the weights are in place)
        if (k + 1 < n) {
            const float4 *next = sub + (int64_t)(k + 1) * n_px;
#pragma unroll
            for (int q = 0; q < PER; ++q) pre[q] = src[q] >= 0 ? next[src[q]] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float *wk = w_lds + k * D * D;
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const float w = wk[j * D + i];
                if (w == 0.f) continue;  // wave-uniform
                if (in_x[i] && in_y[j]) {
                    const float4 v = buf[(ty + j) * PW + tx + i];
                    acc.x = acc.x + w * v.x;
                    acc.y = acc.y + w * v.y;
                    acc.z = acc.z + w * v.z;
                    acc.w = acc.w + w * v.w;
                    wsum = wsum + w;
                }
            }
        }
    }
    if (x < width && y < height) write_pixel(acc, wsum, (int64_t)y * width + x, rgba_out, rgba8_out);
}

}  // namespace

extern "C" int mnv_resolve_samples(const float *sub_rgba, int32_t n_samples, int32_t width, int32_t height, const float *weights, int32_t radius,
                                   float *rgba_out, uint8_t *rgba8_out, void *hip_stream) {
    if (!sub_rgba || !weights) return set_error(MNV_E_INVALID, "mnv_resolve_samples: null sub-frames / weights");
    if (!rgba_out && !rgba8_out) return set_error(MNV_E_INVALID, "mnv_resolve_samples: no output");
    if (n_samples < 1 || n_samples > MNV_MAX_BATCH) return set_error(MNV_E_INVALID, "mnv_resolve_samples: need 1 .. MNV_MAX_BATCH samples");
    if (radius < 0 || radius > 2) return set_error(MNV_E_INVALID, "mnv_resolve_samples: radius must be 0 .. 2");
    if (width <= 0 || height <= 0) return set_error(MNV_E_INVALID, "mnv_resolve_samples: the frame has no pixels");
    if (((uintptr_t)rgba8_out & 3u) != 0) return set_error(MNV_E_INVALID, "mnv_resolve_samples: rgba8_out must be 4-byte aligned");
    if (((uintptr_t)sub_rgba & 15u) != 0 || ((uintptr_t)rgba_out & 15u) != 0)
        return set_error(MNV_E_INVALID, "mnv_resolve_samples: sub_rgba and rgba_out must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    const float4 *sub = reinterpret_cast<const float4 *>(sub_rgba);
    uint32_t *out8 = reinterpret_cast<uint32_t *>(rgba8_out);
    if (radius == 0) {
        const int64_t n_px = (int64_t)width * height;
        hipLaunchKernelGGL(resolve_point_kernel, dim3((unsigned)((n_px + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, sub, n_samples, n_px, weights,
                           rgba_out, out8);
        return check_hip(hipGetLastError(), "resolve_point_kernel");
    }
    const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH));
    if (grid.y > 65535u) return set_error(MNV_E_UNSUPPORTED, "mnv_resolve_samples: frames of more than 524280 rows");
    if (radius == 1)
        hipLaunchKernelGGL(resolve_window_kernel<1>, grid, dim3(kThreads), 0, stream, sub, n_samples, width, height, weights, rgba_out, out8);
    else
        hipLaunchKernelGGL(resolve_window_kernel<2>, grid, dim3(kThreads), 0, stream, sub, n_samples, width, height, weights, rgba_out, out8);
    return check_hip(hipGetLastError(), "resolve_window_kernel");
}
