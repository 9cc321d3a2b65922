// mnv_metrics.hip -- frame metrics on the device: the squared error (hence PSNR) and SSIM of a float frame against an RGBA8 target image.
// The arithmetic is the metric contract of include/mnv.h (mnv_frame_metrics), float32 in a fixed order under the Makefile's
// -ffp-contract=off and correctly rounded division.  Every term that leaves a lane is an integer -- llrint(term * 2^32), or a count -- so the
// wavefront reduction, the workgroup reduction and the one 64-bit atomicAdd per workgroup and word give the same sums in any order.
//
//   without MNV_METRIC_SSIM (or a frame with no 11 x 11 window): a streaming pass, one pixel per lane and step, a 16-byte load of the frame
//           and a 4-byte load of the target, no LDS but the 4 x 2 words of the workgroup reduction.
//   with MNV_METRIC_SSIM: a workgroup of 256 lanes owns a 32 x 16 tile of the frame -- its pixels for the squared error, and the window
//           origins that lie on them (origins exist for x' <= width - 11, y' <= height - 11) -- and stages x and t of the 42 x 26 pixels
//           the tile's windows cover (the tile + 10 to the right and below), all three channels, planar: 6 x 1092 floats.  The frame and the
//           target are read once, 1.33 x 1.63 = 2.13 times the tile's own bytes with the halo, mostly from L2 (neighbouring tiles share it).
//           The squared error of an own pixel is taken by the lane that stages it.  Then per channel: the row pass writes the five maps
//           (x, t, x*x, t*t, x*t filtered along x) of 26 rows x 32 origins to LDS, a barrier, the column pass filters them along y (two
//           origins per lane) and forms s, a barrier.  With a mask an integer image of the included pixels goes through the same two
//           passes once (a window is included iff its count is 121).
//           LDS: 6 x 1092 x 4 (staged) + 5 x 832 x 4 (row pass) + 832 x 4 (counts) + 1092 (included) = 47.3 KB, three workgroups
//           (12 wavefronts) per CU.  All three channels' row-pass maps at once would need 76 KB (two workgroups per CU, and more than the
//           64 KB a static allocation may have); one channel at a time costs two more barriers per channel and keeps the inputs read once.
//           Banks: every LDS access is a 4-byte access of 32 consecutive lanes to 32 consecutive words of one row (the row pass: row t / 32,
//           columns t % 32 + i; the column pass: row ty + j, columns tx), conflict-free whatever the pitch, so the planes are unpadded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "mnv_internal.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kTileW = 32, kTileH = 16, kThreads = 256, kWaves = kThreads / 64;
constexpr int kPW = kTileW + kHalo, kPH = kTileH + kHalo, kImg = kPW * kPH;  // the staged image: 42 x 26
constexpr int kRowItems = kPH * kTileW;                                      // row-pass outputs per map: 26 x 32
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;
// Every workgroup ends in one atomicAdd per word on the SAME 40 bytes, and those are served one after the other (about 6 ns each on an
// MI355X: 8100 workgroups of one tile each spent 0.10 ms of a 1080p launch there, in either kernel).  So the grids are bounded and a workgroup
// walks pixels / tiles with the grid's stride: 1024 workgroups (four per CU) stream, 768 (three per CU, what the LDS holds) do SSIM.
constexpr int kStreamGrid = 1024, kSsimGrid = 768;
constexpr int kKnownFlags = MNV_METRIC_QUANTISED | MNV_METRIC_MASK_ALPHA | MNV_METRIC_SSIM;

struct Window {
    float g[kWin];
};

// the contract's x of a frame value
__device__ __forceinline__ float frame_value(float v, bool quantised) {
    if (quantised) return (float)mnv::pack_u8(v) / 255.f;
    return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;
}

// llrint(term * 2^32): the product is exact in double, the rounding is to nearest even
__device__ __forceinline__ long long q32(float term) { return (long long)rint((double)term * 4294967296.0); }

// x, t of the three channels of one pixel, its inclusion and its squared error
struct Pixel {
    float x[3], t[3], se;
    bool included;
};
__device__ __forceinline__ Pixel read_pixel(const float4 *__restrict__ rgba, const uint32_t *__restrict__ target, int64_t p, int flags) {
    const float4 v = rgba[p];
    const uint32_t w = target[p];
    const bool quantised = (flags & MNV_METRIC_QUANTISED) != 0;
    Pixel px;
    px.x[0] = frame_value(v.x, quantised);
    px.x[1] = frame_value(v.y, quantised);
    px.x[2] = frame_value(v.z, quantised);
    px.t[0] = (float)(w & 255u) / 255.f;
    px.t[1] = (float)((w >> 8) & 255u) / 255.f;
    px.t[2] = (float)((w >> 16) & 255u) / 255.f;
    px.included = !(flags & MNV_METRIC_MASK_ALPHA) || (w >> 24) != 0u;
    const float e0 = px.x[0] - px.t[0], e1 = px.x[1] - px.t[1], e2 = px.x[2] - px.t[2];
    px.se = (e0 * e0 + e1 * e1) + e2 * e2;
    return px;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;  // (lane 0 holds the sum)
}

// the workgroup's sums of the first N words of mnv_metric_sums -> one 64-bit atomicAdd per non-zero word; integer additions in every step
template <int N>
__device__ __forceinline__ void add_to_sums(long long (&v)[N], mnv_metric_sums *__restrict__ sums) {
    __shared__ long long part[kWaves][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long s = wave_sum(v[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += part[w][threadIdx.x];
        if (s != 0) atomicAdd(reinterpret_cast<unsigned long long *>(sums) + threadIdx.x, (unsigned long long)s);
    }
}

__global__ void __launch_bounds__(kThreads) metrics_stream_kernel(const float4 *__restrict__ rgba, const uint32_t *__restrict__ target, int64_t n_px,
                                                                  int flags, mnv_metric_sums *__restrict__ sums, float *__restrict__ se_map) {
    long long acc[2] = {0, 0};  // n_px, se_q32
#pragma unroll 4
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n_px; p += (int64_t)gridDim.x * kThreads) {
        const Pixel px = read_pixel(rgba, target, p, flags);
        if (px.included) {
            acc[0] += 1;
            acc[1] += q32(px.se);
        }
        if (se_map) se_map[p] = px.included ? px.se : 0.f;
    }
    add_to_sums(acc, sums);
}

__global__ void __launch_bounds__(kThreads) metrics_ssim_kernel(const float4 *__restrict__ rgba, const uint32_t *__restrict__ target, int width, int height,
                                                                int tiles_x, int n_tiles, int flags, Window win, mnv_metric_sums *__restrict__ sums,
                                                                float *__restrict__ se_map, float *__restrict__ ssim_map) {
    __shared__ float sx[3][kImg], st[3][kImg];  // staged x and t, planar
    __shared__ float hrow[5][kRowItems];        // the row pass of one channel: x, t, x*x, t*t, x*t
    __shared__ int crow[kRowItems];             // the row pass of the included-pixel image
    __shared__ uint8_t inc[kImg];
    const int tid = threadIdx.x;
    const bool masked = (flags & MNV_METRIC_MASK_ALPHA) != 0;
    long long acc[4] = {0, 0, 0, 0};  // n_px, se_q32, n_win, ssim_q32

    // (every LDS array a tile writes was last read before a barrier of the tile before it)
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
        // stage the tile and its halo; the lane that stages an own pixel takes its squared error
        for (int t = tid; t < kImg; t += kThreads) {
            const int lx = t % kPW, ly = t / kPW, gx = x0 + lx, gy = y0 + ly;
            Pixel px;
            px.included = false;
#pragma unroll
            for (int c = 0; c < 3; ++c) px.x[c] = px.t[c] = 0.f;
            if (gx < width && gy < height) {
                const int64_t p = (int64_t)gy * width + gx;
                px = read_pixel(rgba, target, p, flags);
                if (lx < kTileW && ly < kTileH) {
                    if (px.included) {
                        acc[0] += 1;
                        acc[1] += q32(px.se);
                    }
                    if (se_map) se_map[p] = px.included ? px.se : 0.f;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sx[c][t] = px.x[c];
                st[c][t] = px.t[c];
            }
            inc[t] = px.included ? 1 : 0;
        }
        __syncthreads();

        if (x0 > width - kWin || y0 > height - kWin) continue;  // (the whole workgroup) a tile of the right or bottom border without a window origin
        // this lane's two window origins: (tx, ty) and (tx, ty + 8) of the tile
        const int tx = tid & (kTileW - 1), ty = tid / kTileW;
        const int ox = x0 + tx;
        bool valid[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) valid[q] = ox <= width - kWin && y0 + ty + q * (kTileH / 2) <= height - kWin;
        if (masked) {  // (wave-uniform) a window is included iff all of its 121 pixels are
            for (int t = tid; t < kRowItems; t += kThreads) {
                const uint8_t *row = inc + (t / kTileW) * kPW + (t % kTileW);
                int n = 0;
#pragma unroll
                for (int i = 0; i < kWin; ++i) n += row[i];
                crow[t] = n;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int *col = crow + (ty + q * (kTileH / 2)) * kTileW + tx;
                int n = 0;
#pragma unroll
                for (int j = 0; j < kWin; ++j) n += col[j * kTileW];
                valid[q] = valid[q] && n == kWin * kWin;
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (valid[q]) acc[2] += 1;

        for (int c = 0; c < 3; ++c) {
            for (int t = tid; t < kRowItems; t += kThreads) {
                const int at = (t / kTileW) * kPW + (t % kTileW);
                const float *rx = sx[c] + at, *rt = st[c] + at;
                float hx = 0.f, ht = 0.f, hxx = 0.f, htt = 0.f, hxt = 0.f;
#pragma unroll
                for (int i = 0; i < kWin; ++i) {
                    const float g = win.g[i], a = rx[i], b = rt[i];
                    hx = hx + g * a;
                    ht = ht + g * b;
                    hxx = hxx + g * (a * a);
                    htt = htt + g * (b * b);
                    hxt = hxt + g * (a * b);
                }
                hrow[0][t] = hx;
                hrow[1][t] = ht;
                hrow[2][t] = hxx;
                hrow[3][t] = htt;
                hrow[4][t] = hxt;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int oy = ty + q * (kTileH / 2);
                const int at = oy * kTileW + tx;
                float m[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    float a = 0.f;
#pragma unroll
                    for (int j = 0; j < kWin; ++j) a = a + win.g[j] * hrow[k][at + j * kTileW];
                    m[k] = a;
                }
                const float mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
                const float sxx = m[2] - mxx, syy = m[3] - myy, sxy = m[4] - mxy;
                const float num = (2.f * mxy + kC1) * (2.f * sxy + kC2);
                const float den = ((mxx + myy) + kC1) * ((sxx + syy) + kC2);
                const float s = num / den;
                if (valid[q]) acc[3] += q32(s);
                if (ssim_map && ox <= width - kWin && y0 + oy <= height - kWin)
                    ssim_map[((int64_t)(y0 + oy) * (width - kHalo) + ox) * 3 + c] = valid[q] ? s : 0.f;
            }
            __syncthreads();  // (the next channel's row pass overwrites hrow)
        }
    }
    add_to_sums(acc, sums);
}

}  // namespace

extern "C" int mnv_ssim_window(float *out) {
    if (!out) return set_error(MNV_E_INVALID, "mnv_ssim_window: null output");
    double e[kWin], sum = 0.0;
    for (int i = 0; i < kWin; ++i) {
        e[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5);
        sum = sum + e[i];
    }
    for (int i = 0; i < kWin; ++i) out[i] = (float)(e[i] / sum);
    return MNV_OK;
}

extern "C" int mnv_metrics_finish(const mnv_metric_sums *host_copy, mnv_frame_metric_values *out) {
    if (!host_copy || !out) return set_error(MNV_E_INVALID, "mnv_metrics_finish: null argument");
    const double nan = std::nan(""), two32 = 4294967296.0;
    out->n_px = host_copy->n_px;
    out->n_win = host_copy->n_win;
    out->mse = host_copy->n_px > 0 ? (double)host_copy->se_q32 / two32 / (3.0 * (double)host_copy->n_px) : nan;
    out->psnr = host_copy->n_px > 0 ? (out->mse > 0.0 ? -10.0 * std::log10(out->mse) : INFINITY) : nan;
    out->ssim = host_copy->n_win > 0 ? (double)host_copy->ssim_q32 / two32 / (3.0 * (double)host_copy->n_win) : nan;
    return MNV_OK;
}

extern "C" int mnv_frame_metrics(const float *rgba, const uint8_t *target8, int32_t width, int32_t height, int32_t flags, const float *window,
                                 mnv_metric_sums *sums, float *se_map_out, float *ssim_map_out, void *hip_stream) {
    if (!rgba || !target8 || !sums) return set_error(MNV_E_INVALID, "mnv_frame_metrics: null frame / target / sums");
    if (width <= 0 || height <= 0) return set_error(MNV_E_INVALID, "mnv_frame_metrics: the frame has no pixels");
    const int64_t n_px = (int64_t)width * height;
    if (n_px > ((int64_t)1 << 28)) return set_error(MNV_E_INVALID, "mnv_frame_metrics: frames of more than 2^28 pixels");
    if ((flags & ~kKnownFlags) != 0) return set_error(MNV_E_INVALID, "mnv_frame_metrics: unknown flag bits");
    if (((uintptr_t)rgba & 15u) != 0) return set_error(MNV_E_INVALID, "mnv_frame_metrics: rgba must be 16-byte aligned");
    if (((uintptr_t)target8 & 3u) != 0 || ((uintptr_t)se_map_out & 3u) != 0 || ((uintptr_t)ssim_map_out & 3u) != 0)
        return set_error(MNV_E_INVALID, "mnv_frame_metrics: target8 and the maps must be 4-byte aligned");
    if (((uintptr_t)sums & 7u) != 0) return set_error(MNV_E_INVALID, "mnv_frame_metrics: sums must be 8-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    const float4 *frame = reinterpret_cast<const float4 *>(rgba);
    const uint32_t *target = reinterpret_cast<const uint32_t *>(target8);
    const int rc = check_hip(hipMemsetAsync(sums, 0, sizeof(mnv_metric_sums), stream), "mnv_frame_metrics: clear sums");
    if (rc != MNV_OK) return rc;
    if (!(flags & MNV_METRIC_SSIM) || width < kWin || height < kWin) {  // no window: the streaming pass
        const int64_t blocks = (n_px + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(metrics_stream_kernel, dim3((unsigned)std::min<int64_t>(blocks, kStreamGrid)), dim3(kThreads), 0, stream, frame, target, n_px, flags,
                           sums, se_map_out);
        return check_hip(hipGetLastError(), "metrics_stream_kernel");
    }
    Window win;
    if (window) {
        for (int i = 0; i < kWin; ++i) win.g[i] = window[i];
    } else {
        (void)mnv_ssim_window(win.g);
    }
    // (width, height >= 11 and width * height <= 2^28: at most 2^28 / 11 / 16 + 1 tiles per column, fewer than 2^21 tiles in all)
    const int tiles_x = (width + kTileW - 1) / kTileW, n_tiles = tiles_x * ((height + kTileH - 1) / kTileH);
    hipLaunchKernelGGL(metrics_ssim_kernel, dim3((unsigned)std::min(n_tiles, kSsimGrid)), dim3(kThreads), 0, stream, frame, target, width, height, tiles_x,
                       n_tiles, flags, win, sums, se_map_out, ssim_map_out);
    return check_hip(hipGetLastError(), "metrics_ssim_kernel");
}
