// mnv_rays.hip -- the ray generator: world-space origins and directions of a rectangle of a camera's image for the three projections of
// include/mnv.h (mnv_generate_rays: pinhole, orthographic, equirectangular), the input of mnv_render_rays_accel.  The arithmetic is the
// contract stated there: float32, every sum left to right, products and sums rounded separately (the Makefile's -ffp-contract=off and the
// pragma below), correctly rounded division; no sine or cosine on the device -- the equirectangular frame reads the table that
// mnv_equirect_tables (host, binary64 libm) makes.
//
// One ray per lane, rays numbered row-major over the rectangle, 256 per workgroup.  A ray is 12 bytes of each output, so a lane's own store
// would be three dwords at a 12-byte pitch; instead the workgroup's 768 floats per output go through LDS (stride 3 dwords: no two lanes of a
// wavefront meet in a bank) and 192 lanes store one aligned 16-byte vector each.  A workgroup starts at float 768 * b of the output, so
// the vectors are aligned whenever the output is; an output that is not takes the lanes' own stores, and so does the last partial vector.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mnv_internal.h"

#pragma clang fp contract(off)

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kThreads = 256;

struct RayGen {
    float fx, fy, cx, cy;
    float m[12];
    int32_t projection;
    int32_t x0, y0, w, h;
    int32_t image_w;             // EQUIRECT: row y of the table is entry image_w + y
    const float2 *tables;        // EQUIRECT: (sin, cos) of every column's longitude, then of every row's latitude
    float *origins, *dirs;
    int32_t vector_stores;       // both outputs are 16-byte aligned
};

__global__ void __launch_bounds__(kThreads) generate_rays_kernel(const RayGen G) {
    __shared__ __attribute__((aligned(16))) float s_o[kThreads * 3];
    __shared__ __attribute__((aligned(16))) float s_d[kThreads * 3];
    const int64_t n = (int64_t)G.w * G.h;
    const int64_t first = (int64_t)blockIdx.x * kThreads, i = first + threadIdx.x;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (i < n) {
        const int ry = (int)(i / G.w), rx = (int)(i - (int64_t)ry * G.w);
        const int ix = G.x0 + rx, iy = G.y0 + ry;
        const float *m = G.m;
        if (G.projection == MNV_PROJ_EQUIRECT) {
            const float2 lon = G.tables[ix], lat = G.tables[G.image_w + iy];  // (sin, cos)
            const float dx = lat.y * lon.x, dy = lat.x, dz = -(lat.y * lon.y);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[k] = m[9 + k];
                d[k] = m[k] * dx + m[3 + k] * dy + m[6 + k] * dz;
            }
        } else {
            const float u = (ix + 0.5f - G.cx) / G.fx, v = -(iy + 0.5f - G.cy) / G.fy;
            if (G.projection == MNV_PROJ_ORTHO) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o[k] = (m[9 + k] + m[k] * u) + m[3 + k] * v;
                    d[k] = m[6 + k] * -1.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o[k] = m[9 + k];
                    d[k] = m[k] * u + m[3 + k] * v + m[6 + k] * -1.f;
                }
            }
        }
    }
    if (!G.vector_stores) {
        if (i < n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                G.origins[i * 3 + k] = o[k];
                G.dirs[i * 3 + k] = d[k];
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s_o[threadIdx.x * 3 + k] = o[k];
        s_d[threadIdx.x * 3 + k] = d[k];
    }
    __syncthreads();
    const int64_t left = n - first;                                      // rays of this workgroup and behind it
    const int floats = (int)(left < kThreads ? left : kThreads) * 3;     // floats this workgroup writes to each output
    const int t = threadIdx.x;
    if (4 * t + 4 <= floats) {
        reinterpret_cast<float4 *>(G.origins + first * 3)[t] = reinterpret_cast<const float4 *>(s_o)[t];
        reinterpret_cast<float4 *>(G.dirs + first * 3)[t] = reinterpret_cast<const float4 *>(s_d)[t];
    } else {
        for (int f = 4 * t; f < floats; ++f) {
            G.origins[first * 3 + f] = s_o[f];
            G.dirs[first * 3 + f] = s_d[f];
        }
    }
}

}  // namespace

extern "C" {

int mnv_equirect_tables(int32_t width, int32_t height, float *out) {
    if (width < 1 || height < 1 || !out) return set_error(MNV_E_INVALID, "mnv_equirect_tables: need width >= 1, height >= 1 and a table");
    const double pi = 3.14159265358979323846;
    for (int32_t x = 0; x < width; ++x) {
        const double lon = (((double)x + 0.5) / (double)width - 0.5) * (2.0 * pi);
        out[2 * x] = (float)std::sin(lon);
        out[2 * x + 1] = (float)std::cos(lon);
    }
    for (int32_t y = 0; y < height; ++y) {
        const double lat = (0.5 - ((double)y + 0.5) / (double)height) * pi;
        out[2 * ((int64_t)width + y)] = (float)std::sin(lat);
        out[2 * ((int64_t)width + y) + 1] = (float)std::cos(lat);
    }
    return MNV_OK;
}

int mnv_generate_rays(int32_t projection, const mnv_camera *cam, mnv_rect tile, const float *equirect_tables, float *origins_out, float *dirs_out,
                      void *hip_stream) {
    // every argument before any device call
    if (projection != MNV_PROJ_PINHOLE && projection != MNV_PROJ_ORTHO && projection != MNV_PROJ_EQUIRECT)
        return set_error(MNV_E_INVALID, "mnv_generate_rays: unknown projection");
    if (!cam || !origins_out || !dirs_out) return set_error(MNV_E_INVALID, "mnv_generate_rays: null camera or output");
    if (cam->width < 1 || cam->height < 1) return set_error(MNV_E_INVALID, "mnv_generate_rays: the camera has no pixels");
    if (tile.w < 1 || tile.h < 1) return set_error(MNV_E_INVALID, "mnv_generate_rays: the rectangle needs w >= 1 and h >= 1");
    if (tile.x0 < 0 || tile.y0 < 0 || (int64_t)tile.x0 + tile.w > cam->width || (int64_t)tile.y0 + tile.h > cam->height)
        return set_error(MNV_E_INVALID, "mnv_generate_rays: the rectangle leaves the camera's image");
    if ((int64_t)tile.w * (int64_t)tile.h > ((int64_t)1 << 28)) return set_error(MNV_E_INVALID, "mnv_generate_rays: more than 2^28 rays in one call");
    if (projection == MNV_PROJ_EQUIRECT && !equirect_tables)
        return set_error(MNV_E_INVALID, "mnv_generate_rays: the equirectangular projection needs the table of mnv_equirect_tables on the device");
    if ((((uintptr_t)origins_out | (uintptr_t)dirs_out) & 3u) != 0 || ((uintptr_t)equirect_tables & 7u) != 0)
        return set_error(MNV_E_INVALID, "mnv_generate_rays: outputs must be 4-byte aligned, the table 8-byte aligned");
    RayGen G;
    G.fx = cam->fx;
    G.fy = cam->fy;
    G.cx = cam->cx;
    G.cy = cam->cy;
    for (int k = 0; k < 12; ++k) G.m[k] = cam->c2w[k];
    G.projection = projection;
    G.x0 = tile.x0;
    G.y0 = tile.y0;
    G.w = tile.w;
    G.h = tile.h;
    G.image_w = cam->width;
    G.tables = reinterpret_cast<const float2 *>(equirect_tables);
    G.origins = origins_out;
    G.dirs = dirs_out;
    G.vector_stores = (((uintptr_t)origins_out | (uintptr_t)dirs_out) & 15u) == 0 ? 1 : 0;
    const int64_t n = (int64_t)tile.w * tile.h;
    hipLaunchKernelGGL(generate_rays_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)hip_stream, G);
    return check_hip(hipGetLastError(), "generate_rays_kernel");
}

}  // extern "C"
