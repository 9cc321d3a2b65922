// mnv_raster.h -- device code shared by the two rasterisers that write the frame's inputs (mnv_wireframe.hip: the octree grid;
// mnv_mesh.hip: triangle / line / point meshes): steps 1-5 of the raster contract of include/mnv.h (mnv_render_wireframe) for one segment,
// the 32 x 32 screen tiles and the scan of the per-tile pair counts -- and, host side, the tile-bin scratch that both passes keep per stream.  Every float operation is float32 in the order the contract
// states, under the Makefile's -ffp-contract=off.  Included by .hip units only; everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mnv_internal.h"

namespace mnv_raster {

constexpr float kNear = 1e-3f;  // camera.cpp:104 CLIP_NEAR
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kTile = 32;  // kTile x kTile pixels: 8 KiB of keys in LDS

struct View {
    float c2w[12];
    float fx, fy, cx, cy;
    int32_t x0, y0, w, h;  // the tile of the camera image that is drawn
};

struct TileGrid {
    int ntx, nty;
};

// raster contract step 1
__device__ __forceinline__ void to_camera(const View &P, const float p[3], float &X, float &Y, float &z) {
    const float *m = P.c2w;
    const float d0 = p[0] - m[9], d1 = p[1] - m[10], d2 = p[2] - m[11];
    X = (m[0] * d0 + m[1] * d1) + m[2] * d2;
    Y = (m[3] * d0 + m[4] * d1) + m[5] * d2;
    z = -((m[6] * d0 + m[7] * d1) + m[8] * d2);
}

// A segment after steps 2-3 of the contract with its fragment range (step 4): columns (x-major) or rows [s0, s1) of the tile whose centres lie in
// [min, max) of the segment; the other coordinate must fall in [b0, b1).  Every raster method walks fragments through this one form.
struct Seg {
    float pxa, pya, dx, dy, dd, Xa, Ya, za, Xb, Yb, zb;
    float ua, va, du, dv;  // along the major axis / the other one
    int s0, s1, b0, b1;
    bool xm;
};

// steps 2-4 for the camera-space segment (Xa, Ya, za) - (Xb, Yb, zb); false: no fragment
__device__ __forceinline__ bool project_segment(float Xa, float Ya, float za, float Xb, float Yb, float zb, const View &P, Seg &S) {
    // step 2: near clip
    if (za < kNear && zb < kNear) return false;
    if (za < kNear) {
        const float t = (kNear - za) / (zb - za);
        Xa = Xa + t * (Xb - Xa);
        Ya = Ya + t * (Yb - Ya);
        za = kNear;
    } else if (zb < kNear) {
        const float t = (kNear - zb) / (za - zb);
        Xb = Xb + t * (Xa - Xb);
        Yb = Yb + t * (Ya - Yb);
        zb = kNear;
    }
    // step 3: pixel coordinates
    const float pxa = P.cx + P.fx * (Xa / za), pya = P.cy - P.fy * (Ya / za);
    const float pxb = P.cx + P.fx * (Xb / zb), pyb = P.cy - P.fy * (Yb / zb);
    const float dx = pxb - pxa, dy = pyb - pya;
    const float dd = dx * dx + dy * dy;
    if (!(dd > 0.f) || !isfinite(dd)) return false;  // zero-length (or unrepresentable) projection: nothing
    // step 4: one fragment per column (x-major) / row (y-major) whose centre lies in [min, max) of the segment
    const bool xm = fabsf(dx) >= fabsf(dy);
    const float ua = xm ? pxa : pya, ub = xm ? pxb : pyb;
    const int a0 = xm ? P.x0 : P.y0, a1 = a0 + (xm ? P.w : P.h);
    const float lo = fminf(fmaxf(fminf(ua, ub), (float)(a0 - 1)), (float)(a1 + 1)), hi = fminf(fmaxf(fmaxf(ua, ub), (float)(a0 - 1)), (float)(a1 + 1));
    S.s0 = max((int)ceilf(lo - 0.5f), a0);
    S.s1 = min((int)ceilf(hi - 0.5f), a1);
    if (S.s0 >= S.s1) return false;
    S.b0 = xm ? P.y0 : P.x0;
    S.b1 = S.b0 + (xm ? P.h : P.w);
    S.pxa = pxa, S.pya = pya, S.dx = dx, S.dy = dy, S.dd = dd;
    S.Xa = Xa, S.Ya = Ya, S.za = za, S.Xb = Xb, S.Yb = Yb, S.zb = zb;
    S.ua = ua, S.va = xm ? pya : pxa, S.du = xm ? dx : dy, S.dv = xm ? dy : dx;
    S.xm = xm;
    return true;
}

// the floored other coordinate of fragment u (monotone in u: so is every float operation on the way)
__device__ __forceinline__ float minor_floor(const Seg &S, int u) {
    const float uc = (float)u + 0.5f;
    return floorf(S.va + ((uc - S.ua) / S.du) * S.dv);
}

// step 5: window-space parameter of the pixel centre's orthogonal projection, clamped; perspective-correct camera-space point; the key.
// qa / s and qb / s are the perspective-correct weights of the two endpoints.
struct Frag {
    float qa, qb, s, X, Y, Z, dist;
};

__device__ __forceinline__ unsigned long long make_key(float Z, float dist) {
    return ((unsigned long long)__float_as_uint(Z) << 32) | (unsigned long long)__float_as_uint(dist);
}

__device__ __forceinline__ unsigned long long fragment_key(const Seg &S, int u, float vf, Frag &f) {
    const float uc = (float)u + 0.5f, vc = vf + 0.5f;
    const float xc = S.xm ? uc : vc, yc = S.xm ? vc : uc;
    float t = ((xc - S.pxa) * S.dx + (yc - S.pya) * S.dy) / S.dd;
    t = fminf(fmaxf(t, 0.f), 1.f);
    const float qa = (1.f - t) / S.za, qb = t / S.zb, s = qa + qb;
    const float X = (qa * S.Xa + qb * S.Xb) / s, Y = (qa * S.Ya + qb * S.Yb) / s, Z = (qa * S.za + qb * S.zb) / s;
    const float dist = sqrtf((X * X + Y * Y) + Z * Z);
    f.qa = qa, f.qb = qb, f.s = s, f.X = X, f.Y = Y, f.Z = Z, f.dist = dist;
    return make_key(Z, dist);
}

__device__ __forceinline__ unsigned long long fragment_key(const Seg &S, int u, float vf) {
    Frag f;
    return fragment_key(S, u, vf, f);
}

// f(tile) for every tile the fragments of S may land in.  A (segment, tile) pair covers the segment's fragments whose major coordinate
// lies in the tile's span; the tiles of the other axis it reaches come from the floored other coordinate at the span's first and last
// fragment (monotone along the span, so no fragment is missed).
template <typename F>
__device__ __forceinline__ void for_each_tile(const Seg &S, const View &P, const TileGrid &G, F f) {
    const int a0 = S.xm ? P.x0 : P.y0;
    for (int u = S.s0; u < S.s1;) {
        const int k = (u - a0) / kTile;
        const int ue = min(S.s1, a0 + (k + 1) * kTile);
        const float v0 = minor_floor(S, u), v1 = minor_floor(S, ue - 1);
        const float lo = fminf(v0, v1), hi = fmaxf(v0, v1);
        if (hi >= (float)S.b0 && lo < (float)S.b1) {
            const int ilo = lo < (float)S.b0 ? S.b0 : (int)lo, ihi = hi >= (float)S.b1 ? S.b1 - 1 : (int)hi;
            for (int m = (ilo - S.b0) / kTile; m <= (ihi - S.b0) / kTile; ++m) f(S.xm ? m * G.ntx + k : k * G.ntx + m);
        }
        u = ue;
    }
}

// the fragments of S inside the tile whose first pixel is (gx0, gy0): f(local x, local y, u, vf)
template <typename F>
__device__ __forceinline__ void for_each_fragment_in_tile(const Seg &S, int gx0, int gy0, F f) {
    const int ma = S.xm ? gx0 : gy0, mb = S.xm ? gy0 : gx0;  // the tile's first pixel on the major / the other axis
    const int u0 = max(S.s0, ma), u1 = min(S.s1, ma + kTile);
    const float vlo = (float)max(S.b0, mb), vhi = (float)min(S.b1, mb + kTile);
    for (int u = u0; u < u1; ++u) {
        const float vf = minor_floor(S, u);
        if (!(vf >= vlo && vf < vhi)) continue;
        const int v = (int)vf;
        f((S.xm ? u : v) - gx0, (S.xm ? v : u) - gy0, u, vf);
    }
}

// exclusive scan of the per-tile counts (one workgroup of 1024 threads); the total -> *total, the fill cursors cleared
static __global__ void __launch_bounds__(1024) bin_scan_kernel(const unsigned *__restrict__ count, int n, unsigned long long *__restrict__ offset,
                                                               unsigned *__restrict__ cursor, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024, lo = min(n, tid * per), hi = min(n, lo + per);
    unsigned long long s = 0;
    for (int i = lo; i < hi; ++i) s += count[i];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long v = tid >= d ? part[tid - d] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned long long run = part[tid] - s;
    for (int i = lo; i < hi; ++i) {
        offset[i] = run;
        run += count[i];
        cursor[i] = 0;
    }
    if (tid == 1023) *total = part[1023];
}

// step 6's colour word: floor(clamp(c, 0, 1) * 255 + 0.5) (host and device)
__host__ __device__ __forceinline__ uint32_t pack_unit(float c) {
    const float k = fminf(fmaxf(c, 0.f), 1.f);
    return (uint32_t)floorf(k * 255.f + 0.5f);
}

// Host side: the scratch of a binned pass.  Each pass keeps one per stream under its own lock, and every call leaves the counts zero.
struct TileBins {
    mnv::Buffer<unsigned> count, cursor;      // [tiles] each
    mnv::Buffer<unsigned long long> offset;   // [tiles]
    mnv::Mirrored<unsigned long long> total;  // [1] pairs of the call, read back through the pinned word
    mnv::Buffer<uint32_t> list;               // the pair list (grow-only)

    // room for n_tiles tiles (a new set waits for the stream, which may use the old one, and starts with cleared counts) and the pair total
    int ensure(int64_t n_tiles, hipStream_t stream, const char *what) {
        int rc;
        if ((int64_t)count.count() < n_tiles) {
            if ((rc = mnv::check_hip(hipStreamSynchronize(stream), what))) return rc;
            cursor.reset();
            offset.reset();
            if ((rc = mnv::check_hip(count.alloc((size_t)n_tiles), "hipMalloc(tile counts)")) ||
                (rc = mnv::check_hip(cursor.alloc((size_t)n_tiles), "hipMalloc(tile cursors)")) ||
                (rc = mnv::check_hip(offset.alloc((size_t)n_tiles), "hipMalloc(tile offsets)")) ||
                (rc = mnv::check_hip(hipMemsetAsync(count.get(), 0, count.bytes(), stream), "clear tile counts"))) {
                count.reset();  // (the next call starts over)
                return rc;
            }
        }
        if (!total && (rc = mnv::alloc_pair(total, 1, "hipMalloc(pair total)", "hipHostMalloc(pair total)"))) return rc;
        return MNV_OK;
    }
    // room for `need` pairs.  The caller has just waited for the stream to read the pair total, so nothing uses the old list.
    int grow_list(int64_t need, int64_t slack, const char *what) { return mnv::check_hip(mnv::grow(list, (size_t)need, (size_t)slack, nullptr, false), what); }
};

}  // namespace mnv_raster
