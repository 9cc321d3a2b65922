// mnv_wireframe.hip -- the octree grid overlay (RenderOptions::show_grid / grid_max_depth): the edges the reference's
// N3Tree::gen_wireframe emits (n3tree.cpp:249-329), generated on the device, and a line rasteriser that writes the two images the
// reference's GL pass leaves behind for the march (cuda_renderer.cpp:68-90: an RGBA8 image and an R32F "Depth" attachment).
//
// Generation: one top-down, level-synchronous pass over the chunk tree.  Level d holds a frontier of (chunk, integer corner) pairs;
// one thread per (frontier chunk, child) either emits the voxel as a cube (child == 0 || d >= max_depth, as the reference) or pushes
// the child chunk into the next frontier.  Cubes are kept in lattice form (integer corner + level); world corners come from the
// reference's float formula ((float)i / gridsz - offset[a]) / scale[a] where they are needed.  Appends are wave-aggregated (one atomic
// per wavefront).  The host reads two counters per level (the frontier size and a fault flag): a regeneration costs one wait per level.
//
// Raster: one thread per cube edge (12 per cube, in _push_wireframe_bb's order) projects and near-clips its edge and walks its
// fragments, each a 64-bit atomicMin of (bits(z) << 32 | bits(dist)) into a key image; a resolve pass turns the key image into the
// two outputs (with the clear values where no fragment landed) and resets it for the next call.  The key image is scratch owned by
// the wireframe object, one per HIP stream, so frames in flight on different streams do not share one.  The arithmetic is the raster
// contract of include/mnv.h (mnv_render_wireframe), float32 in a fixed order under the Makefile's -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "mnv_raster.h"
#include "mnv_tree_walk.h"

using mnv::check_hip;
using mnv::set_error;
using namespace mnv_raster;

namespace {

constexpr int kMaxLevel = 30;        // lattice corners are uint32: gridsz = 2^(level+1) <= 2^31

// ---------------------------------------------------------------------------------------------------- generation

// one level of the walk: thread t handles child (t & 7) of frontier entry t >> 3
// front / next: (chunk, xi, yi, zi); cubes: (i, j, k, level); ctr[0] next frontier size, ctr[1] cubes so far, ctr[2] fault flag
__global__ void __launch_bounds__(256) wire_level_kernel(const int32_t *__restrict__ child, int32_t capacity, const int4 *__restrict__ front,
                                                          int64_t n_front, int32_t depth, int32_t max_depth, int4 *__restrict__ next,
                                                          int64_t cap_next, uint4 *__restrict__ cubes, int64_t cap_cubes,
                                                          unsigned long long *__restrict__ ctr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool emit = false, push = false;
    int4 f = make_int4(0, 0, 0, 0);
    int32_t nid = 0;
    unsigned gi = 0, gj = 0, gk = 0;
    if (t < n_front * 8) {
        f = front[t >> 3];
        const int c = (int)(t & 7);  // cnt of n3tree.cpp:283-286 for N == 2: i, j, k with k fastest
        gi = (unsigned)f.y * 2u + (unsigned)(c >> 2);
        gj = (unsigned)f.z * 2u + (unsigned)((c >> 1) & 1);
        gk = (unsigned)f.w * 2u + (unsigned)(c & 1);
        const int32_t ch = child[(int64_t)f.x * 8 + c];
        if (ch == 0 || depth >= max_depth) {
            emit = true;
        } else {
            const int64_t n = (int64_t)f.x + ch;
            if (n <= 0 || n >= capacity) {
                atomicOr(&ctr[2], 1ull);  // a link outside the tree: report, do not follow
            } else {
                nid = (int32_t)n;
                push = true;
            }
        }
    }
    mnv::wave_append(emit, &ctr[1], [=](unsigned long long slot) {
        if ((int64_t)slot < cap_cubes)
            cubes[slot] = make_uint4(gi, gj, gk, (unsigned)depth);
        else
            atomicOr(&ctr[2], 2ull);
    });
    mnv::wave_append(push, &ctr[0], [=](unsigned long long slot) {
        if ((int64_t)slot < cap_next)
            next[slot] = make_int4(nid, (int)gi, (int)gj, (int)gk);
        else
            atomicOr(&ctr[2], 2ull);  // more frontier entries than chunks: not a tree
    });
}

// ---------------------------------------------------------------------------------------------------- edges

struct WireTransform {
    float offset[3], scale[3];
};

// corner box of a lattice cube, n3tree.cpp:288-306: ((float)i / gridsz - offset[a]) / scale[a]
__device__ __forceinline__ void cube_box(const uint4 q, const WireTransform &T, float bb[6]) {
    const float g = (float)(1u << (q.w + 1u));
    const unsigned lo[3] = {q.x, q.y, q.z};
    for (int a = 0; a < 3; ++a) {
        bb[a] = ((float)lo[a] / g - T.offset[a]) / T.scale[a];
        bb[3 + a] = ((float)(lo[a] + 1u) / g - T.offset[a]) / T.scale[a];
    }
}

// edge e (0..11) of _push_wireframe_bb (n3tree.cpp:249-273): for i, for j: (0,i,j)-(1,i,j), (i,0,j)-(i,1,j), (i,j,0)-(i,j,1)
__device__ __forceinline__ void cube_edge(const float bb[6], int e, float A[3], float B[3]) {
    const int q = e / 3, r = e - q * 3, i = q >> 1, j = q & 1;
    int a[3], b[3];
    if (r == 0) {
        a[0] = 0, a[1] = i, a[2] = j, b[0] = 1, b[1] = i, b[2] = j;
    } else if (r == 1) {
        a[0] = i, a[1] = 0, a[2] = j, b[0] = i, b[1] = 1, b[2] = j;
    } else {
        a[0] = i, a[1] = j, a[2] = 0, b[0] = i, b[1] = j, b[2] = 1;
    }
    for (int c = 0; c < 3; ++c) {
        A[c] = bb[a[c] * 3 + c];
        B[c] = bb[b[c] * 3 + c];
    }
}

__global__ void __launch_bounds__(256) wire_segments_kernel(const uint4 *__restrict__ cubes, int64_t n_edges, WireTransform T, float *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    float bb[6], A[3], B[3];
    cube_box(cubes[e / 12], T, bb);
    cube_edge(bb, (int)(e % 12), A, B);
    float *o = out + e * 6;
    o[0] = A[0], o[1] = A[1], o[2] = A[2], o[3] = B[0], o[4] = B[1], o[5] = B[2];
}

// ---------------------------------------------------------------------------------------------------- raster

struct RasterParams {
    WireTransform T;
    View V;
};

// steps 1-4 of the raster contract for edge e (csrc/mnv_raster.h has the steps themselves, shared with the mesh pass)
__device__ __forceinline__ bool project_edge(const uint4 *__restrict__ cubes, int64_t e, const RasterParams &P, Seg &S) {
    float bb[6], A[3], B[3];
    cube_box(cubes[e / 12], P.T, bb);
    cube_edge(bb, (int)(e % 12), A, B);
    float Xa, Ya, za, Xb, Yb, zb;
    to_camera(P.V, A, Xa, Ya, za);
    to_camera(P.V, B, Xb, Yb, zb);
    return project_segment(Xa, Ya, za, Xb, Yb, zb, P.V, S);
}

// ---- MNV_WIREFRAME_GLOBAL: thread per edge, every fragment a 64-bit atomicMin into a key image, then a resolve pass

__global__ void __launch_bounds__(256) wire_raster_kernel(const uint4 *__restrict__ cubes, int64_t n_edges, RasterParams P,
                                                           unsigned long long *__restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    Seg S;
    if (!project_edge(cubes, e, P, S)) return;
    for (int u = S.s0; u < S.s1; ++u) {
        const float vf = minor_floor(S, u);
        if (!(vf >= (float)S.b0 && vf < (float)S.b1)) continue;
        const int v = (int)vf;
        const int x = S.xm ? u : v, y = S.xm ? v : u;
        atomicMin(&keys[(int64_t)(y - P.V.y0) * P.V.w + (x - P.V.x0)], fragment_key(S, u, vf));
    }
}

// step 6: outputs (and the key image reset for the next call on this stream)
__global__ void __launch_bounds__(256) wire_resolve_kernel(unsigned long long *__restrict__ keys, int64_t n_px, uint32_t background_word,
                                                            float *__restrict__ tmax_out, uint32_t *__restrict__ rgba8_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    const unsigned long long k = keys[i];
    keys[i] = kEmpty;
    const bool hit = k != kEmpty;
    if (tmax_out) tmax_out[i] = hit ? __uint_as_float((uint32_t)k) : 1e9f;
    if (rgba8_out) rgba8_out[i] = hit ? 0xff000000u : background_word;
}

// ---- MNV_WIREFRAME_BINNED: (edge, screen tile) pairs are counted, scanned and listed per tile; one workgroup per tile resolves its fragments
// with 64-bit atomicMin in LDS and writes both images of the tile with coalesced stores.  A pair covers the edge's fragments whose major
// coordinate lies in the tile's span; the tiles of the other axis it reaches come from the floored other coordinate at the span's first and
// last fragment (monotone along the span, so no fragment is missed).

// MNV_WIREFRAME_AUTO takes the binned method up to this many edges and the global one beyond.  Measured on cfg2 at 1080p:
// 63 k edges binned 0.14 ms / global 0.29 ms, 126 M edges binned 97.6 ms / global 4.4 ms (the binned count and fill passes are bound by
// their 32-bit atomics on a few thousand tile counters); the crossover between the two, interpolated linearly, lies near 200 k edges.
constexpr int64_t kBinnedMaxEdges = int64_t(1) << 18;

__global__ void __launch_bounds__(256) wire_bin_count_kernel(const uint4 *__restrict__ cubes, int64_t n_edges, RasterParams P, TileGrid G,
                                                              unsigned *__restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    Seg S;
    if (!project_edge(cubes, e, P, S)) return;
    for_each_tile(S, P.V, G, [&](int t) { atomicAdd(&count[t], 1u); });
}

__global__ void __launch_bounds__(256) wire_bin_fill_kernel(const uint4 *__restrict__ cubes, int64_t n_edges, RasterParams P, TileGrid G,
                                                             const unsigned long long *__restrict__ offset, unsigned *__restrict__ cursor,
                                                             uint32_t *__restrict__ list) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    Seg S;
    if (!project_edge(cubes, e, P, S)) return;
    for_each_tile(S, P.V, G, [&](int t) { list[offset[t] + atomicAdd(&cursor[t], 1u)] = (uint32_t)e; });
}

__global__ void __launch_bounds__(256) wire_tile_kernel(const uint4 *__restrict__ cubes, RasterParams P, TileGrid G, unsigned *__restrict__ count,
                                                        const unsigned long long *__restrict__ offset, const uint32_t *__restrict__ list,
                                                        uint32_t background_word, float *__restrict__ tmax_out, uint32_t *__restrict__ rgba8_out) {
    __shared__ unsigned long long keys[kTile * kTile];
    const int t = blockIdx.x, tx = t % G.ntx, ty = t / G.ntx;
    const int gx0 = P.V.x0 + tx * kTile, gy0 = P.V.y0 + ty * kTile;  // the tile: pixels [gx0, gx0 + kTile) x [gy0, gy0 + kTile), cut by the frame
    for (int i = threadIdx.x; i < kTile * kTile; i += blockDim.x) keys[i] = kEmpty;
    const unsigned n = count[t];
    const unsigned long long base = offset[t];
    __syncthreads();
    if (threadIdx.x == 0) count[t] = 0;  // ready for the next call on this stream
    for (unsigned j = threadIdx.x; j < n; j += blockDim.x) {
        Seg S;
        if (!project_edge(cubes, (int64_t)list[base + j], P, S)) continue;
        const int ma = S.xm ? gx0 : gy0, mb = S.xm ? gy0 : gx0;  // the tile's first pixel on the major / the other axis
        const int u0 = max(S.s0, ma), u1 = min(S.s1, ma + kTile);
        const float vlo = (float)max(S.b0, mb), vhi = (float)min(S.b1, mb + kTile);
        for (int u = u0; u < u1; ++u) {
            const float vf = minor_floor(S, u);
            if (!(vf >= vlo && vf < vhi)) continue;
            const int v = (int)vf;
            const int lx = (S.xm ? u : v) - gx0, ly = (S.xm ? v : u) - gy0;
            atomicMin(&keys[ly * kTile + lx], fragment_key(S, u, vf));
        }
    }
    __syncthreads();
    const int wx = min(kTile, P.V.x0 + P.V.w - gx0), wy = min(kTile, P.V.y0 + P.V.h - gy0);
    for (int i = threadIdx.x; i < kTile * kTile; i += blockDim.x) {
        const int lx = i % kTile, ly = i / kTile;
        if (lx >= wx || ly >= wy) continue;
        const unsigned long long k = keys[i];
        const bool hit = k != kEmpty;
        const int64_t o = (int64_t)(gy0 - P.V.y0 + ly) * P.V.w + (gx0 - P.V.x0 + lx);
        if (tmax_out) tmax_out[o] = hit ? __uint_as_float((uint32_t)k) : 1e9f;
        if (rgba8_out) rgba8_out[o] = hit ? 0xff000000u : background_word;
    }
}

}  // namespace

struct mnv_wireframe {
    int32_t max_depth = 0;
    WireTransform T{};
    mnv::Buffer<uint4> cubes;
    int64_t n_cubes = 0;
    mnv::Buffer<int4> front[2];
    mnv::Mirrored<unsigned long long> ctr;  // [3]: device counters and their pinned mirror
    int32_t method = MNV_WIREFRAME_AUTO;
    // raster scratch, one set per HIP stream (left reset by every call: key image all ones, tile counts zero).  mnv_render_wireframe holds
    // `mu` from its first launch to its last, so calls from several host threads on one stream do not interleave their passes.
    struct Scratch {
        hipStream_t stream = nullptr;
        mnv::Buffer<unsigned long long> keys;  // MNV_WIREFRAME_GLOBAL: [pixels]
        TileBins bins;                         // MNV_WIREFRAME_BINNED
    };
    mutable std::mutex mu;
    mutable std::vector<Scratch> scratch;

    ~mnv_wireframe() { (void)hipDeviceSynchronize(); }
};

namespace {

size_t with_slack(int64_t need) { return (size_t)(need + need / 4 + 64); }

int generate(mnv_wireframe *w, const mnv_tree_view *tree, int32_t max_depth, hipStream_t stream) {
    if (!tree || (tree->capacity > 0 && !tree->child)) return set_error(MNV_E_INVALID, "mnv_wireframe: null tree view / child array");
    if (tree->capacity > 0 && tree->N != 2) return set_error(MNV_E_UNSUPPORTED, "mnv_wireframe: only N == 2 trees");
    if (tree->capacity < 0) return set_error(MNV_E_INVALID, "mnv_wireframe: negative capacity");
    if (tree->capacity > 0 && !mnv::on_device(tree->child)) return set_error(MNV_E_INVALID, "mnv_wireframe: the tree view must hold device arrays");
    w->max_depth = max_depth;
    for (int a = 0; a < 3; ++a) {
        w->T.offset[a] = tree->offset[a];
        w->T.scale[a] = tree->scale[a];
    }
    w->n_cubes = 0;
    if (tree->capacity == 0) return MNV_OK;
    int rc;
    if (!w->ctr && (rc = mnv::alloc_pair(w->ctr, 3, "hipMalloc(wireframe counters)", "hipHostMalloc"))) return rc;
    unsigned long long *ctr = w->ctr.dev.get(), *ctr_host = w->ctr.host.get();
    if ((rc = check_hip(mnv::grow(w->front[0], 1, with_slack(1), stream, false), "hipMalloc(wireframe)"))) return rc;
    const int4 root = make_int4(0, 0, 0, 0);
    if ((rc = check_hip(hipMemcpyAsync(w->front[0].get(), &root, sizeof(root), hipMemcpyHostToDevice, stream), "wireframe root"))) return rc;
    if ((rc = check_hip(hipMemsetAsync(ctr, 0, 3 * sizeof(unsigned long long), stream), "wireframe counters"))) return rc;
    int64_t n_front = 1;
    int cur = 0;
    for (int depth = 0; n_front > 0; ++depth) {
        if (depth > kMaxLevel) return set_error(MNV_E_UNSUPPORTED, "mnv_wireframe: tree deeper than 31 levels (or a cycle)");
        // a level emits at most 8 cubes per frontier chunk; a tree visits each chunk once, so no frontier exceeds the capacity
        // (the cubes found so far move to the new array; a frontier's contents are not kept)
        const int64_t need_cubes = w->n_cubes + 8 * n_front;
        if ((rc = check_hip(mnv::grow(w->cubes, (size_t)need_cubes, with_slack(need_cubes), stream, false, (size_t)w->n_cubes), "hipMalloc(wireframe)"))) return rc;
        const int64_t cap_next = std::min<int64_t>(8 * n_front, tree->capacity);
        if ((rc = check_hip(mnv::grow(w->front[cur ^ 1], (size_t)cap_next, with_slack(cap_next), stream, false), "hipMalloc(wireframe)"))) return rc;
        if ((rc = check_hip(hipMemsetAsync(ctr, 0, sizeof(unsigned long long), stream), "wireframe counters"))) return rc;
        hipLaunchKernelGGL(wire_level_kernel, dim3(mnv::blocks_for(n_front * 8)), dim3(256), 0, stream, tree->child, tree->capacity, w->front[cur].get(), n_front,
                           depth, max_depth, w->front[cur ^ 1].get(), cap_next, w->cubes.get(), (int64_t)w->cubes.count(), ctr);
        if ((rc = check_hip(hipGetLastError(), "wire_level_kernel"))) return rc;
        if ((rc = check_hip(hipMemcpyAsync(ctr_host, ctr, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "wireframe counters")) ||
            (rc = check_hip(hipStreamSynchronize(stream), "wire_level_kernel")))
            return rc;
        if (ctr_host[2]) {
            w->n_cubes = 0;
            return set_error(MNV_E_INVALID, "mnv_wireframe: a child link leaves the tree (not a valid N3Tree)");
        }
        n_front = (int64_t)ctr_host[0];
        w->n_cubes = (int64_t)ctr_host[1];
        cur ^= 1;
    }
    return MNV_OK;
}

}  // namespace

extern "C" {

int mnv_wireframe_create(const mnv_tree_view *device_tree, int32_t max_depth, void *hip_stream, mnv_wireframe **out) {
    if (!out) return set_error(MNV_E_INVALID, "null output");
    *out = nullptr;
    int dev = -1, rc;
    if ((rc = mnv::current_device(&dev))) return rc;
    mnv_wireframe *w = new mnv_wireframe();
    rc = generate(w, device_tree, max_depth, (hipStream_t)hip_stream);
    if (rc) {
        delete w;
        return rc;
    }
    *out = w;
    return MNV_OK;
}

int mnv_wireframe_update(mnv_wireframe *w, const mnv_tree_view *device_tree, int32_t max_depth, void *hip_stream) {
    if (!w) return set_error(MNV_E_INVALID, "null wireframe");
    return generate(w, device_tree, max_depth, (hipStream_t)hip_stream);
}

void mnv_wireframe_destroy(mnv_wireframe *w) { delete w; }

int mnv_wireframe_segments(const mnv_wireframe *w, float *segments_out, int64_t cap_segments, int64_t *n_segments, void *hip_stream) {
    if (!w) return set_error(MNV_E_INVALID, "null wireframe");
    const int64_t n = w->n_cubes * 12;
    if (n_segments) *n_segments = n;
    if (!segments_out) return cap_segments == 0 ? MNV_OK : set_error(MNV_E_INVALID, "null segment buffer");
    if (cap_segments < n) return set_error(MNV_E_INVALID, "segment buffer too small (n_segments holds the count)");
    if (n == 0) return MNV_OK;
    hipLaunchKernelGGL(wire_segments_kernel, dim3(mnv::blocks_for(n)), dim3(256), 0, (hipStream_t)hip_stream, w->cubes.get(), n, w->T, segments_out);
    return check_hip(hipGetLastError(), "wire_segments_kernel");
}

int mnv_render_wireframe(const mnv_wireframe *w, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile, float *tmax_px_out,
                         uint8_t *rgba8_out, void *hip_stream) {
    if (!w || !cam || !opt) return set_error(MNV_E_INVALID, "null wireframe / camera / options");
    if (cam->width <= 0 || cam->height <= 0) return set_error(MNV_E_INVALID, "camera has no pixels");
    if (tile.w < 0 || tile.h < 0) return set_error(MNV_E_INVALID, "negative tile extent");
    if (((uintptr_t)rgba8_out & 3u) != 0) return set_error(MNV_E_INVALID, "rgba8_out must be 4-byte aligned");
    if (!tmax_px_out && !rgba8_out) return MNV_OK;
    const int64_t n_px = (int64_t)tile.w * tile.h;
    if (n_px == 0) return MNV_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    std::lock_guard<std::mutex> lock(w->mu);
    mnv_wireframe::Scratch *S = nullptr;
    for (auto &e : w->scratch)
        if (e.stream == stream) S = &e;
    if (!S) {
        w->scratch.emplace_back();
        S = &w->scratch.back();
        S->stream = stream;
    }
    RasterParams P{};
    P.T = w->T;
    std::memcpy(P.V.c2w, cam->c2w, sizeof(P.V.c2w));
    P.V.fx = cam->fx, P.V.fy = cam->fy, P.V.cx = cam->cx, P.V.cy = cam->cy;
    P.V.x0 = tile.x0, P.V.y0 = tile.y0, P.V.w = tile.w, P.V.h = tile.h;
    const int64_t n_edges = w->n_cubes * 12;
    // background: floor(clamp(background_brightness, 0, 1) * 255 + 0.5), alpha 255
    const float bb = std::fmin(std::fmax(opt->background_brightness, 0.f), 1.f);
    const uint32_t c = (uint32_t)std::floor(bb * 255.f + 0.5f);
    const uint32_t bg = c | (c << 8) | (c << 16) | 0xff000000u;
    int method = w->method;
    if (method == MNV_WIREFRAME_AUTO) method = n_edges <= kBinnedMaxEdges ? MNV_WIREFRAME_BINNED : MNV_WIREFRAME_GLOBAL;
    if (n_edges > (int64_t)UINT32_MAX) method = MNV_WIREFRAME_GLOBAL;  // the pair list names edges in 32 bits
    int rc;
    if (method == MNV_WIREFRAME_GLOBAL) {
        if ((int64_t)S->keys.count() < n_px) {
            if ((rc = check_hip(hipStreamSynchronize(stream), "wireframe scratch"))) return rc;  // the old image may be in use by this stream
            if ((rc = check_hip(S->keys.alloc((size_t)n_px), "hipMalloc(wireframe key image)"))) return rc;
            if ((rc = check_hip(hipMemsetAsync(S->keys.get(), 0xff, S->keys.bytes(), stream), "clear key image"))) {
                S->keys.reset();  // (every call relies on an image it finds being all ones)
                return rc;
            }
        }
        if (n_edges > 0) {
            hipLaunchKernelGGL(wire_raster_kernel, dim3(mnv::blocks_for(n_edges)), dim3(256), 0, stream, w->cubes.get(), n_edges, P, S->keys.get());
            if ((rc = check_hip(hipGetLastError(), "wire_raster_kernel"))) return rc;
        }
        hipLaunchKernelGGL(wire_resolve_kernel, dim3(mnv::blocks_for(n_px)), dim3(256), 0, stream, S->keys.get(), n_px, bg, tmax_px_out, (uint32_t *)rgba8_out);
        return check_hip(hipGetLastError(), "wire_resolve_kernel");
    }
    const TileGrid G = {(tile.w + kTile - 1) / kTile, (tile.h + kTile - 1) / kTile};
    const int64_t n_tiles = (int64_t)G.ntx * G.nty;
    TileBins &B = S->bins;
    if ((rc = B.ensure(n_tiles, stream, "wireframe scratch"))) return rc;
    if (n_edges > 0) {
        hipLaunchKernelGGL(wire_bin_count_kernel, dim3(mnv::blocks_for(n_edges)), dim3(256), 0, stream, w->cubes.get(), n_edges, P, G, B.count.get());
        hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(1024), 0, stream, B.count.get(), (int)n_tiles, B.offset.get(), B.cursor.get(), B.total.dev.get());
        if ((rc = check_hip(hipGetLastError(), "wire_bin_count / scan")) ||
            (rc = check_hip(hipMemcpyAsync(B.total.host.get(), B.total.dev.get(), 8, hipMemcpyDeviceToHost, stream), "read pair total")) ||
            (rc = check_hip(hipStreamSynchronize(stream), "wire_bin_count / scan")))
            return rc;
        const int64_t pairs = (int64_t)*B.total.host.get();
        if ((rc = B.grow_list(pairs, pairs + pairs / 4 + 1024, "hipMalloc(pair list)"))) return rc;
        if (pairs > 0) {
            hipLaunchKernelGGL(wire_bin_fill_kernel, dim3(mnv::blocks_for(n_edges)), dim3(256), 0, stream, w->cubes.get(), n_edges, P, G, B.offset.get(), B.cursor.get(), B.list.get());
            if ((rc = check_hip(hipGetLastError(), "wire_bin_fill_kernel"))) return rc;
        }
    }
    hipLaunchKernelGGL(wire_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, w->cubes.get(), P, G, B.count.get(), B.offset.get(), B.list.get(), bg, tmax_px_out,
                       (uint32_t *)rgba8_out);
    return check_hip(hipGetLastError(), "wire_tile_kernel");
}

int mnv_wireframe_set_method(mnv_wireframe *w, int32_t method) {
    if (!w) return set_error(MNV_E_INVALID, "null wireframe");
    if (method != MNV_WIREFRAME_AUTO && method != MNV_WIREFRAME_BINNED && method != MNV_WIREFRAME_GLOBAL)
        return set_error(MNV_E_INVALID, "unknown raster method");
    std::lock_guard<std::mutex> lock(w->mu);
    w->method = method;
    return MNV_OK;
}

int64_t mnv_wireframe_cube_count(const mnv_wireframe *w) { return w ? w->n_cubes : 0; }

}  // extern "C"
