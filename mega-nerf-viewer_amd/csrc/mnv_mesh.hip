// mnv_mesh.hip -- the mesh pass: what the reference's Mesh::draw (src/mesh.cpp) leaves in the two attachments its march reads with
// offscreen == false, for any list of triangle / line / point meshes, as a visibility-buffer rasteriser.
//
//   setup   one thread per primitive: model matrix, camera transform, edge normals and the conservative screen bound of a triangle -> a
//           96-byte record per primitive (camera-space vertices, edge normals, bound, mesh and face)
//   bins    (primitive, 32 x 32 screen tile) pairs are counted, scanned and listed per tile, as mnv_wireframe.hip does (one wait for the total)
//   tiles   one workgroup per tile: pass 0 resolves the smallest (Z, dist) key of every pixel with 64-bit atomicMin in LDS, pass 1 the
//           lowest draw ordinal among the fragments that carry that key (32-bit atomicMin in LDS); then every pixel shades its winner and
//           both images are written with coalesced stores.  The tile's list is walked 256 primitives at a time, however long it is.  A thread
//           rasterises a line, a point or a triangle whose bound covers at most 16 pixels of the tile by itself; larger triangles go to a
//           queue in LDS and the workgroup walks them together as (triangle, row, 8-pixel span) items, so that a full-frame quad keeps every
//           lane busy.
//
// The arithmetic is the raster contract of include/mnv.h (mnv_render_meshes), float32 in a fixed order under the Makefile's
// -ffp-contract=off; the line steps are csrc/mnv_raster.h, shared with the grid pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "mnv_internal.h"
#include "mnv_raster.h"

using mnv::check_hip;
using mnv::set_error;
using namespace mnv_raster;

struct mnv_mesh {
    mnv::Buffer<float> vert;      // device [n_verts][9]
    mnv::Buffer<uint32_t> faces;  // device [n_prims][face_size] or empty
    int64_t n_verts = 0, n_prims = 0;
    int32_t face_size = 3;
    bool unlit = false, visible = true;
    float M[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

    ~mnv_mesh() {
        if (vert || faces) (void)hipDeviceSynchronize();
    }
};

namespace {

struct MeshDesc {
    const float *vert;
    const uint32_t *faces;
    int64_t first, n_prims;  // draw ordinals [first, first + n_prims)
    float M[12];             // row-major 3 x 4
    int32_t face_size, unlit;
};

// a primitive after setup.  Triangle: V = camera-space vertices, N = the normals of the edges (V1,V2), (V2,V0), (V0,V1), b = the pixels
// that are evaluated.  Line: V[0..5] = the two camera-space endpoints.  Point: V[0..2], b = its pixel.  bx0 >= bx1: dropped.
struct alignas(16) PrimRec {
    float V[9];
    float N[9];
    int32_t bx0, by0, bx1, by1;
    int32_t mesh_kind;  // mesh << 2 | face_size
    int32_t face;
};
static_assert(sizeof(PrimRec) == 96, "PrimRec is six 16-byte words");

struct DrawParams {
    View V;
    float cam_pos[3];
    const MeshDesc *descs;
    int32_t n_meshes;
    int64_t n_prims;
};

__device__ __forceinline__ uint32_t vertex_index(const MeshDesc &D, int64_t face, int i) {
    const int64_t k = face * D.face_size + i;
    return D.faces ? D.faces[k] : (uint32_t)k;
}

// contract: w = ((M0*x + M1*y) + M2*z) + t
__device__ __forceinline__ void model_point(const float *M, const float *p, float w[3]) {
    for (int c = 0; c < 3; ++c) w[c] = ((M[c * 4] * p[0] + M[c * 4 + 1] * p[1]) + M[c * 4 + 2] * p[2]) + M[c * 4 + 3];
}

// contract: the vertex shader's normalize(mat3(M) * aNormal)
__device__ __forceinline__ void model_normal(const float *M, const float *a, float n[3]) {
    float t[3];
    for (int c = 0; c < 3; ++c) t[c] = (M[c * 4] * a[0] + M[c * 4 + 1] * a[1]) + M[c * 4 + 2] * a[2];
    const float len = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int c = 0; c < 3; ++c) n[c] = t[c] / len;
}

// the edge value of the pair (A, B) is d . (A x B): computed with the endpoints in canonical order (the smaller first, comparing X, then Y,
// then Z) and negated for the other direction, so two triangles that share an edge see exactly opposite values
__device__ __forceinline__ bool vertex_less(const float *a, const float *b) {
    if (a[0] != b[0]) return a[0] < b[0];
    if (a[1] != b[1]) return a[1] < b[1];
    return a[2] < b[2];
}

__device__ __forceinline__ void edge_normal(const float *A, const float *B, float n[3]) {
    const bool swap = vertex_less(B, A);
    const float *a = swap ? B : A, *b = swap ? A : B;
    const float nx = a[1] * b[2] - a[2] * b[1], ny = a[2] * b[0] - a[0] * b[2], nz = a[0] * b[1] - a[1] * b[0];
    n[0] = swap ? -nx : nx, n[1] = swap ? -ny : ny, n[2] = swap ? -nz : nz;
}

__global__ void __launch_bounds__(256) mesh_setup_kernel(DrawParams P, PrimRec *__restrict__ recs) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.n_prims) return;
    int m = 0;
    while (m + 1 < P.n_meshes && g >= P.descs[m].first + P.descs[m].n_prims) ++m;
    const MeshDesc &D = P.descs[m];
    const int64_t face = g - D.first;
    const int fs = D.face_size;
    PrimRec R;
    for (int i = 0; i < 9; ++i) R.V[i] = 0.f, R.N[i] = 0.f;
    R.bx0 = R.by0 = R.bx1 = R.by1 = 0;
    R.mesh_kind = (m << 2) | fs;
    R.face = (int32_t)face;
    const View &V = P.V;
    bool behind_all = true, behind_any = false;
    for (int i = 0; i < fs; ++i) {
        const float *p = D.vert + (int64_t)vertex_index(D, face, i) * 9;
        float w[3];
        model_point(D.M, p, w);
        to_camera(V, w, R.V[i * 3], R.V[i * 3 + 1], R.V[i * 3 + 2]);
        const bool behind = R.V[i * 3 + 2] < kNear;
        behind_all = behind_all && behind;
        behind_any = behind_any || behind;
    }
    if (fs == 2) {
        Seg S;
        if (project_segment(R.V[0], R.V[1], R.V[2], R.V[3], R.V[4], R.V[5], V, S)) R.bx1 = R.by1 = 1;
    } else if (fs == 1) {
        if (!behind_all) {
            const float px = V.cx + V.fx * (R.V[0] / R.V[2]), py = V.cy - V.fy * (R.V[1] / R.V[2]);
            const float fx = floorf(px), fy = floorf(py);
            if (fx >= (float)V.x0 && fx < (float)(V.x0 + V.w) && fy >= (float)V.y0 && fy < (float)(V.y0 + V.h)) {  // (false for NaN)
                R.bx0 = (int)fx, R.by0 = (int)fy;
                R.bx1 = R.bx0 + 1, R.by1 = R.by0 + 1;
            }
        }
    } else if (!behind_all) {
        edge_normal(R.V + 3, R.V + 6, R.N);
        edge_normal(R.V + 6, R.V, R.N + 3);
        edge_normal(R.V, R.V + 3, R.N + 6);
        bool whole = behind_any;
        float xlo = 0.f, xhi = 0.f, ylo = 0.f, yhi = 0.f;
        if (!whole) {
            for (int i = 0; i < 3; ++i) {
                const float px = V.cx + V.fx * (R.V[i * 3] / R.V[i * 3 + 2]), py = V.cy - V.fy * (R.V[i * 3 + 1] / R.V[i * 3 + 2]);
                if (!isfinite(px) || !isfinite(py)) whole = true;
                xlo = i ? fminf(xlo, px) : px, xhi = i ? fmaxf(xhi, px) : px;
                ylo = i ? fminf(ylo, py) : py, yhi = i ? fmaxf(yhi, py) : py;
            }
        }
        if (whole) {
            R.bx0 = V.x0, R.by0 = V.y0, R.bx1 = V.x0 + V.w, R.by1 = V.y0 + V.h;
        } else {  // columns floor(min px) - 1 .. floor(max px) + 1, rows alike, cut by the tile
            const float ax0 = (float)(V.x0 - 2), ax1 = (float)(V.x0 + V.w + 2), ay0 = (float)(V.y0 - 2), ay1 = (float)(V.y0 + V.h + 2);
            R.bx0 = max((int)floorf(fminf(fmaxf(xlo, ax0), ax1)) - 1, V.x0);
            R.bx1 = min((int)floorf(fminf(fmaxf(xhi, ax0), ax1)) + 2, V.x0 + V.w);
            R.by0 = max((int)floorf(fminf(fmaxf(ylo, ay0), ay1)) - 1, V.y0);
            R.by1 = min((int)floorf(fminf(fmaxf(yhi, ay0), ay1)) + 2, V.y0 + V.h);
            if (R.by0 >= R.by1) R.bx1 = R.bx0;  // (one test says "dropped")
        }
    }
    recs[g] = R;
}

// f(tile) for every screen tile primitive R may touch
template <typename F>
__device__ __forceinline__ void for_each_prim_tile(const PrimRec &R, const View &V, const TileGrid &G, F f) {
    if (R.bx0 >= R.bx1) return;
    if ((R.mesh_kind & 3) == 2) {
        Seg S;
        if (project_segment(R.V[0], R.V[1], R.V[2], R.V[3], R.V[4], R.V[5], V, S)) for_each_tile(S, V, G, f);
        return;
    }
    const int tx0 = (R.bx0 - V.x0) / kTile, tx1 = (R.bx1 - 1 - V.x0) / kTile, ty0 = (R.by0 - V.y0) / kTile, ty1 = (R.by1 - 1 - V.y0) / kTile;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) f(ty * G.ntx + tx);
}

__global__ void __launch_bounds__(256) mesh_bin_count_kernel(const PrimRec *__restrict__ recs, int64_t n_prims, View V, TileGrid G,
                                                              unsigned *__restrict__ count) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_prims) return;
    for_each_prim_tile(recs[g], V, G, [&](int t) { atomicAdd(&count[t], 1u); });
}

__global__ void __launch_bounds__(256) mesh_bin_fill_kernel(const PrimRec *__restrict__ recs, int64_t n_prims, View V, TileGrid G,
                                                             const unsigned long long *__restrict__ offset, unsigned *__restrict__ cursor,
                                                             uint32_t *__restrict__ list) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_prims) return;
    for_each_prim_tile(recs[g], V, G, [&](int t) { list[offset[t] + atomicAdd(&cursor[t], 1u)] = (uint32_t)g; });
}

// the triangle fragment of pixel (x, y): contract, triangles.  b: the perspective-correct barycentrics
__device__ __forceinline__ bool tri_fragment(const View &V, const PrimRec &R, int x, int y, float b[3], Frag &f) {
    const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;
    const float u = (xc - V.cx) / V.fx, v = (V.cy - yc) / V.fy;
    const float e0 = (R.N[0] * u + R.N[1] * v) + R.N[2];
    const float e1 = (R.N[3] * u + R.N[4] * v) + R.N[5];
    const float e2 = (R.N[6] * u + R.N[7] * v) + R.N[8];
    const float s = (e0 + e1) + e2;
    const bool in = (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f && s > 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f && s < 0.f);
    if (!in) return false;
    b[0] = e0 / s, b[1] = e1 / s, b[2] = e2 / s;
    f.X = (b[0] * R.V[0] + b[1] * R.V[3]) + b[2] * R.V[6];
    f.Y = (b[0] * R.V[1] + b[1] * R.V[4]) + b[2] * R.V[7];
    f.Z = (b[0] * R.V[2] + b[1] * R.V[5]) + b[2] * R.V[8];
    if (!(f.Z >= kNear)) return false;
    f.dist = sqrtf((f.X * f.X + f.Y * f.Y) + f.Z * f.Z);
    return true;
}

// pass 0: the smallest key; pass 1: the lowest ordinal among the fragments with that key
__device__ __forceinline__ void emit(int pass, unsigned long long *keys, uint32_t *owner, int l, unsigned long long key, uint32_t ordinal) {
    if (pass == 0)
        atomicMin(&keys[l], key);
    else if (keys[l] == key)
        atomicMin(&owner[l], ordinal);
}

// contract, colour: the fragment shader of src/mesh.cpp:50-72
__device__ __forceinline__ uint32_t shade(const DrawParams &P, const MeshDesc &D, int64_t face, int nv, const float w[3], const Frag &f) {
    float col[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < nv; ++i) {
        const float *p = D.vert + (int64_t)vertex_index(D, face, i) * 9;
        float n[3] = {0.f, 0.f, 0.f};
        if (!D.unlit) model_normal(D.M, p + 6, n);
        for (int c = 0; c < 3; ++c) {
            col[c] = i ? col[c] + w[i] * p[3 + c] : w[0] * p[3 + c];
            nrm[c] = i ? nrm[c] + w[i] * n[c] : w[0] * n[c];
        }
    }
    float k = 1.f;
    if (!D.unlit) {
        const float L1[3] = {0.4402254521846771f, 0.17609018087387085f, 0.8804509043693542f};
        const float L2[3] = {-0.40824830532073975f, -0.8164966106414795f, -0.40824830532073975f};
        const float d1 = (L1[0] * nrm[0] + L1[1] * nrm[1]) + L1[2] * nrm[2];
        const float d2 = (L2[0] * nrm[0] + L2[1] * nrm[1]) + L2[2] * nrm[2];
        const float diffuse = 0.7f * (d1 > 0.f ? d1 : 0.f), diffuse2 = 0.2f * (d2 > 0.f ? d2 : 0.f);
        // viewDir = normalize(camPos - FragPos.xyz): camPos in world space, FragPos = (X, Y, -Z) in camera space, as the reference mixes them
        const float v0 = P.cam_pos[0] - f.X, v1 = P.cam_pos[1] - f.Y, v2 = P.cam_pos[2] + f.Z;
        const float vl = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        const float w0 = v0 / vl, w1 = v1 / vl, w2 = v2 / vl;
        // reflect(-L1, N) = -L1 - 2 * dot(N, -L1) * N
        const float i0 = -L1[0], i1 = -L1[1], i2 = -L1[2];
        const float dn = (nrm[0] * i0 + nrm[1] * i1) + nrm[2] * i2;
        const float t = 2.f * dn;
        const float r0 = i0 - t * nrm[0], r1 = i1 - t * nrm[1], r2 = i2 - t * nrm[2];
        const float sd = (w0 * r0 + w1 * r1) + w2 * r2;
        float sp = sd > 0.f ? sd : 0.f;
        for (int q = 0; q < 5; ++q) sp = sp * sp;  // pow(., 32)
        const float specular = 0.6f * sp;
        k = ((0.3f + diffuse) + diffuse2) + specular;
    }
    uint32_t word = 0xff000000u;
    for (int c = 0; c < 3; ++c) word |= pack_unit(D.unlit ? col[c] : k * col[c]) << (8 * c);
    return word;
}

__global__ void __launch_bounds__(256) mesh_tile_kernel(DrawParams P, const PrimRec *__restrict__ recs, TileGrid G, unsigned *__restrict__ count,
                                                        const unsigned long long *__restrict__ offset, const uint32_t *__restrict__ list,
                                                        uint32_t background_word, const float *under_tmax, const uint32_t *under_rgba8, int has_under,
                                                        float *tmax_out, uint32_t *rgba8_out) {
    __shared__ unsigned long long keys[kTile * kTile];
    __shared__ uint32_t owner[kTile * kTile];
    __shared__ uint32_t big[256];
    __shared__ unsigned n_big;
    const View &V = P.V;
    const int t = blockIdx.x, tx = t % G.ntx, ty = t / G.ntx, tid = threadIdx.x;
    const int gx0 = V.x0 + tx * kTile, gy0 = V.y0 + ty * kTile;  // the tile: pixels [gx0, gx0 + kTile) x [gy0, gy0 + kTile), cut by the frame
    for (int i = tid; i < kTile * kTile; i += 256) keys[i] = kEmpty, owner[i] = ~0u;
    const unsigned n = count ? count[t] : 0u;
    const unsigned long long base = n ? offset[t] : 0ull;
    __syncthreads();
    if (tid == 0 && count) count[t] = 0;  // ready for the next call on this stream
    for (int pass = 0; pass < 2 && n > 0; ++pass) {
        for (unsigned b0 = 0; b0 < n; b0 += 256) {
            if (tid == 0) n_big = 0;
            __syncthreads();
            const unsigned j = b0 + tid;
            if (j < n) {
                const uint32_t g = list[base + j];
                const PrimRec &R = recs[g];
                const int kind = R.mesh_kind & 3;
                if (kind == 3) {
                    const int x0 = max(R.bx0, gx0), x1 = min(R.bx1, gx0 + kTile), y0 = max(R.by0, gy0), y1 = min(R.by1, gy0 + kTile);
                    if (x0 < x1 && y0 < y1) {
                        if ((x1 - x0) * (y1 - y0) <= 16) {
                            for (int y = y0; y < y1; ++y)
                                for (int x = x0; x < x1; ++x) {
                                    float b[3];
                                    Frag f;
                                    if (tri_fragment(V, R, x, y, b, f)) emit(pass, keys, owner, (y - gy0) * kTile + (x - gx0), make_key(f.Z, f.dist), g);
                                }
                        } else {
                            big[atomicAdd(&n_big, 1u)] = g;
                        }
                    }
                } else if (kind == 2) {
                    Seg S;
                    if (project_segment(R.V[0], R.V[1], R.V[2], R.V[3], R.V[4], R.V[5], V, S))
                        for_each_fragment_in_tile(S, gx0, gy0, [&](int lx, int ly, int u, float vf) {
                            emit(pass, keys, owner, ly * kTile + lx, fragment_key(S, u, vf), g);
                        });
                } else {
                    const int lx = R.bx0 - gx0, ly = R.by0 - gy0;
                    if (lx >= 0 && lx < kTile && ly >= 0 && ly < kTile) {
                        const float dist = sqrtf((R.V[0] * R.V[0] + R.V[1] * R.V[1]) + R.V[2] * R.V[2]);
                        emit(pass, keys, owner, ly * kTile + lx, make_key(R.V[2], dist), g);
                    }
                }
            }
            __syncthreads();
            const unsigned items = n_big * 128u;  // (triangle, row, span of 8 pixels)
            for (unsigned it = tid; it < items; it += 256) {
                const uint32_t g = big[it >> 7];
                const PrimRec &R = recs[g];
                const int y = gy0 + (int)((it >> 2) & 31u), xs = gx0 + (int)(it & 3u) * 8;
                if (y < R.by0 || y >= R.by1) continue;
                const int x0 = max(R.bx0, xs), x1 = min(R.bx1, xs + 8);
                for (int x = x0; x < x1; ++x) {
                    float b[3];
                    Frag f;
                    if (tri_fragment(V, R, x, y, b, f)) emit(pass, keys, owner, (y - gy0) * kTile + (x - gx0), make_key(f.Z, f.dist), g);
                }
            }
            __syncthreads();
        }
    }
    const int wx = min(kTile, V.x0 + V.w - gx0), wy = min(kTile, V.y0 + V.h - gy0);
    for (int i = tid; i < kTile * kTile; i += 256) {
        const int lx = i % kTile, ly = i / kTile;
        if (lx >= wx || ly >= wy) continue;
        const int64_t o = (int64_t)(gy0 - V.y0 + ly) * V.w + (gx0 - V.x0 + lx);
        const unsigned long long key = keys[i];
        float tmax = 1e9f;
        uint32_t word = background_word;
        if (has_under) {
            if (under_tmax) tmax = under_tmax[o];
            if (under_rgba8) word = under_rgba8[o];
        }
        const float dist = __uint_as_float((uint32_t)key);
        const uint32_t g = owner[i];
        if (key != kEmpty && (int64_t)g < P.n_prims && (!has_under || dist < tmax)) {
            const PrimRec &R = recs[g];
            const MeshDesc &D = P.descs[R.mesh_kind >> 2];
            const int kind = R.mesh_kind & 3, x = gx0 + lx, y = gy0 + ly;
            float w[3] = {1.f, 0.f, 0.f};
            Frag f;
            f.X = R.V[0], f.Y = R.V[1], f.Z = R.V[2];
            if (kind == 3) {
                (void)tri_fragment(V, R, x, y, w, f);
            } else if (kind == 2) {
                Seg S;
                (void)project_segment(R.V[0], R.V[1], R.V[2], R.V[3], R.V[4], R.V[5], V, S);
                const int u = S.xm ? x : y;
                (void)fragment_key(S, u, minor_floor(S, u), f);
                w[0] = f.qa / f.s, w[1] = f.qb / f.s;
            }
            tmax = dist;
            word = shade(P, D, R.face, kind, w, f);
        }
        if (tmax_out) tmax_out[o] = tmax;
        if (rgba8_out) rgba8_out[o] = word;
    }
}

// scratch of the pass, one set per (device, HIP stream), left reset by every call (tile counts zero).  mnv_render_meshes holds `mu` from its
// first launch to its last, so calls from several host threads do not interleave their passes.
struct Scratch {
    int device = -1;
    hipStream_t stream = nullptr;
    mnv::Buffer<MeshDesc> descs;
    mnv::Buffer<PrimRec> recs;
    TileBins bins;
};
std::mutex g_mu;
std::vector<Scratch *> g_scratch;  // (heap objects that live as long as the process: never freed, so no hipFree after the runtime is gone)

size_t with_slack(int64_t need) { return (size_t)(need + need / 4 + 64); }

int validate_mesh_arrays(const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_faces, int32_t face_size) {
    if (face_size < 1 || face_size > 3) return set_error(MNV_E_INVALID, "mnv_mesh: face_size must be 1 (points), 2 (lines) or 3 (triangles)");
    if (!vert || n_verts <= 0) return set_error(MNV_E_INVALID, "mnv_mesh: null / empty vertex array");
    if (n_faces < 0 || (!faces && n_faces != 0)) return set_error(MNV_E_INVALID, "mnv_mesh: null index array with a non-zero face count");
    if (!faces && n_verts % face_size != 0) return set_error(MNV_E_INVALID, "mnv_mesh: the vertex count of a non-indexed mesh must be a multiple of face_size");
    if (faces && n_faces == 0) return set_error(MNV_E_INVALID, "mnv_mesh: an index array with no faces");
    if (n_verts > (int64_t)UINT32_MAX) return set_error(MNV_E_INVALID, "mnv_mesh: more vertices than a 32-bit index names");
    if (faces)
        for (int64_t i = 0; i < n_faces * face_size; ++i)
            if ((int64_t)faces[i] >= n_verts) return set_error(MNV_E_INVALID, "mnv_mesh: a face index >= n_verts");
    return MNV_OK;
}

}  // namespace

// A triangle / line / point mesh over device arrays the caller allocated and hands over (mnv_surface_to_mesh): the handle
// owns them from a MNV_OK on, and the caller releases its owners.  The indices are the producer's and are not read back for validation.
int mnv::mesh_adopt_device(float *vert, int64_t n_verts, uint32_t *faces, int64_t n_indices, int32_t face_size, int unlit, mnv_mesh **out) {
    if (!out || !vert || n_verts <= 0 || face_size < 1 || face_size > 3 || (faces ? n_indices <= 0 || n_indices % face_size != 0 : n_indices != 0) ||
        n_verts > (int64_t)UINT32_MAX)
        return set_error(MNV_E_INVALID, "mnv_mesh: bad device arrays");
    mnv_mesh *m = new mnv_mesh();
    m->vert.adopt(vert, (size_t)n_verts * 9);
    m->faces.adopt(faces, (size_t)n_indices);
    m->n_verts = n_verts;
    m->n_prims = faces ? n_indices / face_size : n_verts / face_size;
    m->face_size = face_size;
    m->unlit = unlit != 0;
    *out = m;
    return MNV_OK;
}

extern "C" {

static int upload_mesh(mnv_mesh *m, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size, int unlit) {
    if (face_size >= 1 && face_size <= 3 && n_indices % face_size != 0)
        return set_error(MNV_E_INVALID, "mnv_mesh: the index count must be a multiple of face_size");
    int rc = validate_mesh_arrays(vert, n_verts, faces, face_size >= 1 && face_size <= 3 ? n_indices / face_size : 0, face_size);
    if (rc) return rc;
    int dev = -1;
    if ((rc = mnv::current_device(&dev))) return rc;
    mnv::Buffer<float> dv;
    mnv::Buffer<uint32_t> df;
    if ((rc = check_hip(dv.alloc((size_t)n_verts * 9), "hipMalloc(mesh vertices)")) ||
        (rc = check_hip(hipMemcpy(dv.get(), vert, dv.bytes(), hipMemcpyHostToDevice), "upload mesh vertices")) ||
        (faces && ((rc = check_hip(df.alloc((size_t)n_indices), "hipMalloc(mesh indices)")) ||
                   (rc = check_hip(hipMemcpy(df.get(), faces, df.bytes(), hipMemcpyHostToDevice), "upload mesh indices")))))
        return rc;
    std::lock_guard<std::mutex> lock(g_mu);
    if (m->vert || m->faces) (void)hipDeviceSynchronize();  // (frames that drew the old arrays)
    m->vert = std::move(dv);
    m->faces = std::move(df);
    m->n_verts = n_verts;
    m->n_prims = faces ? n_indices / face_size : n_verts / face_size;
    m->face_size = face_size;
    m->unlit = unlit != 0;
    return MNV_OK;
}

int mnv_mesh_create(const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size, int unlit, mnv_mesh **out) {
    if (!out) return set_error(MNV_E_INVALID, "null output");
    *out = nullptr;
    mnv_mesh *m = new mnv_mesh();
    const int rc = upload_mesh(m, vert, n_verts, faces, n_indices, face_size, unlit);
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return MNV_OK;
}

int mnv_mesh_update(mnv_mesh *m, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int32_t face_size, int unlit) {
    if (!m) return set_error(MNV_E_INVALID, "null mesh");
    return upload_mesh(m, vert, n_verts, faces, n_indices, face_size, unlit);
}

void mnv_mesh_destroy(mnv_mesh *m) { delete m; }

int mnv_mesh_model_matrix(mnv_mesh *m, const float *matrix3x4) {
    if (!m || !matrix3x4) return set_error(MNV_E_INVALID, "null mesh / matrix");
    std::lock_guard<std::mutex> lock(g_mu);
    std::memcpy(m->M, matrix3x4, sizeof(m->M));
    return MNV_OK;
}

int mnv_mesh_show(mnv_mesh *m, int visible) {
    if (!m) return set_error(MNV_E_INVALID, "null mesh");
    std::lock_guard<std::mutex> lock(g_mu);
    m->visible = visible != 0;
    return MNV_OK;
}

int mnv_mesh_visible(const mnv_mesh *m) { return m && m->visible ? 1 : 0; }
int64_t mnv_mesh_vertex_count(const mnv_mesh *m) { return m ? m->n_verts : 0; }
int64_t mnv_mesh_face_count(const mnv_mesh *m) { return m ? m->n_prims : 0; }
int32_t mnv_mesh_face_size(const mnv_mesh *m) { return m ? m->face_size : 0; }

int mnv_render_meshes(const mnv_mesh *const *meshes, int32_t n_meshes, const mnv_camera *cam, const mnv_render_options *opt, mnv_rect tile,
                      const mnv_frame_inputs *under, float *tmax_px_out, uint8_t *rgba8_out, void *hip_stream) {
    if (!cam || !opt) return set_error(MNV_E_INVALID, "null camera / options");
    if (n_meshes < 0 || (n_meshes > 0 && !meshes)) return set_error(MNV_E_INVALID, "null mesh list");
    for (int32_t i = 0; i < n_meshes; ++i)
        if (!meshes[i]) return set_error(MNV_E_INVALID, "null mesh in the list");
    if (cam->width <= 0 || cam->height <= 0) return set_error(MNV_E_INVALID, "camera has no pixels");
    if (tile.w < 0 || tile.h < 0) return set_error(MNV_E_INVALID, "negative tile extent");
    if (((uintptr_t)rgba8_out & 3u) != 0 || (under && ((uintptr_t)under->rgba8_init & 3u) != 0))
        return set_error(MNV_E_INVALID, "rgba8 images must be 4-byte aligned");
    if (n_meshes > (1 << 28)) return set_error(MNV_E_INVALID, "too many meshes");
    int dev = -1;
    if (const int no_device = mnv::current_device(&dev)) return no_device;
    if (!tmax_px_out && !rgba8_out) return MNV_OK;
    const int64_t n_px = (int64_t)tile.w * tile.h;
    if (n_px == 0) return MNV_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    std::lock_guard<std::mutex> lock(g_mu);
    Scratch *S = nullptr;
    for (Scratch *e : g_scratch)
        if (e->device == dev && e->stream == stream) S = e;
    if (!S) {
        S = new Scratch();
        S->device = dev;
        S->stream = stream;
        g_scratch.push_back(S);
    }
    // the draw list: visible meshes in order, their primitives numbered through (the draw ordinal)
    std::vector<MeshDesc> descs;
    int64_t n_prims = 0;
    for (int32_t i = 0; i < n_meshes; ++i) {
        const mnv_mesh *m = meshes[i];
        if (!m->visible || m->n_prims == 0) continue;
        MeshDesc d;
        d.vert = m->vert.get(), d.faces = m->faces.get(), d.first = n_prims, d.n_prims = m->n_prims;
        std::memcpy(d.M, m->M, sizeof(d.M));
        d.face_size = m->face_size, d.unlit = m->unlit ? 1 : 0;
        descs.push_back(d);
        n_prims += m->n_prims;
    }
    if (n_prims >= (int64_t)UINT32_MAX) return set_error(MNV_E_UNSUPPORTED, "mnv_render_meshes: the draw ordinal is 32 bits (fewer than 2^32 - 1 primitives per call)");
    DrawParams P{};
    std::memcpy(P.V.c2w, cam->c2w, sizeof(P.V.c2w));
    P.V.fx = cam->fx, P.V.fy = cam->fy, P.V.cx = cam->cx, P.V.cy = cam->cy;
    P.V.x0 = tile.x0, P.V.y0 = tile.y0, P.V.w = tile.w, P.V.h = tile.h;
    for (int a = 0; a < 3; ++a) P.cam_pos[a] = cam->c2w[9 + a];
    P.n_meshes = (int32_t)descs.size();
    P.n_prims = n_prims;
    // background: floor(clamp(background_brightness, 0, 1) * 255 + 0.5), alpha 255
    const uint32_t c = pack_unit(opt->background_brightness);
    const uint32_t bg = c | (c << 8) | (c << 16) | 0xff000000u;
    const TileGrid G = {(tile.w + kTile - 1) / kTile, (tile.h + kTile - 1) / kTile};
    const int64_t n_tiles = (int64_t)G.ntx * G.nty;
    const float *u_tmax = under ? under->tmax_px : nullptr;
    const uint32_t *u_rgba8 = under ? (const uint32_t *)under->rgba8_init : nullptr;
    int rc;
    if (n_prims == 0) {  // clear (or copy through): the tile kernel with empty lists
        hipLaunchKernelGGL(mesh_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, P, (const PrimRec *)nullptr, G, (unsigned *)nullptr,
                           (const unsigned long long *)nullptr, (const uint32_t *)nullptr, bg, u_tmax, u_rgba8, under ? 1 : 0, tmax_px_out,
                           (uint32_t *)rgba8_out);
        return check_hip(hipGetLastError(), "mesh_tile_kernel");
    }
    // (the stream may still use the old arrays: grow waits for it before they go)
    if ((rc = check_hip(mnv::grow(S->descs, descs.size(), with_slack((int64_t)descs.size()), stream, true), "mesh descriptors")) ||
        (rc = check_hip(mnv::grow(S->recs, (size_t)n_prims, with_slack(n_prims), stream, true), "primitive records")))
        return rc;
    // (`descs` outlives the copy: this call waits for the stream below, for the pair total)
    if ((rc = check_hip(hipMemcpyAsync(S->descs.get(), descs.data(), descs.size() * sizeof(MeshDesc), hipMemcpyHostToDevice, stream), "upload mesh descriptors")))
        return rc;
    P.descs = S->descs.get();
    TileBins &B = S->bins;
    if ((rc = B.ensure(n_tiles, stream, "mesh scratch"))) return rc;
    hipLaunchKernelGGL(mesh_setup_kernel, dim3(mnv::blocks_for(n_prims)), dim3(256), 0, stream, P, S->recs.get());
    hipLaunchKernelGGL(mesh_bin_count_kernel, dim3(mnv::blocks_for(n_prims)), dim3(256), 0, stream, S->recs.get(), n_prims, P.V, G, B.count.get());
    hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(1024), 0, stream, B.count.get(), (int)n_tiles, B.offset.get(), B.cursor.get(), B.total.dev.get());
    if ((rc = check_hip(hipGetLastError(), "mesh setup / count / scan")) ||
        (rc = check_hip(hipMemcpyAsync(B.total.host.get(), B.total.dev.get(), 8, hipMemcpyDeviceToHost, stream), "read pair total")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "mesh setup / count / scan")))
        return rc;
    const int64_t pairs = (int64_t)*B.total.host.get(), list_need = std::max<int64_t>(pairs, 1);
    if ((rc = B.grow_list(list_need, (int64_t)with_slack(list_need), "pair list"))) return rc;
    if (pairs > 0) {
        hipLaunchKernelGGL(mesh_bin_fill_kernel, dim3(mnv::blocks_for(n_prims)), dim3(256), 0, stream, S->recs.get(), n_prims, P.V, G, B.offset.get(), B.cursor.get(), B.list.get());
        if ((rc = check_hip(hipGetLastError(), "mesh_bin_fill_kernel"))) return rc;
    }
    hipLaunchKernelGGL(mesh_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, P, (const PrimRec *)S->recs.get(), G, B.count.get(),
                       (const unsigned long long *)B.offset.get(), (const uint32_t *)B.list.get(), bg, u_tmax, u_rgba8, under ? 1 : 0, tmax_px_out,
                       (uint32_t *)rgba8_out);
    return check_hip(hipGetLastError(), "mesh_tile_kernel");
}

}  // extern "C"
