// mnv_lod_view.hip -- view-dependent levels of detail: mnv_tree_select_cut decides, for a list of viewpoints, which chunks of a tree are worth
// keeping (the contract of include/mnv.h: a voxel's children stay when the voxel could cover `pixels` pixels from some viewpoint),
// mnv_tree_cut compacts the tree along that set.  With mnv_tree_mip_rows (mnv_lod.hip) in front the result is an ordinary N3Tree that is
// fine near the viewpoints and coarse far away; every march kernel renders it unchanged.
//
// Selection: one top-down, level-synchronous walk over KEPT chunks only, so the cost follows the survivors, not the tree.  Level d holds
// the list of (chunk, integer corner of the voxel above it); a thread per (entry, voxel) computes the voxel's corner at depth d, tests the
// views and, where the voxel refines, marks the child chunk and appends it to the next level's list -- one atomic per wavefront (ballot +
// popcount prefix).  The order inside a level depends on the schedule; it only decides which wavefront handles a chunk, no output byte:
// keep[] receives the constant 1 from whoever arrives, the counts are list sizes.  The view loop is wave-uniform (its index and its exit
// are the same in every lane), so the eye and the threshold of a view come through scalar loads; a lane stops testing at the first view
// that passes and the wavefront leaves the loop when no lane is left.
//
// Cut: the compaction of mnv_tree_walk.h with keep[c] != 0 as the survivor predicate.
//
// Build flags as everywhere: -ffp-contract=off, correctly rounded division; binary32 subnormals are kept (the default of the target).
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "mnv_tree_walk.h"

using mnv::check_hip;
using mnv::set_error;

namespace {

constexpr int kMaxViews = 4096;

// ---------------------------------------------------------------------------------------------------- selection

struct LevelArgs {
    int32_t capacity, depth, always, n_views;  // always: depth < min_depth, every interior voxel refines
    float inv;                                  // 2^-depth
    float sx, sy, sz;                           // the tree's scale
};

// thread t: voxel (t & 7) of list entry t >> 3 (chunk, corner of the voxel above it at depth - 1).  q: [n_views] (q_x, q_y, q_z, unused),
// r2: [n_views][24].  ctr[0]: size of the next level, ctr[1]: fault bits (1 link outside the tree, 2 a chunk reached twice)
__global__ void __launch_bounds__(256) lodv_level_kernel(const int32_t *__restrict__ child, const int4 *__restrict__ front, int64_t n_front, LevelArgs A,
                                                          const float4 *__restrict__ q, const float *__restrict__ r2, int4 *__restrict__ next, int64_t cap_next,
                                                          int32_t *__restrict__ mark, uint8_t *__restrict__ keep, unsigned long long *__restrict__ ctr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t c = 0, ch = 0, ix = 0, iy = 0, iz = 0;
    if (t < n_front * 8) {
        const int4 e = front[t >> 3];
        const int j = (int)(t & 7);
        c = e.x;
        ch = child[(int64_t)c * 8 + j];
        ix = e.y * 2 + (j >> 2), iy = e.z * 2 + ((j >> 1) & 1), iz = e.w * 2 + (j & 1);
    }
    bool refine = ch != 0 && A.always;
    if (!A.always) {
        // the voxel is [lo, hi] per axis, both exact; the gap to the eye per axis, in world units; its square against the view's threshold
        const float lox = (float)ix * A.inv, loy = (float)iy * A.inv, loz = (float)iz * A.inv;
        const float hix = (float)(ix + 1) * A.inv, hiy = (float)(iy + 1) * A.inv, hiz = (float)(iz + 1) * A.inv;
        bool need = ch != 0;
        for (int v = 0; v < A.n_views && __ballot(need) != 0ull; ++v) {
            const float4 e = q[v];
            const float R2 = r2[(size_t)v * 24 + A.depth];
            const float gx = fmaxf(fmaxf(lox - e.x, e.x - hix), 0.f), gy = fmaxf(fmaxf(loy - e.y, e.y - hiy), 0.f), gz = fmaxf(fmaxf(loz - e.z, e.z - hiz), 0.f);
            const float wx = gx / A.sx, wy = gy / A.sy, wz = gz / A.sz;
            const float D2 = (wx * wx + wy * wy) + wz * wz;
            if (need && D2 <= R2) {
                refine = true;
                need = false;
            }
        }
    }
    bool push = false;
    int32_t nid = 0;
    if (refine) {
        const int64_t n = (int64_t)c + ch;
        if (n < 1 || n >= A.capacity) {
            atomicOr(&ctr[1], 1ull);
        } else if (atomicCAS(&mark[n], 0, 1) != 0) {
            atomicOr(&ctr[1], 2ull);
        } else {
            nid = (int32_t)n;
            keep[n] = 1;
            push = true;
        }
    }
    mnv::wave_append(push, &ctr[0], [=](unsigned long long slot) {
        if ((int64_t)slot < cap_next)
            next[slot] = make_int4(nid, ix, iy, iz);
        else
            atomicOr(&ctr[1], 2ull);  // more arrivals than chunks left
    });
}

}  // namespace

extern "C" {

int mnv_tree_select_cut(const mnv_tree_view *tree, const mnv_lod_view *views, int32_t n_views, float pixels, int32_t min_depth, int32_t max_depth, uint8_t *keep_out,
                        int64_t kept_at_depth[24], void *hip_stream) {
    const char *who = "mnv_tree_select_cut";
    int rc;
    if (!views || !keep_out || !kept_at_depth) return set_error(MNV_E_INVALID, std::string(who) + ": null views / output");
    for (int d = 0; d < 24; ++d) kept_at_depth[d] = 0;
    if ((rc = mnv::check_view(tree, who))) return rc;
    if (n_views < 1 || n_views > kMaxViews) return set_error(MNV_E_INVALID, std::string(who) + ": n_views outside [1, 4096]");
    if (!std::isfinite(pixels) || pixels < 0.f) return set_error(MNV_E_INVALID, std::string(who) + ": pixels must be finite and not negative");
    if (min_depth < 1 || max_depth < min_depth) return set_error(MNV_E_INVALID, std::string(who) + ": need 1 <= min_depth <= max_depth");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(tree->scale[k]) || !(tree->scale[k] > 0.f) || !std::isfinite(tree->offset[k]))
            return set_error(MNV_E_INVALID, std::string(who) + ": the tree's scale must be finite and positive, its offset finite");
    // the host half of the contract: q and R2 per view, binary32, one operation at a time
    std::vector<float> table((size_t)n_views * 28);
    float *q = table.data(), *r2 = table.data() + (size_t)n_views * 4;
    for (int v = 0; v < n_views; ++v) {
        const float focal = views[v].focal_px;
        if (!std::isfinite(focal) || !(focal > 0.f)) return set_error(MNV_E_INVALID, std::string(who) + ": focal_px must be finite and positive");
        for (int k = 0; k < 3; ++k) {
            const float eye = views[v].eye[k];
            if (!std::isfinite(eye)) return set_error(MNV_E_INVALID, std::string(who) + ": an eye is not finite");
            const float p = tree->scale[k] * eye;
            q[v * 4 + k] = tree->offset[k] + p;
            if (!std::isfinite(q[v * 4 + k])) return set_error(MNV_E_INVALID, std::string(who) + ": an eye leaves binary32 in tree space");
        }
        q[v * 4 + 3] = 0.f;
        for (int d = 0; d < 24; ++d) {
            float R2 = INFINITY;
            if (pixels != 0.f) {
                const float h = std::ldexp(1.f, -d);
                float e = h / tree->scale[0];
                for (int k = 1; k < 3; ++k) {
                    const float ek = h / tree->scale[k];
                    e = ek > e ? ek : e;
                }
                const float fe = focal * e;
                const float r = fe / pixels;
                R2 = r * r;
            }
            r2[(size_t)v * 24 + d] = R2;
        }
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    const int32_t cap = tree->capacity;
    int dev = -1;
    if ((rc = mnv::current_device(&dev))) return rc;

    // the scratch is kept between calls (grow-only): the call holds the lock until it has waited for the stream
    std::lock_guard<std::mutex> lock(mnv::stream_scratch_mutex());
    mnv::StreamScratch &S = mnv::stream_scratch(dev, stream);
    struct Drain {  // ... also when an error leaves this function early: queued work may still use the scratch and `table`
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{stream};
    if ((rc = check_hip(mnv::grow(S.order, (size_t)cap, (size_t)cap + cap / 4, stream, true), "hipMalloc(level lists)")) ||
        (rc = check_hip(mnv::grow(S.mark, (size_t)cap, (size_t)cap + cap / 4, stream, true), "hipMalloc(chunk marks)")) ||
        (rc = check_hip(mnv::grow(S.views, table.size(), table.size(), stream, true), "hipMalloc(view tables)")))
        return rc;
    if (!S.ctr && (rc = mnv::alloc_pair(S.ctr, 2, "hipMalloc(level counters)", "hipHostMalloc(level counters)"))) return rc;
    int4 *order = S.order.get();
    const float4 *q_dev = reinterpret_cast<const float4 *>(S.views.get());
    const float *r2_dev = S.views.get() + (size_t)n_views * 4;

    const int4 root = make_int4(0, 0, 0, 0);
    const uint8_t one = 1;
    if ((rc = check_hip(hipMemsetAsync(keep_out, 0, (size_t)cap, stream), "clear keep")) ||
        (rc = check_hip(hipMemcpyAsync(keep_out, &one, 1, hipMemcpyHostToDevice, stream), "root keep")) ||
        (rc = check_hip(hipMemsetAsync(S.mark.get(), 0, (size_t)cap * 4, stream), "clear chunk marks")) ||
        (rc = check_hip(hipMemcpyAsync(order, &root, sizeof(root), hipMemcpyHostToDevice, stream), "root entry")) ||
        (rc = check_hip(hipMemcpyAsync(S.views.get(), table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, stream), "view tables")) ||
        (rc = check_hip(hipMemsetAsync(S.ctr.dev.get(), 0, 16, stream), "level counters")))
        return rc;
    mnv::LevelLists L;
    rc = mnv::walk_loop(L, cap, max_depth, S.ctr, who, "lodv_level_kernel", stream, [&](int d, int64_t front, int64_t n_front, int64_t next, int64_t cap_next) {
        const LevelArgs A = {cap, d, d < min_depth ? 1 : 0, n_views, std::ldexp(1.f, -d), tree->scale[0], tree->scale[1], tree->scale[2]};
        hipLaunchKernelGGL(lodv_level_kernel, dim3(mnv::blocks_for(n_front * 8)), dim3(256), 0, stream, tree->child, order + front, n_front, A, q_dev, r2_dev, order + next,
                           cap_next, S.mark.get(), keep_out, S.ctr.dev.get());
    });
    for (int d = 1; d <= L.levels; ++d) kept_at_depth[d] = L.size(d);
    if (rc) return rc;
    return check_hip(hipStreamSynchronize(stream), who);
}

int mnv_tree_cut(const mnv_tree_view *tree, const uint8_t *keep, int32_t new_capacity, int32_t *child_out, uint16_t *data_out, int32_t *parent_out,
                 int16_t *sample_counts_out, void *hip_stream) {
    const char *who = "mnv_tree_cut";
    int rc;
    if (!keep || !child_out || !data_out) return set_error(MNV_E_INVALID, std::string(who) + ": null keep / output");
    if ((rc = mnv::check_view(tree, who))) return rc;
    if (new_capacity < 1 || new_capacity > tree->capacity) return set_error(MNV_E_INVALID, std::string(who) + ": new_capacity outside [1, capacity]");
    if (((uintptr_t)data_out & 15u) != 0) return set_error(MNV_E_INVALID, std::string(who) + ": data_out must be 16-byte aligned");
    if (!mnv::on_device(keep)) return set_error(MNV_E_INVALID, std::string(who) + ": keep must be a device array");
    hipStream_t stream = (hipStream_t)hip_stream;
    int dev = -1;
    if ((rc = mnv::current_device(&dev))) return rc;

    std::lock_guard<std::mutex> lock(mnv::stream_scratch_mutex());
    mnv::StreamScratch &S = mnv::stream_scratch(dev, stream);
    if (!S.ctr && (rc = mnv::alloc_pair(S.ctr, 2, "hipMalloc(level counters)", "hipHostMalloc(level counters)"))) return rc;
    // the root's byte decides whether there is a tree to cut: read it behind what the stream holds (the one wait of this call)
    uint8_t *root_keep = reinterpret_cast<uint8_t *>(S.ctr.host.get());
    if ((rc = check_hip(hipMemcpyAsync(root_keep, keep, 1, hipMemcpyDeviceToHost, stream), "read keep[0]")) ||
        (rc = check_hip(hipStreamSynchronize(stream), "read keep[0]")))
        return rc;
    if (*root_keep == 0) return set_error(MNV_E_INVALID, std::string(who) + ": the root chunk is not kept (keep[0] == 0)");
    return mnv::compact_tree(tree, mnv::ByteKeep{keep}, new_capacity, child_out, data_out, parent_out, sample_counts_out, "cut", S, stream);
}

}  // extern "C"
