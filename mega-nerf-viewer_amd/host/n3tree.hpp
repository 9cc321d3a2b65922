// n3tree.hpp -- viewer::N3Tree, the drop-in tree loader of the reference
// (reference include/n3tree/n3tree.hpp:17-69, src/n3tree/n3tree.cpp:16-246).
//
// Same public surface (open, move_to_device, N, data_dim, data_format, scale, offset,
// data, child, parent, sample_counts, capacity, pack_index, unpack_index); the
// torch::Tensor members of the reference become plain host vectors plus raw HIP
// device buffers -- there is no libtorch in the product.  gen_wireframe (the grid overlay's
// vertex list) is carried on the host arrays; the renderer draws the grid from a device
// edge list instead (mnv_wireframe, include/mnv.h).
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mnv.h"
#include "../csrc/mnv_devmem.h"
#include "data_format.hpp"
#include "mesh.hpp"

namespace viewer {

// An error that carries its C-ABI status code: the extern "C" wrappers return `code` for it (other exceptions become MNV_E_IO).
struct StatusError : std::runtime_error {
    int code;
    StatusError(int c, const std::string &msg) : std::runtime_error(msg), code(c) {}
};

struct N3Tree {
    N3Tree();
    explicit N3Tree(const std::string &path);
    ~N3Tree();
    N3Tree(const N3Tree &) = delete;
    N3Tree &operator=(const N3Tree &) = delete;

    // Open an svox / PlenOctree .npz.  A missing file prints a message and leaves N == 0
    // ("draw nothing"), malformed content throws std::runtime_error -- as n3tree.cpp:16-26,
    // :114,:121,:180,:196,:200.
    void open(const std::string &path);

    // Allocate [max_capacity, ...] device arrays, copy the first `capacity` rows and build
    // the packed accel used by the tuned march kernel (n3tree.cpp:207-246).
    // Throws std::runtime_error on HIP failure.
    void move_to_device(long max_capacity, bool need_parent, bool need_sample_counts, void *hip_stream = nullptr);
    void free_device();
    // Rebuild the packed accel from the current device arrays (after pruning renumbered the chunks).
    void rebuild_accel(void *hip_stream = nullptr);
    // Patch the accel after chunks [old_capacity, capacity) were appended and / or the rows of `changed_nodes`
    // (device (chunk, child) pairs) were rewritten (mnv_accel_refresh).
    void refresh_accel(int old_capacity, const int32_t *changed_nodes, int n_changed, void *hip_stream = nullptr);
    // Copy the first `capacity` chunks of the device arrays back into the host vectors (after refinement).
    void copy_from_device(void *hip_stream = nullptr);

    // Spatial branching factor. Only 2 is supported on the device.
    int N = 0;
    // Halfs per voxel row
    int data_dim = 0;
    DataFormat data_format;
    // Scaling / translation of world coordinates into the unit cube
    std::array<float, 3> scale{{1.f, 1.f, 1.f}};
    std::array<float, 3> offset{{0.f, 0.f, 0.f}};

    int64_t pack_index(int nd, int i, int j, int k);
    std::tuple<int, int, int, int> unpack_index(int64_t packed);

    // Host arrays, reference layout
    std::vector<uint16_t> data;          // [capacity][N^3][data_dim] binary16
    std::vector<int32_t> child;          // [capacity][N^3] relative offsets, 0 = leaf
    std::vector<int32_t> parent;         // [capacity]
    std::vector<int16_t> sample_counts;  // [capacity][N^3], initialised to 8

    // Number of chunks in the tree
    int capacity = 0;

    struct Device {
        mnv::Buffer<uint16_t> data;
        mnv::Buffer<int32_t> child;
        mnv::Buffer<int32_t> parent;          // empty unless asked for
        mnv::Buffer<int16_t> sample_counts;   // empty unless asked for
        long max_capacity = 0;
        mnv_accel *accel = nullptr;
    } device;

    mnv_tree_view host_view() const;
    mnv_tree_view device_view() const;  // pointers are null before move_to_device
    bool on_device() const { return (bool)device.data; }

    // Vertices of the grid overlay (n3tree.cpp:249-329): every voxel with child == 0 || depth >= max_depth as a cube of
    // 12 edges = 24 vertices of 9 floats (position, colour 0,0,0, normal 0,0,1), in the reference's order and float arithmetic.
    // Reads the host arrays (after refinement on the device: copy_from_device first).  A child link outside the tree throws
    // StatusError(MNV_E_INVALID).  gen_wireframe_floats: the length alone (no vertex is built); gen_wireframe_into: the same vertices
    // written to out[0 .. gen_wireframe_floats(max_depth)).
    std::vector<float> gen_wireframe(int max_depth = 100000) const;
    int64_t gen_wireframe_floats(int max_depth = 100000) const;
    void gen_wireframe_into(int max_depth, float *out) const;

    // The iso-surface of the density as a triangle mesh with per-vertex colour and normal (mnv_extract_surface, include/mnv.h: the
    // contract, level 3 .. 10), extracted on the device from the packed accel and downloaded; colour == false leaves the vertices white.
    // Needs move_to_device (StatusError(MNV_E_INVALID) before).  The mesh has no device handle yet: update() uploads it for drawing.
    Mesh extract_surface(int level, float iso, bool colour = true, void *hip_stream = nullptr) const;

    // A level of detail: this tree with every interior row mipped from its children (mnv_tree_mip_rows) and cut at max_depth
    // (mnv_tree_truncate; the root chunk's voxels have depth 1), as a new tree on the device -- parent, sample counts where this tree has
    // them there, the packed accel where this tree has one -- with the same offset / scale / format and its host arrays downloaded
    // (save_npz writes it).  This tree is not changed.  Needs move_to_device (StatusError(MNV_E_INVALID) before); waits for the stream.
    std::unique_ptr<N3Tree> make_lod(int max_depth, void *hip_stream = nullptr) const;
    void make_lod_into(N3Tree &out, int max_depth, void *hip_stream = nullptr) const;  // the same into an existing (empty) tree

    // A view-dependent level of detail: the rows mipped as above, then the tree cut where mnv_tree_select_cut says so for the listed
    // viewpoints (a voxel's children stay when, from some eye, the voxel could cover `pixels` pixels; nothing below min_depth is cut,
    // nothing beyond max_depth is kept) and compacted by mnv_tree_cut.  The result is what make_lod's is: a new tree on the device with
    // this tree's accel / parent / sample counts where it has them, host arrays downloaded.  kept_at_depth: int64 [24] or null.
    std::unique_ptr<N3Tree> make_view_lod(const std::vector<mnv_lod_view> &views, float pixels, int min_depth = 1, int max_depth = 23,
                                          void *hip_stream = nullptr, int64_t *kept_at_depth = nullptr) const;
    void make_view_lod_into(N3Tree &out, const std::vector<mnv_lod_view> &views, float pixels, int min_depth = 1, int max_depth = 23,
                            void *hip_stream = nullptr, int64_t *kept_at_depth = nullptr) const;

    // This tree without what the pinhole frames of `cams` cannot see (include/mnv.h, "culling a tree to a pose set"): wmax cleared, then per
    // camera mnv_generate_rays + mnv_rays_visibility, then mnv_tree_cull at weight_thresh and mnv_tree_cut.  The result is what make_lod's
    // is: a new tree on the device with this tree's accel / parent / sample counts where it has them, host arrays downloaded.  This tree is
    // not changed.  kept_at_depth: int64 [24] or null; counts: or null.  Needs move_to_device; waits for the stream.
    std::unique_ptr<N3Tree> make_culled(const std::vector<mnv_camera> &cams, const mnv_render_options &opt, float weight_thresh, void *hip_stream = nullptr,
                                        int64_t *kept_at_depth = nullptr, mnv_cull_counts *counts = nullptr) const;
    void make_culled_into(N3Tree &out, const std::vector<mnv_camera> &cams, const mnv_render_options &opt, float weight_thresh, void *hip_stream = nullptr,
                          int64_t *kept_at_depth = nullptr, mnv_cull_counts *counts = nullptr) const;

    // Optimise this tree's rows (on the device) against one device float target frame [height][width][4] per camera, full batch:
    // params.iterations times { for every camera mnv_generate_rays + mnv_rays_grad, then one mnv_rows_sgd_step } on a float32 master copy
    // of the rows (include/mnv.h, mnv_n3tree_fit).  The structure does not change.  At the end the accel is rebuilt and the host arrays
    // are refreshed.  Returns the se_q32 of every iteration's rays before its step.  Waits for the stream.
    std::vector<int64_t> fit(const std::vector<mnv_camera> &cams, const std::vector<const float *> &targets, const mnv_render_options &opt,
                             const mnv_fit_params &params, void *hip_stream = nullptr);
    // fit against the frames of `teacher` (on the device with its accel) at the cameras: a level of detail fitted to its full tree.
    std::vector<int64_t> fit_to(const N3Tree &teacher, const std::vector<mnv_camera> &cams, const mnv_render_options &opt, const mnv_fit_params &params,
                                void *hip_stream = nullptr);
    // The same with a choice of row step (SGD, Adam) and of batching (full batch, or ray batches drawn across all cameras by a
    // mnv_ray_batcher; include/mnv.h, mnv_n3tree_fit_ex).  fit / fit_to are these with SGD and full batch.  Returns every step's sums
    // (se_q32 and n_rays among them) before its step.
    std::vector<mnv_fit_sums> fit_ex(const std::vector<mnv_camera> &cams, const std::vector<const float *> &targets, const mnv_render_options &opt,
                                     const mnv_fit_params_ex &params, void *hip_stream = nullptr);
    std::vector<mnv_fit_sums> fit_to_ex(const N3Tree &teacher, const std::vector<mnv_camera> &cams, const mnv_render_options &opt,
                                        const mnv_fit_params_ex &params, void *hip_stream = nullptr);

    // A tree from a coloured point cloud (include/mnv.h, "a tree from a coloured point cloud": mnv_point_tree_create / add / finish /
    // write): occupancy at depth params.depth, the chunks above it, mean colours and one density, as a new tree on the device with parent,
    // sample counts and the packed accel, host arrays downloaded -- what make_lod's result is, so save_npz, make_lod, fit and
    // extract_surface work on it at once.  xyz_dev / rgb_dev: device arrays [n][3].  stats: or null.  Waits for the stream.
    static std::unique_ptr<N3Tree> from_points(const mnv_points_params &params, const float *xyz_dev, const uint8_t *rgb_dev, int64_t n, void *hip_stream = nullptr,
                                               mnv_points_stats *stats = nullptr);
    // The same from host vectors (xyz: 3 floats per point; rgb: 3 bytes per point, or empty for white), uploaded in tiles through repeated add.
    static std::unique_ptr<N3Tree> from_points(const mnv_points_params &params, const std::vector<float> &xyz, const std::vector<uint8_t> &rgb,
                                               void *hip_stream = nullptr, mnv_points_stats *stats = nullptr);
    static void from_points_into(N3Tree &out, const mnv_points_params &params, const float *xyz_dev, const uint8_t *rgb_dev, int64_t n, void *hip_stream = nullptr,
                                 mnv_points_stats *stats = nullptr);
    static void from_points_into(N3Tree &out, const mnv_points_params &params, const std::vector<float> &xyz, const std::vector<uint8_t> &rgb,
                                 void *hip_stream = nullptr, mnv_points_stats *stats = nullptr);

    // This tree with `other` placed into its depth-params.level voxel with corner params.corner (include/mnv.h, "merging two trees":
    // mnv_tree_merge_plan / write): the union of the two structures in canonical breadth-first order, rows by params.mode.  The result is
    // what make_lod's is: a new tree on the device with this tree's offset / scale / format, its accel / parent / sample counts where it
    // has them, host arrays downloaded.  Neither tree is changed; both need move_to_device.  stats: or null.  Waits for the stream.
    std::unique_ptr<N3Tree> merge(const N3Tree &other, const mnv_merge_params &params, void *hip_stream = nullptr, mnv_merge_stats *stats = nullptr) const;
    void merge_into(N3Tree &out, const N3Tree &other, const mnv_merge_params &params, void *hip_stream = nullptr, mnv_merge_stats *stats = nullptr) const;
    // The offset and scale a tile must be built with so that it merges into this tree at level : corner (mnv_tree_voxel_cube).
    void voxel_cube(int level, const std::array<int32_t, 3> &corner, std::array<float, 3> &offset_out, std::array<float, 3> &scale_out) const;

    // Write the tree in the svox .npz layout the loader reads (plain `data` form).
    void save_npz(const std::string &path) const;

    // Adopt arrays (copies); validates sizes like load_npz.
    void assign(const mnv_tree_view &host_view);
    // Same, taking ownership of the vectors (no copy); `meta` supplies N, data_dim, format, scale, offset.
    void adopt(const mnv_tree_view &meta, std::vector<uint16_t> &&data, std::vector<int32_t> &&child,
               std::vector<int32_t> &&parent);

private:
    int N2_ = 0, N3_ = 0;
    void check_sizes();
    // the common end of make_lod_into / make_view_lod_into / make_culled_into: `o` becomes a device tree of new_cap chunks that `cut` fills
    // (child, data, parent, sample counts or null), with host arrays and, where this tree has one, an accel
    void compact_into(N3Tree &o, int64_t new_cap, const std::function<void(int32_t *, uint16_t *, int32_t *, int16_t *)> &cut, void *hip_stream) const;
    // the common end of the two from_points_into: finish, the device arrays, write, host arrays, accel
    static void finish_points_into(N3Tree &o, const mnv_points_params &params, mnv_point_tree *handle, void *hip_stream, mnv_points_stats *stats);
};

}  // namespace viewer
