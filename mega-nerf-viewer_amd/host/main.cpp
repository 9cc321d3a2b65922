// mnv_render -- offline batch renderer: the reference's `nerf-viewer` command line without the window.
//
// Flag names and defaults follow the reference (src/opts.cpp:17-32 common flags, main.cpp:491-505
// viewer flags).  --grid D draws the octree grid down to depth D over the volume, as the reference's --grid (src/opts.cpp:53-55):
// the edges of N3Tree::gen_wireframe(D) in black on background_brightness, the march stopping at them (VolumeRenderer, options.show_grid);
// --bounds_only --grid 0 shows the scene bounds as the root cube cut in eight.  --model_path names a model container
// (an .npz, see VolumeRenderer::load_model) and enables the refinement flags, which the reference exposes as
// window check boxes (main.cpp:270-300) rather than flags:
//   --use_splitting          grow / resample / prune the tree from the per-ray trackers while rendering
//   --use_guided_sampling    composite per-sample network outputs instead of the tree's colours
//   --max_depth D  --max_sample_count C  --seed S
//   --save_tree FILE.npz     write the refined tree after the last frame
// Added for batch use:
//   --out PREFIX     write PREFIX_%04d.ppm (RGB from the RGBA8 output) per frame
//   --raw            also write PREFIX_%04d.f32 (float RGBA, row-major, little endian)
//   --frames N       render N frames; with --orbit DEG the camera is rotated about --origin around
//                    --world_up by DEG degrees per frame (default 0: N identical frames, for timing)
//   --gpu ID         HIP device
//   --gpus N         one process per GPU (forked before any HIP call), devices --gpu .. --gpu + N - 1: the tree is replicated, every
//                    frame is cut into interleaved 64x24 macro tiles (mnv_partition), each rank renders its tiles of up to 64
//                    frames with one launch, the compact buffers are gathered to rank 0 over RCCL (mnv_gather_tiles) and
//                    un-permuted there (mnv_assemble_tiles); rank 0 writes the frames.  --gpus 1 runs the same path with one
//                    rank.  --reserve_cus R (default 32 when N > 1) keeps R compute units free for the RCCL kernels.
//                    With --model_path + --use_guided_sampling every rank runs the fused guided-sampling kernel on its tiles
//                    (mnv_render_guided_fused_part: the networks read the tree only).  With --use_splitting the ranks refine the
//                    scene in lock step, one frame at a time (VolumeRenderer::set_ranks: tracker rows and visit marks are
//                    all-gathered, every rank applies the same tree edits to its replica).
//   --in_flight K    plain frames in flight (default 3; VolumeRenderer::frames_in_flight): frame k is downloaded and written
//                    after frames k+1 .. k+K-1 have been issued
//   --guided_in_flight   guided-sampling frames without splitting rotate over the slots as well (VolumeRenderer::guided_in_flight); their
//                    sample counts are printed when the frame is written
//   --aa K           anti-aliased frames (default 1: off): K jittered sub-frames per frame in one launch, resolved on the device
//                    (VolumeRenderer::aa_samples; 1 .. 64).  --aa_filter box|tent (default tent) names the reconstruction filter: the mean
//                    of a pixel's own samples, or a tent of one pixel radius over the samples of the 3x3 pixels around it.
//                    Refused with --gpus: that path gathers RGBA8 tiles, and resolving across ranks would need the float sub-frames
//                    of every rank on the wire -- out of scope.  Refused (by the renderer) while refining or sampling through a model.
//   --projection pinhole|ortho|equirect   (default pinhole) an orthographic frame (--fx / --fy: pixels per world unit; the camera plane
//                    belongs outside the volume; with --render_depth a height map) or a 360-degree equirectangular panorama from the
//                    camera's centre (VolumeRenderer::projection: rays from mnv_generate_rays, marched by mnv_render_rays_accel).
//                    Refused with --gpus, --grid, --mesh and --aa other than 1: those passes draw through a pinhole camera.
//   --mesh PATH[,unlit]   draw a Wavefront OBJ file under the volume (viewer::Mesh::load_obj, VolumeRenderer::meshes); repeatable.
//                    --mesh_color r,g,b (vertices without a colour; default white), --mesh_translate x,y,z, --mesh_rotate x,y,z
//                    (axis-angle) and --mesh_scale s apply to the mesh named before them.  Refused with --gpus, as --grid is.
//   --extract_mesh OUT.obj   write the iso-surface of the density as a Wavefront OBJ file with a colour and a normal per vertex
//                    (N3Tree::extract_surface, mnv_extract_surface: --extract_level L, default 7, the lattice has 2^L samples per axis;
//                    --extract_iso S, default 10, the density the surface follows).  Frames rendered by the same run draw the mesh under
//                    the volume like --mesh (--extract_unlit: with its vertex colours alone); --frames 0 writes the file only.  Refused
//                    with --gpus and a projection other than pinhole, as --mesh is.
//   --lod D          the frames march the tree truncated at depth D (the root chunk's voxels have depth 1), every interior row mipped
//                    from its children first (VolumeRenderer::set_lod, N3Tree::make_lod: mnv_tree_mip_rows + mnv_tree_truncate).
//                    --save_lod OUT.npz writes that tree.  Refused with --gpus, --use_splitting and --use_guided_sampling.
//   --lod_pixels P   the frames march a view-dependent cut of the tree (VolumeRenderer::set_view_lod, N3Tree::make_view_lod:
//                    mnv_tree_mip_rows + mnv_tree_select_cut + mnv_tree_cut): a voxel's children stay where the voxel could cover P pixels
//                    from the eye of one of the poses this run renders (the --frames / --orbit loop is stepped on a copy of the camera
//                    first; focal length max(fx, fy)); nothing is cut above depth --lod_min (default 1), nothing kept below --lod_max
//                    (default 23).  Prints the kept chunks per depth; --save_lod OUT.npz writes the tree.  Refused with --lod, --gpus,
//                    --use_splitting and --use_guided_sampling.
//   --cull W         the frames march the tree without what the poses of this run cannot see (VolumeRenderer::set_cull,
//                    N3Tree::make_culled: leaves no ray of those frames weights above W are emptied, chunks left all-empty collapse);
//                    the poses are the --frames / --orbit loop stepped on a copy of the camera, as --lod_pixels does.  Prints the chunks
//                    per depth before and after and the counts; --save_lod OUT.npz writes the tree.  Refused with --lod, --lod_pixels,
//                    --lod_fit, --gpus, --use_splitting and --use_guided_sampling.
//   --lod_fit ITERS  with --lod or --lod_pixels: fit the level of detail to the full tree before it is marched or written
//                    (VolumeRenderer::set_lod_fit, N3Tree::fit_to: mnv_rays_grad + mnv_rows_sgd_step, ITERS full-batch gradient steps) at
//                    the poses of this run -- the --frames / --orbit loop stepped on a copy of the camera, as --lod_pixels does -- and print
//                    the PSNR of the fitted rays before every step.  --fit_lr_colour X / --fit_lr_sigma Y: the learning rates (defaults
//                    1 and 20: the rates at which the numpy restatement's loss falls at every step on the test suite's fit scene, where
//                    a leaf of the cut covers a few pixels of a frame; the gradient of a row is a SUM over the rays through its voxel,
//                    so larger frames want smaller rates).  At most 2^24 pixels over the poses.
//                    --fit_optimizer sgd|adam: the row step (mnv_rows_sgd_step; mnv_rows_adam_step, whose step does not depend on the
//                    gradient's scale: rates 0.03 and 1 unless given, beta 0.9 / 0.999, eps 1e-8).  --fit_batch RAYS: every step takes
//                    RAYS rays drawn across all poses (mnv_ray_batcher, N3Tree::fit_to_ex) in units of --fit_tile 1|8 pixels squared, in
//                    the order --fit_seed S gives; the 2^24 bound does not apply then.  Defaults sgd / 0 (full batch) / 8 / 0.
//                    --fit_seed takes all 64 bits (decimal, or hexadecimal with 0x).
//   --fit_images PREFIX --fit_steps N [--fit_holdout K]   fit the tree this run is about to march -- the input tree (.npz, --points, --merge)
//                    or its --lod / --lod_pixels cut -- to photographs: frame f of the --frames / --orbit loop has the target
//                    PREFIX_%04d.ppm (the P6 files --out writes; channel = byte / 255, alpha 1), N steps of N3Tree::fit_ex with the
//                    --fit_* flags above (sgd, full batch unless given).  Poses with f % K == K - 1 are held out.  Prints the mean PSNR
//                    (mnv_frame_metrics, quantised) of the fitted and of the held-out poses before and after; --save_lod OUT.npz writes
//                    the fitted tree; the frames then show it.  Refused with --lod_fit, --cull, --gpus, --use_splitting,
//                    --use_guided_sampling.
//   --merge B.npz    place the tree of B.npz into the input tree before anything else is done with it (N3Tree::merge: mnv_tree_merge_plan /
//                    write): the union of the two structures in canonical breadth-first order.  --merge_at k:x,y,z after it names the
//                    voxel of the base tree that is B's cube (depth k, integer corner); without it k and the corner are derived from the
//                    two trees' offsets and scales, which must match mnv_tree_voxel_cube bit for bit (no tolerance: otherwise the run
//                    fails and names --merge_at).  --merge_mode over|add after it (default over): where B holds density its row / where
//                    both do the density-weighted blend.  Repeatable: the merges fold left to right.  With --points the cloud's tree is
//                    the base.  The merge happens before --lod, --lod_pixels, --cull and --lod_fit; --save_lod OUT.npz writes the merged
//                    tree (the level of detail of it when one of those is given too).  Refused with --gpus and --use_splitting.
//   --points FILE    build the tree from a coloured point cloud in place of opening one (N3Tree::from_points: mnv_point_tree_create / add /
//                    finish / write).  FILE is an .npz holding `points` (float32 [n][3]) and optionally `colors` (uint8 [n][3], default
//                    255), or an .obj whose `v x y z [r g b]` lines are the points (float colours become (int)(c * 255 + 0.5), clamped).
//                    --points_depth D (default 8) the leaf voxels' depth, --points_sigma S (default 100) their density, --points_min N
//                    (default 1) the points a voxel needs, --points_format RGBA|SH1|SH4|SH9|SH16|SH25 (default RGBA) the rows,
//                    --points_cube ox,oy,oz,sx,sy,sz the world -> unit cube map (default: the smallest cube around the cloud's finite
//                    points, widened by 2^-12 of its edge).  Prints the stats with the chunks per depth: the depth at which the counts
//                    stop growing eightfold is where the cloud stops filling voxels.  --save_lod OUT.npz writes the tree (the level of
//                    detail of it when --lod, --lod_pixels or --cull is given too).  Refused with an input tree and with --gpus.
//   --target PREFIX  score frame f against PREFIX_%04d.ppm (the P6 files --out writes) on the device (VolumeRenderer::set_target,
//                    mnv_frame_metrics with MNV_METRIC_QUANTISED: the file --out would write against the file that was read) and print
//                    "frame F: psnr ..." when the frame is collected, then the means over the frames.  --ssim adds SSIM (11 x 11 Gaussian
//                    window, valid windows only).  --target_mask PREFIX reads PREFIX_%04d.pgm (P5) per frame: pixels whose mask byte is 0
//                    are excluded (Mega-NeRF's per-image masks).  Files of another size than the frame are refused.  Refused with --gpus.
//                    Out of scope: pose lists (the camera poses stay --orbit or the API) and LPIPS (it needs a network this repository
//                    does not have).
#include <hip/hip_runtime_api.h>

#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <csignal>
#include <deque>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "mesh.hpp"
#include "npz.hpp"
#include "volume_renderer.hpp"

namespace {

struct Args {
    std::map<std::string, std::string> kv;
    std::string file;
    std::vector<std::pair<std::string, std::string>> mesh_flags;  // --mesh and the --mesh_* flags after it, in command-line order
    std::vector<std::pair<std::string, std::string>> merge_flags;  // --merge and the --merge_at / --merge_mode after it, in command-line order
    bool has(const std::string &k) const { return kv.count(k) != 0; }
    std::string get(const std::string &k, const std::string &d) const { return has(k) ? kv.at(k) : d; }
    float f(const std::string &k, float d) const { return has(k) ? std::strtof(kv.at(k).c_str(), nullptr) : d; }
    long l(const std::string &k, long d) const { return has(k) ? std::strtol(kv.at(k).c_str(), nullptr, 10) : d; }
    std::vector<float> vec(const std::string &k, std::vector<float> d) const {
        if (!has(k)) return d;
        std::vector<float> out;
        const std::string s = kv.at(k);
        size_t i = 0;
        while (i < s.size()) {
            size_t j = s.find(',', i);
            if (j == std::string::npos) j = s.size();
            out.push_back(std::strtof(s.substr(i, j - i).c_str(), nullptr));
            i = j + 1;
        }
        return out;
    }
};

Args parse(int argc, char **argv) {
    static const std::map<std::string, std::string> shorts = {
        {"s", "step_size"}, {"e", "stop_thresh"}, {"a", "sigma_thresh"}, {"c", "max_tree_capacity"}, {"x", "split_batch_size"},
        {"n", "nerf_batch_size"}, {"v", "samples_per_voxel"}, {"b", "bounds_only"}, {"y", "appearance_embedding"},
        {"z", "max_guided_samples"}, {"w", "width"}, {"h", "height"}};
    static const char *flags[] = {"bounds_only", "raw", "help", "use_splitting", "use_guided_sampling", "guided_in_flight", "ssim", "extract_unlit"};
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string t = argv[i];
        if (t.size() > 1 && t[0] == '-' && !(t[1] >= '0' && t[1] <= '9') && t[1] != '.') {
            std::string name = t.substr(t[1] == '-' ? 2 : 1), val;
            const size_t eq = name.find('=');
            bool has_val = false;
            if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
            if (shorts.count(name)) name = shorts.at(name);
            bool is_flag = false;
            for (const char *f : flags) is_flag |= name == f;
            if (!has_val && !is_flag) {
                if (i + 1 >= argc) throw std::runtime_error("missing value for --" + name);
                val = argv[++i];
            }
            a.kv[name] = is_flag && !has_val ? "1" : val;
            if (name.rfind("mesh", 0) == 0) a.mesh_flags.emplace_back(name, val);
            if (name == "merge" || name == "merge_at" || name == "merge_mode") a.merge_flags.emplace_back(name, val);
        } else {
            a.file = t;
        }
    }
    if (a.has("file")) a.file = a.kv["file"];
    return a;
}

void usage() {
    std::puts("usage: mnv_render npz_file [--bg 0.0] [-s step_size] [-e stop_thresh] [-a sigma_thresh] [-c max_tree_capacity]\n"
              "                  [-w width] [-h height] [--fx 1111] [--fy -1] [--cx -1] [--cy -1] [--center x,y,z] [--back x,y,z]\n"
              "                  [--origin x,y,z] [--world_up x,y,z] [-b] [--grid D] [--out PREFIX] [--raw] [--frames N] [--orbit DEG] [--gpu ID]\n"
              "                  [--in_flight K] [--guided_in_flight] [--aa K [--aa_filter box|tent]] [--projection pinhole|ortho|equirect] [--gpus N [--reserve_cus R] [--root_period M]]\n"
              "                  [--mesh FILE.obj[,unlit] [--mesh_color r,g,b] [--mesh_translate x,y,z] [--mesh_rotate x,y,z] [--mesh_scale s]]...\n"
              "                  [--extract_mesh OUT.obj [--extract_level L] [--extract_iso S] [--extract_unlit]]   the density's iso-surface as a mesh\n"
              "                  [--lod D [--save_lod OUT.npz]]   march (and write) the tree truncated at depth D, interior rows mipped from their children\n"
              "                  [--lod_pixels P [--lod_min D] [--lod_max D] [--save_lod OUT.npz]]   march (and write) the tree cut where a voxel covers\n"
              "                   less than P pixels from every pose of this run\n"
              "                  [--cull W [--save_lod OUT.npz]]   march (and write) the tree without what this run's poses cannot see (weights <= W)\n"
              "                  [--lod_fit ITERS [--fit_lr_colour X] [--fit_lr_sigma Y]]   with --lod / --lod_pixels: fit that tree's rows to the full\n"
              "                   tree's frames at the poses of this run first (ITERS gradient steps)\n"
              "                  [--fit_optimizer sgd|adam] [--fit_batch RAYS] [--fit_tile 1|8] [--fit_seed S]   with --lod_fit: the row step (adam: rates\n"
              "                                     0.03 / 1 unless given) and ray batches drawn over all poses in pixel or 8 x 8 tile units (0: full batch)\n"
              "                  [--fit_images PREFIX --fit_steps N [--fit_holdout K] [--save_lod OUT.npz]]   fit the tree this run marches (the input, --points,\n"
              "                                     --merge, --lod or --lod_pixels tree) to PREFIX_%04d.ppm of this run's poses (the files --out writes) in N steps\n"
              "                                     with the --fit_* flags above; poses f % K == K - 1 are held out; prints the PSNR before and after\n"
              "                  [--merge B.npz [--merge_at k:x,y,z] [--merge_mode over|add]]... [--save_lod OUT.npz]   place B's tree into a voxel of the\n"
              "                   input tree (default: the voxel its offset and scale name exactly); repeatable, folds left to right\n"
              "                  [--points FILE.npz|FILE.obj [--points_depth D] [--points_sigma S] [--points_min N] [--points_format RGBA|SH9...]\n"
              "                   [--points_cube ox,oy,oz,sx,sy,sz] [--save_lod OUT.npz]]   build the tree from a coloured point cloud (no npz_file then)\n"
              "                  [--target PREFIX [--target_mask PREFIX] [--ssim]]   score frame f against PREFIX_%04d.ppm (mask: PREFIX_%04d.pgm,\n"
              "                   0 = excluded): PSNR and, with --ssim, SSIM per frame and their means; not with --gpus.  Out of scope: pose\n"
              "                   lists (poses stay --orbit or the API) and LPIPS (it needs a network this repository does not have)\n"
              "                  [--model_path MODEL.npz [--use_splitting] [--use_guided_sampling] [-x split_batch_size] [-v samples_per_voxel]\n"
              "                   [-y appearance_embedding] [-z max_guided_samples] [--max_depth D] [--max_sample_count C] [--seed S]\n"
              "                   [--save_tree FILE.npz]]");
}

// rotate v about unit axis k by angle (Rodrigues), double precision
void rotate(float v[3], const float k[3], double ang) {
    const double c = std::cos(ang), s = std::sin(ang);
    const double x = v[0], y = v[1], z = v[2], kx = k[0], ky = k[1], kz = k[2];
    const double dot = kx * x + ky * y + kz * z;
    v[0] = (float)(x * c + (ky * z - kz * y) * s + kx * dot * (1 - c));
    v[1] = (float)(y * c + (kz * x - kx * z) * s + ky * dot * (1 - c));
    v[2] = (float)(z * c + (kx * y - ky * x) * s + kz * dot * (1 - c));
}

}  // namespace


namespace {

void hip_ok(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
void mnv_ok(int rc, const char *what) {
    if (rc != MNV_OK) throw std::runtime_error(std::string(what) + ": " + mnv_last_error());
}

// the options / camera part of the command line (render_options_from_args src/opts.cpp:49-67, camera flags main.cpp:550-582)
void configure(const Args &args, viewer::VolumeRenderer &rend, int width, int height) {
    rend.options.background_brightness = args.f("bg", 0.0f);
    rend.options.step_size = args.f("step_size", 1e-4f);
    rend.options.stop_thresh = args.f("stop_thresh", 1e-2f);
    rend.options.sigma_thresh = args.f("sigma_thresh", 1e-2f);
    rend.options.split_batch_size = (int)args.l("split_batch_size", 4096);
    rend.options.nerf_batch_size = (int)args.l("nerf_batch_size", 4096);
    rend.options.samples_per_corner = (int)args.l("samples_per_voxel", 8);
    rend.options.appearance_embedding = (int)args.l("appearance_embedding", -1);
    rend.options.max_guided_samples = (int)args.l("max_guided_samples", 128);
    if (args.has("grid")) {  // src/opts.cpp:53-55
        rend.options.show_grid = true;
        rend.options.grid_max_depth = (int)args.l("grid", rend.options.grid_max_depth);
    }
    rend.camera = viewer::Camera(width, height, args.f("fx", 1111.f), args.f("fy", -1.f), args.f("cx", -1.f), args.f("cy", -1.f));
    const std::vector<float> center = args.vec("center", {-3.5f, 0.f, 3.5f}), back = args.vec("back", {-0.7071068f, 0.f, 0.7071068f}),
                             origin = args.vec("origin", {0.f, 0.f, 0.f}), up = args.vec("world_up", {0.f, 0.f, 1.f});
    if (center.size() != 3 || back.size() != 3 || origin.size() != 3 || up.size() != 3) throw std::runtime_error("vector flags need 3 components");
    rend.camera.center = {center[0], center[1], center[2]};
    rend.camera.v_back = {back[0], back[1], back[2]};
    rend.camera.origin = {origin[0], origin[1], origin[2]};
    rend.camera.v_world_up = {up[0], up[1], up[2]};
}

std::vector<float> floats_of(const std::string &name, const std::string &s, size_t want) {
    std::vector<float> out;
    for (size_t i = 0; i <= s.size();) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        char *end = nullptr;
        const std::string t = s.substr(i, j - i);
        out.push_back(std::strtof(t.c_str(), &end));
        if (t.empty() || end != t.c_str() + t.size()) throw std::runtime_error("--" + name + ": malformed number '" + t + "'");
        i = j + 1;
    }
    if (out.size() != want) throw std::runtime_error("--" + name + " takes " + std::to_string(want) + " number(s)");
    return out;
}

// --mesh PATH[,unlit] and the --mesh_* flags that follow each: loaded, uploaded and listed in `rend`
void load_meshes(const Args &args, std::vector<viewer::Mesh> &meshes, viewer::VolumeRenderer &rend) {
    struct Spec {
        std::string path;
        bool unlit = false;
        float color[3] = {1.f, 1.f, 1.f}, translate[3] = {0.f, 0.f, 0.f}, rotate[3] = {0.f, 0.f, 0.f}, scale = 1.f;
    };
    std::vector<Spec> specs;
    for (const auto &kv : args.mesh_flags) {
        if (kv.first == "mesh") {
            Spec sp;
            sp.path = kv.second;
            const std::string suffix = ",unlit";
            if (sp.path.size() > suffix.size() && sp.path.compare(sp.path.size() - suffix.size(), suffix.size(), suffix) == 0) {
                sp.unlit = true;
                sp.path.resize(sp.path.size() - suffix.size());
            }
            specs.push_back(sp);
            continue;
        }
        if (specs.empty()) throw std::runtime_error("--" + kv.first + " applies to the --mesh named before it");
        Spec &sp = specs.back();
        if (kv.first == "mesh_scale") {
            sp.scale = floats_of(kv.first, kv.second, 1)[0];
        } else {
            float *dst = kv.first == "mesh_color" ? sp.color : kv.first == "mesh_translate" ? sp.translate : kv.first == "mesh_rotate" ? sp.rotate : nullptr;
            if (!dst) throw std::runtime_error("unknown flag --" + kv.first);
            const std::vector<float> v = floats_of(kv.first, kv.second, 3);
            std::copy(v.begin(), v.end(), dst);
        }
    }
    meshes.reserve(specs.size());
    for (const Spec &sp : specs) {
        meshes.push_back(viewer::Mesh::load_obj(sp.path, sp.color, sp.unlit));
        viewer::Mesh &m = meshes.back();
        std::copy(sp.translate, sp.translate + 3, m.translation);
        std::copy(sp.rotate, sp.rotate + 3, m.rotation);
        m.scale = sp.scale;
        m.update();
        rend.meshes.push_back(m.handle());
    }
}

// --orbit: rotate the camera about `origin` around world_up by `ang`
void orbit_step(viewer::Camera &cam, double ang) {
    float axis[3] = {cam.v_world_up.x, cam.v_world_up.y, cam.v_world_up.z};
    const float an = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    for (float &v : axis) v /= an;
    float c[3] = {cam.center.x - cam.origin.x, cam.center.y - cam.origin.y, cam.center.z - cam.origin.z};
    float b[3] = {cam.v_back.x, cam.v_back.y, cam.v_back.z};
    rotate(c, axis, ang);
    rotate(b, axis, ang);
    cam.center = {c[0] + cam.origin.x, c[1] + cam.origin.y, c[2] + cam.origin.z};
    cam.v_back = {b[0], b[1], b[2]};
}

void write_frame(const std::string &out, long f, int width, int height, const uint8_t *rgba8, const float *rgba) {
    char name[4096];
    std::snprintf(name, sizeof(name), "%s_%04ld.ppm", out.c_str(), f);
    if (std::FILE *fp = std::fopen(name, "wb")) {
        std::fprintf(fp, "P6\n%d %d\n255\n", width, height);
        static thread_local std::vector<uint8_t> rgb;
        rgb.resize((size_t)width * height * 3);
        for (size_t p = 0; p < (size_t)width * height; ++p) {
            rgb[p * 3 + 0] = rgba8[p * 4 + 0];
            rgb[p * 3 + 1] = rgba8[p * 4 + 1];
            rgb[p * 3 + 2] = rgba8[p * 4 + 2];
        }
        std::fwrite(rgb.data(), 1, rgb.size(), fp);
        std::fclose(fp);
    } else {
        throw std::runtime_error(std::string("cannot write ") + name);
    }
    if (rgba) {
        std::snprintf(name, sizeof(name), "%s_%04ld.f32", out.c_str(), f);
        std::FILE *fp = std::fopen(name, "wb");
        if (!fp) throw std::runtime_error(std::string("cannot write ") + name);
        std::fwrite(rgba, sizeof(float), (size_t)width * height * 4, fp);
        std::fclose(fp);
    }
}

// ---- multi-GPU mode: one process per GPU --------------------------------------------------------------------------------

struct Rendezvous {  // anonymous shared mapping created before the fork
    std::atomic<int> id_ready;
    std::atomic<int> failed;
    char id[MNV_COMM_ID_BYTES];
};

constexpr int kMacroW = 64, kMacroH = 24;  // per-rank launch times within 3 % of each other at world 8

// communicator: rank 0 draws the id, the others read it from the shared page
mnv_comm *join_ranks(int rank, int world, Rendezvous *rv) {
    if (rank == 0) {
        mnv_ok(mnv_comm_get_unique_id(rv->id), "mnv_comm_get_unique_id");
        rv->id_ready.store(1, std::memory_order_release);
    } else {
        while (!rv->id_ready.load(std::memory_order_acquire)) {
            if (rv->failed.load()) throw std::runtime_error("another rank failed before the rendezvous");
            usleep(1000);
        }
    }
    mnv_comm *comm = nullptr;
    mnv_ok(mnv_comm_init_rank(rv->id, world, rank, &comm), "mnv_comm_init_rank");
    return comm;
}

void print_refine_stats(long f, const viewer::VolumeRenderer::FrameStats &st) {
    std::printf("frame %ld: capacity %ld", f, st.capacity);
    if (st.split_candidates || st.added) std::printf("  split candidates %d, added %d%s", st.split_candidates, st.added, st.full ? " (full)" : "");
    if (st.sample_candidates) std::printf("  sample candidates %d, resampled %d", st.sample_candidates, st.resampled);
    if (st.pruned) std::printf("  pruned %d", st.pruned > 0 ? st.pruned : 0);
    if (st.guided_samples > 0) std::printf("  guided samples %ld", st.guided_samples);
    if (st.guided_samples < 0) std::printf("  guided samples: in flight");
    std::printf("\n");
}

// --gpus N with --use_splitting: the ranks refine ONE scene in lock step (VolumeRenderer::set_ranks) -- every rank marches its macro
// tiles, the tracker rows are all-gathered, every rank applies the same splits / resamples / prunes to its replica of the tree, and
// rank 0 assembles and writes the frames.  One frame at a time: a frame reads the tree the previous one left.
// Test hook, compiled only into the -DMNV_TEST_HOOKS build (testhooks/mnv_render): MNV_RANKS_SHARE_GPU=1 puts every rank on device --gpu
// (with a transport stand-in for RCCL, which refuses two ranks on one device: tests/shim/fake_rccl.cpp) so that the world > 1 paths can
// run on a one-GPU machine.  The shipped binary gives rank r device --gpu + r, always.
static bool save_every_rank() {  // test hook as well: every rank writes its replica of the refined tree
#ifdef MNV_TEST_HOOKS
    return std::getenv("MNV_SAVE_EVERY_RANK") != nullptr;
#else
    return false;
#endif
}
static bool ranks_share_gpu() {
#ifdef MNV_TEST_HOOKS
    return std::getenv("MNV_RANKS_SHARE_GPU") != nullptr;
#else
    return false;
#endif
}

int run_rank_refine(const Args &args, int rank, int world, Rendezvous *rv) {
    const bool share = ranks_share_gpu();
    if (hipSetDevice((int)args.l("gpu", 0) + (share ? 0 : rank)) != hipSuccess)
        throw std::runtime_error("rank " + std::to_string(rank) + ": no usable HIP device");
    viewer::N3Tree tree(args.file);
    if (tree.N <= 0) throw std::runtime_error("--gpus needs a tree (N > 0)");
    const int width = (int)args.l("width", 800), height = (int)args.l("height", 800);
    viewer::VolumeRenderer rend;
    configure(args, rend, width, height);
    const long max_capacity = std::max<long>(tree.capacity, args.l("max_tree_capacity", 20000000));
    rend.set(tree, max_capacity);
    rend.resize(width, height);
    rend.load_model(args.get("model_path", ""));
    rend.options.use_splitting = args.has("use_splitting");
    rend.options.use_guided_sampling = args.has("use_guided_sampling");
    rend.options.max_depth = (int)args.l("max_depth", rend.options.max_depth);
    rend.options.max_sample_count = (int)args.l("max_sample_count", rend.options.max_sample_count);
    rend.seed = (uint64_t)args.l("seed", 0);
    mnv_comm *comm = join_ranks(rank, world, rv);
    rend.set_ranks(comm, kMacroW, kMacroH);

    const long frames = args.l("frames", 1);
    const double orbit = args.f("orbit", 0.f) * M_PI / 180.0;
    const std::string out = args.get("out", "");
    std::vector<float> rgba;
    std::vector<uint8_t> rgba8;
    const auto wall0 = std::chrono::steady_clock::now();
    for (long f = 0; f < frames; ++f) {
        rend.render();
        if (rank == 0) {
            print_refine_stats(f, rend.stats);
            if (!out.empty()) {
                rend.download(args.has("raw") ? &rgba : nullptr, &rgba8);
                write_frame(out, f, width, height, rgba8.data(), args.has("raw") ? rgba.data() : nullptr);
            }
        }
        if (orbit != 0.0) orbit_step(rend.camera, orbit);
    }
    rend.sync_tree_streams();
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (args.has("save_tree")) {  // every rank holds the same tree; rank r > 0 writes <name>.rank<r> when asked to (MNV_SAVE_EVERY_RANK: tests)
        const std::string name = args.get("save_tree", "");
        if (rank == 0 || save_every_rank()) {
            rend.sync_tree();
            tree.save_npz(rank == 0 ? name : name + ".rank" + std::to_string(rank) + ".npz");
        }
    }
    if (rank == 0)
        std::printf("%s x %d (RCCL %d): %ld refinement frame(s) %dx%d in lock step, interleaved %dx%d macro tiles, %.3f ms/frame wall%s\n", rend.get_backend(),
                    world, (int)mnv_comm_rccl_version(), frames, width, height, kMacroW, kMacroH, wall_ms / std::max<long>(frames, 1),
                    out.empty() ? "" : " incl. download + file output");
    rend.set_ranks(nullptr);
    mnv_comm_destroy(comm);
    return 0;
}

int run_rank(const Args &args, int rank, int world, Rendezvous *rv) {
    const bool share = ranks_share_gpu();
    if (hipSetDevice((int)args.l("gpu", 0) + (share ? 0 : rank)) != hipSuccess)
        throw std::runtime_error("rank " + std::to_string(rank) + ": no usable HIP device");
    viewer::N3Tree tree(args.file);
    if (tree.N <= 0) throw std::runtime_error("--gpus needs a tree (N > 0)");
    const int width = (int)args.l("width", 800), height = (int)args.l("height", 800);
    viewer::VolumeRenderer rend;
    configure(args, rend, width, height);
    rend.set(tree, tree.capacity);  // every rank holds the whole tree: the march needs no exchange
    rend.resize(width, height);
    if (!tree.device.accel) throw std::runtime_error("--gpus needs the packed accel (N == 2, RGBA or SH1/4/9/16/25 rows)");
    const bool guided = args.has("model_path") && args.has("use_guided_sampling");
    if (guided) {
        rend.load_model(args.get("model_path", ""));  // sets need_viewdir / appearance_embedding as the single-GPU path does
        rend.options.max_guided_samples = (int)args.l("max_guided_samples", 128);
    }

    mnv_comm *comm = join_ranks(rank, world, rv);

    const long frames = args.l("frames", 1);
    const double orbit = args.f("orbit", 0.f) * M_PI / 180.0;
    const std::string out = args.get("out", "");
    const bool raw = args.has("raw");
    std::vector<mnv_camera> cams;  // the whole camera path, as the single-GPU loop would walk it
    for (long f = 0; f < frames; ++f) {
        rend.camera._update();
        cams.push_back(rend.camera.c_abi());
        if (orbit != 0.0) orbit_step(rend.camera, orbit);
    }

    const mnv_rect full = {0, 0, width, height};
    const int32_t root_period = world > 1 ? (int32_t)std::max<long>(2, args.l("root_period", std::lround(64.0 / world))) : 0;
    const mnv_partition part = {rank, world, kMacroW, kMacroH, root_period};
    int32_t j_max = 0;
    for (int r = 0; r < world; ++r) {
        const mnv_partition pr = {r, world, kMacroW, kMacroH, root_period};
        j_max = std::max(j_max, mnv_partition_local_tiles(full, pr));
    }
    const int batch = (int)std::min<long>(MNV_MAX_BATCH, std::max<long>(frames, 1));
    const size_t tile_px = (size_t)j_max * kMacroW * kMacroH, local_px = tile_px * batch, frame_px = (size_t)width * height;

    // the march runs on a stream that leaves `reserve` compute units to the RCCL kernels of the gather
    const int reserve = (int)args.l("reserve_cus", world > 1 ? 32 : 0);
    void *march_stream = nullptr;
    int32_t enabled = 0;
    if (mnv_stream_create_reserved(reserve, &march_stream, &enabled) != MNV_OK) {
        // no CU masking on this system: run unmasked (the gather of a batch then waits for the next batch's march to drain)
        std::fprintf(stderr, "mnv_render[rank %d]: %s; continuing without reserved compute units\n", rank, mnv_last_error());
        mnv_ok(mnv_stream_create_reserved(0, &march_stream, &enabled), "mnv_stream_create_reserved");
    }
    mnv_ok(mnv_accel_set_cu_budget(tree.device.accel, enabled), "mnv_accel_set_cu_budget");
    hipStream_t side = nullptr;
    hip_ok(hipStreamCreateWithFlags(&side, hipStreamNonBlocking), "hipStreamCreate");

    constexpr int RING = 2;
    struct Slot {
        mnv::Buffer<uint8_t> local8, gathered8, frames8;
        mnv::Buffer<float> local, gathered, framesf;
        mnv::Event rendered, sent, assembled;
        long first = -1;
        int count = 0;
    } slots[RING];
    for (Slot &s : slots) {
        hip_ok(s.local8.alloc(local_px * 4), "hipMalloc(local tiles)");
        if (raw) hip_ok(s.local.alloc(local_px * 4), "hipMalloc(local tiles f32)");
        if (rank == 0) {
            hip_ok(s.gathered8.alloc(local_px * 4 * world), "hipMalloc(gather table)");
            hip_ok(s.frames8.alloc(frame_px * 4 * batch), "hipMalloc(frames)");
            if (raw) {
                hip_ok(s.gathered.alloc(local_px * 4 * world), "hipMalloc(gather table f32)");
                hip_ok(s.framesf.alloc(frame_px * 4 * batch), "hipMalloc(frames f32)");
            }
        }
        hip_ok(s.rendered.create(hipEventDisableTiming), "hipEventCreate");
        hip_ok(s.sent.create(hipEventDisableTiming), "hipEventCreate");
        hip_ok(s.assembled.create(hipEventDisableTiming), "hipEventCreate");
    }
    std::vector<uint8_t> host8;
    std::vector<float> hostf;
    auto flush = [&](Slot &s) {  // rank 0: wait for the slot's assembled frames and write them
        if (s.first < 0) return;
        hip_ok(hipEventSynchronize(s.assembled.get()), "assemble");
        if (rank == 0 && !out.empty()) {
            host8.resize(frame_px * 4 * s.count);
            hip_ok(hipMemcpy(host8.data(), s.frames8.get(), host8.size(), hipMemcpyDeviceToHost), "download frames");
            if (raw) {
                hostf.resize(frame_px * 4 * s.count);
                hip_ok(hipMemcpy(hostf.data(), s.framesf.get(), hostf.size() * 4, hipMemcpyDeviceToHost), "download frames f32");
            }
            for (int i = 0; i < s.count; ++i)
                write_frame(out, s.first + i, width, height, host8.data() + frame_px * 4 * i, raw ? hostf.data() + frame_px * 4 * i : nullptr);
        }
        s.first = -1;
    };

    const auto wall0 = std::chrono::steady_clock::now();
    int b = 0;
    for (long f0 = 0; f0 < frames; f0 += batch, ++b) {
        Slot &s = slots[b % RING];
        flush(s);  // frames of the batch that used this slot two batches ago
        const int n = (int)std::min<long>(batch, frames - f0);
        s.first = f0;
        s.count = n;
        // one launch per rank and batch; the buffer is reused only after the gather that last read it
        hip_ok(hipStreamWaitEvent((hipStream_t)march_stream, s.sent.get(), 0), "wait(sent)");
        if (!guided) {
            mnv_ok(mnv_render_voxels_accel_batch(tree.device.accel, cams.data() + f0, n, rend.options.c_abi(), full, part, s.local.get(), s.local8.get(), march_stream),
                   "mnv_render_voxels_accel_batch");
        } else {
            // guided sampling: one fused launch (march + networks + composite) per frame, into the frame's place in the batch buffer
            for (int i = 0; i < n; ++i)
                mnv_ok(mnv_render_guided_fused_part(tree.device.accel, &cams[f0 + i], rend.options.c_abi(), full, part, rend.model(), &rend.cluster_grid(),
                                                    s.local ? s.local.get() + (size_t)i * tile_px * 4 : nullptr, s.local8.get() + (size_t)i * tile_px * 4, nullptr,
                                                    march_stream),
                       "mnv_render_guided_fused_part");
        }
        hip_ok(hipEventRecord(s.rendered.get(), (hipStream_t)march_stream), "record(rendered)");
        // gather + un-permute on the side stream, overlapping the next batch's march
        hip_ok(hipStreamWaitEvent(side, s.rendered.get(), 0), "wait(rendered)");
        mnv_ok(mnv_gather_tiles(comm, s.local8.get(), s.gathered8.get(), tile_px * 4 * n, 0, side), "mnv_gather_tiles");
        if (raw) mnv_ok(mnv_gather_tiles(comm, s.local.get(), s.gathered.get(), tile_px * 16 * n, 0, side), "mnv_gather_tiles(f32)");
        hip_ok(hipEventRecord(s.sent.get(), side), "record(sent)");
        if (rank == 0) {
            mnv_ok(mnv_assemble_tiles(s.gathered8.get(), s.frames8.get(), width, height, part, n, 4, side), "mnv_assemble_tiles");
            if (raw) mnv_ok(mnv_assemble_tiles(s.gathered.get(), s.framesf.get(), width, height, part, n, 16, side), "mnv_assemble_tiles(f32)");
        }
        hip_ok(hipEventRecord(s.assembled.get(), side), "record(assembled)");
    }
    for (int k = 0; k < RING; ++k) flush(slots[(b + k) % RING]);
    hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (rank == 0)
        std::printf("%s x %d (RCCL %d): %ld frame(s) %dx%d, interleaved %dx%d macro tiles, %.3f ms/frame wall%s, %.1f Mrays/s\n", rend.get_backend(), world,
                    (int)mnv_comm_rccl_version(), frames, width, height, kMacroW, kMacroH, wall_ms / std::max<long>(frames, 1),
                    out.empty() ? "" : " incl. download + file output", wall_ms > 0 ? (double)width * height * frames / wall_ms / 1e3 : 0.0);
    (void)hipStreamDestroy(side);
    mnv_comm_destroy(comm);
    (void)mnv_stream_destroy(march_stream);
    return 0;
}

// Fork one child per rank BEFORE anything in this process touches HIP, wait for them, and take a failing rank's peers down
// with it (they would otherwise wait in RCCL forever).
int run_distributed(const Args &args, int world) {
    if (world < 1 || world > 64) throw std::runtime_error("--gpus must be 1 .. 64");
    if (args.has("use_splitting") && !args.has("model_path")) throw std::runtime_error("--use_splitting needs --model_path");
    if (args.has("use_guided_sampling") && !args.has("model_path")) throw std::runtime_error("--use_guided_sampling needs --model_path");
    void *page = mmap(nullptr, sizeof(Rendezvous), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (page == MAP_FAILED) throw std::runtime_error("mmap failed");
    Rendezvous *rv = new (page) Rendezvous();
    rv->id_ready.store(0);
    rv->failed.store(0);
    std::vector<pid_t> kids;
    for (int r = 0; r < world; ++r) {
        std::fflush(nullptr);
        const pid_t pid = fork();
        if (pid < 0) throw std::runtime_error("fork failed");
        if (pid == 0) {
            int rc = 1;
            try {
                rc = args.has("use_splitting") ? run_rank_refine(args, r, world, rv) : run_rank(args, r, world, rv);
            } catch (const std::exception &e) {
                std::fprintf(stderr, "mnv_render[rank %d]: %s\n", r, e.what());
                rv->failed.store(1);
            }
            std::fflush(nullptr);
            _exit(rc);
        }
        kids.push_back(pid);
    }
    int worst = 0, left = world;
    while (left > 0) {
        int status = 0;
        const pid_t pid = wait(&status);
        if (pid < 0) break;
        --left;
        const int rc = WIFEXITED(status) ? WEXITSTATUS(status) : 128 + (WIFSIGNALED(status) ? WTERMSIG(status) : 0);
        if (rc != 0 && worst == 0) {
            worst = rc;
            for (pid_t k : kids)
                if (k != pid) (void)kill(k, SIGTERM);  // exactly the processes started above
        }
    }
    munmap(page, sizeof(Rendezvous));
    return worst;
}

// --points: the cloud of an .npz or .obj file as a tree on the device
void tree_from_points(const Args &args, viewer::N3Tree &tree) {
    const std::string path = args.get("points", "");
    auto ends_with = [&](const char *suffix) { return path.size() >= 4 && path.compare(path.size() - 4, 4, suffix) == 0; };
    std::vector<float> xyz;
    std::vector<uint8_t> rgb;
    if (ends_with(".npz")) {
        const viewer::npz::Archive z = viewer::npz::load(path);
        const auto p = z.find("points");
        if (p == z.end()) throw std::runtime_error("--points: " + path + " lacks the array 'points'");
        const viewer::npz::Array &a = p->second;
        if (a.kind != 'f' || a.word_size != 4 || a.fortran_order || a.shape.size() != 2 || a.shape[1] != 3) throw std::runtime_error("--points: 'points' must be float32 [n][3]");
        xyz.assign(a.data<float>(), a.data<float>() + a.num_vals());
        const auto c = z.find("colors");
        if (c != z.end()) {
            const viewer::npz::Array &b = c->second;
            if (b.kind != 'u' || b.word_size != 1 || b.fortran_order || b.shape != a.shape) throw std::runtime_error("--points: 'colors' must be uint8 [n][3]");
            rgb.assign(b.data<uint8_t>(), b.data<uint8_t>() + b.num_vals());
        }
    } else if (ends_with(".obj")) {
        const viewer::Mesh m = viewer::Mesh::load_obj(path);
        const size_t n = m.vert.size() / 9;
        xyz.resize(n * 3);
        rgb.resize(n * 3);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                xyz[i * 3 + k] = m.vert[i * 9 + k];
                const float v = m.vert[i * 9 + 3 + k] * 255.f + 0.5f;
                rgb[i * 3 + k] = (uint8_t)(v >= 255.f ? 255 : v > 0.f ? (int)v : 0);
            }
    } else {
        throw std::runtime_error("--points takes an .npz or an .obj file");
    }
    mnv_points_params p{};
    viewer::DataFormat fmt;
    fmt.parse(args.get("points_format", "RGBA"));
    p.format = fmt.format == viewer::DataFormat::SH ? MNV_FORMAT_SH : MNV_FORMAT_RGBA;
    p.basis_dim = fmt.basis_dim;
    p.depth = (int32_t)args.l("points_depth", 8);
    p.sigma = args.f("points_sigma", 100.f);
    const long min_points = args.l("points_min", 1);
    if (min_points < 1 || min_points > 0x7fffffffl) throw std::runtime_error("--points_min takes a count of at least 1");
    p.min_points = (uint32_t)min_points;
    if (args.has("points_cube")) {
        const std::vector<float> cube = args.vec("points_cube", {});
        if (cube.size() != 6) throw std::runtime_error("--points_cube takes ox,oy,oz,sx,sy,sz");
        for (int k = 0; k < 3; ++k) p.offset[k] = cube[k], p.scale[k] = cube[3 + k];
    } else {  // the smallest cube around the finite points, widened so that none sits on an upper face
        float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
        bool any = false;
        for (size_t i = 0; i + 2 < xyz.size(); i += 3) {
            if (!std::isfinite(xyz[i]) || !std::isfinite(xyz[i + 1]) || !std::isfinite(xyz[i + 2])) continue;
            for (int k = 0; k < 3; ++k) {
                lo[k] = any ? std::min(lo[k], xyz[i + k]) : xyz[i + k];
                hi[k] = any ? std::max(hi[k], xyz[i + k]) : xyz[i + k];
            }
            any = true;
        }
        float pad = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]) / 4096.f;
        if (!(pad > 0.f)) pad = 0.5f;
        for (int k = 0; k < 3; ++k) lo[k] -= pad, hi[k] += pad;
        mnv_ok(mnv_points_bounds_to_cube(lo, hi, p.offset, p.scale), "--points");
    }
    mnv_points_stats st{};
    viewer::N3Tree::from_points_into(tree, p, xyz, rgb, nullptr, &st);
    std::printf("points: %zu point(s), %lld accepted, %lld dropped; depth %d: %lld distinct voxel(s), %lld occupied (>= %u points); %d chunk(s), per depth:",
                xyz.size() / 3, (long long)st.accepted, (long long)st.dropped, p.depth, (long long)st.distinct_voxels, (long long)st.occupied_voxels, p.min_points,
                tree.capacity);
    for (int d = 1; d < 24 && st.chunks_at_depth[d] > 0; ++d) std::printf(" %lld", (long long)st.chunks_at_depth[d]);
    std::printf("; offset %.9g,%.9g,%.9g scale %.9g,%.9g,%.9g\n", p.offset[0], p.offset[1], p.offset[2], p.scale[0], p.scale[1], p.scale[2]);
}


// --merge B [--merge_at k:x,y,z] [--merge_mode over|add], as often as given, in command-line order (checked before a device is touched)
struct MergeSpec {
    std::string path, mode = "over";
    bool has_at = false;
    mnv_merge_params p{};
};

std::vector<MergeSpec> merge_specs(const Args &args) {
    std::vector<MergeSpec> specs;
    for (const auto &kv : args.merge_flags) {
        if (kv.first == "merge") {
            specs.push_back(MergeSpec{});
            specs.back().path = kv.second;
            continue;
        }
        if (specs.empty()) throw std::runtime_error("--" + kv.first + " needs --merge in front of it: it applies to the --merge it follows");
        MergeSpec &s = specs.back();
        if (kv.first == "merge_at") {
            long long k = -1, x = -1, y = -1, z = -1;
            char end = 0;
            if (std::sscanf(kv.second.c_str(), "%lld:%lld,%lld,%lld%c", &k, &x, &y, &z, &end) != 4 || k < 0 || k > 22 || x < 0 || y < 0 || z < 0 || x >= (1ll << k) ||
                y >= (1ll << k) || z >= (1ll << k))
                throw std::runtime_error("--merge_at takes k:x,y,z with k in 0 .. 22 and 0 <= x, y, z < 2^k");
            s.has_at = true;
            s.p.level = (int32_t)k, s.p.corner[0] = (int32_t)x, s.p.corner[1] = (int32_t)y, s.p.corner[2] = (int32_t)z;
        } else {
            if (kv.second != "over" && kv.second != "add") throw std::runtime_error("--merge_mode is over or add");
            s.mode = kv.second;
        }
        s.p.mode = s.mode == "add" ? MNV_MERGE_ADD : MNV_MERGE_OVER;
    }
    return specs;
}

// --merge: every B placed into the tree so far, left to right; `tree` ends as the merged tree (on the device, host arrays filled)
void merge_trees(const std::vector<MergeSpec> &specs, std::unique_ptr<viewer::N3Tree> &tree) {
    if (tree->N <= 0) throw std::runtime_error("--merge needs a base tree (N > 0)");
    for (const MergeSpec &s : specs) {
        mnv_merge_params p = s.p;
        viewer::N3Tree b;
        b.open(s.path);
        if (b.N <= 0) throw std::runtime_error("--merge: cannot open " + s.path);
        if (!s.has_at) {  // the voxel of the base tree that B's offset and scale name exactly
            bool found = false;
            for (int k = 0; k <= 22 && !found; ++k) {
                const float two = (float)(1 << k);
                bool same = true;
                for (int i = 0; i < 3; ++i) same = same && b.scale[i] == tree->scale[i] * two;
                if (!same) continue;
                int32_t corner[3];
                bool inside = true;
                for (int i = 0; i < 3; ++i) {
                    const double r = std::nearbyint((double)(tree->offset[i] * two) - (double)b.offset[i]);
                    inside = inside && r >= 0.0 && r < (double)two;
                    corner[i] = inside ? (int32_t)r : 0;
                }
                if (!inside) continue;
                float o[3], sc[3];
                mnv_ok(mnv_tree_voxel_cube(tree->offset.data(), tree->scale.data(), k, corner, o, sc), "--merge");
                if (std::memcmp(o, b.offset.data(), 12) != 0 || std::memcmp(sc, b.scale.data(), 12) != 0) continue;
                p.level = k, p.corner[0] = corner[0], p.corner[1] = corner[1], p.corner[2] = corner[2];
                found = true;
            }
            if (!found)
                throw std::runtime_error("--merge: the cube of " + s.path + " is no voxel of the base tree's cube (offset and scale must match exactly): say where it goes with --merge_at k:x,y,z");
        }
        if (!tree->on_device()) tree->move_to_device(tree->capacity, true, true);
        b.move_to_device(b.capacity, false, true);
        mnv_merge_stats st{};
        std::unique_ptr<viewer::N3Tree> merged = tree->merge(b, p, nullptr, &st);
        std::printf("merge: %s at %d:%d,%d,%d (%s): %d + %d -> %lld chunk(s); rows from the base %lld, from the merged tree %lld, blended %lld; pushed down %lld + %lld; per depth:",
                    s.path.c_str(), p.level, p.corner[0], p.corner[1], p.corner[2], s.mode.c_str(), tree->capacity, b.capacity, (long long)st.capacity, (long long)st.rows_from_a,
                    (long long)st.rows_from_b, (long long)st.rows_blended, (long long)st.pushed_a, (long long)st.pushed_b);
        for (int d = 1; d < 24 && st.chunks_at_depth[d]; ++d) std::printf(" %lld", (long long)st.chunks_at_depth[d]);
        std::printf("\n");
        tree = std::move(merged);
    }
}

}  // namespace

int main(int argc, char **argv) {
    try {
        const Args args = parse(argc, argv);
        if (args.has("points") && !args.file.empty())
            throw std::runtime_error("--points builds the tree: it cannot be combined with an input tree (" + args.file + ")");
        if (args.has("points") && args.has("gpus")) throw std::runtime_error("--points builds the tree on one GPU: it cannot be combined with --gpus");
        for (const char *k : {"points_depth", "points_sigma", "points_min", "points_format", "points_cube"})
            if (args.has(k) && !args.has("points")) throw std::runtime_error(std::string("--") + k + " needs --points");
        const std::vector<MergeSpec> merges = merge_specs(args);
        if (args.has("merge") && (args.has("gpus") || args.has("use_splitting")))
            throw std::runtime_error("--merge merges on one GPU into a tree that is then fixed: it cannot be combined with --gpus or --use_splitting");
        if (args.has("help") || (args.file.empty() && !args.has("points"))) {
            usage();
            return args.has("help") ? 0 : 2;
        }
        if (args.has("gpus") && args.has("grid")) throw std::runtime_error("--grid draws on one GPU: it cannot be combined with --gpus");
        if (args.has("gpus") && !args.mesh_flags.empty()) throw std::runtime_error("--mesh draws on one GPU: it cannot be combined with --gpus");
        if (args.has("gpus") && args.has("extract_mesh")) throw std::runtime_error("--extract_mesh extracts on one GPU: it cannot be combined with --gpus");
        const std::string aa_filter = args.get("aa_filter", "tent");
        if (aa_filter != "box" && aa_filter != "tent") throw std::runtime_error("--aa_filter is box or tent");
        if (args.has("gpus") && args.l("aa", 1) != 1)
            throw std::runtime_error("--aa resolves its sub-frames on one GPU: it cannot be combined with --gpus");
        const std::string projection = args.get("projection", "pinhole");
        if (projection != "pinhole" && projection != "ortho" && projection != "equirect") throw std::runtime_error("--projection is pinhole, ortho or equirect");
        if (projection != "pinhole" && (args.has("gpus") || args.has("grid") || !args.mesh_flags.empty() || args.has("extract_mesh") || args.l("aa", 1) != 1))
            throw std::runtime_error("--projection " + projection + " marches a ray list: it cannot be combined with --gpus, --grid, --mesh, --extract_mesh or --aa other than 1");
        if (args.has("gpus") && (args.has("target") || args.has("target_mask") || args.has("ssim")))
            throw std::runtime_error("--target scores the frames of one GPU: it cannot be combined with --gpus");
        if ((args.has("target_mask") || args.has("ssim")) && !args.has("target")) throw std::runtime_error("--target_mask and --ssim need --target");
        const long lod = args.l("lod", 0);
        if (args.has("lod") && lod < 1) throw std::runtime_error("--lod takes a depth of at least 1");
        if (args.has("save_lod") && !args.has("lod") && !args.has("lod_pixels") && !args.has("cull") && !args.has("points") && !args.has("merge") && !args.has("fit_images"))
            throw std::runtime_error("--save_lod needs --lod, --lod_pixels or --cull");
        const float cull_thresh = args.f("cull", 0.f);
        if (args.has("cull") && (!std::isfinite(cull_thresh) || cull_thresh < 0.f)) throw std::runtime_error("--cull takes a finite weight threshold, 0 or more");
        if (args.has("cull") && (args.has("lod") || args.has("lod_pixels") || args.has("lod_fit") || args.has("gpus") || args.has("use_splitting") || args.has("use_guided_sampling")))
            throw std::runtime_error("--cull renders a culled copy of the tree on one GPU: it cannot be combined with --lod, --lod_pixels, --lod_fit, --gpus, --use_splitting or --use_guided_sampling");
        const float lod_pixels = args.f("lod_pixels", 0.f);
        const long lod_min = args.l("lod_min", 1), lod_max = args.l("lod_max", 23);
        if (args.has("lod_pixels") && (!std::isfinite(lod_pixels) || lod_pixels < 0.f)) throw std::runtime_error("--lod_pixels takes a finite size in pixels, 0 or more");
        if ((args.has("lod_min") || args.has("lod_max")) && !args.has("lod_pixels")) throw std::runtime_error("--lod_min and --lod_max need --lod_pixels");
        if (args.has("lod_pixels") && (lod_min < 1 || lod_max < lod_min)) throw std::runtime_error("--lod_pixels: need 1 <= --lod_min <= --lod_max");
        if (args.has("lod_pixels") && (args.has("lod") || args.has("gpus") || args.has("use_splitting") || args.has("use_guided_sampling")))
            throw std::runtime_error("--lod_pixels renders a cut copy of the tree on one GPU: it cannot be combined with --lod, --gpus, --use_splitting or --use_guided_sampling");
        const long lod_fit = args.l("lod_fit", 0);
        const std::string fit_optimizer = args.get("fit_optimizer", "sgd");
        if (fit_optimizer != "sgd" && fit_optimizer != "adam") throw std::runtime_error("--fit_optimizer takes sgd or adam");
        const bool fit_adam = fit_optimizer == "adam";
        // the rates: SGD's were chosen on the test suite's fit scene (tests/fit_cases.py), Adam's likewise (tests/fit_adam_ref.py)
        const float fit_lr_colour = args.f("fit_lr_colour", fit_adam ? 0.03f : 1.f), fit_lr_sigma = args.f("fit_lr_sigma", fit_adam ? 1.f : 20.f);
        const long fit_batch = args.l("fit_batch", 0), fit_tile = args.l("fit_tile", 8);
        uint64_t fit_seed = 0;  // all 64 bits: decimal, or hexadecimal with 0x
        if (args.has("fit_seed")) {
            const std::string text = args.get("fit_seed", "");
            size_t used = 0;
            try {
                if (text.empty() || text[0] == '-') throw std::invalid_argument(text);
                fit_seed = std::stoull(text, &used, 0);
            } catch (const std::exception &) {
                used = 0;
            }
            if (used == 0 || used != text.size()) throw std::runtime_error("--fit_seed takes an unsigned 64-bit seed");
        }
        if (args.has("lod_fit") && lod_fit < 1) throw std::runtime_error("--lod_fit takes an iteration count of at least 1");
        const bool fit_flag = args.has("fit_lr_colour") || args.has("fit_lr_sigma") || args.has("fit_optimizer") || args.has("fit_batch") || args.has("fit_tile") ||
                              args.has("fit_seed");
        const std::string fit_images = args.get("fit_images", "");
        const long fit_steps = args.l("fit_steps", 0), fit_holdout = args.l("fit_holdout", 0);
        if (args.has("fit_images")) {
            if (fit_images.empty()) throw std::runtime_error("--fit_images takes the prefix of the target files (PREFIX_%04d.ppm)");
            if (!args.has("fit_steps") || fit_steps < 1) throw std::runtime_error("--fit_images needs --fit_steps N with N of at least 1");
            if (args.has("fit_holdout") && fit_holdout < 2) throw std::runtime_error("--fit_holdout takes K of at least 2 (every K-th pose is held out)");
            if (args.has("lod_fit") || args.has("cull") || args.has("gpus") || args.has("use_splitting") || args.has("use_guided_sampling"))
                throw std::runtime_error("--fit_images fits the tree this run marches on one GPU: it cannot be combined with --lod_fit, --cull, --gpus, --use_splitting or --use_guided_sampling");
        } else if (args.has("fit_steps") || args.has("fit_holdout")) {
            throw std::runtime_error("--fit_steps and --fit_holdout need --fit_images");
        }
        if (!args.has("fit_images") && (args.has("lod_fit") || fit_flag) && !((args.has("lod") || args.has("lod_pixels")) && args.has("lod_fit")))
            throw std::runtime_error("--lod_fit needs --lod or --lod_pixels; --fit_lr_colour, --fit_lr_sigma, --fit_optimizer, --fit_batch, --fit_tile and --fit_seed need --lod_fit or --fit_images");
        if (fit_tile != 1 && fit_tile != 8) throw std::runtime_error("--fit_tile takes 1 or 8");
        if (fit_batch < 0 || fit_batch > (1L << 22) || fit_batch % (fit_tile * fit_tile) != 0)
            throw std::runtime_error("--fit_batch takes a ray count that is a multiple of the tile's pixels, at most 4194304 (0: full batch)");
        if (args.has("lod") && (args.has("gpus") || args.has("use_splitting") || args.has("use_guided_sampling")))
            throw std::runtime_error("--lod renders a truncated copy of the tree on one GPU: it cannot be combined with --gpus, --use_splitting or --use_guided_sampling");
        if (args.has("gpus")) return run_distributed(args, (int)args.l("gpus", 1));  // before any HIP call in this process
        if (hipSetDevice((int)args.l("gpu", 0)) != hipSuccess) throw std::runtime_error("no usable HIP device");

        std::unique_ptr<viewer::N3Tree> tree_owner = std::make_unique<viewer::N3Tree>();
        if (args.has("points"))
            tree_from_points(args, *tree_owner);
        else
            tree_owner->open(args.file);  // main.cpp:528
        if (!merges.empty()) merge_trees(merges, tree_owner);
        viewer::N3Tree &tree = *tree_owner;
        if ((args.has("points") || args.has("merge")) && args.has("save_lod") && !args.has("lod") && !args.has("lod_pixels") && !args.has("cull") &&
            !args.has("fit_images")) {  // (--fit_images writes the tree after its fit)
            tree.save_npz(args.get("save_lod", ""));
            std::printf("save_lod: %d chunks -> %s\n", tree.capacity, args.get("save_lod", "").c_str());
        }
        if (args.has("bounds_only") && tree.N > 0) {  // main.cpp:529-538: keep one empty root chunk
            tree.capacity = 1;
            tree.data.assign((size_t)8 * tree.data_dim, 0);
            tree.child.assign(8, 0);
            tree.parent.assign(1, -1);
            tree.sample_counts.assign(8, 8);
        }
        const int width = (int)args.l("width", 800), height = (int)args.l("height", 800);  // main.cpp:491-492
        viewer::VolumeRenderer rend;
        configure(args, rend, width, height);
        const bool refine = args.has("model_path") && (args.has("use_splitting") || args.has("use_guided_sampling"));
        // the reference reserves max_tree_capacity (default 20M chunks) up front; without refinement the tree cannot grow
        const long max_capacity = refine ? std::max<long>(tree.capacity, args.l("max_tree_capacity", 20000000)) : tree.capacity;
        if (tree.N > 0) rend.set(tree, max_capacity);
        rend.resize(width, height);
        std::vector<viewer::Mesh> meshes;
        load_meshes(args, meshes, rend);
        const long frames = args.l("frames", 1);
        viewer::Mesh extracted;  // --extract_mesh: written, then drawn under the volume by the frames of this run
        if (args.has("extract_mesh")) {
            if (tree.N <= 0) throw std::runtime_error("--extract_mesh needs a tree (N > 0)");
            extracted = tree.extract_surface((int)args.l("extract_level", 7), args.f("extract_iso", 10.f), true);
            extracted.save_obj(args.get("extract_mesh", ""));
            std::printf("extract_mesh: %zu vertices, %zu triangles -> %s\n", extracted.vert.size() / 9, extracted.faces.size() / 3, args.get("extract_mesh", "").c_str());
            if (frames > 0 && !extracted.faces.empty()) {
                extracted.unlit = args.has("extract_unlit");
                extracted.update();
                rend.meshes.push_back(extracted.handle());
            }
        }
        if (args.has("model_path")) {  // main.cpp:585-589
            rend.load_model(args.get("model_path", ""));
            rend.options.use_splitting = args.has("use_splitting");
            rend.options.use_guided_sampling = args.has("use_guided_sampling");
            rend.options.max_depth = (int)args.l("max_depth", rend.options.max_depth);
            rend.options.max_sample_count = (int)args.l("max_sample_count", rend.options.max_sample_count);
            rend.seed = (uint64_t)args.l("seed", 0);
        }

        const double orbit = args.f("orbit", 0.f) * M_PI / 180.0;
        const std::string out = args.get("out", "");
        std::vector<float> rgba;
        std::vector<uint8_t> rgba8;
        rend.frames_in_flight = (int)std::max<long>(1, args.l("in_flight", rend.frames_in_flight));
        rend.guided_in_flight = args.has("guided_in_flight");
        rend.aa_samples = (int)args.l("aa", 1);
        rend.aa_filter = aa_filter == "box" ? MNV_AA_BOX : MNV_AA_TENT;
        rend.projection = projection == "ortho" ? MNV_PROJ_ORTHO : projection == "equirect" ? MNV_PROJ_EQUIRECT : MNV_PROJ_PINHOLE;
        // --lod_fit: the camera of every pose this run renders (the frame loop below, stepped on a copy of the camera), and the fit of a cut
        std::vector<mnv_camera> fit_cams;
        mnv_fit_params_ex fit_params = {};  // (sgd, no batch: what --lod_fit was before it had these flags, N3Tree::fit_to)
        fit_params.steps = (int32_t)lod_fit;
        fit_params.optimizer = fit_adam ? MNV_FIT_ADAM : MNV_FIT_SGD;
        fit_params.lr_colour = fit_lr_colour, fit_params.lr_sigma = fit_lr_sigma;
        fit_params.beta1 = 0.9f, fit_params.beta2 = 0.999f, fit_params.eps = 1e-8f;
        fit_params.batch_rays = (int32_t)fit_batch, fit_params.tile = (int32_t)fit_tile;
        fit_params.seed = fit_seed;
        if (lod_fit > 0) {
            viewer::Camera walk = rend.camera;
            for (long f = 0; f < std::max<long>(frames, 1) && fit_cams.size() < 4096; ++f) {
                walk._update();
                fit_cams.push_back(walk.c_abi());
                if (orbit == 0.0) break;  // (every frame has the same pose)
                orbit_step(walk, orbit);
            }
            rend.set_lod_fit(fit_cams, fit_params);
        }
        auto fit_cut = [&](viewer::N3Tree &cut) {
            if (lod_fit < 1) return;
            const std::vector<mnv_fit_sums> sums = cut.fit_to_ex(tree, fit_cams, *rend.options.c_abi(), fit_params);
            std::printf("lod_fit: %zu pose(s), lr_colour %g, lr_sigma %g; mean squared error of the fitted rays before each step (x 1e6):", fit_cams.size(),
                        (double)fit_lr_colour, (double)fit_lr_sigma);
            // full batch: over every pixel of the poses, as before; a batch: over the rays of that batch that count
            for (const mnv_fit_sums &q : sums)
                std::printf(" %.3f", (double)q.se_q32 / 4294967296.0 /
                                         (3.0 * (fit_batch > 0 ? (double)std::max<int64_t>(q.n_rays, 1) : (double)width * height * (double)fit_cams.size())) * 1e6);
            std::printf("\n");
        };
        // --fit_images: the tree this run marches -- the input tree, or its --lod / --lod_pixels cut -- is fitted to photographs of this run's
        // poses (PREFIX_%04d.ppm, the files --out writes: byte / 255, alpha 1) with N3Tree::fit_ex, then marched by the frames below
        std::unique_ptr<viewer::N3Tree> fit_owner;  // the cut, where there is one: the renderer marches it in place of its own
        if (args.has("fit_images")) {
            if (tree.N <= 0) throw std::runtime_error("--fit_images needs a tree (N > 0)");
            if (frames < 1 || frames > 4096) throw std::runtime_error("--fit_images serves 1 to 4096 poses (--frames)");
            std::vector<mnv_camera> cams;
            std::vector<mnv_lod_view> views;
            viewer::Camera walk = rend.camera;
            for (long f = 0; f < frames; ++f) {
                walk._update();
                cams.push_back(walk.c_abi());
                views.push_back({{walk.center.x, walk.center.y, walk.center.z}, std::max(walk.fx, walk.fy)});
                if (orbit != 0.0) orbit_step(walk, orbit);
            }
            if (lod > 0)
                fit_owner = tree.make_lod((int)lod);
            else if (args.has("lod_pixels"))
                fit_owner = tree.make_view_lod(views, lod_pixels, (int)lod_min, (int)lod_max);
            viewer::N3Tree &subject = fit_owner ? *fit_owner : tree;
            const size_t px = (size_t)width * height;
            std::vector<mnv::Buffer<float>> image((size_t)frames);
            std::vector<mnv::Buffer<uint8_t>> image8((size_t)frames);
            std::vector<uint8_t> rgb(px * 3), rgba8_host(px * 4);
            std::vector<float> rgba_host(px * 4);
            for (long f = 0; f < frames; ++f) {
                char name[4096];
                int32_t w = 0, h = 0, ch = 0;
                std::snprintf(name, sizeof(name), "%s_%04ld.ppm", fit_images.c_str(), f);
                mnv_ok(mnv_pnm_read(name, width, height, rgb.data(), (int64_t)rgb.size(), &w, &h, &ch), "--fit_images");
                if (ch != 3) throw std::runtime_error(std::string("--fit_images: ") + name + " is not a P6 file");
                for (size_t p = 0; p < px; ++p) {
                    for (int k = 0; k < 3; ++k) {
                        rgba8_host[p * 4 + k] = rgb[p * 3 + k];
                        rgba_host[p * 4 + k] = (float)rgb[p * 3 + k] / 255.f;
                    }
                    rgba8_host[p * 4 + 3] = 255;
                    rgba_host[p * 4 + 3] = 1.f;
                }
                hip_ok(image[(size_t)f].alloc(px * 4), "hipMalloc(fit image)");
                hip_ok(image8[(size_t)f].alloc(px * 4), "hipMalloc(fit image, bytes)");
                hip_ok(hipMemcpy(image[(size_t)f].get(), rgba_host.data(), px * 16, hipMemcpyHostToDevice), "upload fit image");
                hip_ok(hipMemcpy(image8[(size_t)f].get(), rgba8_host.data(), px * 4, hipMemcpyHostToDevice), "upload fit image, bytes");
            }
            std::vector<mnv_camera> train_cams;
            std::vector<const float *> train_images;
            std::vector<long> train, held;
            for (long f = 0; f < frames; ++f) {
                if (fit_holdout > 0 && f % fit_holdout == fit_holdout - 1) {
                    held.push_back(f);
                } else {
                    train.push_back(f);
                    train_cams.push_back(cams[(size_t)f]);
                    train_images.push_back(image[(size_t)f].get());
                }
            }
            if (train.empty()) throw std::runtime_error("--fit_images: every pose is held out");
            mnv_render_options march = *rend.options.c_abi();
            march.render_depth = false;
            mnv::Buffer<float> frame;
            mnv::Buffer<mnv_metric_sums> sums_dev;
            hip_ok(frame.alloc(px * 4), "hipMalloc(fit frame)");
            hip_ok(sums_dev.alloc(1), "hipMalloc(metric sums)");
            auto mean_psnr = [&](const std::vector<long> &poses) {  // mnv_frame_metrics of the tree's frames against the files, quantised
                double sum = 0.0;
                for (long f : poses) {
                    mnv_ok(mnv_render_voxels_accel(subject.device.accel, &cams[(size_t)f], &march, mnv_rect{0, 0, width, height}, frame.get(), nullptr, nullptr),
                           "mnv_render_voxels_accel (--fit_images)");
                    hip_ok(hipMemset(sums_dev.get(), 0, sizeof(mnv_metric_sums)), "clear metric sums");
                    mnv_ok(mnv_frame_metrics(frame.get(), image8[(size_t)f].get(), width, height, MNV_METRIC_QUANTISED, nullptr, sums_dev.get(), nullptr, nullptr, nullptr),
                           "mnv_frame_metrics");
                    mnv_metric_sums host{};
                    hip_ok(hipMemcpy(&host, sums_dev.get(), sizeof(host), hipMemcpyDeviceToHost), "download metric sums");
                    mnv_frame_metric_values m{};
                    mnv_ok(mnv_metrics_finish(&host, &m), "mnv_metrics_finish");
                    sum += m.psnr;
                }
                return poses.empty() ? 0.0 : sum / (double)poses.size();
            };
            if (!subject.device.accel) throw std::runtime_error("--fit_images: the tree has no packed accel to march");
            const double train_before = mean_psnr(train), held_before = mean_psnr(held);
            mnv_fit_params_ex p = fit_params;
            p.steps = (int32_t)fit_steps;
            subject.fit_ex(train_cams, train_images, march, p);
            const double train_after = mean_psnr(train), held_after = mean_psnr(held);
            std::printf("fit_images: %zu pose(s) fitted, %zu held out, %ld %s step(s), lr_colour %g, lr_sigma %g, batch %ld; PSNR of the fitted poses %.4f -> %.4f dB",
                        train.size(), held.size(), fit_steps, fit_adam ? "adam" : "sgd", (double)fit_lr_colour, (double)fit_lr_sigma, fit_batch, train_before, train_after);
            if (!held.empty()) std::printf(", of the held-out poses %.4f -> %.4f dB", held_before, held_after);
            std::printf("\n");
            if (args.has("save_lod")) {
                subject.save_npz(args.get("save_lod", ""));
                std::printf("save_lod: %d of %d chunks -> %s\n", subject.capacity, tree.capacity, args.get("save_lod", "").c_str());
            }
            rend.set(subject, fit_owner ? (long)subject.capacity : max_capacity);  // the frames below show the fitted tree
        }
        if (lod > 0 && !args.has("fit_images")) {
            if (tree.N <= 0) throw std::runtime_error("--lod needs a tree (N > 0)");
            rend.set_lod((int)lod);
            if (args.has("save_lod")) {
                const std::unique_ptr<viewer::N3Tree> cut = tree.make_lod((int)lod);
                fit_cut(*cut);
                cut->save_npz(args.get("save_lod", ""));
                std::printf("save_lod: depth %ld, %d of %d chunks -> %s\n", lod, cut->capacity, tree.capacity, args.get("save_lod", "").c_str());
            }
        }
        if (args.has("lod_pixels") && !args.has("fit_images")) {
            if (tree.N <= 0) throw std::runtime_error("--lod_pixels needs a tree (N > 0)");
            // the eye of every pose this run renders: the frame loop below, stepped on a copy of the camera
            std::vector<mnv_lod_view> views;
            viewer::Camera walk = rend.camera;
            for (long f = 0; f < std::max<long>(frames, 1) && views.size() < 4096; ++f) {
                views.push_back({{walk.center.x, walk.center.y, walk.center.z}, std::max(walk.fx, walk.fy)});
                if (orbit == 0.0) break;  // (every frame has the same pose)
                orbit_step(walk, orbit);
            }
            if (orbit != 0.0 && frames > 4096) throw std::runtime_error("--lod_pixels serves at most 4096 poses (--frames)");
            rend.set_view_lod(views, lod_pixels, (int)lod_min, (int)lod_max);
            int64_t kept[24];
            const std::unique_ptr<viewer::N3Tree> cut = tree.make_view_lod(views, lod_pixels, (int)lod_min, (int)lod_max, nullptr, kept);
            std::printf("lod_pixels: %g pixels, %zu view(s), %d of %d chunks, kept per depth:", (double)lod_pixels, views.size(), cut->capacity, tree.capacity);
            for (int d = 1; d < 24 && kept[d] > 0; ++d) std::printf(" %lld", (long long)kept[d]);
            std::printf("\n");
            if (args.has("save_lod")) {
                fit_cut(*cut);
                cut->save_npz(args.get("save_lod", ""));
                std::printf("save_lod: %d of %d chunks -> %s\n", cut->capacity, tree.capacity, args.get("save_lod", "").c_str());
            }
        }
        if (args.has("cull")) {
            if (tree.N <= 0) throw std::runtime_error("--cull needs a tree (N > 0)");
            // the camera of every pose this run renders: the frame loop below, stepped on a copy of the camera
            std::vector<mnv_camera> cams;
            viewer::Camera walk = rend.camera;
            for (long f = 0; f < std::max<long>(frames, 1) && cams.size() < 4096; ++f) {
                walk._update();
                cams.push_back(walk.c_abi());
                if (orbit == 0.0) break;  // (every frame has the same pose)
                orbit_step(walk, orbit);
            }
            if (orbit != 0.0 && frames > 4096) throw std::runtime_error("--cull serves at most 4096 poses (--frames)");
            rend.set_cull(cams, cull_thresh);
            int64_t kept[24];
            mnv_cull_counts cc;
            mnv_render_options march = *rend.options.c_abi();
            march.render_depth = false;
            const std::unique_ptr<viewer::N3Tree> cut = tree.make_culled(cams, march, cull_thresh, nullptr, kept, &cc);
            // the chunks per depth before: a walk over the host links
            int64_t before[24] = {0};
            std::vector<std::pair<int32_t, int>> todo{{0, 1}};
            while (!todo.empty()) {
                const auto [c, d] = todo.back();
                todo.pop_back();
                if (d < 24) ++before[d];
                for (int j = 0; j < 8; ++j) {
                    const int32_t ch = tree.child[(size_t)c * 8 + j];
                    if (ch != 0) todo.push_back({c + ch, d + 1});
                }
            }
            std::printf("cull: weight_thresh %g, %zu pose(s), %d of %d chunks, chunks per depth before:", (double)cull_thresh, cams.size(), cut->capacity, tree.capacity);
            for (int d = 1; d < 24 && before[d] > 0; ++d) std::printf(" %lld", (long long)before[d]);
            std::printf(", kept per depth:");
            for (int d = 1; d < 24 && kept[d] > 0; ++d) std::printf(" %lld", (long long)kept[d]);
            std::printf("; leaves seen %lld, non-empty leaves culled %lld, dead chunks %lld\n", (long long)cc.leaves_seen, (long long)cc.leaves_culled,
                        (long long)cc.dead_chunks);
            if (args.has("save_lod")) {
                cut->save_npz(args.get("save_lod", ""));
                std::printf("save_lod: %d of %d chunks -> %s\n", cut->capacity, tree.capacity, args.get("save_lod", "").c_str());
            }
        }
        // --target: one device image per frame slot, filled before the frame that takes the slot is issued
        const std::string target = args.get("target", ""), target_mask = args.get("target_mask", "");
        const bool score = !target.empty(), ssim = args.has("ssim");
        const int score_flags = MNV_METRIC_QUANTISED | (target_mask.empty() ? 0 : MNV_METRIC_MASK_ALPHA) | (ssim ? MNV_METRIC_SSIM : 0);
        const size_t frame_px = (size_t)width * height;
        std::vector<mnv::Buffer<uint8_t>> target_dev(score ? (size_t)rend.frames_in_flight : 0);
        std::vector<uint8_t> target_rgb, target_alpha, target_rgba;
        auto load_target = [&](long f, int slot) {
            char name[4096];
            int32_t w = 0, h = 0, ch = 0;
            std::snprintf(name, sizeof(name), "%s_%04ld.ppm", target.c_str(), f);
            target_rgb.resize(frame_px * 3);
            mnv_ok(mnv_pnm_read(name, width, height, target_rgb.data(), (int64_t)target_rgb.size(), &w, &h, &ch), "--target");
            if (ch != 3) throw std::runtime_error(std::string("--target: ") + name + " is not a P6 file");
            target_alpha.assign(frame_px, 255);
            if (!target_mask.empty()) {
                std::snprintf(name, sizeof(name), "%s_%04ld.pgm", target_mask.c_str(), f);
                mnv_ok(mnv_pnm_read(name, width, height, target_alpha.data(), (int64_t)target_alpha.size(), &w, &h, &ch), "--target_mask");
                if (ch != 1) throw std::runtime_error(std::string("--target_mask: ") + name + " is not a P5 file");
            }
            target_rgba.resize(frame_px * 4);
            for (size_t p = 0; p < frame_px; ++p) {
                target_rgba[p * 4 + 0] = target_rgb[p * 3 + 0];
                target_rgba[p * 4 + 1] = target_rgb[p * 3 + 1];
                target_rgba[p * 4 + 2] = target_rgb[p * 3 + 2];
                target_rgba[p * 4 + 3] = target_alpha[p];
            }
            if (!target_dev[slot]) hip_ok(target_dev[slot].alloc(frame_px * 4), "hipMalloc(target image)");
            hip_ok(hipMemcpy(target_dev[slot].get(), target_rgba.data(), frame_px * 4, hipMemcpyHostToDevice), "upload target image");
            rend.set_target(target_dev[slot].get(), score_flags);
        };
        double psnr_sum = 0.0, ssim_sum = 0.0;
        long scored = 0;
        std::deque<std::pair<long, int>> pending;  // (frame, slot) rendered but not yet written
        auto write_oldest = [&]() {
            const long f = pending.front().first;
            const int slot = pending.front().second;
            pending.pop_front();
            if (score) {
                mnv_frame_metric_values m{};
                rend.slot_metrics(slot, &m);
                if (ssim)
                    std::printf("frame %ld: psnr %.4f ssim %.6f\n", f, m.psnr, m.ssim);
                else
                    std::printf("frame %ld: psnr %.4f\n", f, m.psnr);
                psnr_sum += m.psnr;
                ssim_sum += m.ssim;
                ++scored;
            }
            if (out.empty()) return;
            rend.download_slot(slot, args.has("raw") ? &rgba : nullptr, &rgba8);
            if (refine && rend.guided_in_flight) std::printf("frame %ld: guided samples %ld\n", f, rend.slot_guided_samples(slot));
            write_frame(out, f, width, height, rgba8.data(), args.has("raw") ? rgba.data() : nullptr);
        };
        const auto wall0 = std::chrono::steady_clock::now();
        for (long f = 0; f < frames; ++f) {
            // the slot frame f is about to take must have been written: the renderer says which one that is (frames that cannot
            // overlap -- refinement, a tree without a packed accel -- all take slot 0, whatever --in_flight says)
            const int next = rend.next_slot();
            size_t keep = pending.size();
            for (size_t i = 0; i < pending.size(); ++i)
                if (pending[i].second == next) keep = pending.size() - 1 - i;
            while (pending.size() > keep) write_oldest();
            if (score) load_target(f, next);
            rend.render();
            if (refine) print_refine_stats(f, rend.stats);
            if (!out.empty() || score) pending.emplace_back(f, rend.last_slot());
            if (orbit != 0.0) orbit_step(rend.camera, orbit);
        }
        while (!pending.empty()) write_oldest();
        rend.sync_tree_streams();
        if (score) {
            rend.set_target(nullptr);
            target_dev.clear();
            if (ssim)
                std::printf("mean over %ld frame(s): psnr %.4f ssim %.6f\n", scored, psnr_sum / std::max<long>(scored, 1), ssim_sum / std::max<long>(scored, 1));
            else
                std::printf("mean over %ld frame(s): psnr %.4f\n", scored, psnr_sum / std::max<long>(scored, 1));
        }
        const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        if (args.has("save_tree") && tree.N > 0) {
            rend.sync_tree();
            tree.save_npz(args.get("save_tree", ""));
        }
        std::printf("%s: %ld frame(s) %dx%d, %.3f ms/frame wall (%d in flight%s), %.1f Mrays/s\n", rend.get_backend(), frames,
                    width, height, wall_ms / std::max<long>(frames, 1), refine && !rend.overlaps_next() ? 1 : rend.frames_in_flight, out.empty() ? "" : ", incl. download + file output",
                    wall_ms > 0 ? (double)width * height * frames / wall_ms / 1e3 : 0.0);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mnv_render: %s\n", e.what());
        return 1;
    }
}
