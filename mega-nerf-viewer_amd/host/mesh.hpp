// mesh.hpp -- viewer::Mesh (reference include/mesh.hpp, src/mesh.cpp): a vertex list of 9 floats per vertex (position, colour, normal), an
// optional index list, face_size 1 / 2 / 3 (points, lines, triangles), a lit or unlit shader and an axis-angle / scale / translation model
// transform.  The GL objects of the reference become a device handle (mnv_mesh, include/mnv.h) that mnv_render_meshes draws; `draw` is
// VolumeRenderer's job (VolumeRenderer::meshes).
#pragma once

#include <string>
#include <vector>

#include "../../include/mnv.h"

namespace viewer {

// The model matrix of Mesh::draw (src/mesh.cpp:137-150), row-major 3 x 4: identity rotation when |rotation| < 1e-3, else
// angleAxis(|rotation|, rotation / |rotation|); times scale; translation in the fourth column.  In double, rounded to float once.
void model_matrix(const float rotation[3], const float translation[3], float scale, float out[12]);

struct Mesh {
    explicit Mesh(int n_verts = 0, int n_faces = 0, int face_size = 3, bool unshaded = false);
    ~Mesh();
    Mesh(Mesh &&o) noexcept;
    Mesh &operator=(Mesh &&o) noexcept;
    Mesh(const Mesh &) = delete;
    Mesh &operator=(const Mesh &) = delete;

    // Upload to GPU: creates the device handle, or refreshes it in place (arrays, model transform, visibility); the handle keeps its
    // address, so a renderer that lists it sees the new state.  Frames that draw the mesh must have finished.
    void update();
    // The model transform and `visible` alone (no upload); needs update() once before.
    void update_transform();
    // The device handle (null before update()); owned by this object.
    const mnv_mesh *handle() const { return handle_; }

    // A Wavefront OBJ file, read without a library: `v x y z [r g b]`, `vn`, `f` with the v, v/vt, v//vn and v/vt/vn forms and negative
    // indices (polygons are fanned), `l` polylines; everything else is skipped.
    //   faces with a normal at every corner: one vertex per distinct (v, vn) pair in order of first use, indexed triangles
    //   faces with a normal missing anywhere: face normals normalize((p1 - p0) x (p2 - p0)) of each fanned triangle ((0, 0, 1) when it
    //     has no area), three vertices of its own per triangle, non-indexed
    //   no faces but `l`: one vertex per `v` (normal 0, 0, 1), indexed segments, face_size 2
    //   neither: one point per `v`, non-indexed, face_size 1
    // A vertex without r g b takes `color`.  A file with both `f` and `l`, an index outside the file, a malformed number, a face with
    // fewer than three corners or a polyline with fewer than two: std::runtime_error naming "line N".
    static Mesh load_obj(const std::string &path, const float color[3] = nullptr, bool unlit = false);
    // The vertex and index lists as a Wavefront OBJ file (write_obj below); face_size 2 or 3.
    void save_obj(const std::string &path) const;

    // Vertex list: position, colour, normal
    std::vector<float> vert;
    // Indices, face_size per primitive (empty: non-indexed)
    std::vector<unsigned int> faces;

    // Model transform, rotation is axis-angle
    float rotation[3] = {0.f, 0.f, 0.f}, translation[3] = {0.f, 0.f, 0.f};
    float scale = 1.f;

    int face_size;
    bool visible = true;
    bool unlit = false;

private:
    mnv_mesh *handle_ = nullptr;
};

// mnv_obj_write (include/mnv.h): `v x y z r g b` and `vn x y z` per vertex, then `f a//a b//b c//c` or `l a b` per primitive, every float as
// %.9g (load_obj reads the same bits back).  StatusError(MNV_E_INVALID) for arrays that are no mesh, std::runtime_error when the file cannot
// be written.
void write_obj(const std::string &path, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int face_size);

}  // namespace viewer
