// mesh.cpp -- viewer::Mesh: the model transform of Mesh::draw, the device handle and a small Wavefront OBJ reader.
#include "mesh.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <utility>

#include "n3tree.hpp"  // StatusError

namespace viewer {

void model_matrix(const float rotation[3], const float translation[3], float scale, float out[12]) {
    const double rx = rotation[0], ry = rotation[1], rz = rotation[2];
    const double norm = std::sqrt(rx * rx + ry * ry + rz * rz);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!(norm < 1e-3)) {  // glm::angleAxis(norm, rotation / norm) -> mat4_cast
        const double s = std::sin(norm * 0.5), w = std::cos(norm * 0.5);
        const double x = rx / norm * s, y = ry / norm * s, z = rz / norm * s;
        R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - w * z), R[2] = 2 * (x * z + w * y);
        R[3] = 2 * (x * y + w * z), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - w * x);
        R[6] = 2 * (x * z - w * y), R[7] = 2 * (y * z + w * x), R[8] = 1 - 2 * (x * x + y * y);
    }
    for (int c = 0; c < 3; ++c) {
        for (int k = 0; k < 3; ++k) out[c * 4 + k] = (float)(R[c * 3 + k] * (double)scale);
        out[c * 4 + 3] = translation[c];
    }
}

Mesh::Mesh(int n_verts, int n_faces, int face_size, bool unshaded)
    : vert((size_t)n_verts * 9), faces((size_t)n_faces * face_size), face_size(face_size), unlit(unshaded) {}

Mesh::~Mesh() {
    if (handle_) mnv_mesh_destroy(handle_);
}

Mesh::Mesh(Mesh &&o) noexcept { *this = std::move(o); }

Mesh &Mesh::operator=(Mesh &&o) noexcept {
    if (this != &o) {
        if (handle_) mnv_mesh_destroy(handle_);
        vert = std::move(o.vert);
        faces = std::move(o.faces);
        std::memcpy(rotation, o.rotation, sizeof(rotation));
        std::memcpy(translation, o.translation, sizeof(translation));
        scale = o.scale, face_size = o.face_size, visible = o.visible, unlit = o.unlit;
        handle_ = o.handle_;
        o.handle_ = nullptr;
    }
    return *this;
}

void Mesh::update() {
    const uint32_t *idx = faces.empty() ? nullptr : faces.data();
    const int rc = handle_ ? mnv_mesh_update(handle_, vert.data(), (int64_t)(vert.size() / 9), idx, (int64_t)faces.size(), face_size, unlit)
                           : mnv_mesh_create(vert.data(), (int64_t)(vert.size() / 9), idx, (int64_t)faces.size(), face_size, unlit, &handle_);
    if (rc != MNV_OK) throw StatusError(rc, std::string("Mesh::update: ") + mnv_last_error());
    update_transform();
}

void Mesh::update_transform() {
    if (!handle_) throw StatusError(MNV_E_INVALID, "Mesh::update_transform before update()");
    float M[12];
    model_matrix(rotation, translation, scale, M);
    mnv_mesh_model_matrix(handle_, M);
    mnv_mesh_show(handle_, visible ? 1 : 0);
}

namespace {

[[noreturn]] void fail(const std::string &path, int line, const std::string &what) {
    throw std::runtime_error(path + ": line " + std::to_string(line) + ": " + what);
}

bool parse_float(const std::string &s, float *out) {
    if (s.empty()) return false;
    char *end = nullptr;
    const float v = std::strtof(s.c_str(), &end);
    if (end != s.c_str() + s.size()) return false;
    *out = v;
    return true;
}

// one index of a corner ("7", "-1"): 1-based, negative = from the end; -> 0-based, or false
bool parse_index(const std::string &s, size_t count, long *out) {
    if (s.empty()) return false;
    char *end = nullptr;
    const long v = std::strtol(s.c_str(), &end, 10);
    if (end != s.c_str() + s.size() || v == 0) return false;
    const long k = v > 0 ? v - 1 : (long)count + v;
    if (k < 0 || k >= (long)count) return false;
    *out = k;
    return true;
}

struct Corner {
    long v = -1, vn = -1;
};

}  // namespace

Mesh Mesh::load_obj(const std::string &path, const float color[3], bool unlit) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error(path + ": cannot open");
    const float white[3] = {1.f, 1.f, 1.f};
    const float *def = color ? color : white;
    std::vector<float> pos, col, nrm;       // per `v`: xyz, rgb; per `vn`: xyz
    std::vector<Corner> tris;               // fanned triangles, three corners each
    std::vector<unsigned int> segs;         // polyline segments, two `v` indices each
    bool normals_everywhere = true;
    int first_face_line = 0, first_line_line = 0;
    std::string text;
    for (int line = 1; std::getline(in, text); ++line) {
        const size_t hash = text.find('#');
        if (hash != std::string::npos) text.resize(hash);
        std::istringstream ss(text);
        std::string tag;
        if (!(ss >> tag)) continue;
        std::vector<std::string> tok;
        for (std::string t; ss >> t;) tok.push_back(t);
        if (tag == "v") {
            if (tok.size() != 3 && tok.size() != 4 && tok.size() != 6) fail(path, line, "a vertex takes x y z [w] or x y z r g b");
            float f[6] = {0, 0, 0, def[0], def[1], def[2]};
            for (size_t i = 0; i < tok.size(); ++i) {
                float x;
                if (!parse_float(tok[i], &x)) fail(path, line, "malformed number '" + tok[i] + "'");
                if (tok.size() == 6 || i < 3) f[i] = x;
            }
            pos.insert(pos.end(), f, f + 3);
            col.insert(col.end(), f + 3, f + 6);
        } else if (tag == "vn") {
            if (tok.size() != 3) fail(path, line, "a normal takes x y z");
            for (const std::string &t : tok) {
                float x;
                if (!parse_float(t, &x)) fail(path, line, "malformed number '" + t + "'");
                nrm.push_back(x);
            }
        } else if (tag == "f" || tag == "l") {
            const bool face = tag == "f";
            if (face && !first_face_line) first_face_line = line;
            if (!face && !first_line_line) first_line_line = line;
            if (first_face_line && first_line_line) fail(path, line, "the file mixes faces (f) and polylines (l): one Mesh has one face_size");
            if (tok.size() < (face ? 3u : 2u)) fail(path, line, face ? "a face needs at least three corners" : "a polyline needs at least two vertices");
            std::vector<Corner> cs;
            for (const std::string &t : tok) {
                std::string part[3];
                int n = 0;
                for (char ch : t) {
                    if (ch == '/') {
                        if (++n > 2) fail(path, line, "malformed corner '" + t + "'");
                    } else {
                        part[n] += ch;
                    }
                }
                Corner c;
                if (!parse_index(part[0], pos.size() / 3, &c.v)) fail(path, line, "bad vertex index in '" + t + "'");
                if (n >= 1 && !part[1].empty()) {  // the texture index is checked for form only
                    char *end = nullptr;
                    (void)std::strtol(part[1].c_str(), &end, 10);
                    if (end != part[1].c_str() + part[1].size()) fail(path, line, "malformed corner '" + t + "'");
                }
                if (n == 2) {
                    if (!face || !parse_index(part[2], nrm.size() / 3, &c.vn)) fail(path, line, "bad normal index in '" + t + "'");
                } else if (face) {
                    normals_everywhere = false;
                }
                cs.push_back(c);
            }
            if (face) {
                for (size_t i = 1; i + 1 < cs.size(); ++i) tris.push_back(cs[0]), tris.push_back(cs[i]), tris.push_back(cs[i + 1]);
            } else {
                for (size_t i = 0; i + 1 < cs.size(); ++i) segs.push_back((unsigned)cs[i].v), segs.push_back((unsigned)cs[i + 1].v);
            }
        }
    }
    auto push_vertex = [&](Mesh &m, long v, const float n[3]) {
        m.vert.insert(m.vert.end(), pos.begin() + v * 3, pos.begin() + v * 3 + 3);
        m.vert.insert(m.vert.end(), col.begin() + v * 3, col.begin() + v * 3 + 3);
        m.vert.insert(m.vert.end(), n, n + 3);
    };
    const float up[3] = {0.f, 0.f, 1.f};
    Mesh m(0, 0, !tris.empty() ? 3 : !segs.empty() ? 2 : 1, unlit);
    if (!tris.empty() && normals_everywhere) {
        std::map<std::pair<long, long>, unsigned> seen;
        for (const Corner &c : tris) {
            auto it = seen.find({c.v, c.vn});
            if (it == seen.end()) {
                it = seen.emplace(std::make_pair(c.v, c.vn), (unsigned)(m.vert.size() / 9)).first;
                push_vertex(m, c.v, &nrm[c.vn * 3]);
            }
            m.faces.push_back(it->second);
        }
    } else if (!tris.empty()) {
        for (size_t t = 0; t + 2 < tris.size(); t += 3) {
            const float *p0 = &pos[tris[t].v * 3], *p1 = &pos[tris[t + 1].v * 3], *p2 = &pos[tris[t + 2].v * 3];
            const double a[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
            const double b[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
            const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
            const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            float n[3] = {0.f, 0.f, 1.f};
            if (len > 0)
                for (int k = 0; k < 3; ++k) n[k] = (float)(c[k] / len);
            for (int k = 0; k < 3; ++k) push_vertex(m, tris[t + k].v, n);
        }
    } else {
        for (size_t v = 0; v < pos.size() / 3; ++v) push_vertex(m, (long)v, up);
        m.faces = segs;
    }
    return m;
}

void write_obj(const std::string &path, const float *vert, int64_t n_verts, const uint32_t *faces, int64_t n_indices, int face_size) {
    if (n_verts < 0 || (n_verts > 0 && !vert)) throw StatusError(MNV_E_INVALID, "mnv_obj_write: null vertex array");
    if (n_indices < 0 || (n_indices > 0 && !faces)) throw StatusError(MNV_E_INVALID, "mnv_obj_write: null index array with a non-zero count");
    if (n_indices > 0 && face_size != 2 && face_size != 3) throw StatusError(MNV_E_INVALID, "mnv_obj_write: face_size must be 2 (lines) or 3 (triangles)");
    if (n_indices > 0 && n_indices % face_size != 0) throw StatusError(MNV_E_INVALID, "mnv_obj_write: the index count must be a multiple of face_size");
    for (int64_t i = 0; i < n_indices; ++i)
        if ((int64_t)faces[i] >= n_verts) throw StatusError(MNV_E_INVALID, "mnv_obj_write: a face index >= n_verts");
    std::FILE *f = std::fopen(path.c_str(), "w");
    if (!f) throw std::runtime_error(path + ": cannot open for writing");
    bool ok = true;
    for (int64_t i = 0; i < n_verts && ok; ++i) {
        const float *v = vert + i * 9;
        ok = std::fprintf(f, "v %.9g %.9g %.9g %.9g %.9g %.9g\n", v[0], v[1], v[2], v[3], v[4], v[5]) > 0;
    }
    for (int64_t i = 0; i < n_verts && ok; ++i) {
        const float *v = vert + i * 9;
        ok = std::fprintf(f, "vn %.9g %.9g %.9g\n", v[6], v[7], v[8]) > 0;
    }
    for (int64_t i = 0; i + face_size <= n_indices && ok; i += face_size) {
        if (face_size == 3) {
            const unsigned long a = faces[i] + 1ul, b = faces[i + 1] + 1ul, c = faces[i + 2] + 1ul;
            ok = std::fprintf(f, "f %lu//%lu %lu//%lu %lu//%lu\n", a, a, b, b, c, c) > 0;
        } else {
            ok = std::fprintf(f, "l %lu %lu\n", faces[i] + 1ul, faces[i + 1] + 1ul) > 0;
        }
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) throw std::runtime_error(path + ": write failed");
}

void Mesh::save_obj(const std::string &path) const {
    write_obj(path, vert.data(), (int64_t)(vert.size() / 9), faces.empty() ? nullptr : faces.data(), (int64_t)faces.size(), face_size);
}

}  // namespace viewer
