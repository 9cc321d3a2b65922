// extract.cpp -- viewer::N3Tree::extract_surface: the iso-surface of the density as a viewer::Mesh (mnv_extract_surface on the packed accel,
// downloaded).  A unit of its own: it is the one place where the tree model calls the surface entry points of the C ABI.
#include <string>

#include "mesh.hpp"
#include "n3tree.hpp"

namespace viewer {

Mesh N3Tree::extract_surface(int level, float iso, bool colour, void *hip_stream) const {
    if (!device.accel) throw StatusError(MNV_E_INVALID, "N3Tree::extract_surface: the tree has no packed accel (move_to_device first)");
    const mnv_extract_params prm = {level, iso, colour ? MNV_EXTRACT_COLOUR : 0};
    mnv_surface *s = nullptr;
    int rc = mnv_extract_surface(device.accel, &prm, hip_stream, &s);
    if (rc != MNV_OK) throw StatusError(rc, std::string("N3Tree::extract_surface: ") + mnv_last_error());
    int64_t nv = 0, ni = 0;
    mnv_surface_counts(s, &nv, &ni);
    Mesh m((int)nv, (int)(ni / 3), 3, false);
    rc = mnv_surface_download(s, m.vert.data(), (int64_t)m.vert.size(), m.faces.data(), (int64_t)m.faces.size());
    mnv_surface_destroy(s);
    if (rc != MNV_OK) throw StatusError(rc, std::string("N3Tree::extract_surface: ") + mnv_last_error());
    return m;
}

}  // namespace viewer
