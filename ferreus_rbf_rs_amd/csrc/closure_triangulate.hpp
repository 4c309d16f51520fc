// The host part of the boundary closure (DESIGN.md "Boundary closure"): a constrained triangulation of the band of cut
// cells of one face of the extents.  Free of HIP, so that it runs and is tested without a device
// (bbfmm_debug_closure_triangulate, bbfmm_debug_orient2d).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bbfmm {
namespace iso {
namespace closure {

// The exact sign of det [b - a; c - a] on doubles (-1, 0, 1; 1: a, b, c counter-clockwise): the six products of the
// expanded determinant as FMA two-products, their twelve parts summed as an expansion.  No tolerance.
int orient2d_sign(const double *a, const double *b, const double *c);

// point_on_segment2 (boundary_closure.rs:780-789)
bool point_on_segment2(const double *p, const double *a, const double *b, double eps);

struct Band {
    // ---- in
    int32_t nu = 0, nv = 0;                    // cells along u and v
    const double *gu = nullptr, *gv = nullptr; // nu + 1 and nv + 1 grid coordinates
    const double *points = nullptr;            // n_points x 2: the mesh vertices on the face
    int64_t n_points = 0;
    const int64_t *edges = nullptr; // n_edges x 2 indices into points: the open edges
    int64_t n_edges = 0;
    const int32_t *cut = nullptr; // n_cut cut cells v * nu + u, ascending
    int64_t n_cut = 0;
    double tol = 0.0;      // 1e-9 * resolution
    double key_cell = 1.0; // max(eps, 1e-12): a grid point with the weld key of a mesh vertex is that vertex
    // ---- out
    std::vector<double> xy;   // 2 per band point
    std::vector<int64_t> id;  // per band point: the index of a mesh point, or -1 - (gv index * (nu + 1) + gu index)
    std::vector<int64_t> tri; // 3 band points per triangle, counter-clockwise
    int64_t dropped = 0, constraint_flips = 0, lawson_flips = 0;
};

// The band triangulated: exactly the union of the cut cells, with every open edge, every grid edge between a cut and a
// whole cell and the perimeter pieces as edges.  false with *err set where the constraints cannot be met.
bool triangulate_band(Band *band, std::string *err);

} // namespace closure
} // namespace iso
} // namespace bbfmm
