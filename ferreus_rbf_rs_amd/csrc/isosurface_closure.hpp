// Boundary closure of a clipped and cleaned mesh on the six faces of the extents (ferreus_rmt/src/boundary_closure.rs;
// contract: DESIGN.md "Boundary closure"; numpy restatement: tests/isosurface_closure_restatement.py).  The regular part
// of the caps (whole cells, their regions, their vertices) is made on the device; only the band of cut cells along the
// contours goes to the host triangulator (closure_triangulate.hpp).
#pragma once
#include "isosurface.hpp"

namespace bbfmm {
namespace iso {

// Mesh::closure_stats (BBFMM_CLOSURE_* of the header)
enum ClosureStat : int {
    kCloOpen = 0,      // [0, 6) open edges per face
    kCloOffBox = 6,    // open edges with an empty face mask
    kCloCut = 7,       // [7, 13) cut cells per face
    kCloWholeKept = 13, // [13, 19) whole cells kept per face
    kCloRegions = 19,
    kCloBandPoints = 20,
    kCloBandKept = 21,
    kCloBandDropped = 22,
    kCloConstraintFlips = 23,
    kCloLawsonFlips = 24,
    kCloVerticesAdded = 25,
    kCloConflicts = 26,
    kCloBandHostUs = 27,
    kCloStats = 32
};

// axis_grid_coordinates (boundary_closure.rs:816-828): false with *err set for more than 2^31 - 2 intervals.
bool closure_axis(double lo, double hi, double resolution, double eps, std::vector<double> *out, std::string *err);

// The closure of the finished mesh on the device (d_vertices: nv x 3, d_facets: nf x 3 ids below nv), mode
// kFinishClosePositive or kFinishCloseNegative: the closed mesh and its closure_stats go to *mesh on the host in one
// download.  Returns a bbfmm_status.
int closure_device(const double *d_vertices, int64_t nv, const int64_t *d_facets, int64_t nf, const ClipBox &box,
                   double resolution, int mode, hipStream_t stream, Mesh *mesh, std::string *err);

} // namespace iso
} // namespace bbfmm
