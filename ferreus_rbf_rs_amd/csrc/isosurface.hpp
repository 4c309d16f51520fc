// Dense marching tetrahedra on the regularised-marching-tetrahedra (RMT) sampling lattice: the raw triangles of
// ferreus_rmt's build_isosurface with ClusterMethod::None, before clipping, cleaning and boundary closure, taken from
// every sample point of the extraction domain in one device pass instead of a CPU wavefront.  Contract: DESIGN.md
// "Isosurfaces on the RMT lattice"; numpy restatement: tests/isosurface_restatement.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace bbfmm {
namespace iso {

// ---- the reference's tables (ferreus_rmt/src/constants.rs; values checked against tests/golden/rmt_tables.json)
// IJK offsets of the 14 edges of a sample point; 0..6 are the edges it owns.
constexpr int kEdgeDeltas[14][3] = {{-1, 1, 0}, {-2, 0, 0}, {-1, -1, 0}, {0, 1, -1}, {-1, 0, -1}, {0, -1, -1}, {1, 0, -1},
                                    {1, -1, 0}, {2, 0, 0},  {1, 1, 0},   {0, -1, 1}, {1, 0, 1},   {0, 1, 1},   {-1, 0, 1}};
constexpr int kReverseEdge[14] = {7, 8, 9, 10, 11, 12, 13, 0, 1, 2, 3, 4, 5, 6};
// the 6 tetrahedra a sample point owns (edge labels of its 3 other corners)
constexpr int kOwnedTetEdges[6][3] = {{0, 4, 1}, {0, 3, 4}, {3, 6, 4}, {1, 4, 2}, {2, 4, 5}, {4, 6, 5}};
// tetrahedron edges as corner pairs
constexpr int kTetEdgePairs[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// marching-tetrahedra table: per case (bit i = corner i inside) its triangle count and up to 2 triangles of tet edges
constexpr int kMtCount[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
constexpr int kMtTable[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{3, 1, 2}, {3, 2, 4}},
    {{1, 3, 5}, {0, 0, 0}}, {{5, 2, 0}, {5, 0, 3}}, {{5, 1, 0}, {5, 0, 4}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{4, 0, 1}, {4, 1, 5}}, {{3, 0, 2}, {3, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{4, 2, 1}, {4, 1, 3}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};
constexpr int kPad = 2;             // OPEN_CLIP_IJK_PADDING (lattice.rs:119)
constexpr double kInsideEps = 1e-9; // is_inside (isosurface.rs:286-289)

// The extraction domain of (extents, resolution), host-side (SampleLattice::new, lattice.rs:55-96).
struct Lattice {
    double lo_world[3] = {0, 0, 0}, spacing[3] = {0, 0, 0};
    int64_t max_ijk[3] = {0, 0, 0};
    int64_t lo[3] = {0, 0, 0};   // ijk of entry (0, 0, 0) of a field array: the bounding box of E
    int64_t dims[3] = {0, 0, 0}; // ni, nj, nk of that box (arrays are (nk, nj, ni), i fastest)
    int64_t n_keys = 0, n_nodes = 0; // |K| and |E|
    // per row (j, k) of the box (index k * nj + j): the i ranges [begin, end] of E and of the keys (begin > end: none)
    std::vector<int32_t> e_rows, key_rows; // 2 ints per row
};

// Validates (finite extents with lo <= hi, finite resolution > 0, a lattice of at most 2^36 box nodes) and fills *out.
bool make_lattice(const double *extents, double resolution, Lattice *out, std::string *err);

// One mesh: row-major vertices (n x 3) and facets (m x 3).
struct Mesh {
    std::vector<double> vertices;
    std::vector<int64_t> facets;
};

// Field values at m lattice nodes (SoA world coordinates on the device), written to d_vals[0..m) on the stream.
// d_vals == nullptr: only check that every node can be evaluated (BBFMM_POINT_OUTSIDE_TREE otherwise).
using FieldFn = std::function<int(const double *d_x0, const double *d_x1, const double *d_x2, int64_t m, double *d_vals)>;

struct Request {
    const double *isovalues = nullptr;
    int n_iso = 0;
    const double *drift = nullptr;     // 4 values a, b0, b1, b2: a + b . x added to the field (null: none)
    const double *host_field = nullptr; // caller's field over the box of E (then no FieldFn is used)
    double *d_field_out = nullptr;     // device array over the box of E receiving the field (NaN off E), or null
    int64_t budget_bytes = 0;          // device memory for one batch of k-planes (<= 0: the default)
};

// Runs the extraction on `stream`.  Returns a bbfmm_status; *err holds the message of a failure.
int extract(const Lattice &lat, const FieldFn &field, const Request &req, hipStream_t stream, std::vector<Mesh> *out,
            std::string *err);

} // namespace iso
} // namespace bbfmm
