// The nodes of a regular grid (bbfmm_grid: a block model, a section, a volume) as evaluation targets.  One definition of
// a node's coordinate for the host entry and the kernel of evaluate_grid.hip: every product and sum rounded, in a fixed
// order, never fused -- the pattern of interpolant_terms.hpp, so that a numpy restatement equals both bit for bit.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BBFMM_GRID_HD __host__ __device__
#else
#define BBFMM_GRID_HD
#endif

struct bbfmm_grid; // ferreus_bbfmm_hip.h

namespace bbfmm {

// max_job_targets = -1 of bbfmm_evaluate_options: the cap measured best on full-size grids
constexpr int32_t kDefaultMaxJobTargets = 512;

// The checked copy of the ABI's struct.  Axes at or beyond d are absent: shape 1, no term.
struct GridSpec {
    int d = 3;
    int64_t shape[3] = {1, 1, 1};
    double origin[3] = {0, 0, 0};
    double steps[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; // row j: the world step of index j
    int64_t rows() const { return shape[0] * shape[1] * shape[2]; }
    int64_t plane() const { return shape[1] * shape[2]; } // rows of one value of the leading index
};
// false on a bad one (size, d, a negative shape, non-finite origin or steps, 2^62 rows or more)
bool grid_from_abi(const ::bbfmm_grid *in, GridSpec *g);

// Row r = (i0 n1 + i1) n2 + i2 (C order): x_a = ((origin_a + i0 S[0][a]) + i1 S[1][a]) + i2 S[2][a], the terms of the
// axes below d only.
BBFMM_GRID_HD inline void grid_node(const GridSpec &g, int64_t r, double *x) {
#pragma clang fp contract(off)
    int64_t i[3];
    i[2] = r % g.shape[2];
    r /= g.shape[2];
    i[1] = r % g.shape[1];
    i[0] = r / g.shape[1];
    for (int a = 0; a < g.d; ++a) {
        double s = g.origin[a];
        for (int j = 0; j < g.d; ++j) s = s + static_cast<double>(i[j]) * g.steps[j * 3 + a];
        x[a] = s;
    }
}

// Rows [r0, r0 + n) as SoA columns: column a at out + a * ld (host loop / one kernel on `stream`, nothing synchronised).
void grid_coords_host(const GridSpec &g, int64_t r0, int64_t n, double *out, int64_t ld);
int grid_coords_device(const GridSpec &g, int64_t r0, int64_t n, double *d_out, int64_t ld, hipStream_t stream);

} // namespace bbfmm
