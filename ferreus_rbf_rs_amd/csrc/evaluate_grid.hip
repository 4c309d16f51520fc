// See evaluate_grid.hpp: the coordinates of a slab of grid rows, one thread per row, grid-stride over SoA columns.
#include "evaluate_grid.hpp"

#include <algorithm>
#include <cmath>

#include "ferreus_bbfmm_hip.h"

namespace bbfmm {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void grid_coords_kernel(GridSpec g, int64_t r0, int64_t n, double *__restrict__ out,
                                                               int64_t ld) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        double x[3];
        grid_node(g, r0 + i, x);
        for (int a = 0; a < g.d; ++a) out[a * ld + i] = x[a];
    }
}

} // namespace

bool grid_from_abi(const ::bbfmm_grid *in, GridSpec *g) {
    if (!in || in->size < static_cast<int64_t>(sizeof(::bbfmm_grid)) || in->d < 1 || in->d > 3) return false;
    *g = GridSpec();
    g->d = in->d;
    int64_t rows = 1;
    for (int a = 0; a < g->d; ++a) {
        if (in->shape[a] < 0 || !std::isfinite(in->origin[a])) return false;
        g->shape[a] = in->shape[a];
        g->origin[a] = in->origin[a];
        if (in->shape[a] > 0 && rows > (int64_t(1) << 62) / in->shape[a]) return false;
        rows *= in->shape[a];
        for (int c = 0; c < g->d; ++c) {
            if (!std::isfinite(in->steps[a * 3 + c])) return false;
            g->steps[a * 3 + c] = in->steps[a * 3 + c];
        }
    }
    return true;
}

void grid_coords_host(const GridSpec &g, int64_t r0, int64_t n, double *out, int64_t ld) {
    for (int64_t i = 0; i < n; ++i) {
        double x[3];
        grid_node(g, r0 + i, x);
        for (int a = 0; a < g.d; ++a) out[a * ld + i] = x[a];
    }
}

int grid_coords_device(const GridSpec &g, int64_t r0, int64_t n, double *d_out, int64_t ld, hipStream_t stream) {
    if (n <= 0) return 0;
    const int blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
    hipLaunchKernelGGL(grid_coords_kernel, dim3(blocks), dim3(kThreads), 0, stream, g, r0, n, d_out, ld);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bbfmm
