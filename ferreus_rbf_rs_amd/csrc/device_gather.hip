// Gather / scatter between the caller's row order and the tree's sorted order: HBM streaming.
#include "device_common.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ gather/scatter
__global__ void gather_weights_kernel(const double *__restrict__ w, int64_t ldw, const int32_t *__restrict__ order,
                                      int64_t N, double *__restrict__ ws) {
    const int k = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        ws[k * N + i] = w[k * ldw + order[i]];
}

__global__ void scatter_output_kernel(const double *__restrict__ os, int64_t n, const int32_t *__restrict__ perm,
                                      double *__restrict__ out, int64_t ldo, int accumulate) {
    const int k = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t dst = k * ldo + perm[i];
        if (accumulate)
            out[dst] += os[k * n + i];
        else
            out[dst] = os[k * n + i];
    }
}

__global__ void gather_rows_kernel(const double *__restrict__ src, int64_t ld_src, const int32_t *__restrict__ idx,
                                   int64_t n, double *__restrict__ dst, int64_t ld_dst) {
    const int c = blockIdx.y;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[c * ld_dst + i] = src[c * ld_src + idx[i]];
}

static inline int grid_for(int64_t n, int block) {
    int64_t g = (n + block - 1) / block;
    if (g > 2048) g = 2048; // 256 CUs x 8 blocks, grid-stride the rest
    if (g < 1) g = 1;
    return (int)g;
}

// the same for a subset of the sorted positions (a partition reads the weights of its subtree and halo only)
__global__ void gather_weights_subset_kernel(const double *__restrict__ w, int64_t ldw, const int32_t *__restrict__ order,
                                             const int32_t *__restrict__ pos, int64_t n_pos, int64_t N, double *__restrict__ ws) {
    const int k = blockIdx.y;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_pos; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = pos[t];
        ws[k * N + i] = w[k * ldw + order[i]];
    }
}
void launch_gather_weights_subset(const double *w, int64_t ldw, int K, const int32_t *order, const int32_t *pos, int64_t n_pos,
                                  int64_t N, double *w_sorted, hipStream_t s) {
    if (n_pos == 0) return;
    hipLaunchKernelGGL(gather_weights_subset_kernel, dim3(grid_for(n_pos, 256), K), dim3(256), 0, s, w, ldw, order, pos, n_pos, N,
                       w_sorted);
}

void launch_gather_weights(const double *w, int64_t ldw, int K, const int32_t *order, int64_t N, double *w_sorted,
                           hipStream_t s) {
    if (N == 0) return;
    hipLaunchKernelGGL(gather_weights_kernel, dim3(grid_for(N, 256), K), dim3(256), 0, s, w, ldw, order, N, w_sorted);
}
__global__ void scatter_parts_kernel(const double *__restrict__ all, ScatterParts parts, int64_t m_max, int K,
                                     const int32_t *__restrict__ order, double *__restrict__ out, int64_t ldo) {
    const int k = blockIdx.y;
    const int64_t n = parts.bound[parts.n] - parts.bound[0];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = parts.bound[0] + i; // sorted position
        int r = 0;
        while (r + 1 < parts.n && g >= parts.bound[r + 1]) ++r;
        out[k * ldo + order[g]] = all[((int64_t)r * K + k) * m_max + (g - parts.bound[r])];
    }
}
void launch_scatter_parts(const double *all, const ScatterParts &parts, int64_t m_max, int K, const int32_t *order, double *out,
                          int64_t ldo, hipStream_t s) {
    const int64_t n = parts.bound[parts.n] - parts.bound[0];
    if (n <= 0) return;
    hipLaunchKernelGGL(scatter_parts_kernel, dim3(grid_for(n, 256), K), dim3(256), 0, s, all, parts, m_max, K, order, out, ldo);
}

// out[i] = slots[0][i] + slots[1][i] + ... in that order (the coarse multipoles of a device group: every device adds the
// parts' partial sums in the same fixed order, so all of them hold the same bits)
__global__ void sum_slots_kernel(const double *__restrict__ slots, int n_slots, int64_t len, double *__restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
        double acc = slots[i];
        for (int g = 1; g < n_slots; ++g) acc += slots[(int64_t)g * len + i];
        out[i] = acc;
    }
}
void launch_sum_slots(const double *slots, int n_slots, int64_t len, double *out, hipStream_t s) {
    if (len <= 0 || n_slots < 1) return;
    hipLaunchKernelGGL(sum_slots_kernel, dim3(grid_for(len, 256)), dim3(256), 0, s, slots, n_slots, len, out);
}

void launch_scatter_output(const double *out_sorted, int64_t n, int K, const int32_t *perm, double *out, int64_t ldo,
                           int accumulate, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(scatter_output_kernel, dim3(grid_for(n, 256), K), dim3(256), 0, s, out_sorted, n, perm, out,
                       ldo, accumulate);
}
void launch_gather_rows(const double *src, int64_t ld_src, int ncols, const int32_t *idx, int64_t n, double *dst,
                        int64_t ld_dst, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(n, 256), ncols), dim3(256), 0, s, src, ld_src, idx, n, dst,
                       ld_dst);
}

} // namespace bbfmm
