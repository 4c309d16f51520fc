// See solver_vectors.hpp.
#include "solver_vectors.hpp"

// The products and sums below round separately, like the loops of the host solver: no fused multiply-add.
#pragma clang fp contract(off)

namespace bbfmm {

namespace {
__device__ inline double mul_rn(double a, double b) { return a * b; }
__device__ inline double add_rn(double a, double b) { return a + b; }
__device__ inline double sub_rn(double a, double b) { return a - b; }

constexpr int kThreads = 1024;                                   // 16 waves: one block per chunk of 65,536 elements
constexpr int kPairsPerThread = kSolverChunk / (2 * kThreads);   // 32
constexpr int kWaves = kThreads / 64;

__device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// elements i, i + 1 of p (i even relative to the chunk, whose first element is a multiple of 65,536): one 16-byte access
// when `vec` says every pointer of the launch is 16-byte aligned, two 8-byte ones otherwise; have1: i + 1 < n
__device__ inline void load2(const double *__restrict__ p, int64_t i, bool vec, bool have1, double &v0, double &v1) {
    if (vec && have1) {
        const double2 t = *reinterpret_cast<const double2 *>(p + i);
        v0 = t.x, v1 = t.y;
    } else {
        v0 = p[i];
        v1 = have1 ? p[i + 1] : 0.0;
    }
}
__device__ inline void store2(double *__restrict__ p, int64_t i, bool vec, bool have1, double v0, double v1) {
    if (vec && have1) {
        *reinterpret_cast<double2 *>(p + i) = make_double2(v0, v1);
    } else {
        p[i] = v0;
        if (have1) p[i + 1] = v1;
    }
}

__device__ inline double read_alpha(const double *__restrict__ slot, int32_t mode, double imm) {
    if (mode == kAlphaImmediate) return imm;
    const double a = *slot;
    if (mode == kAlphaNegSlot) return -a;
    if (mode == kAlphaInvSlot) return a != 0.0 ? __ddiv_rn(1.0, a) : 0.0;
    return a;
}

// The block's value from its threads': lanes by shuffles (32, 16, .. 1), the waves in wave order.  Thread 0 returns it.
template <bool kMax> __device__ inline double block_reduce(double v, double *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = kMax ? fmax(v, o) : add_rn(v, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads(); // (lds may still be read by the block's previous reduction)
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = lds[0];
        for (int w = 1; w < kWaves; ++w) r = kMax ? fmax(r, lds[w]) : add_rn(r, lds[w]);
    }
    return r;
}

__global__ __launch_bounds__(kThreads) void sub_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                       double *__restrict__ y, int64_t n, double *__restrict__ part_sum,
                                                       double *__restrict__ part_max) {
    __shared__ double lds[kWaves];
    const bool vec = aligned16(a) && aligned16(b) && aligned16(y);
    const int64_t base = (int64_t)blockIdx.x * kSolverChunk;
    double sum = 0.0, mx = 0.0;
    for (int it = 0; it < kPairsPerThread; ++it) {
        const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 2;
        if (i >= n) break;
        const bool have1 = i + 1 < n;
        double a0, a1, b0, b1;
        load2(a, i, vec, have1, a0, a1);
        load2(b, i, vec, have1, b0, b1);
        const double y0 = sub_rn(a0, b0), y1 = sub_rn(a1, b1);
        store2(y, i, vec, have1, y0, y1);
        sum = add_rn(sum, mul_rn(y0, y0));
        mx = fmax(mx, fabs(y0));
        if (have1) {
            sum = add_rn(sum, mul_rn(y1, y1));
            mx = fmax(mx, fabs(y1));
        }
    }
    if (part_sum) {
        const double r = block_reduce<false>(sum, lds);
        if (threadIdx.x == 0) part_sum[blockIdx.x] = r;
    }
    if (part_max) {
        const double r = block_reduce<true>(mx, lds);
        if (threadIdx.x == 0) part_max[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(kThreads) void scale_kernel(const double *__restrict__ x, const double *__restrict__ slot,
                                                         int32_t mode, double imm, double *__restrict__ y, int64_t n) {
    const bool vec = aligned16(x) && aligned16(y);
    const double alpha = read_alpha(slot, mode, imm);
    const int64_t base = (int64_t)blockIdx.x * kSolverChunk;
    for (int it = 0; it < kPairsPerThread; ++it) {
        const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 2;
        if (i >= n) break;
        const bool have1 = i + 1 < n;
        double x0, x1;
        load2(x, i, vec, have1, x0, x1);
        store2(y, i, vec, have1, mul_rn(alpha, x0), mul_rn(alpha, x1));
    }
}

// (x, y and d never alias in the drivers; y is read and written by the same thread)
__global__ __launch_bounds__(kThreads) void axpy_reduce_kernel(const double *__restrict__ x, const double *__restrict__ slot,
                                                               int32_t mode, double imm, double *__restrict__ y,
                                                               const double *__restrict__ d, int64_t n, int32_t reduce,
                                                               double *__restrict__ part) {
    __shared__ double lds[kWaves];
    const bool vec = aligned16(y) && (!x || aligned16(x)) && (!d || aligned16(d));
    const double alpha = x ? read_alpha(slot, mode, imm) : 0.0;
    const int64_t base = (int64_t)blockIdx.x * kSolverChunk;
    double acc = 0.0;
    for (int it = 0; it < kPairsPerThread; ++it) {
        const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 2;
        if (i >= n) break;
        const bool have1 = i + 1 < n;
        double y0, y1;
        load2(y, i, vec, have1, y0, y1);
        if (x) {
            double x0, x1;
            load2(x, i, vec, have1, x0, x1);
            y0 = add_rn(y0, mul_rn(alpha, x0));
            y1 = add_rn(y1, mul_rn(alpha, x1));
            store2(y, i, vec, have1, y0, y1);
        }
        if (reduce == kReduceDot) {
            double d0 = y0, d1 = y1;
            if (d) load2(d, i, vec, have1, d0, d1);
            acc = add_rn(acc, mul_rn(d0, y0));
            if (have1) acc = add_rn(acc, mul_rn(d1, y1));
        } else if (reduce == kReduceMax) {
            acc = fmax(acc, fabs(y0));
            if (have1) acc = fmax(acc, fabs(y1));
        }
    }
    if (reduce == kReduceDot) {
        const double r = block_reduce<false>(acc, lds);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    } else if (reduce == kReduceMax) {
        const double r = block_reduce<true>(acc, lds);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    }
}

__global__ void reduce_finish_kernel(const double *__restrict__ part, int64_t n_chunks, int take_max, int take_sqrt,
                                     double *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double r = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) r = take_max ? fmax(r, part[c]) : add_rn(r, part[c]);
    *out = take_sqrt ? __dsqrt_rn(r) : r;
}

__global__ __launch_bounds__(kThreads) void update_kernel(const double *__restrict__ z, int64_t ldz, const double *__restrict__ y,
                                                          int32_t count, double *__restrict__ x, int64_t n) {
    const bool vec = aligned16(x) && aligned16(z) && (ldz & 1) == 0;
    const int64_t base = (int64_t)blockIdx.x * kSolverChunk;
    for (int it = 0; it < kPairsPerThread; ++it) {
        const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 2;
        if (i >= n) break;
        const bool have1 = i + 1 < n;
        double x0, x1;
        load2(x, i, vec, have1, x0, x1);
        for (int32_t c = 0; c < count; ++c) {
            const double yc = y[c];
            double z0, z1;
            load2(z + (int64_t)c * ldz, i, vec, have1, z0, z1);
            x0 = add_rn(x0, mul_rn(yc, z0));
            x1 = add_rn(x1, mul_rn(yc, z1));
        }
        store2(x, i, vec, have1, x0, x1);
    }
}

__global__ __launch_bounds__(256) void rbf_system_tail_kernel(const double *__restrict__ x, const double *__restrict__ P, int64_t ldp,
                                                              int32_t basis, double nugget, int64_t N, double *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N + basis) return;
    if (i >= N) {
        y[i] = 0.0;
        return;
    }
    double v = add_rn(y[i], mul_rn(x[i], nugget));
    if (basis > 0) {
        double sacc = 0.0;
        for (int32_t q = 0; q < basis; ++q) sacc = add_rn(sacc, mul_rn(P[(int64_t)q * ldp + i], x[N + q]));
        v = add_rn(v, sacc);
    }
    y[i] = v;
}

__global__ void set_tail_kernel(SolverTail t, int32_t count, double *__restrict__ out) {
    const int i = threadIdx.x;
    if (i < count) out[i] = t.v[i];
}

inline unsigned grid_of(int64_t n) { return static_cast<unsigned>(solver_chunks(n)); }
} // namespace

void launch_solver_sub(const double *a, const double *b, double *y, int64_t n, double *part_sum, double *part_max, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(sub_kernel, dim3(grid_of(n)), dim3(kThreads), 0, s, a, b, y, n, part_sum, part_max);
}

void launch_solver_scale(const double *x, const double *slot, int32_t mode, double imm, double *y, int64_t n, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(scale_kernel, dim3(grid_of(n)), dim3(kThreads), 0, s, x, slot, mode, imm, y, n);
}

void launch_solver_axpy_reduce(const double *x, const double *slot, int32_t mode, double imm, double *y, const double *d, int64_t n,
                               int32_t reduce, double *part, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(axpy_reduce_kernel, dim3(grid_of(n)), dim3(kThreads), 0, s, x, slot, mode, imm, y, d, n, reduce, part);
}

void launch_solver_reduce_finish(const double *part, int64_t n_chunks, bool take_max, bool take_sqrt, double *out, hipStream_t s) {
    hipLaunchKernelGGL(reduce_finish_kernel, dim3(1), dim3(64), 0, s, part, n_chunks, take_max ? 1 : 0, take_sqrt ? 1 : 0, out);
}

void launch_solver_update(const double *z, int64_t ldz, const double *y, int32_t count, double *x, int64_t n, hipStream_t s) {
    if (n < 1 || count < 1) return;
    hipLaunchKernelGGL(update_kernel, dim3(grid_of(n)), dim3(kThreads), 0, s, z, ldz, y, count, x, n);
}

void launch_rbf_system_tail(const double *x, const double *P, int64_t ldp, int32_t basis, double nugget, int64_t N, double *y,
                            hipStream_t s) {
    const int64_t total = N + basis;
    if (total < 1) return;
    hipLaunchKernelGGL(rbf_system_tail_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, x, P, ldp, basis,
                       nugget, N, y);
}

void launch_solver_set_tail(SolverTail t, int32_t count, double *out, hipStream_t s) {
    if (count < 1) return;
    hipLaunchKernelGGL(set_tail_kernel, dim3(1), dim3(64), 0, s, t, count, out);
}

} // namespace bbfmm
