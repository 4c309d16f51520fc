// Kernels of interpolant_terms.hpp: the global trend's map of the targets, the polynomial part and the trend's chain
// rule on gradients, one thread per target, grid-stride over SoA columns (bandwidth-bound streaming); and
// remove_duplicates on a uniform grid: rocPRIM sort by cell key, then rounds to the fixed point of the sequential
// greedy rule.  No floating-point atomics and no dependence on thread order anywhere.
#include "interpolant_terms.hpp"

#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

namespace bbfmm {

namespace {

constexpr int kThreads = 256;

int grid_for(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
}

// Device allocations of one call, freed on every exit.
struct Pool {
    std::vector<void *> ptrs;
    ~Pool() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T> hipError_t get(T **p, size_t n) {
        *p = nullptr;
        if (n == 0) n = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
};

#define TERMS_HIP(call)                                                                                                                  \
    do {                                                                                                                                 \
        if ((call) != hipSuccess) return 1;                                                                                              \
    } while (0)

__global__ __launch_bounds__(kThreads) void affine_points_kernel(InterpolantTerms t, const double *__restrict__ x, int64_t m,
                                                                 double *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads)
        affine_row(t, x, m, out, m, i);
}

// trend_gradients, nugget * w and polynomial_terms, each optional, in _evaluate's order (rbf.rs:1221-1266)
__global__ __launch_bounds__(kThreads) void interpolant_terms_kernel(InterpolantTerms t, const double *__restrict__ x, int64_t m,
                                                                     double *__restrict__ values, double *__restrict__ grad,
                                                                     int trend, int poly, double nugget,
                                                                     const double *__restrict__ w) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        if (trend) trend_gradients_row(t, grad, m, i);
        if (w)
            for (int c = 0; c < t.k; ++c) values[c * m + i] = values[c * m + i] + w[c * m + i] * nugget;
        if (poly) polynomial_row(t, x, m, values, m, grad, m, i);
    }
}

// Host columns (leading dimension ld) to a packed device array of `cols` columns of m, and back.
hipError_t columns_up(double *dst, const double *src, int64_t ld, int64_t m, int cols) {
    return hipMemcpy2D(dst, sizeof(double) * (size_t)m, src, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)m, (size_t)cols,
                       hipMemcpyHostToDevice);
}
hipError_t columns_down(double *dst, int64_t ld, const double *src, int64_t m, int cols) {
    return hipMemcpy2D(dst, sizeof(double) * (size_t)ld, src, sizeof(double) * (size_t)m, sizeof(double) * (size_t)m, (size_t)cols,
                       hipMemcpyDeviceToHost);
}

int terms_pass(const InterpolantTerms &t_host, const double *x, int64_t m, int64_t ldx, double *values, int64_t ldv, double *grad,
               int64_t ldg, int trend, int poly, double nugget, const double *w, int64_t ldw) {
    if (m == 0) return 0;
    if ((poly || w) && !values) return 1;
    Pool pool;
    InterpolantTerms t = t_host;
    const int nb = terms_basis_size(t.d, t.degree);
    double *dx = nullptr, *dv = nullptr, *dg = nullptr, *dw = nullptr, *dl = nullptr;
    if (poly && nb > 0) {
        if (!x || !t_host.lambda) return 1;
        TERMS_HIP(pool.get(&dl, (size_t)nb * t.k));
        TERMS_HIP(hipMemcpy2D(dl, sizeof(double) * nb, t_host.lambda, sizeof(double) * (size_t)t_host.ld_lambda, sizeof(double) * nb,
                              (size_t)t.k, hipMemcpyHostToDevice));
        t.lambda = dl;
        t.ld_lambda = nb;
        TERMS_HIP(pool.get(&dx, (size_t)m * t.d));
        TERMS_HIP(columns_up(dx, x, ldx, m, t.d));
    } else {
        poly = 0;
    }
    if (values) {
        TERMS_HIP(pool.get(&dv, (size_t)m * t.k));
        TERMS_HIP(columns_up(dv, values, ldv, m, t.k));
    }
    if (grad) {
        TERMS_HIP(pool.get(&dg, (size_t)m * t.k * t.d));
        TERMS_HIP(columns_up(dg, grad, ldg, m, t.k * t.d));
    }
    if (w) {
        TERMS_HIP(pool.get(&dw, (size_t)m * t.k));
        TERMS_HIP(columns_up(dw, w, ldw, m, t.k));
    }
    hipLaunchKernelGGL(interpolant_terms_kernel, dim3(grid_for(m)), dim3(kThreads), 0, 0, t, dx, m, dv, dg, trend && dg ? 1 : 0, poly,
                       nugget, dw);
    TERMS_HIP(hipGetLastError());
    TERMS_HIP(hipDeviceSynchronize());
    if (values && (poly || w)) TERMS_HIP(columns_down(values, ldv, dv, m, t.k));
    if (grad && (poly || trend)) TERMS_HIP(columns_down(grad, ldg, dg, m, t.k * t.d));
    return 0;
}

} // namespace

int terms_affine_device(const InterpolantTerms &t, const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo) {
    if (m == 0) return 0;
    Pool pool;
    double *dx = nullptr, *dy = nullptr;
    TERMS_HIP(pool.get(&dx, (size_t)m * t.d));
    TERMS_HIP(pool.get(&dy, (size_t)m * t.d));
    TERMS_HIP(columns_up(dx, x, ldx, m, t.d));
    hipLaunchKernelGGL(affine_points_kernel, dim3(grid_for(m)), dim3(kThreads), 0, 0, t, dx, m, dy);
    TERMS_HIP(hipGetLastError());
    TERMS_HIP(hipDeviceSynchronize());
    TERMS_HIP(columns_down(out, ldo, dy, m, t.d));
    return 0;
}

int terms_polynomial_device(const InterpolantTerms &t, const double *x, int64_t m, int64_t ldx, double *values, int64_t ldv,
                            double *grad, int64_t ldg) {
    return terms_pass(t, x, m, ldx, values, ldv, grad, ldg, 0, 1, 0.0, nullptr, 0);
}

int terms_trend_gradients_device(const InterpolantTerms &t, int64_t m, double *grad, int64_t ldg) {
    return terms_pass(t, nullptr, m, 0, nullptr, 0, grad, ldg, 1, 0, 0.0, nullptr, 0);
}

int terms_finish_device(const InterpolantTerms &t, const double *x, int64_t m, int64_t ldx, double *values, int64_t ldv,
                        double *grad, int64_t ldg, double nugget, const double *w, int64_t ldw) {
    return terms_pass(t, x, m, ldx, values, ldv, grad, ldg, t.has_affine, 1, nugget, w, ldw);
}

// ---- device-resident targets (one column; the coordinate arrays past t.d are not read and may be null)

namespace {

__global__ __launch_bounds__(kThreads) void affine_soa_kernel(InterpolantTerms t, const double *__restrict__ x0,
                                                              const double *__restrict__ x1, const double *__restrict__ x2, int64_t m,
                                                              double *__restrict__ y0, double *__restrict__ y1, double *__restrict__ y2) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        const double p[3] = {x0[i], t.d > 1 ? x1[i] : 0.0, t.d > 2 ? x2[i] : 0.0};
        double q[3];
        affine_point(t, p, q);
        y0[i] = q[0];
        if (t.d > 1) y1[i] = q[1];
        if (t.d > 2) y2[i] = q[2];
    }
}

__global__ __launch_bounds__(kThreads) void field_soa_kernel(InterpolantTerms t, const double *__restrict__ x0,
                                                             const double *__restrict__ x1, const double *__restrict__ x2, int64_t m,
                                                             double *__restrict__ vals, double *__restrict__ grad) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        const double p[3] = {x0[i], t.d > 1 ? x1[i] : 0.0, t.d > 2 ? x2[i] : 0.0};
        double v = vals[i], g[3] = {0, 0, 0};
        if (grad) {
            for (int a = 0; a < t.d; ++a) g[a] = grad[a * m + i];
            if (t.has_affine) trend_gradient_column(t, g);
        }
        double mono[kMaxMonomials], dm[kMaxMonomials][3];
        const int nb = monomials_and_gradients(t, p, mono, grad ? dm : nullptr);
        if (nb > 0) polynomial_column(t, nb, mono, dm, 0, &v, grad ? g : nullptr);
        vals[i] = v;
        if (grad)
            for (int a = 0; a < t.d; ++a) grad[a * m + i] = g[a];
    }
}

// t.k columns: value column c at vals + c * ldv, gradient column c * t.d + a at grad + (c * t.d + a) * ldg; per point and
// column the arithmetic of field_soa_kernel (the monomials are formed once per point)
__global__ __launch_bounds__(kThreads) void field_soa_k_kernel(InterpolantTerms t, const double *__restrict__ x0,
                                                               const double *__restrict__ x1, const double *__restrict__ x2, int64_t m,
                                                               double *__restrict__ vals, int64_t ldv, double *__restrict__ grad,
                                                               int64_t ldg) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        const double p[3] = {x0[i], t.d > 1 ? x1[i] : 0.0, t.d > 2 ? x2[i] : 0.0};
        double mono[kMaxMonomials], dm[kMaxMonomials][3];
        const int nb = monomials_and_gradients(t, p, mono, grad ? dm : nullptr);
        for (int c = 0; c < t.k; ++c) {
            double v = vals[c * ldv + i], g[3] = {0, 0, 0};
            if (grad) {
                for (int a = 0; a < t.d; ++a) g[a] = grad[(c * t.d + a) * ldg + i];
                if (t.has_affine) trend_gradient_column(t, g);
            }
            if (nb > 0) polynomial_column(t, nb, mono, dm, c, &v, grad ? g : nullptr);
            vals[c * ldv + i] = v;
            if (grad)
                for (int a = 0; a < t.d; ++a) grad[(c * t.d + a) * ldg + i] = g[a];
        }
    }
}

} // namespace

int terms_field_soa_device_k(const InterpolantTerms &t, const double *x0, const double *x1, const double *x2, int64_t m, double *vals,
                             int64_t ldv, double *grad, int64_t ldg, hipStream_t stream) {
    if (m <= 0) return 0;
    if (t.d < 1 || t.d > 3 || t.k < 1 || !vals || ldv < m || (grad && ldg < m) || !x0 || (t.d > 1 && !x1) || (t.d > 2 && !x2)) return 1;
    hipLaunchKernelGGL(field_soa_k_kernel, dim3(grid_for(m)), dim3(kThreads), 0, stream, t, x0, x1, x2, m, vals, ldv, grad, ldg);
    TERMS_HIP(hipGetLastError());
    return 0;
}

int terms_affine_soa_device(const InterpolantTerms &t, const double *x0, const double *x1, const double *x2, int64_t m, double *y0,
                            double *y1, double *y2, hipStream_t stream) {
    if (m <= 0) return 0;
    if (t.d < 1 || t.d > 3 || !x0 || !y0 || (t.d > 1 && (!x1 || !y1)) || (t.d > 2 && (!x2 || !y2))) return 1;
    hipLaunchKernelGGL(affine_soa_kernel, dim3(grid_for(m)), dim3(kThreads), 0, stream, t, x0, x1, x2, m, y0, y1, y2);
    TERMS_HIP(hipGetLastError());
    return 0;
}

int terms_field_soa_device(const InterpolantTerms &t, const double *x0, const double *x1, const double *x2, int64_t m, double *vals,
                           double *grad, hipStream_t stream) {
    if (m <= 0) return 0;
    if (t.d < 1 || t.d > 3 || t.k != 1 || !vals || !x0 || (t.d > 1 && !x1) || (t.d > 2 && !x2)) return 1;
    hipLaunchKernelGGL(field_soa_kernel, dim3(grid_for(m)), dim3(kThreads), 0, stream, t, x0, x1, x2, m, vals, grad);
    TERMS_HIP(hipGetLastError());
    return 0;
}

// ---- remove_duplicates

namespace {

enum : uint8_t { kUnknown = 0, kKept = 1, kDropped = 2 };

__global__ __launch_bounds__(kThreads) void dedup_keys_kernel(DedupGrid g, const double *__restrict__ x, int64_t n,
                                                              uint64_t *__restrict__ key, int32_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        double p[3] = {0, 0, 0};
        int64_t cell[3] = {0, 0, 0};
        for (int a = 0; a < g.d; ++a) p[a] = x[a * n + i];
        dedup_cell(g, p, cell);
        key[i] = dedup_key(g, cell);
        idx[i] = static_cast<int32_t>(i);
    }
}

__global__ __launch_bounds__(kThreads) void dedup_gather_kernel(int d, const double *__restrict__ x, int64_t n,
                                                                const int32_t *__restrict__ sidx, double *__restrict__ sx) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads)
        for (int a = 0; a < d; ++a) sx[a * n + p] = x[a * n + sidx[p]];
}

__device__ __forceinline__ int64_t dedup_lower_bound(const uint64_t *__restrict__ skey, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (skey[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One round of the greedy rule at sorted position p (original index sidx[p]), from the states of the round before:
// an earlier neighbour within tol that is kept drops the point; no earlier neighbour left undecided keeps it.  The
// cells x-1 .. x+1 of one (y, z) are consecutive keys, so each of the 3^(d-1) rows around is one range of the sorted keys.
__global__ __launch_bounds__(kThreads) void dedup_round_kernel(DedupGrid g, const double *__restrict__ sx, int64_t n,
                                                               const uint64_t *__restrict__ skey, const int32_t *__restrict__ sidx,
                                                               const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                               unsigned long long *__restrict__ undecided) {
    const int64_t top = (int64_t(1) << g.bits) + 1;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        uint8_t state = in[p];
        if (state == kUnknown) {
            double x[3] = {0, 0, 0};
            int64_t cell[3] = {0, 0, 0};
            for (int a = 0; a < g.d; ++a) x[a] = sx[a * n + p];
            dedup_cell(g, x, cell);
            const int32_t i = sidx[p];
            bool kept_before = false, unknown_before = false;
            const int ny = g.d >= 2 ? 3 : 1, nz = g.d >= 3 ? 3 : 1;
            for (int dz = 0; dz < nz && !kept_before; ++dz)
                for (int dy = 0; dy < ny && !kept_before; ++dy) {
                    int64_t c[3] = {cell[0], cell[1] + (g.d >= 2 ? dy - 1 : 0), cell[2] + (g.d >= 3 ? dz - 1 : 0)};
                    if (c[1] < 0 || c[1] > top || c[2] < 0 || c[2] > top) continue;
                    c[0] = cell[0] > 0 ? cell[0] - 1 : 0;
                    const uint64_t first = dedup_key(g, c);
                    c[0] = cell[0] < top ? cell[0] + 1 : top;
                    const uint64_t last = dedup_key(g, c);
                    for (int64_t q = dedup_lower_bound(skey, n, first); q < n && skey[q] <= last; ++q) {
                        if (sidx[q] >= i) continue;
                        double y[3] = {0, 0, 0};
                        for (int a = 0; a < g.d; ++a) y[a] = sx[a * n + q];
                        if (!dedup_close(g, x, y)) continue;
                        const uint8_t s = in[q];
                        if (s == kKept) {
                            kept_before = true;
                            break;
                        }
                        if (s == kUnknown) unknown_before = true;
                    }
                }
            state = kept_before ? kDropped : (unknown_before ? kUnknown : kKept);
            if (state == kUnknown) atomicAdd(undecided, 1ull);
        }
        out[p] = state;
    }
}

__global__ __launch_bounds__(kThreads) void dedup_flags_kernel(int64_t n, const int32_t *__restrict__ sidx,
                                                               const uint8_t *__restrict__ state, uint8_t *__restrict__ keep) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads)
        keep[sidx[p]] = state[p] == kKept ? 1 : 0;
}

} // namespace

int remove_duplicates_device(const double *points, int64_t n, int d, int64_t ld, const DedupGrid &g, int64_t *keep, int64_t *n_keep,
                             int64_t *rounds) {
    *n_keep = 0;
    if (rounds) *rounds = 0;
    if (n == 0) return 0;
    if (n >= (int64_t(1) << 31)) return 2; // 32-bit point indices: the caller takes the host path
    Pool pool;
    const size_t N = static_cast<size_t>(n);
    double *x = nullptr, *sx = nullptr;
    uint64_t *key = nullptr, *skey = nullptr;
    int32_t *idx = nullptr, *sidx = nullptr;
    uint8_t *state[2] = {nullptr, nullptr}, *flags = nullptr, *sort_tmp = nullptr;
    unsigned long long *undecided = nullptr;
    TERMS_HIP(pool.get(&x, N * d));
    TERMS_HIP(pool.get(&sx, N * d));
    TERMS_HIP(pool.get(&key, N));
    TERMS_HIP(pool.get(&skey, N));
    TERMS_HIP(pool.get(&idx, N));
    TERMS_HIP(pool.get(&sidx, N));
    TERMS_HIP(pool.get(&state[0], N));
    TERMS_HIP(pool.get(&state[1], N));
    TERMS_HIP(pool.get(&flags, N));
    TERMS_HIP(pool.get(&undecided, 1));
    TERMS_HIP(columns_up(x, points, ld, n, d));
    const int grid = grid_for(n);
    hipLaunchKernelGGL(dedup_keys_kernel, dim3(grid), dim3(kThreads), 0, 0, g, x, n, key, idx);
    TERMS_HIP(hipGetLastError());
    size_t sort_bytes = 0;
    const unsigned end_bit = static_cast<unsigned>(d * (g.bits + 1));
    TERMS_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, key, skey, idx, sidx, N, 0, end_bit, 0));
    TERMS_HIP(pool.get(&sort_tmp, sort_bytes));
    TERMS_HIP(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, key, skey, idx, sidx, N, 0, end_bit, 0)); // stable: index order within a cell
    hipLaunchKernelGGL(dedup_gather_kernel, dim3(grid), dim3(kThreads), 0, 0, d, x, n, sidx, sx);
    TERMS_HIP(hipGetLastError());
    TERMS_HIP(hipMemsetAsync(state[0], kUnknown, N, 0));
    int cur = 0;
    for (int64_t round = 1;; ++round) { // the undecided point of smallest index is decided in every round
        unsigned long long left = 0;
        TERMS_HIP(hipMemsetAsync(undecided, 0, sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(dedup_round_kernel, dim3(grid), dim3(kThreads), 0, 0, g, sx, n, skey, sidx, state[cur], state[cur ^ 1],
                           undecided);
        TERMS_HIP(hipGetLastError());
        TERMS_HIP(hipMemcpy(&left, undecided, sizeof(left), hipMemcpyDeviceToHost));
        cur ^= 1;
        if (rounds) *rounds = round;
        if (left == 0) break;
        if (round > n) return 1; // cannot happen: at least one point is decided per round
    }
    hipLaunchKernelGGL(dedup_flags_kernel, dim3(grid), dim3(kThreads), 0, 0, n, sidx, state[cur], flags);
    TERMS_HIP(hipGetLastError());
    std::vector<uint8_t> h(N);
    TERMS_HIP(hipMemcpy(h.data(), flags, N, hipMemcpyDeviceToHost));
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i)
        if (h[static_cast<size_t>(i)]) keep[m++] = i;
    *n_keep = m;
    return 0;
}

} // namespace bbfmm
