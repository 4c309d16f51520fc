// What RBFInterpolator adds around the kernel sum (ferreus_rbf/src/rbf.rs:1180-1298): the global trend's affine map of
// the targets (global_trend.rs:266-272), the polynomial part with its gradient (polynomials.rs:30-116 on the points
// scaled by common.rs:330-336) and the trend's chain rule on the kernel gradients (rbf.rs:1272-1298); and the uniform
// grid of remove_duplicates (rbf.rs:1430-1467).  One definition of the arithmetic for the host entries and the kernels
// of interpolant_terms.hip: every sum in a fixed order, products and sums never fused.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BBFMM_TERMS_HD __host__ __device__
#else
#define BBFMM_TERMS_HD
#endif

struct bbfmm_interpolant_terms; // ferreus_bbfmm_hip.h

namespace bbfmm {

struct InterpolantTerms;
// the checked copy of the ABI's struct (interpolant.cpp); false on a bad one
bool terms_from_abi(const ::bbfmm_interpolant_terms *in, InterpolantTerms *t);

constexpr int kMaxMonomials = 10; // quadratic in 3-D

// The terms of one interpolant.  B is d x d row-major and x' = x B + b for a row-vector point; lambda is
// basis_size x k, column c at lambda + c * ld_lambda (a device pointer for the kernels, a host pointer for the host entries).
struct InterpolantTerms {
    int d = 3;
    int degree = -1; // -1: no polynomial
    int k = 1;
    int has_affine = 0;
    const double *lambda = nullptr;
    int64_t ld_lambda = 0;
    double translation[3] = {0, 0, 0};
    double scale[3] = {1, 1, 1};
    double B[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double b[3] = {0, 0, 0};
};

BBFMM_TERMS_HD inline int terms_basis_size(int d, int degree) { // set_basis_size, interpolant_config.rs:150-178
    const int k = degree + 1;
    return degree < 0 ? 0 : (d == 1 ? k : (d == 2 ? k * (k + 1) / 2 : k * (k + 1) * (k + 2) / 6));
}

// x' = x B + b: a = 0 .. d-1 in order, then + b.
BBFMM_TERMS_HD inline void affine_point(const InterpolantTerms &t, const double *x, double *out) {
#pragma clang fp contract(off)
    for (int c = 0; c < t.d; ++c) {
        double s = x[0] * t.B[c];
        for (int a = 1; a < t.d; ++a) s = s + x[a] * t.B[a * t.d + c];
        out[c] = s + t.b[c];
    }
}

// The monomials 1 | s_a | s_a s_b (a <= b) of the scaled point, in the order of ddm_monomials.hpp, and for each axis e
// the derivative d m_j / d x_e in world coordinates (polynomials.rs:79-113: 1 / scale_e, 2 s_a / scale_a, s_b / scale_a).
BBFMM_TERMS_HD inline int monomials_and_gradients(const InterpolantTerms &t, const double *x, double *m,
                                                  double (*dm)[3]) {
#pragma clang fp contract(off)
    const int nb = terms_basis_size(t.d, t.degree);
    if (nb == 0) return 0;
    double s[3] = {0, 0, 0};
    for (int a = 0; a < t.d; ++a) s[a] = (x[a] - t.translation[a]) / t.scale[a];
    if (dm)
        for (int j = 0; j < nb; ++j) dm[j][0] = dm[j][1] = dm[j][2] = 0.0;
    m[0] = 1.0;
    if (t.degree >= 1)
        for (int a = 0; a < t.d; ++a) {
            m[1 + a] = s[a];
            if (dm) dm[1 + a][a] = 1.0 / t.scale[a];
        }
    if (t.degree == 2) {
        int j = 1 + t.d;
        for (int a = 0; a < t.d; ++a)
            for (int c = a; c < t.d; ++c, ++j) {
                m[j] = s[a] * s[c];
                if (!dm) continue;
                if (a == c) {
                    dm[j][a] = 2.0 * s[a] / t.scale[a];
                } else {
                    dm[j][a] = s[c] / t.scale[a];
                    dm[j][c] = s[a] / t.scale[c];
                }
            }
    }
    return nb;
}

// Column c of one point: *value += sum_j m_j lambda[j, c] (j ascending, the sum formed first and added once), and with
// grad (the d entries of that column) grad[e] += sum_j (d m_j / d x_e) lambda[j, c].
BBFMM_TERMS_HD inline void polynomial_column(const InterpolantTerms &t, int nb, const double *m, const double (*dm)[3], int c,
                                             double *value, double *grad) {
#pragma clang fp contract(off)
    const double *l = t.lambda + static_cast<size_t>(c) * t.ld_lambda;
    double s = m[0] * l[0];
    for (int j = 1; j < nb; ++j) s = s + m[j] * l[j];
    *value = *value + s;
    if (!grad) return;
    for (int e = 0; e < t.d; ++e) {
        double g = dm[0][e] * l[0];
        for (int j = 1; j < nb; ++j) g = g + dm[j][e] * l[j];
        grad[e] = grad[e] + g;
    }
}

// grad_x = grad_x' B^T for one column's d entries: out[e] = sum_a g[a] B[e, a], a ascending (rbf.rs:1289-1295).
BBFMM_TERMS_HD inline void trend_gradient_column(const InterpolantTerms &t, double *grad) {
#pragma clang fp contract(off)
    double g[3] = {0, 0, 0};
    for (int a = 0; a < t.d; ++a) g[a] = grad[a];
    for (int e = 0; e < t.d; ++e) {
        double acc = 0.0;
        for (int a = 0; a < t.d; ++a) acc = acc + g[a] * t.B[e * t.d + a];
        grad[e] = acc;
    }
}

// Row i of SoA arrays (column a at + a * ld): what one thread of the kernels and one iteration of the host loops does.
BBFMM_TERMS_HD inline void affine_row(const InterpolantTerms &t, const double *x, int64_t ldx, double *out, int64_t ldo,
                                      int64_t i) {
    double p[3] = {0, 0, 0}, q[3];
    for (int a = 0; a < t.d; ++a) p[a] = x[a * ldx + i];
    affine_point(t, p, q);
    for (int a = 0; a < t.d; ++a) out[a * ldo + i] = q[a];
}

BBFMM_TERMS_HD inline void trend_gradients_row(const InterpolantTerms &t, double *grad, int64_t ldg, int64_t i) {
    for (int c = 0; c < t.k; ++c) {
        double g[3] = {0, 0, 0};
        for (int a = 0; a < t.d; ++a) g[a] = grad[(c * t.d + a) * ldg + i];
        trend_gradient_column(t, g);
        for (int a = 0; a < t.d; ++a) grad[(c * t.d + a) * ldg + i] = g[a];
    }
}

BBFMM_TERMS_HD inline void polynomial_row(const InterpolantTerms &t, const double *x, int64_t ldx, double *values, int64_t ldv,
                                          double *grad, int64_t ldg, int64_t i) {
    double p[3] = {0, 0, 0}, m[kMaxMonomials], dm[kMaxMonomials][3];
    for (int a = 0; a < t.d; ++a) p[a] = x[a * ldx + i];
    const int nb = monomials_and_gradients(t, p, m, grad ? dm : nullptr);
    if (nb == 0) return;
    for (int c = 0; c < t.k; ++c) {
        double v = values[c * ldv + i], g[3] = {0, 0, 0};
        if (grad)
            for (int a = 0; a < t.d; ++a) g[a] = grad[(c * t.d + a) * ldg + i];
        polynomial_column(t, nb, m, dm, c, &v, grad ? g : nullptr);
        values[c * ldv + i] = v;
        if (grad)
            for (int a = 0; a < t.d; ++a) grad[(c * t.d + a) * ldg + i] = g[a];
    }
}

// ---- remove_duplicates: the uniform grid both paths hash the points into
// The cell side is at least tol (so every point within tol, in the infinity norm, lies in the 3^d cells around) and at
// least extent / 2^bits (so a cell index fits `bits + 1` bits and the key 64).  The factor 1 + 2^-10 covers the
// rounding of (x - lo) / side: cell indices are below 2^30, so that quotient is off by less than 2^-22 of a cell.
struct DedupGrid {
    int d = 3;
    int bits = 20; // per axis: indices 0 .. 2^bits + 1
    double lo[3] = {0, 0, 0};
    double side = 1.0;
    double tol = 0.0;
};

inline DedupGrid make_dedup_grid(int d, const double *lo, const double *hi, double tol) {
    DedupGrid g;
    g.d = d;
    g.bits = d == 3 ? 20 : 30;
    g.tol = tol;
    double extent = 0.0;
    for (int a = 0; a < d; ++a) {
        g.lo[a] = lo[a];
        if (hi[a] - lo[a] > extent) extent = hi[a] - lo[a];
    }
    const double by_tol = tol * (1.0 + 1.0 / 1024.0), by_extent = extent / static_cast<double>(int64_t(1) << g.bits);
    g.side = by_tol > by_extent ? by_tol : by_extent;
    if (!(g.side > 0.0)) g.side = 1.0; // every point the same and tol = 0
    return g;
}

BBFMM_TERMS_HD inline void dedup_cell(const DedupGrid &g, const double *x, int64_t *cell) {
    for (int a = 0; a < g.d; ++a) cell[a] = static_cast<int64_t>((x[a] - g.lo[a]) / g.side);
}

BBFMM_TERMS_HD inline uint64_t dedup_key(const DedupGrid &g, const int64_t *cell) { // cells 0 .. 2^bits + 1 per axis
    uint64_t key = 0;
    for (int a = g.d - 1; a >= 0; --a) key = (key << (g.bits + 1)) | static_cast<uint64_t>(cell[a]);
    return key;
}

BBFMM_TERMS_HD inline bool dedup_close(const DedupGrid &g, const double *x, const double *y) { // inclusive, kdtree.rs:187
    for (int a = 0; a < g.d; ++a) {
        const double diff = x[a] - y[a];
        if (!((diff < 0.0 ? -diff : diff) <= g.tol)) return false;
    }
    return true;
}

// interpolant_terms.hip.  x, out: SoA on the host (column a at + a * ld); 0 on success.
int terms_affine_device(const InterpolantTerms &t, const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo);
int terms_polynomial_device(const InterpolantTerms &t, const double *x, int64_t m, int64_t ldx, double *values, int64_t ldv,
                            double *grad, int64_t ldg);
int terms_trend_gradients_device(const InterpolantTerms &t, int64_t m, double *grad, int64_t ldg);
// _evaluate's additions on host arrays in one device pass: trend_gradients, nugget * w, polynomial_terms, in that order.
int terms_finish_device(const InterpolantTerms &t, const double *x, int64_t m, int64_t ldx, double *values, int64_t ldv,
                        double *grad, int64_t ldg, double nugget, const double *w, int64_t ldw);
// The same on device-resident targets, one pointer per axis, on `stream` (the lattice field of the isosurfacer, k = 1;
// t.lambda is a DEVICE pointer here): y = x B + b; and vals[i] += polynomial, grad[a * m + i] <- (grad B^T)[a] + its
// gradient (grad may be null, the trend applies when t.has_affine).  Nothing is synchronised.  t.d = 1 or 2 (a height
// operand of a composite field): the arrays past t.d are not read and may be null, grad holds t.d columns of m, and the
// arithmetic per point is that of the AoS entries above.
int terms_affine_soa_device(const InterpolantTerms &t, const double *x0, const double *x1, const double *x2, int64_t m, double *y0,
                            double *y1, double *y2, hipStream_t stream);
int terms_field_soa_device(const InterpolantTerms &t, const double *x0, const double *x1, const double *x2, int64_t m, double *vals,
                           double *grad, hipStream_t stream);
// The K-column variant (FmmTree::evaluate_device): t.k value columns, column c at vals + c * ldv, and gradient column
// c * t.d + a at grad + (c * t.d + a) * ldg, the layout of the host entries; t.lambda a device pointer.  (The trend's map of
// the targets has no column count: terms_affine_soa_device serves every k.)
int terms_field_soa_device_k(const InterpolantTerms &t, const double *x0, const double *x1, const double *x2, int64_t m, double *vals,
                             int64_t ldv, double *grad, int64_t ldg, hipStream_t stream);
int remove_duplicates_device(const double *points, int64_t n, int d, int64_t ld, const DedupGrid &g, int64_t *keep,
                             int64_t *n_keep, int64_t *rounds);

} // namespace bbfmm
