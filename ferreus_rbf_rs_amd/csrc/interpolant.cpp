// The C ABI of what RBFInterpolator adds around the tree (ferreus_rbf/src/rbf.rs, global_trend.rs): the trend's
// matrices, the duplicate cutoff and duplicate removal, and _evaluate in one call.  The per-target arithmetic is
// interpolant_terms.hpp; its kernels and the device duplicate removal are interpolant_terms.hip.
#include <cmath>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "capi_handle.hpp"
#include "ferreus_bbfmm_hip.h"
#include "interpolant_terms.hpp"
#include "kernels.hpp"

namespace {

using Mat4 = double[4][4]; // the leading (d + 1) x (d + 1) block is used

void mat_identity(Mat4 m) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) m[i][j] = i == j ? 1.0 : 0.0;
}

void mat_mul(int n, const Mat4 a, const Mat4 b, Mat4 out) { // out = a b, out distinct from both
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += a[i][k] * b[k][j];
            out[i][j] = s;
        }
}

void rotation_z(double angle, Mat4 m) { // global_trend.rs:170-174, 217-222
    mat_identity(m);
    m[0][0] = std::cos(angle);
    m[0][1] = std::sin(angle);
    m[1][0] = -std::sin(angle);
    m[1][1] = std::cos(angle);
}

// inverse by LU with partial pivoting, column by column of the identity; false when a pivot is zero
bool mat_inverse(int n, const Mat4 a, Mat4 inv) {
    double lu[4][4];
    int perm[4];
    for (int i = 0; i < n; ++i) {
        perm[i] = i;
        for (int j = 0; j < n; ++j) lu[i][j] = a[i][j];
    }
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(lu[r][c]) > std::fabs(lu[p][c])) p = r;
        if (lu[p][c] == 0.0 || !std::isfinite(lu[p][c])) return false;
        if (p != c) {
            for (int j = 0; j < n; ++j) std::swap(lu[p][j], lu[c][j]);
            std::swap(perm[p], perm[c]);
        }
        for (int r = c + 1; r < n; ++r) {
            lu[r][c] /= lu[c][c];
            for (int j = c + 1; j < n; ++j) lu[r][j] -= lu[r][c] * lu[c][j];
        }
    }
    for (int col = 0; col < n; ++col) {
        double y[4];
        for (int i = 0; i < n; ++i) {
            y[i] = perm[i] == col ? 1.0 : 0.0;
            for (int j = 0; j < i; ++j) y[i] -= lu[i][j] * y[j];
        }
        for (int i = n - 1; i >= 0; --i) {
            for (int j = i + 1; j < n; ++j) y[i] -= lu[i][j] * y[j];
            y[i] /= lu[i][i];
        }
        for (int i = 0; i < n; ++i) inv[i][col] = y[i];
    }
    return true;
}

bool have_device() {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

// |phi(r) - phi(0)| without the cancellation of the subtraction near r = 0 (rbf_kernels.rs: -r, r^2 ln r, r^3 and the
// spheroidal family's sill - slope r below its inflexion point); the other kernels as the difference itself.
double phi_rise(const bbfmm::KernelSpec &ks, double r) {
    switch (ks.id) {
    case bbfmm::kLinear: return r;
    case bbfmm::kThinPlateSpline: return std::fabs(r) < std::numeric_limits<double>::epsilon() ? 0.0 : std::fabs(r * r * std::log(r));
    case bbfmm::kCubic: return r * r * r;
    case bbfmm::kSpheroidal3:
    case bbfmm::kSpheroidal5:
    case bbfmm::kSpheroidal7:
    case bbfmm::kSpheroidal9:
        if (ks.s2 * (r * r) <= ks.ip2) return ks.near_slope * r;
        return std::fabs(bbfmm::kernel_value_r2_rt(ks, r * r) - ks.total_sill);
    default: return std::fabs(bbfmm::kernel_value_r2_rt(ks, r * r) - bbfmm::kernel_value_r2_rt(ks, 0.0));
    }
}

int remove_duplicates_host(const double *points, int64_t n, int d, int64_t ld, const bbfmm::DedupGrid &g, int64_t *keep,
                           int64_t *n_keep) {
    std::unordered_map<uint64_t, std::vector<int64_t>> kept_in; // the kept points of each cell
    kept_in.reserve(static_cast<size_t>(n));
    const int64_t top = (int64_t(1) << g.bits) + 1;
    const int n1 = d >= 2 ? 3 : 1, n2 = d >= 3 ? 3 : 1;
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        double x[3] = {0, 0, 0};
        int64_t cell[3] = {0, 0, 0};
        for (int a = 0; a < d; ++a) x[a] = points[a * ld + i];
        bbfmm::dedup_cell(g, x, cell);
        bool dropped = false;
        for (int o2 = 0; o2 < n2 && !dropped; ++o2)
            for (int o1 = 0; o1 < n1 && !dropped; ++o1)
                for (int o0 = 0; o0 < 3 && !dropped; ++o0) {
                    const int64_t c[3] = {cell[0] + o0 - 1, cell[1] + (d >= 2 ? o1 - 1 : 0), cell[2] + (d >= 3 ? o2 - 1 : 0)};
                    if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] > top || c[1] > top || c[2] > top) continue;
                    const auto it = kept_in.find(bbfmm::dedup_key(g, c));
                    if (it == kept_in.end()) continue;
                    for (int64_t j : it->second) {
                        double y[3] = {0, 0, 0};
                        for (int a = 0; a < d; ++a) y[a] = points[a * ld + j];
                        if (bbfmm::dedup_close(g, x, y)) {
                            dropped = true;
                            break;
                        }
                    }
                }
        if (dropped) continue;
        kept_in[bbfmm::dedup_key(g, cell)].push_back(i);
        keep[m++] = i;
    }
    *n_keep = m;
    return BBFMM_OK;
}

} // namespace

namespace bbfmm {
bool terms_from_abi(const ::bbfmm_interpolant_terms *in, InterpolantTerms *t) {
    if (!in || in->size < static_cast<int64_t>(sizeof(bbfmm_interpolant_terms))) return false;
    if (in->d < 1 || in->d > 3 || in->polynomial_degree < -1 || in->polynomial_degree > 2 || in->k < 1) return false;
    const int nb = bbfmm::terms_basis_size(in->d, in->polynomial_degree);
    if (nb > 0 && (!in->coefficients || in->ld_coefficients < nb)) return false;
    t->d = in->d;
    t->degree = in->polynomial_degree;
    t->k = in->k;
    t->has_affine = in->has_affine ? 1 : 0;
    t->lambda = in->coefficients;
    t->ld_lambda = in->ld_coefficients;
    for (int a = 0; a < 3; ++a) {
        t->translation[a] = in->translation[a];
        t->scale[a] = in->scale[a];
        t->b[a] = in->b[a];
    }
    for (int a = 0; a < in->d; ++a)
        if (nb > 1 && !(in->scale[a] != 0.0)) return false;
    for (int q = 0; q < 9; ++q) t->B[q] = in->B[q];
    return true;
}

} // namespace bbfmm

extern "C" {

int bbfmm_global_trend_transform(int32_t d, const double *params, const double *center, double *affine_out, double *inverse_out) {
    if (d < 1 || d > 3 || !params || !center || !affine_out || !inverse_out) return BBFMM_BAD_ARGUMENT;
    const int n = d + 1;
    const int n_params = d == 1 ? 1 : (d == 2 ? 3 : 6);
    for (int q = 0; q < n_params; ++q)
        if (!std::isfinite(params[q])) return BBFMM_BAD_ARGUMENT;
    const double *ratios = params + (n_params - d);
    for (int a = 0; a < d; ++a)
        if (!(ratios[a] != 0.0) || !std::isfinite(center[a])) return BBFMM_BAD_ARGUMENT;
    const double to_radians = 3.14159265358979323846 / 180.0; // f64::to_radians
    Mat4 to_origin, back, scale, rotation, t0, t1, m;
    mat_identity(to_origin);
    mat_identity(back);
    mat_identity(scale);
    mat_identity(rotation);
    for (int a = 0; a < d; ++a) {
        to_origin[a][d] = -center[a];
        back[a][d] = center[a];
        scale[a][a] = 1.0 / ratios[a];
    }
    if (d == 2) {
        rotation_z(-params[0] * to_radians, rotation);
    } else if (d == 3) { // rot_z_2 * rot_x * rot_z: dip direction, then dip, then pitch
        Mat4 rz, rx, rz2, tmp;
        rotation_z(-params[1] * to_radians, rz);
        rotation_z(-params[2] * to_radians, rz2);
        const double dip = -params[0] * to_radians;
        mat_identity(rx);
        rx[1][1] = std::cos(dip);
        rx[1][2] = std::sin(dip);
        rx[2][1] = -std::sin(dip);
        rx[2][2] = std::cos(dip);
        mat_mul(n, rz2, rx, tmp);
        mat_mul(n, tmp, rz, rotation);
    }
    mat_mul(n, back, scale, t0); // transform_back * scale * rotation * transform, left to right
    mat_mul(n, t0, rotation, t1);
    mat_mul(n, t1, to_origin, m);
    Mat4 affine, inverse;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) affine[i][j] = m[j][i]; // row-vector points: [x 1] * affine
    if (!mat_inverse(n, affine, inverse)) return BBFMM_BAD_ARGUMENT;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            affine_out[i * n + j] = affine[i][j];
            inverse_out[i * n + j] = inverse[i][j];
        }
    return BBFMM_OK;
}

int bbfmm_duplicate_cutoff_distance(const bbfmm_interpolant *interpolant, double h_ref, double *out) {
    if (!interpolant || !out || !bbfmm::kernel_id_valid(interpolant->kernel_type) || !(h_ref >= 0.0) || !std::isfinite(h_ref))
        return BBFMM_BAD_ARGUMENT;
    const bbfmm::KernelSpec ks = bbfmm::make_kernel_spec(interpolant->kernel_type, interpolant->base_range, interpolant->total_sill);
    const double target = std::numeric_limits<double>::epsilon() * phi_rise(ks, h_ref);
    auto resid = [&](double r) { return phi_rise(ks, r) - target; };
    *out = h_ref;
    if (!(resid(h_ref) > 0.0)) return BBFMM_OK; // rbf.rs:1407, and a NaN kernel value
    double hi = h_ref, lo = 0.0; // resid(0) = -target <= 0
    if (!(resid(lo) < 0.0)) { // target = 0
        *out = 0.0;
        return BBFMM_OK;
    }
    for (int q = 0; q < 1100 && resid(0.5 * hi) > 0.0; ++q) hi *= 0.5; // towards the first crossing (r^2 ln r is not monotone)
    lo = 0.5 * hi;
    if (resid(lo) > 0.0) lo = 0.0;
    for (int q = 0; q < 200 && hi - lo > 1e-13 * hi; ++q) {
        const double mid = 0.5 * (lo + hi);
        if (resid(mid) > 0.0) hi = mid;
        else lo = mid;
    }
    *out = 0.5 * (lo + hi);
    return BBFMM_OK;
}

int bbfmm_remove_duplicates(const double *points, int64_t n, int32_t d, int64_t ld, double tol, int32_t where, int64_t *keep_out,
                            int64_t *n_keep_out, int64_t *rounds_out) {
    if (n_keep_out) *n_keep_out = 0;
    if (rounds_out) *rounds_out = 0;
    if (n < 0 || d < 1 || d > 3 || ld < n || (where != 0 && where != 1) || !n_keep_out || !(tol >= 0.0) || !std::isfinite(tol))
        return BBFMM_BAD_ARGUMENT;
    if (n == 0) return BBFMM_OK;
    if (!points || !keep_out) return BBFMM_BAD_ARGUMENT;
    try {
        double lo[3], hi[3];
        for (int a = 0; a < d; ++a) {
            lo[a] = hi[a] = points[a * ld];
            for (int64_t i = 0; i < n; ++i) {
                const double v = points[a * ld + i];
                if (!std::isfinite(v)) return BBFMM_BAD_ARGUMENT;
                lo[a] = v < lo[a] ? v : lo[a];
                hi[a] = v > hi[a] ? v : hi[a];
            }
            if (!std::isfinite(hi[a] - lo[a])) return BBFMM_BAD_ARGUMENT;
        }
        const bbfmm::DedupGrid g = bbfmm::make_dedup_grid(d, lo, hi, tol);
        if (where == 1 && have_device()) { // (no device at all: the host path below, the same set)
            const int rc = bbfmm::remove_duplicates_device(points, n, d, ld, g, keep_out, n_keep_out, rounds_out);
            if (rc != 2) return rc == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
        }
        return remove_duplicates_host(points, n, d, ld, g, keep_out, n_keep_out);
    } catch (...) {
        return BBFMM_BAD_ARGUMENT;
    }
}

int bbfmm_debug_interpolant_terms(int32_t where, int32_t which, const bbfmm_interpolant_terms *terms, const double *x, int64_t m,
                                  int64_t ldx, double *points_out, int64_t ldp, double *values, int64_t ldv, double *grad,
                                  int64_t ldg) {
    bbfmm::InterpolantTerms t;
    if ((where != 0 && where != 1) || which < 0 || which > 2 || m < 0 || !bbfmm::terms_from_abi(terms, &t)) return BBFMM_BAD_ARGUMENT;
    if (which == 0 && (!x || !points_out || ldx < m || ldp < m)) return BBFMM_BAD_ARGUMENT;
    if (which == 1 && (!x || !values || ldx < m || ldv < m || (grad && ldg < m))) return BBFMM_BAD_ARGUMENT;
    if (which == 2 && (!grad || ldg < m)) return BBFMM_BAD_ARGUMENT;
    if (where == 1) {
        if (!have_device()) return BBFMM_DEVICE_ERROR;
        int rc = 0;
        try {
            if (which == 0) rc = bbfmm::terms_affine_device(t, x, m, ldx, points_out, ldp);
            else if (which == 1) rc = bbfmm::terms_polynomial_device(t, x, m, ldx, values, ldv, grad, ldg);
            else rc = bbfmm::terms_trend_gradients_device(t, m, grad, ldg);
        } catch (...) {
            return BBFMM_BAD_ARGUMENT;
        }
        return rc == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
    }
    for (int64_t i = 0; i < m; ++i) {
        if (which == 0) bbfmm::affine_row(t, x, ldx, points_out, ldp, i);
        else if (which == 1) bbfmm::polynomial_row(t, x, ldx, values, ldv, grad, ldg, i);
        else bbfmm::trend_gradients_row(t, grad, ldg, i);
    }
    return BBFMM_OK;
}

int bbfmm_evaluate_interpolant(bbfmm_handle *h, int32_t mode, int32_t with_gradients, const double *w, int64_t rows, int32_t k,
                               int64_t ldw, const double *x, int64_t m, int64_t ldx, const bbfmm_interpolant_terms *terms,
                               double nugget, double *values_out, int64_t ldo, double *grad_out, int64_t ldg,
                               int64_t *bad_point_index) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    auto fail = [h](int rc, const char *message) { // (the entries this forwards to set their own message)
        bbfmm::set_handle_error(h, message);
        return rc;
    };
    if ((mode != BBFMM_EVALUATE_FULL && mode != BBFMM_EVALUATE_LEAVES) || m < 0 || !values_out || (with_gradients && !grad_out))
        return fail(BBFMM_BAD_ARGUMENT, "evaluate_interpolant: bad mode, target count or output arrays");
    bbfmm_tree_stats stats;
    int rc = bbfmm_get_tree_stats(h, &stats);
    if (rc != BBFMM_OK) return rc;
    bbfmm::InterpolantTerms t;
    t.d = stats.d;
    t.k = k;
    if (terms && (!bbfmm::terms_from_abi(terms, &t) || t.d != stats.d || t.k != k))
        return fail(BBFMM_BAD_ARGUMENT, "evaluate_interpolant: bad terms (size, d and k of the tree and the weights, degree -1 .. 2, coefficients, scale != 0)");
    if (nugget != 0.0 && (!w || m != stats.n_points))
        return fail(BBFMM_BAD_ARGUMENT, "evaluate_interpolant: a nugget needs the weights and the source points as targets"); // the at-source case alone (rbf.rs:1230-1235)
    int cur = -1;
    const int dev = bbfmm_part_device(h, 0); // the terms run beside the tree (of a device group: its primary part)
    if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) != hipSuccess)
        return fail(BBFMM_DEVICE_ERROR, "evaluate_interpolant: hipSetDevice");
    struct Restore {
        int cur, dev;
        ~Restore() {
            if (cur >= 0 && dev >= 0 && cur != dev) (void)hipSetDevice(cur);
        }
    } restore{cur, dev};
    try {
        const double *xt = x;
        int64_t ldt = ldx;
        std::vector<double> moved;
        if (t.has_affine && m > 0) {
            if (!x || ldx < m) return fail(BBFMM_BAD_ARGUMENT, "evaluate_interpolant: bad target array");
            moved.resize(static_cast<size_t>(m) * t.d);
            if (bbfmm::terms_affine_device(t, x, m, ldx, moved.data(), m) != 0)
                return fail(BBFMM_DEVICE_ERROR, "evaluate_interpolant: the trend's map of the targets failed on the device");
            xt = moved.data();
            ldt = m;
        }
        if (mode == BBFMM_EVALUATE_FULL)
            rc = with_gradients ? bbfmm_evaluate_with_gradients(h, w, rows, k, ldw, xt, m, ldt, values_out, ldo, grad_out, ldg, bad_point_index)
                                : bbfmm_evaluate(h, w, rows, k, ldw, xt, m, ldt, values_out, ldo, bad_point_index);
        else
            rc = with_gradients
                     ? bbfmm_evaluate_leaves_with_gradients(h, w, rows, k, ldw, xt, m, ldt, values_out, ldo, grad_out, ldg, bad_point_index)
                     : bbfmm_evaluate_leaves(h, w, rows, k, ldw, xt, m, ldt, values_out, ldo, bad_point_index);
        if (rc != BBFMM_OK) return rc;
        const bool poly = bbfmm::terms_basis_size(t.d, t.degree) > 0;
        if (m == 0 || (!poly && nugget == 0.0 && !(t.has_affine && with_gradients))) return BBFMM_OK;
        if (poly && (!x || ldx < m)) return fail(BBFMM_BAD_ARGUMENT, "evaluate_interpolant: bad target array");
        if (bbfmm::terms_finish_device(t, x, m, ldx, values_out, ldo, with_gradients ? grad_out : nullptr, ldg, nugget,
                                       nugget != 0.0 ? w : nullptr, ldw) != 0)
            return fail(BBFMM_DEVICE_ERROR, "evaluate_interpolant: the terms kernel failed on the device");
        return BBFMM_OK;
    } catch (...) {
        return fail(BBFMM_BAD_ARGUMENT, "evaluate_interpolant: out of host memory");
    }
}

} // extern "C"
