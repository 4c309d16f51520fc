// The iterative solvers of ferreus_rbf (iterative_solvers.rs:38-281) with every vector on the device: the drivers of
// solver.cpp statement for statement, their vector work as the kernels of solver_vectors.hpp on one stream, the
// scalars those kernels exchange in device memory.  The host keeps H, g and the Givens rotations and waits for the
// stream once per inner iteration (the new Hessenberg column and the norm) and once per restart or return.  Also the
// device twin of the RBF system operator (rbf.rs:105-117) and the test hook of the vector kernels.
#include "../../include/ferreus_bbfmm_hip.h"
#include "capi_handle.hpp"
#include "solver_vectors.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

struct bbfmm_rbf_system_device {
    bbfmm_handle *tree = nullptr;
    int64_t n_points = 0, basis = 0;
    double nugget = 0.0;
    double *d_poly = nullptr; // N x basis column-major, ld N
    void *stream = nullptr;   // the tree's stream (not owned)
    ~bbfmm_rbf_system_device() {
        if (d_poly) (void)hipFree(d_poly);
    }
};

namespace bbfmm {
bbfmm_handle *rbf_system_device_tree(const void *user) {
    return user ? static_cast<const bbfmm_rbf_system_device *>(user)->tree : nullptr;
}
} // namespace bbfmm

namespace {
using namespace bbfmm;

double progress_from_rel(double cur, double start, double target) { // progress.rs:124-130
    if (cur <= target) return 1.0;
    return (std::log10(start) - std::log10(cur)) / (std::log10(start) - std::log10(target));
}

// Device and pinned memory of one solve, released on every return path.  The stream is drained first: kernels of a
// solve that ends early (an operator's error) may still be reading the vectors.
struct Workspace {
    hipStream_t stream = nullptr;
    double *d_mem = nullptr, *h_pin = nullptr;
    ~Workspace() {
        if (d_mem || h_pin) (void)hipStreamSynchronize(stream);
        if (d_mem) (void)hipFree(d_mem);
        if (h_pin) (void)hipHostFree(h_pin);
    }
    int allocate(size_t device_doubles, size_t pinned_doubles) {
        if (hipMalloc(reinterpret_cast<void **>(&d_mem), device_doubles * sizeof(double)) != hipSuccess) return BBFMM_DEVICE_ERROR;
        if (hipHostMalloc(reinterpret_cast<void **>(&h_pin), pinned_doubles * sizeof(double), hipHostMallocDefault) != hipSuccess)
            return BBFMM_DEVICE_ERROR;
        return BBFMM_OK;
    }
};

// BBFMM_VERBOSE: where the solve's wall time goes.  The stream is drained around the operators only then.
struct StageClock {
    const char *what;
    hipStream_t stream;
    bool verbose = std::getenv("BBFMM_VERBOSE") != nullptr;
    double t_a = 0, t_m = 0;
    std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now();
    StageClock(const char *w, hipStream_t s) : what(w), stream(s) {}
    int timed(double &acc, bbfmm_apply_device_fn f, void *user, const double *in, double *out, int64_t len) {
        if (!verbose) return f(user, in, out, len, stream);
        (void)hipStreamSynchronize(stream);
        const auto t0 = std::chrono::steady_clock::now();
        const int r = f(user, in, out, len, stream);
        (void)hipStreamSynchronize(stream);
        acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return r;
    }
    ~StageClock() {
        if (!verbose) return;
        (void)hipStreamSynchronize(stream);
        const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        std::fprintf(stderr, "[bbfmm] %s: total %.3f s = operator %.3f + preconditioner %.3f + device vectors %.3f\n", what, total,
                     t_a, t_m, total - t_a - t_m);
    }
};

// Native operators answer for one tree and its stream; anything else is the caller's callback and is taken as it is.
int check_native_operators(bbfmm_apply_device_fn a, void *a_user, bbfmm_apply_device_fn m, void *m_user, void *stream) {
    bbfmm_handle *trees[2] = {nullptr, nullptr};
    int count = 0;
    const bbfmm_apply_device_fn fns[2] = {a, m};
    void *users[2] = {a_user, m_user};
    for (int i = 0; i < 2; ++i) {
        bbfmm_handle *t = nullptr;
        if (fns[i] == bbfmm_rbf_system_apply_device) t = rbf_system_device_tree(users[i]);
        else if (fns[i] == bbfmm_schwarz_apply_device) t = schwarz_tree(static_cast<const bbfmm_schwarz *>(users[i]));
        else continue;
        if (!t) return BBFMM_BAD_ARGUMENT;
        trees[count++] = t;
    }
    if (count == 2 && trees[0] != trees[1]) {
        set_handle_error(trees[0], "device solver: the system operator and the preconditioner belong to different trees");
        return BBFMM_BAD_ARGUMENT;
    }
    if (count > 0 && bbfmm_stream(trees[0]) != stream) {
        set_handle_error(trees[0], "device solver: native operators run on their tree's stream (bbfmm_stream), pass that one");
        return BBFMM_BAD_ARGUMENT;
    }
    return BBFMM_OK;
}

#define HIPOK(expr)                                          \
    do {                                                     \
        if ((expr) != hipSuccess) return BBFMM_DEVICE_ERROR; \
    } while (0)

size_t pad_even(int64_t n) { return static_cast<size_t>(n + (n & 1)); } // vectors of a workspace start 16-byte aligned

int fgmres_device(int64_t n, bbfmm_apply_device_fn a, void *a_user, const double *b, bbfmm_apply_device_fn m, void *m_user,
                  const double *x0, int32_t max_outer_iterations, int32_t max_inner_iterations, int32_t tolerance_type,
                  double tolerance, bbfmm_iteration_fn callback, void *cb_user, double *x, int64_t *iterations,
                  double *final_residual, hipStream_t stream) {
    const int mi = max_inner_iterations, ldh = mi + 1;
    const bool absolute = tolerance_type == BBFMM_ACCURACY_ABSOLUTE;
    const size_t nb = static_cast<size_t>(n) * sizeof(double), np = pad_even(n);
    const int64_t nch = solver_chunks(n);
    StageClock clock("fgmres (device vectors)", stream);
    // V (mi + 1), Z (mi), r, wj; two rows of chunk partials; the scalar slots; the coefficients of a solution update
    Workspace ws;
    ws.stream = stream;
    const size_t n_vec = static_cast<size_t>(2 * mi + 3), n_slot = static_cast<size_t>(mi + 4);
    int rc = ws.allocate(n_vec * np + 2 * static_cast<size_t>(nch) + n_slot + static_cast<size_t>(mi), n_slot + static_cast<size_t>(mi));
    if (rc) return rc;
    double *v = ws.d_mem, *z = v + static_cast<size_t>(mi + 1) * np, *r = z + static_cast<size_t>(mi) * np, *wj = r + np;
    double *part = wj + np, *part2 = part + nch, *slot = part2 + nch, *d_y = slot + n_slot;
    double *h_slot = ws.h_pin, *h_y = ws.h_pin + n_slot;
    auto V = [&](int i) { return v + static_cast<size_t>(i) * np; };
    auto Z = [&](int i) { return z + static_cast<size_t>(i) * np; };
    // slots: [0 .. mi) the Hessenberg column, [mi] the norm of the new vector; [mi + 1] r_norm, [mi + 2] max |r|
    double *s_norm = slot + mi, *s_rnorm = slot + mi + 1, *s_rmax = slot + mi + 2;
    auto download = [&](int first, int count) -> int { // slots -> the pinned copy, then wait: THE synchronisation of an iteration
        if (hipMemcpyAsync(h_slot + first, slot + first, static_cast<size_t>(count) * sizeof(double), hipMemcpyDeviceToHost, stream) !=
            hipSuccess)
            return BBFMM_DEVICE_ERROR;
        if (hipStreamSynchronize(stream) != hipSuccess) return BBFMM_DEVICE_ERROR;
        return hipGetLastError() == hipSuccess ? BBFMM_OK : BBFMM_DEVICE_ERROR;
    };
    // r = b - A x with both norms of r, on the stream
    auto residual = [&]() -> int {
        const int rr = clock.timed(clock.t_a, a, a_user, x, wj, n);
        if (rr) return rr;
        launch_solver_sub(b, wj, r, n, part, part2, stream);
        launch_solver_reduce_finish(part, nch, false, true, s_rnorm, stream);
        launch_solver_reduce_finish(part2, nch, true, false, s_rmax, stream);
        return BBFMM_OK;
    };
    std::vector<double> h(static_cast<size_t>(ldh) * mi), g(static_cast<size_t>(mi + 1)), cs(mi), sn(mi);
    // get_solution (iterative_solvers.rs:174-183): x += Z[:, :i] (H[:i,:i]^-1 g[:i]), the triangular solve on the host
    auto add_solution = [&](int i) -> int {
        for (int c = 0; c < i; ++c) h_y[c] = g[c];
        for (int rw = i - 1; rw >= 0; --rw) {
            double s = h_y[rw];
            for (int c = rw + 1; c < i; ++c) s -= h[static_cast<size_t>(rw) + static_cast<size_t>(c) * ldh] * h_y[c];
            h_y[rw] = s / h[static_cast<size_t>(rw) + static_cast<size_t>(rw) * ldh];
        }
        if (hipMemcpyAsync(d_y, h_y, static_cast<size_t>(i) * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess)
            return BBFMM_DEVICE_ERROR;
        launch_solver_update(z, static_cast<int64_t>(np), d_y, i, x, n, stream);
        return BBFMM_OK;
    };

    if (x0) HIPOK(hipMemcpyAsync(x, x0, nb, hipMemcpyDeviceToDevice, stream));
    else HIPOK(hipMemsetAsync(x, 0, nb, stream));
    if ((rc = residual())) return rc;
    if ((rc = download(mi + 1, 2))) return rc;
    double r_norm = h_slot[mi + 1]; // the 2-norm of r: beta of a relative tolerance, and the first restart's r_norm
    const double beta = absolute ? h_slot[mi + 2] : r_norm;
    int64_t iteration = 1;
    double res_norm = absolute ? beta : 1.0;
    if (iterations) *iterations = 0;
    if (final_residual) *final_residual = res_norm;
    for (int outer = 0; outer < max_outer_iterations; ++outer) {
        std::fill(h.begin(), h.end(), 0.0);
        std::fill(g.begin(), g.end(), 0.0);
        // (r_norm came down with the residual: s_rnorm still holds it on the device)
        if (r_norm == 0.0) break; // a zero residual is returned as converged (the reference divides by it)
        launch_solver_scale(r, s_rnorm, kAlphaInvSlot, 0.0, V(0), n, stream);
        g[0] = r_norm;
        for (int j = 0; j < mi; ++j) {
            // z_j = M v_j (or v_j); w_j = A z_j
            if (m) {
                if ((rc = clock.timed(clock.t_m, m, m_user, V(j), Z(j), n))) return rc;
            } else {
                HIPOK(hipMemcpyAsync(Z(j), V(j), nb, hipMemcpyDeviceToDevice, stream));
            }
            if ((rc = clock.timed(clock.t_a, a, a_user, Z(j), wj, n))) return rc;
            // modified Gram-Schmidt, h_ij = <v_i, w>; w -= h_ij v_i for i = 0 .. j in turn: the subtraction of step i - 1
            // and the dot product of step i share one pass over w, the last subtraction carries the norm of w
            for (int i = 0; i <= j; ++i) {
                launch_solver_axpy_reduce(i ? V(i - 1) : nullptr, i ? slot + (i - 1) : nullptr, kAlphaNegSlot, 0.0, wj, V(i), n,
                                          kReduceDot, part, stream);
                launch_solver_reduce_finish(part, nch, false, false, slot + i, stream);
            }
            launch_solver_axpy_reduce(V(j), slot + j, kAlphaNegSlot, 0.0, wj, nullptr, n, kReduceDot, part, stream);
            launch_solver_reduce_finish(part, nch, false, true, s_norm, stream);
            // v_{j+1} = w / norm (zero when the norm is): needs the device scalar only, so it is queued before the wait
            launch_solver_scale(wj, s_norm, kAlphaInvSlot, 0.0, V(j + 1), n, stream);
            if ((rc = download(0, mi + 1))) return rc;
            auto H = [&](int rr, int cc) -> double & { return h[static_cast<size_t>(rr) + static_cast<size_t>(cc) * ldh]; };
            for (int i = 0; i <= j; ++i) H(i, j) = h_slot[i];
            const double norm = h_slot[mi];
            H(j + 1, j) = norm;
            for (int i = 0; i < j; ++i) { // previous rotations
                const double temp = cs[i] * H(i, j) + sn[i] * H(i + 1, j);
                H(i + 1, j) = -sn[i] * H(i, j) + cs[i] * H(i + 1, j);
                H(i, j) = temp;
            }
            double c, s, rr;
            bbfmm_givens_rotation(H(j, j), H(j + 1, j), &c, &s, &rr);
            H(j, j) = c * H(j, j) + s * H(j + 1, j);
            H(j + 1, j) = 0.0;
            const double temp = c * g[j] + s * g[j + 1];
            g[j + 1] = -s * g[j] + c * g[j + 1];
            g[j] = temp;
            cs[j] = c, sn[j] = s;
            res_norm = absolute ? std::fabs(g[j + 1]) : std::fabs(g[j + 1]) / beta;
            if (iterations) *iterations = iteration;
            if (final_residual) *final_residual = res_norm;
            if (callback) callback(cb_user, iteration, res_norm, progress_from_rel(res_norm, beta, tolerance));
            if (res_norm < tolerance) {
                if ((rc = add_solution(j + 1))) return rc;
                HIPOK(hipStreamSynchronize(stream));
                HIPOK(hipGetLastError());
                return BBFMM_OK;
            }
            ++iteration;
        }
        if ((rc = add_solution(mi))) return rc; // restart update
        if ((rc = residual())) return rc;
        if ((rc = download(mi + 1, 2))) return rc;
        r_norm = h_slot[mi + 1];
        res_norm = absolute ? h_slot[mi + 2] : r_norm / beta;
        if (final_residual) *final_residual = res_norm;
        if (res_norm < tolerance) break;
    }
    if (iterations) *iterations = iteration - 1;
    HIPOK(hipStreamSynchronize(stream));
    HIPOK(hipGetLastError());
    return BBFMM_OK;
}

int schwarz_ddm_device(int64_t n, bbfmm_apply_device_fn matvec, void *a_user, const double *rhs, bbfmm_apply_device_fn m,
                       void *m_user, int32_t max_iterations, int32_t tolerance_type, double tolerance, bbfmm_iteration_fn callback,
                       void *cb_user, double *x, int64_t *iterations, double *final_residual, hipStream_t stream) {
    const bool absolute = tolerance_type == BBFMM_ACCURACY_ABSOLUTE;
    const size_t nb = static_cast<size_t>(n) * sizeof(double), np = pad_even(n);
    const int64_t nch = solver_chunks(n);
    StageClock clock("schwarz_ddm_solver (device vectors)", stream);
    Workspace ws;
    ws.stream = stream;
    int rc = ws.allocate(2 * np + 2 * static_cast<size_t>(nch) + 2, 2);
    if (rc) return rc;
    double *rg = ws.d_mem, *t = rg + np, *part = t + np, *part2 = part + nch, *slot = part2 + nch;
    auto norm_down = [&](double *out) -> int { // the norm of rg the tolerance type asks for, from the partials of its last pass
        if (absolute) launch_solver_reduce_finish(part2, nch, true, false, slot, stream);
        else launch_solver_reduce_finish(part, nch, false, true, slot, stream);
        if (hipMemcpyAsync(ws.h_pin, slot, sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess) return BBFMM_DEVICE_ERROR;
        if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return BBFMM_DEVICE_ERROR;
        *out = ws.h_pin[0];
        return BBFMM_OK;
    };
    HIPOK(hipMemcpyAsync(rg, rhs, nb, hipMemcpyDeviceToDevice, stream));
    HIPOK(hipMemsetAsync(x, 0, nb, stream));
    launch_solver_axpy_reduce(nullptr, nullptr, kAlphaImmediate, 0.0, rg, nullptr, n, absolute ? kReduceMax : kReduceDot,
                              absolute ? part2 : part, stream);
    double beta = 0.0;
    if ((rc = norm_down(&beta))) return rc;
    double res_norm = beta;
    int64_t iteration = 0;
    if (m) { // without a preconditioner the reference returns the zero vector (iterative_solvers.rs:256)
        while (res_norm > tolerance && iteration < max_iterations) {
            if ((rc = clock.timed(clock.t_m, m, m_user, rg, t, n))) return rc;
            launch_solver_axpy_reduce(t, nullptr, kAlphaImmediate, 1.0, x, nullptr, n, kReduceNone, nullptr, stream);
            if ((rc = clock.timed(clock.t_a, matvec, a_user, x, t, n))) return rc;
            launch_solver_sub(rhs, t, rg, n, absolute ? nullptr : part, absolute ? part2 : nullptr, stream);
            double nrm = 0.0;
            if ((rc = norm_down(&nrm))) return rc;
            res_norm = absolute ? nrm : nrm / beta;
            ++iteration;
            if (callback) callback(cb_user, iteration, res_norm, progress_from_rel(res_norm, beta, tolerance));
        }
    }
    if (iterations) *iterations = iteration;
    if (final_residual) *final_residual = res_norm;
    HIPOK(hipStreamSynchronize(stream));
    HIPOK(hipGetLastError());
    return BBFMM_OK;
}

} // namespace

#define SOLVER_GUARD try {
#define SOLVER_END_GUARD                                          \
    }                                                             \
    catch (const std::bad_alloc &) { return BBFMM_DEVICE_ERROR; } \
    catch (...) { return BBFMM_BAD_ARGUMENT; }

extern "C" {

int bbfmm_rbf_system_device_create(bbfmm_handle *tree, int64_t basis_size, const double *monomial_matrix, int64_t ld, double nugget,
                                   bbfmm_rbf_system_device **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    *out = nullptr;
    if (!tree || basis_size < 0 || basis_size > 16) return BBFMM_BAD_ARGUMENT;
    SOLVER_GUARD
    bbfmm_tree_stats stats;
    const int rc = bbfmm_get_tree_stats(tree, &stats);
    if (rc != BBFMM_OK) return rc;
    auto fail = [tree](int code, const char *message) -> int {
        set_handle_error(tree, message);
        return code;
    };
    if (handle_is_host_only(tree))
        return fail(BBFMM_DEVICE_ERROR, "device system operator: handle was created with BBFMM_FLAG_HOST_ONLY");
    if (bbfmm_device_count(tree) > 1)
        return fail(BBFMM_UNSUPPORTED, "device system operator: device groups (bbfmm_create_on_devices) are not served by the device solvers");
    const int64_t N = stats.n_points;
    if (basis_size > 0 && (!monomial_matrix || ld < N))
        return fail(BBFMM_BAD_ARGUMENT, "device system operator: the monomial matrix needs N rows");
    bbfmm_rbf_system_device *s = new bbfmm_rbf_system_device();
    s->tree = tree;
    s->n_points = N;
    s->basis = basis_size;
    s->nugget = nugget;
    s->stream = bbfmm_stream(tree); // (binds this thread to the tree's device)
    bool ok = s->stream != nullptr;
    if (ok && basis_size > 0) {
        ok = hipMalloc(reinterpret_cast<void **>(&s->d_poly), static_cast<size_t>(N) * basis_size * sizeof(double)) == hipSuccess;
        if (ok)
            ok = hipMemcpy2D(s->d_poly, static_cast<size_t>(N) * sizeof(double), monomial_matrix, static_cast<size_t>(ld) * sizeof(double),
                             static_cast<size_t>(N) * sizeof(double), static_cast<size_t>(basis_size), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        delete s;
        return fail(BBFMM_DEVICE_ERROR, "device system operator: could not place the monomial matrix on the device");
    }
    *out = s;
    return BBFMM_OK;
    SOLVER_END_GUARD
}

void bbfmm_rbf_system_device_destroy(bbfmm_rbf_system_device *s) {
    delete s; // (the tree is not touched: it may be gone already)
}

int bbfmm_rbf_system_apply_device(void *user, const double *d_x, double *d_y, int64_t n, void *stream) {
    bbfmm_rbf_system_device *s = static_cast<bbfmm_rbf_system_device *>(user);
    if (!s || !s->tree || !d_x || !d_y || n != s->n_points + s->basis || stream != s->stream) return BBFMM_BAD_ARGUMENT;
    const int rc = bbfmm_matvec_device(s->tree, d_x, s->n_points, 1, d_y, s->n_points, 0); // set_weights + evaluate, rbf.rs:1357-1364
    if (rc) return rc;
    launch_rbf_system_tail(d_x, s->d_poly, s->n_points, static_cast<int32_t>(s->basis), s->nugget, s->n_points, d_y,
                           static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? BBFMM_OK : BBFMM_DEVICE_ERROR;
}

int bbfmm_fgmres_device(int64_t n, bbfmm_apply_device_fn a, void *a_user, const double *d_b, bbfmm_apply_device_fn m, void *m_user,
                        const double *d_x0, int32_t max_outer_iterations, int32_t max_inner_iterations, int32_t tolerance_type,
                        double tolerance, bbfmm_iteration_fn callback, void *cb_user, double *d_x, int64_t *iterations,
                        double *final_residual, void *stream) {
    if (n < 1 || !a || !d_b || !d_x || !stream || max_outer_iterations < 0 || max_inner_iterations < 1 ||
        (tolerance_type != BBFMM_ACCURACY_ABSOLUTE && tolerance_type != BBFMM_ACCURACY_RELATIVE))
        return BBFMM_BAD_ARGUMENT;
    SOLVER_GUARD
    const int rc = check_native_operators(a, a_user, m, m_user, stream);
    if (rc) return rc;
    return fgmres_device(n, a, a_user, d_b, m, m_user, d_x0, max_outer_iterations, max_inner_iterations, tolerance_type, tolerance,
                         callback, cb_user, d_x, iterations, final_residual, static_cast<hipStream_t>(stream));
    SOLVER_END_GUARD
}

int bbfmm_schwarz_ddm_solver_device(int64_t n, bbfmm_apply_device_fn matvec, void *a_user, const double *d_rhs,
                                    bbfmm_apply_device_fn m, void *m_user, int32_t max_iterations, int32_t tolerance_type,
                                    double tolerance, bbfmm_iteration_fn callback, void *cb_user, double *d_x, int64_t *iterations,
                                    double *final_residual, void *stream) {
    if (n < 1 || !matvec || !d_rhs || !d_x || !stream || max_iterations < 0 ||
        (tolerance_type != BBFMM_ACCURACY_ABSOLUTE && tolerance_type != BBFMM_ACCURACY_RELATIVE))
        return BBFMM_BAD_ARGUMENT;
    SOLVER_GUARD
    const int rc = check_native_operators(matvec, a_user, m, m_user, stream);
    if (rc) return rc;
    return schwarz_ddm_device(n, matvec, a_user, d_rhs, m, m_user, max_iterations, tolerance_type, tolerance, callback, cb_user, d_x,
                              iterations, final_residual, static_cast<hipStream_t>(stream));
    SOLVER_END_GUARD
}

int bbfmm_debug_solver_vector_op(int32_t op, int32_t alpha_mode, int64_t n, const double *a, const double *b, const double *c,
                                 double alpha, int32_t count, const double *coeffs, int32_t offset, double *out, double *scalars_out) {
    if (op < 0 || op > 6 || alpha_mode < 0 || alpha_mode > 3 || n < 1 || !a || offset < 0 || offset > 1) return BBFMM_BAD_ARGUMENT;
    const bool needs_b = op == 0 || op == 2 || op == 3 || op == 6, writes = op <= 2 || op == 6, reduces = op != 1 && op != 6;
    if ((needs_b && !b) || (writes && !out) || (reduces && !scalars_out)) return BBFMM_BAD_ARGUMENT;
    if (op == 6 && (count < 1 || count > 64 || !coeffs)) return BBFMM_BAD_ARGUMENT;
    SOLVER_GUARD
    const int cols = op == 6 ? count : 1;
    // vectors start `offset` doubles past a 16-byte boundary; the columns of `a` keep that alignment (an even stride)
    const size_t np = pad_even(n) + 2, nb = static_cast<size_t>(n) * sizeof(double);
    const int64_t nch = solver_chunks(n);
    Workspace ws; // (the null stream)
    int rc = ws.allocate((static_cast<size_t>(cols) + 3) * np + 2 * static_cast<size_t>(nch) + 4 + 64, 4);
    if (rc) return rc;
    double *d_a = ws.d_mem + offset, *d_b = ws.d_mem + static_cast<size_t>(cols) * np + offset, *d_c = d_b + np, *d_o = d_c + np;
    double *part = ws.d_mem + (static_cast<size_t>(cols) + 3) * np, *part2 = part + nch, *slot = part2 + nch, *d_co = slot + 4;
    hipStream_t s = nullptr;
    for (int q = 0; q < cols; ++q) HIPOK(hipMemcpy(d_a + static_cast<size_t>(q) * np, a + static_cast<size_t>(q) * n, nb, hipMemcpyHostToDevice));
    if (b) HIPOK(hipMemcpy(d_b, b, nb, hipMemcpyHostToDevice));
    if (c) HIPOK(hipMemcpy(d_c, c, nb, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(slot + 2, &alpha, sizeof(double), hipMemcpyHostToDevice));
    HIPOK(hipMemset(slot, 0, 2 * sizeof(double)));
    const double *result = d_o;
    switch (op) {
    case 0:
        launch_solver_sub(d_a, d_b, d_o, n, part, part2, s);
        launch_solver_reduce_finish(part, nch, false, false, slot, s);
        launch_solver_reduce_finish(part2, nch, true, false, slot + 1, s);
        break;
    case 1:
        launch_solver_scale(d_a, slot + 2, alpha_mode, alpha, d_o, n, s);
        break;
    case 2:
        launch_solver_axpy_reduce(d_a, slot + 2, alpha_mode, alpha, d_b, c ? d_c : nullptr, n, kReduceDot, part, s);
        launch_solver_reduce_finish(part, nch, false, false, slot, s);
        result = d_b;
        break;
    case 3:
        launch_solver_axpy_reduce(nullptr, nullptr, kAlphaImmediate, 0.0, d_a, d_b, n, kReduceDot, part, s);
        launch_solver_reduce_finish(part, nch, false, false, slot, s);
        break;
    case 4:
        launch_solver_axpy_reduce(nullptr, nullptr, kAlphaImmediate, 0.0, d_a, nullptr, n, kReduceDot, part, s);
        launch_solver_reduce_finish(part, nch, false, true, slot, s);
        break;
    case 5:
        launch_solver_axpy_reduce(nullptr, nullptr, kAlphaImmediate, 0.0, d_a, nullptr, n, kReduceMax, part, s);
        launch_solver_reduce_finish(part, nch, true, false, slot, s);
        break;
    default:
        HIPOK(hipMemcpy(d_co, coeffs, static_cast<size_t>(count) * sizeof(double), hipMemcpyHostToDevice));
        launch_solver_update(d_a, static_cast<int64_t>(np), d_co, count, d_b, n, s);
        result = d_b;
        break;
    }
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(s));
    if (writes) HIPOK(hipMemcpy(out, result, nb, hipMemcpyDeviceToHost));
    if (scalars_out) HIPOK(hipMemcpy(scalars_out, slot, 2 * sizeof(double), hipMemcpyDeviceToHost));
    return BBFMM_OK;
    SOLVER_END_GUARD
}

} // extern "C"
