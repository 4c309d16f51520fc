// extern "C" boundary: evaluation at device-resident targets and on regular grids (fmm_tree.hpp evaluate_device,
// evaluate_grid.hpp).
#include <algorithm>
#include <cstddef>
#include <string>

#include "capi_handle.hpp"
#include "evaluate_grid.hpp"
#include "interpolant_terms.hpp"

namespace {

struct EvalOptions {
    bool batch_independent = false;
    int32_t cap = 0;
    int64_t batch_bytes = 0;
    bool outputs_on_device = false;
};

// The fields of *o that its size covers; defaults for the rest and for o == nullptr.
bool eval_options(const bbfmm_evaluate_options *o, const bbfmm::FmmTree &tree, EvalOptions *out, std::string *err) {
    int32_t bi = -1, cap = -1;
    if (o) {
        if (o->size < static_cast<int64_t>(sizeof(int64_t))) {
            *err = "evaluate: options->size must be sizeof(bbfmm_evaluate_options)";
            return false;
        }
        auto covers = [o](size_t off, size_t len) { return o->size >= static_cast<int64_t>(off + len); };
        if (covers(offsetof(bbfmm_evaluate_options, batch_independent), sizeof(int32_t))) bi = o->batch_independent;
        if (covers(offsetof(bbfmm_evaluate_options, max_job_targets), sizeof(int32_t))) cap = o->max_job_targets;
        if (covers(offsetof(bbfmm_evaluate_options, batch_bytes), sizeof(int64_t))) out->batch_bytes = o->batch_bytes;
        if (covers(offsetof(bbfmm_evaluate_options, outputs_on_device), sizeof(int32_t))) out->outputs_on_device = o->outputs_on_device != 0;
    }
    if (bi < -1 || bi > 1 || cap < -1) {
        *err = "evaluate: batch_independent is -1, 0 or 1 and max_job_targets -1, 0 or a positive count";
        return false;
    }
    out->batch_independent = bi < 0 ? tree.deterministic() : bi != 0;
    out->cap = cap < 0 ? bbfmm::kDefaultMaxJobTargets : cap;
    return true;
}

int eval_fail(bbfmm_handle *h, int rc, const std::string &msg) {
    h->err = msg;
    return rc;
}

// Leaves mode on the handle's own tree (of a device group: the primary part with the stored expansions).
int eval_prepare(bbfmm_handle *h) {
    if (h->tree.host_only()) return eval_fail(h, BBFMM_DEVICE_ERROR, "handle was created with BBFMM_FLAG_HOST_ONLY");
    if (h->group) return group_rc(h, h->group->prepare_primary(true));
    return BBFMM_OK;
}

} // namespace

extern "C" {

int bbfmm_evaluate_device(bbfmm_handle *h, int32_t with_gradients, const double *d_x, int64_t m, int64_t ldx,
                          const bbfmm_interpolant_terms *terms, double *d_values, int64_t ldo, double *d_grad, int64_t ldg,
                          const bbfmm_evaluate_options *options, int64_t *bad_point_index) {
    GUARD(h)
    EvalOptions eo;
    std::string err;
    if (!eval_options(options, h->tree, &eo, &err)) return eval_fail(h, BBFMM_BAD_ARGUMENT, err);
    if (with_gradients && !d_grad && m > 0) return eval_fail(h, BBFMM_BAD_ARGUMENT, "evaluate_device: gradients need their array");
    bbfmm::InterpolantTerms t;
    if (terms && !bbfmm::terms_from_abi(terms, &t))
        return eval_fail(h, BBFMM_BAD_ARGUMENT, "evaluate_device: bad terms (size, d, k, degree -1 .. 2, coefficients, scale != 0)");
    const int prc = eval_prepare(h);
    if (prc != BBFMM_OK) return prc;
    return h->tree.evaluate_device(d_x, m, ldx, terms ? &t : nullptr, d_values, ldo, with_gradients ? d_grad : nullptr, ldg,
                                   eo.batch_independent, eo.cap, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_grid(bbfmm_handle *h, int32_t with_gradients, const bbfmm_grid *grid, const bbfmm_interpolant_terms *terms,
                        double *values_out, int64_t ldo, double *grad_out, int64_t ldg, const bbfmm_evaluate_options *options,
                        int64_t *bad_point_index) {
    GUARD(h)
    for (int64_t &v : h->grid_stats) v = 0;
    EvalOptions eo;
    std::string err;
    if (!eval_options(options, h->tree, &eo, &err)) return eval_fail(h, BBFMM_BAD_ARGUMENT, err);
    bbfmm::GridSpec g;
    const int d = h->tree.tree().d;
    if (!bbfmm::grid_from_abi(grid, &g) || g.d != d)
        return eval_fail(h, BBFMM_BAD_ARGUMENT, "evaluate_grid: bad grid (size, d of the tree, shape >= 0, finite origin and steps)");
    bbfmm::InterpolantTerms t;
    if (terms && !bbfmm::terms_from_abi(terms, &t))
        return eval_fail(h, BBFMM_BAD_ARGUMENT, "evaluate_grid: bad terms (size, d, k, degree -1 .. 2, coefficients, scale != 0)");
    const int prc = eval_prepare(h);
    if (prc != BBFMM_OK) return prc;
    bbfmm::FmmTree &tree = h->tree;
    const int k = tree.nrhs();
    const int64_t M = g.rows();
    h->grid_stats[0] = M;
    if (M == 0) return BBFMM_OK;
    if (!values_out || ldo < M || (with_gradients && (!grad_out || ldg < M)))
        return eval_fail(h, BBFMM_BAD_ARGUMENT, "evaluate_grid: bad output arrays (leading dimensions >= the grid's rows)");
    if (k < 1) return eval_fail(h, BBFMM_BAD_ARGUMENT, "set_local_coefficients must be called first");
    // Device memory per node of a slab: the coordinates, their transformed copy under a trend and
    // their copy sorted by leaf (8 d each), cell / sorted cell / permutation / head flag and the sort's scratch (32),
    // the values and gradients in sorted order and, for host outputs, again in row order (8 per column each).
    const int64_t cols = static_cast<int64_t>(k) * (with_gradients ? 1 + d : 1);
    const int64_t per_node = 8 * d * (t.has_affine && terms ? 3 : 2) + 32 + 8 * cols * (eo.outputs_on_device ? 1 : 2);
    const int64_t budget = eo.batch_bytes > 0 ? eo.batch_bytes : (int64_t(1) << 31);
    const int64_t max_rows = std::max<int64_t>(1, std::min<int64_t>(budget / per_node, (int64_t(1) << 31) - 1));
    const int64_t plane = g.plane();
    // whole planes of the leading index while one fits; a plane that does not is cut by rows
    const int64_t planes_per_slab = max_rows / plane, slab_cap = planes_per_slab > 0 ? std::min(M, planes_per_slab * plane) : std::min(plane, max_rows);
    bbfmm::DevBuffer<> x, vals, grads; // (never empty: at least one element each)
    const bool stage = !eo.outputs_on_device;
    if (!x.reserve(std::max<int64_t>(slab_cap * d, 1)) || (stage && !vals.reserve(std::max<int64_t>(slab_cap * k, 1))) ||
        (stage && with_gradients && !grads.reserve(std::max<int64_t>(slab_cap * k * d, 1))))
        return eval_fail(h, BBFMM_DEVICE_ERROR, "evaluate_grid: out of device memory for a slab (lower batch_bytes)");
    auto run_slab = [&](int64_t r0, int64_t n) -> int {
        if (bbfmm::grid_coords_device(g, r0, n, x.p, n, tree.stream()) != 0) return eval_fail(h, BBFMM_DEVICE_ERROR, "evaluate_grid: the coordinate kernel failed");
        double *dv = stage ? vals.p : values_out + r0, *dg = !with_gradients ? nullptr : (stage ? grads.p : grad_out + r0);
        const int64_t lv = stage ? n : ldo, lg = stage ? n : ldg;
        int64_t bad = -1;
        bbfmm::TargetSetStats st;
        const int rc = tree.evaluate_device(x.p, n, n, terms ? &t : nullptr, dv, lv, dg, lg, eo.batch_independent, eo.cap, &bad, &st);
        if (rc != BBFMM_OK) {
            if (rc == BBFMM_POINT_OUTSIDE_TREE && bad_point_index) *bad_point_index = r0 + bad;
            return rc;
        }
        h->grid_stats[1] += 1;
        h->grid_stats[2] += st.runs;
        h->grid_stats[3] += st.jobs;
        h->grid_stats[4] = std::max(h->grid_stats[4], st.largest);
        h->grid_stats[5] += st.w_jobs;
        if (stage) {
            if (hipMemcpy2D(values_out + r0, sizeof(double) * static_cast<size_t>(ldo), dv, sizeof(double) * static_cast<size_t>(n),
                            sizeof(double) * static_cast<size_t>(n), static_cast<size_t>(k), hipMemcpyDeviceToHost) != hipSuccess)
                return eval_fail(h, BBFMM_DEVICE_ERROR, "evaluate_grid: copy of the values to the host");
            if (dg && hipMemcpy2D(grad_out + r0, sizeof(double) * static_cast<size_t>(ldg), dg, sizeof(double) * static_cast<size_t>(n),
                                  sizeof(double) * static_cast<size_t>(n), static_cast<size_t>(k) * d, hipMemcpyDeviceToHost) != hipSuccess)
                return eval_fail(h, BBFMM_DEVICE_ERROR, "evaluate_grid: copy of the gradients to the host");
        }
        return BBFMM_OK;
    };
    if (planes_per_slab > 0) {
        for (int64_t r0 = 0; r0 < M; r0 += slab_cap) {
            const int rc = run_slab(r0, std::min(slab_cap, M - r0));
            if (rc != BBFMM_OK) return rc;
        }
    } else {
        for (int64_t p0 = 0; p0 < M; p0 += plane)
            for (int64_t r0 = p0; r0 < p0 + plane; r0 += slab_cap) {
                const int rc = run_slab(r0, std::min(slab_cap, p0 + plane - r0));
                if (rc != BBFMM_OK) return rc;
            }
    }
    return BBFMM_OK;
    END_GUARD(h)
}

int bbfmm_evaluate_grid_stats(bbfmm_handle *h, int64_t *stats_out) {
    if (!h || !stats_out) return BBFMM_BAD_ARGUMENT;
    std::copy(h->grid_stats, h->grid_stats + 8, stats_out);
    return BBFMM_OK;
}

int bbfmm_debug_grid_coords(int32_t where, const bbfmm_grid *grid, int64_t r0, int64_t n, double *out, int64_t ld) {
    bbfmm::GridSpec g;
    if ((where != 0 && where != 1) || !bbfmm::grid_from_abi(grid, &g) || r0 < 0 || n < 0 || r0 + n > g.rows() || ld < n || (n > 0 && !out))
        return BBFMM_BAD_ARGUMENT;
    if (n == 0) return BBFMM_OK;
    if (where == 0) {
        bbfmm::grid_coords_host(g, r0, n, out, ld);
        return BBFMM_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return BBFMM_DEVICE_ERROR;
    bbfmm::DevBuffer<> x;
    if (!x.reserve(std::max<int64_t>(n * g.d, 1)) || bbfmm::grid_coords_device(g, r0, n, x.p, n, nullptr) != 0 ||
        hipMemcpy2D(out, sizeof(double) * static_cast<size_t>(ld), x.p, sizeof(double) * static_cast<size_t>(n),
                    sizeof(double) * static_cast<size_t>(n), static_cast<size_t>(g.d), hipMemcpyDeviceToHost) != hipSuccess)
        return BBFMM_DEVICE_ERROR;
    return BBFMM_OK;
}

int bbfmm_debug_split_runs(int32_t where, const int32_t *tgt_begin, const int32_t *tgt_end, const int32_t *job_cell, int64_t n_runs,
                           int32_t cap, int32_t *out_begin, int32_t *out_end, int32_t *out_cell, int64_t capacity,
                           int64_t *n_jobs_out) {
    if ((where != 0 && where != 1) || n_runs < 0 || cap < 1 || !n_jobs_out || (n_runs > 0 && (!tgt_begin || !tgt_end || !job_cell)))
        return BBFMM_BAD_ARGUMENT;
    int64_t total = 0;
    for (int64_t r = 0; r < n_runs; ++r) {
        if (tgt_end[r] < tgt_begin[r]) return BBFMM_BAD_ARGUMENT;
        total += tgt_end[r] - tgt_begin[r];
    }
    const int64_t n_jobs = bbfmm::split_runs_host(job_cell, tgt_begin, tgt_end, n_runs, cap, nullptr, nullptr, nullptr);
    *n_jobs_out = n_jobs;
    const bool fill = out_begin && out_end && out_cell;
    if (!fill || n_jobs == 0) return BBFMM_OK;
    if (n_jobs > capacity) return BBFMM_BAD_ARGUMENT;
    if (where == 0) {
        bbfmm::split_runs_host(job_cell, tgt_begin, tgt_end, n_runs, cap, out_cell, out_begin, out_end);
        return BBFMM_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return BBFMM_DEVICE_ERROR;
    // one allocation: the three inputs, cnt, offs (n_runs each), the three outputs (jcap each), the count, the scan's scratch
    const size_t nr = static_cast<size_t>(n_runs), jcap = static_cast<size_t>(bbfmm::split_jobs_capacity(n_runs, total, cap));
    const size_t temp_bytes = bbfmm::split_runs_temp_bytes(n_runs);
    const size_t ints = 5 * nr + 3 * jcap + 2;
    bbfmm::DevBuffer<uint8_t> mem;
    const size_t temp_off = (ints * sizeof(int32_t) + 255) & ~size_t(255);
    if (!mem.reserve(static_cast<int64_t>(temp_off + std::max<size_t>(temp_bytes, 1)))) return BBFMM_DEVICE_ERROR;
    int32_t *base = reinterpret_cast<int32_t *>(mem.p);
    int32_t *d_jc = base, *d_tb = base + nr, *d_te = base + 2 * nr, *d_cnt = base + 3 * nr, *d_offs = base + 4 * nr;
    int32_t *o_jc = base + 5 * nr, *o_tb = o_jc + jcap, *o_te = o_tb + jcap, *d_n = o_te + jcap;
    if (hipMemcpy(d_jc, job_cell, nr * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_tb, tgt_begin, nr * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_te, tgt_end, nr * 4, hipMemcpyHostToDevice) != hipSuccess)
        return BBFMM_DEVICE_ERROR;
    if (bbfmm::split_runs(d_jc, d_tb, d_te, n_runs, cap, d_cnt, d_offs, o_jc, o_tb, o_te, static_cast<int64_t>(jcap), d_n, mem.p + temp_off, temp_bytes,
                          nullptr) != 0)
        return BBFMM_DEVICE_ERROR;
    int32_t got = -1;
    if (hipMemcpy(&got, d_n, 4, hipMemcpyDeviceToHost) != hipSuccess) return BBFMM_DEVICE_ERROR;
    *n_jobs_out = got;
    if (got != n_jobs) return BBFMM_DEVICE_ERROR;
    const size_t nj = static_cast<size_t>(n_jobs);
    if (hipMemcpy(out_cell, o_jc, nj * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(out_begin, o_tb, nj * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out_end, o_te, nj * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return BBFMM_DEVICE_ERROR;
    return BBFMM_OK;
}

} // extern "C"
