// extern "C" boundary, the test hooks: the bbfmm_debug_* entries of the tree, the Morton keys, the kernel functions,
// the arithmetic primitives and the M2L tables, the two pipe self-tests and the host copy rates.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "capi_handle.hpp"
#include "morton.hpp"

// The host loop of bbfmm_debug_kernel_values (a template: outside the extern "C" block).
namespace {
template <int ID>
void debug_kernel_values_host(const bbfmm::KernelSpec &ks, const double *r2, int64_t n, double *value, double *value_g, double *factor) {
    for (int64_t i = 0; i < n; ++i) {
        value[i] = bbfmm::kernel_value_r2<ID>(ks, r2[i]);
        value_g[i] = bbfmm::kernel_value_grad_r2<ID>(ks, r2[i], &factor[i]);
    }
}
} // namespace

extern "C" {

int bbfmm_debug_targets_are_sources(const bbfmm_handle *h, const double *x, int64_t m, int64_t ldx) {
    return (h && h->tree.targets_are_sources(x, m, ldx)) ? 1 : 0;
}
int bbfmm_debug_rows_of_sources(bbfmm_handle *h, const double *x, int64_t m, int64_t ldx, int64_t *rows_out) {
    if (!h || !rows_out) return 0;
    try {
        std::vector<int64_t> rows;
        if (!h->tree.targets_are_rows_of_sources(x, m, ldx, &rows)) return 0;
        std::copy(rows.begin(), rows.end(), rows_out);
        return 1;
    } catch (...) {
        return 0;
    }
}

int bbfmm_fp64_valu_selftest(double *tflops, double *clock_mhz) {
    int ndev = 0;
    if (!tflops || !clock_mhz) return BBFMM_BAD_ARGUMENT;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return BBFMM_DEVICE_ERROR;
    return bbfmm::valu_f64_selftest(tflops, clock_mhz) == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
}

int bbfmm_mfma_f64_selftest(double *tflops, int32_t *layout_errors, double *info6) {
    double tf = 0;
    int errs = -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return BBFMM_DEVICE_ERROR;
    const int rc = bbfmm::mfma_f64_selftest(&tf, &errs, info6);
    if (tflops) *tflops = tf;
    if (layout_errors) *layout_errors = errs;
    return rc == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
}

// Host-side legs of the host-buffer entry points, by themselves (scripts/host_buffer_legs.py): n doubles copied by the
// pool in 2 MB pieces (the staging copy), gathered through a random permutation (the row writes of a device group),
// scattered through it.  out4 = {memcpy ms, gather ms, scatter ms, threads}; medians of five.
int bbfmm_debug_host_copy_rates(int64_t n, double *out4) {
    if (n < 1 || !out4) return BBFMM_BAD_ARGUMENT;
    try {
        std::vector<double, bbfmm::DefaultInitAllocator<double>> a(static_cast<size_t>(n)), b(static_cast<size_t>(n));
        std::vector<int32_t> perm(static_cast<size_t>(n));
        bbfmm::parallel_for_chunks(n, int64_t(1) << 18, [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; ++i) a[static_cast<size_t>(i)] = static_cast<double>(i), b[static_cast<size_t>(i)] = 0.0, perm[static_cast<size_t>(i)] = static_cast<int32_t>(i);
        });
        uint64_t st = 88172645463325252ull;
        for (int64_t i = n; i > 1; --i) {
            st ^= st << 13, st ^= st >> 7, st ^= st << 17;
            std::swap(perm[static_cast<size_t>(i - 1)], perm[static_cast<size_t>(st % static_cast<uint64_t>(i))]);
        }
        auto med5 = [&](auto &&fn) {
            double t[5];
            for (double &v : t) {
                const auto t0 = std::chrono::steady_clock::now();
                fn();
                v = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
            std::sort(t, t + 5);
            return t[2];
        };
        out4[0] = med5([&] {
            bbfmm::parallel_for_chunks(n, int64_t(1) << 18, [&](int64_t lo, int64_t hi) { std::memcpy(&b[static_cast<size_t>(lo)], &a[static_cast<size_t>(lo)], static_cast<size_t>(hi - lo) * 8); });
        });
        out4[1] = med5([&] {
            bbfmm::parallel_for_chunks(n, int64_t(1) << 16, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) b[static_cast<size_t>(i)] = a[static_cast<size_t>(perm[static_cast<size_t>(i)])]; });
        });
        out4[2] = med5([&] {
            bbfmm::parallel_for_chunks(n, int64_t(1) << 16, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) b[static_cast<size_t>(perm[static_cast<size_t>(i)])] = a[static_cast<size_t>(i)]; });
        });
        out4[3] = static_cast<double>(bbfmm::host_threads());
        return BBFMM_OK;
    } catch (...) {
        return BBFMM_BAD_ARGUMENT;
    }
}

// Test hooks: the kernel functions and the arithmetic primitives of kernels.hpp, element by element.  where = 0 runs the
// host branch in a plain loop (no device needed), where = 1 the device branch, one thread per element.
int bbfmm_debug_kernel_values(int32_t where, int32_t kernel_id, double base_range, double total_sill, const double *r2, int64_t n,
                              double *value_out, double *value_g_out, double *factor_out) {
    if ((where != 0 && where != 1) || !bbfmm::kernel_id_valid(kernel_id) || n < 0 || !r2 || !value_out || !value_g_out || !factor_out)
        return BBFMM_BAD_ARGUMENT;
    const bbfmm::KernelSpec ks = bbfmm::make_kernel_spec(kernel_id, base_range, total_sill);
    if (where == 0) {
        switch (kernel_id) {
#define BBFMM_DEBUG_CASE(ID) case bbfmm::ID: debug_kernel_values_host<bbfmm::ID>(ks, r2, n, value_out, value_g_out, factor_out); break;
        BBFMM_DEBUG_CASE(kLinear) BBFMM_DEBUG_CASE(kThinPlateSpline) BBFMM_DEBUG_CASE(kCubic) BBFMM_DEBUG_CASE(kSpheroidal3)
        BBFMM_DEBUG_CASE(kSpheroidal5) BBFMM_DEBUG_CASE(kSpheroidal7) BBFMM_DEBUG_CASE(kSpheroidal9) BBFMM_DEBUG_CASE(kLaplacian)
        BBFMM_DEBUG_CASE(kOneOverR2) BBFMM_DEBUG_CASE(kOneOverR4) BBFMM_DEBUG_CASE(kGaussianExt) BBFMM_DEBUG_CASE(kMultiquadricExt)
#undef BBFMM_DEBUG_CASE
        default: return BBFMM_BAD_ARGUMENT;
        }
        return BBFMM_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return BBFMM_DEVICE_ERROR;
    return bbfmm::debug_kernel_values_device(ks, r2, n, value_out, value_g_out, factor_out) == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
}

int bbfmm_debug_math(int32_t where, int32_t which, const double *x, int64_t n, double *out, double *out2) {
    if ((where != 0 && where != 1) || which < 0 || which > 3 || n < 0 || !x || !out) return BBFMM_BAD_ARGUMENT;
    if (where == 0) {
        for (int64_t i = 0; i < n; ++i) {
            double a = 0.0, b = 0.0;
            switch (which) {
            case 0: a = bbfmm::bb_sqrt(x[i]); break;
            case 1: bbfmm::bb_sqrt_rsqrt(x[i], &a, &b); break;
            case 2: a = bbfmm::bb_rcp(x[i]); break;
            default: a = bbfmm::bb_log(x[i]); break;
            }
            out[i] = a;
            if (out2) out2[i] = b;
        }
        return BBFMM_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return BBFMM_DEVICE_ERROR;
    return bbfmm::debug_math_device(which, x, n, out, out2) == 0 ? BBFMM_OK : BBFMM_DEVICE_ERROR;
}

// Test hooks (host only): dense M2M matrix of the reference and the stacked-table M2L.
int bbfmm_debug_dense_m2m(const bbfmm_handle *h, int32_t child_index, double *out) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    std::vector<double> m;
    bbfmm::dense_m2m_matrix(h->tree.ops(), child_index, &m);
    std::memcpy(out, m.data(), m.size() * sizeof(double));
    return BBFMM_OK;
}

int bbfmm_debug_apply_m2l_tables_host(const bbfmm_handle *h, const double *M, double *L) {
    if (!h || !M || !L) return BBFMM_BAD_ARGUMENT;
    return h->tree.debug_apply_m2l_tables_host(M, L);
}

uint64_t bbfmm_debug_morton_encode(int32_t d, const uint64_t *anchor, uint64_t level) {
    if (d < 1 || d > 3 || !anchor) return 0;
    return bbfmm::encode_morton_point(anchor, level, d);
}
void bbfmm_debug_morton_decode(int32_t d, uint64_t key, uint64_t *anchor_out, uint64_t *level_out) {
    if (d < 1 || d > 3 || !anchor_out || !level_out) return;
    bbfmm::decode_key(key, d, anchor_out, level_out);
}
int32_t bbfmm_debug_morton_neighbours(int32_t d, uint64_t key, uint64_t *keys_out) {
    if (d < 1 || d > 3 || !keys_out) return -1;
    return bbfmm::get_neighbours(key, d, keys_out);
}
int32_t bbfmm_debug_direction_vectors(int32_t d, int32_t *out) {
    if (d < 1 || d > 3 || !out) return -1;
    const int(*dirs)[3];
    const int n = bbfmm::direction_vectors(d, &dirs);
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < d; ++a) out[i * d + a] = dirs[i][a];
    return n;
}
int bbfmm_debug_reference_vectors(const bbfmm_handle *h, int32_t *out, int32_t *n_ref_out) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    const bbfmm::Operators &ops = h->tree.ops();
    if (n_ref_out) *n_ref_out = ops.n_ref;
    if (out) std::copy(ops.ref_vecs.begin(), ops.ref_vecs.end(), out);
    return BBFMM_OK;
}

int bbfmm_debug_m2l_variants(const bbfmm_handle *h, int64_t *n_variants, int64_t *n_cells) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    int64_t nv = 0, nc = 0;
    h->tree.m2l_variant_stats(&nv, &nc);
    if (n_variants) *n_variants = nv;
    if (n_cells) *n_cells = nc;
    return BBFMM_OK;
}

// Pairs and singles of the stage-1 operators (FmmTree::debug_m2l_pairs): *n_out = number of values; out (capacity
// cap, may be NULL) receives the first min(cap, *n_out) of them.  *pairs_on: whether the handle pairs at all.
int bbfmm_debug_m2l_pairs(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out, int32_t *pairs_on) {
    if (!h || !n_out) return BBFMM_BAD_ARGUMENT;
    std::vector<int32_t> v;
    h->tree.debug_m2l_pairs(&v);
    *n_out = static_cast<int64_t>(v.size());
    if (pairs_on) *pairs_on = h->tree.m2l_pairs() ? 1 : 0;
    if (out) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, *n_out), out);
    return BBFMM_OK;
}

// The stage-1 operators with their x pairs, y pairs and column-block kinds (FmmTree::debug_m2l_pairs_axes).
int bbfmm_debug_m2l_pairs_axes(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out) {
    if (!h || !n_out) return BBFMM_BAD_ARGUMENT;
    std::vector<int32_t> v;
    h->tree.debug_m2l_pairs_axes(&v);
    *n_out = static_cast<int64_t>(v.size());
    if (out) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, *n_out), out);
    return BBFMM_OK;
}

// The same for the stage-2 operators (FmmTree::debug_m2l_pairs_stage2).
int bbfmm_debug_m2l_pairs_stage2(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out, int32_t *pairs_on) {
    if (!h || !n_out) return BBFMM_BAD_ARGUMENT;
    std::vector<int32_t> v;
    h->tree.debug_m2l_pairs_stage2(&v);
    *n_out = static_cast<int64_t>(v.size());
    if (pairs_on) *pairs_on = h->tree.m2l_pairs_stage2() ? 1 : 0;
    if (out) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, *n_out), out);
    return BBFMM_OK;
}

// The stage-2 operators with their x pairs, y pairs, singles and slot offsets (FmmTree::debug_m2l_pairs_axes_stage2).
int bbfmm_debug_m2l_pairs_axes_stage2(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out) {
    if (!h || !n_out) return BBFMM_BAD_ARGUMENT;
    std::vector<int32_t> v;
    h->tree.debug_m2l_pairs_axes_stage2(&v);
    *n_out = static_cast<int64_t>(v.size());
    if (out) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, *n_out), out);
    return BBFMM_OK;
}

// The stage-2 kernel instance of the parity basis: ga, gb, ce, co, ya, yb (FmmTree::debug_m2l_s2_plan).
int bbfmm_debug_m2l_s2_plan(const bbfmm_handle *h, int32_t *out) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    h->tree.debug_m2l_s2_plan(out);
    return BBFMM_OK;
}

// The W / X jobs of the resident target set (FmmTree::debug_wx_jobs).
int bbfmm_debug_wx_jobs(const bbfmm_handle *h, int32_t *out) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    return h->tree.debug_wx_jobs(out);
}

// Digests of the integer M2L tables, one per family, and the per-level flop counts (FmmTree::debug_m2l_table_digests).
int bbfmm_debug_m2l_table_digests(const bbfmm_handle *h, uint64_t *digests, int32_t cap, int32_t *n_out, double *flops_level,
                                  int32_t flops_cap, int32_t *n_levels_out) {
    if (!h || !n_out) return BBFMM_BAD_ARGUMENT;
    std::vector<uint64_t> v;
    h->tree.debug_m2l_table_digests(&v);
    *n_out = static_cast<int32_t>(v.size());
    if (digests) std::copy(v.begin(), v.begin() + std::min<int32_t>(cap, *n_out), digests);
    const std::vector<double> &fl = h->tree.m2l_flops_level();
    if (n_levels_out) *n_levels_out = static_cast<int32_t>(fl.size());
    if (flops_level) std::copy(fl.begin(), fl.begin() + std::min<int32_t>(flops_cap, static_cast<int32_t>(fl.size())), flops_level);
    return BBFMM_OK;
}

// Debug only: parts into which the handle's most recent parity-basis stage-2 launch split the contraction (0: no launch yet).
int bbfmm_debug_m2l_s2_last_ksplit(const bbfmm_handle *h, int32_t *ksplit) {
    if (!h || !ksplit) return BBFMM_BAD_ARGUMENT;
    *ksplit = h->tree.debug_m2l_s2_last_ksplit();
    return BBFMM_OK;
}

int bbfmm_debug_leaf_runs(const bbfmm_handle *h, int32_t *counts) {
    if (!h || !counts) return BBFMM_BAD_ARGUMENT;
    h->tree.debug_leaf_runs(counts);
    return BBFMM_OK;
}

// Debug only: what a device group holds and has queued (DeviceGroup::debug_state lists the values); a plain handle is one
// part that owns itself, with zeros.  cap: room in out, at least 9 + the handle's parts.
int bbfmm_debug_group_state(const bbfmm_handle *h, int64_t *out, int64_t cap) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    const int64_t need = bbfmm::DeviceGroup::kStateHeader + (h->group ? h->group->n_parts() : 1);
    if (cap < need) return BBFMM_BAD_ARGUMENT;
    std::fill(out, out + need, int64_t(0));
    if (h->group)
        h->group->debug_state(out);
    else
        out[0] = 1;
    return BBFMM_OK;
}

// Debug only: values per row of the multipoles in stage 1's parity basis (what debug_get_coefficients('P') returns per cell);
// 0 when the handle has none.
int bbfmm_debug_m2l_parity_len(const bbfmm_handle *h, int32_t *len) {
    if (!h || !len) return BBFMM_BAD_ARGUMENT;
    *len = h->tree.debug_m2l_parity_len();
    return BBFMM_OK;
}

int bbfmm_debug_get_coefficients(bbfmm_handle *h, char which, int32_t k, double *out) {
    GUARD(h) return h->tree.debug_get_coefficients(which, k, out);
    END_GUARD(h)
}

} // extern "C"
