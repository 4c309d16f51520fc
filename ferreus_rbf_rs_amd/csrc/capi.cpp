// extern "C" boundary: include/ferreus_bbfmm_hip.h over bbfmm::FmmTree and bbfmm::DeviceGroup.  This file: handles,
// weights, the host evaluations, the matvec entries, partitions and the getters of the tree; the isosurface, field,
// device-evaluation and debug entries are in capi_isosurface.cpp, capi_fields.cpp, capi_evaluate.cpp and capi_debug.cpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi_handle.hpp"

// The four bbfmm_evaluate* inside their guard.  Over a device group the targets are sharded over the parts where the
// group takes them; anything else is the primary's alone.
static int evaluate_any(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw, const double *x, int64_t m, int64_t ldx,
                        double *out, int64_t ldo, double *grad, int64_t ldg, bool with_gradients, bool leaves_only,
                        int64_t *bad_point_index) {
    if (h->group) {
        bool handled = false;
        int rc = h->group->evaluate_sharded(w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, with_gradients, leaves_only, bad_point_index, &handled);
        if (rc != BBFMM_OK || handled) return group_rc(h, rc);
        // (weights_match_staged compared once per entry would be kept here: ADVICE.md)
        const bool null_is_staged = with_gradients || leaves_only; // bbfmm_evaluate itself always compares
        rc = group_rc(h, h->group->prepare_primary((null_is_staged && !w) || h->group->weights_match_staged(w, rows, k, ldw)));
        if (rc != BBFMM_OK) return rc;
    }
    return h->tree.evaluate(w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, with_gradients, leaves_only, bad_point_index);
}

// An entry that a handle over a device group does not take: true with the handle's message set.
static bool refuse_group(bbfmm_handle *h, const char *message) {
    if (h->group) h->err = message;
    return h->group != nullptr;
}
static const char kExchangeIsTheLibrarys[] = "the handle spans a device group: the exchange is the library's";

extern "C" {

void bbfmm_params_defaults(int32_t interpolation_order, bbfmm_params *out) {
    if (!out) return;
    out->max_points_per_cell = 256;
    out->compression_type = BBFMM_COMPRESSION_ACA;
    double eps = 1.0; // 10f64.powi(-order), bbfmm.rs:100
    for (int i = 0; i < interpolation_order; ++i) eps *= 10.0;
    out->epsilon = 1.0 / eps;
    out->eval_chunk_size = 1024;
}

// bbfmm_create on an explicit device list; devices == NULL: the current device (and no group).
static int create_impl(const double *pts, int64_t n, int32_t d, int64_t ld, int32_t interpolation_order, int32_t kernel_type,
                       double base_range, double total_sill, int32_t adaptive_tree, int32_t sparse, const double *extents,
                       const bbfmm_params *params, uint32_t flags, const std::vector<int> &devices, bbfmm_handle **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    *out = nullptr;
    bbfmm_handle *h = nullptr;
    int cur = -1;
    try {
        h = new bbfmm_handle();
        *out = h; // returned even on failure so that bbfmm_last_error can be read; the caller destroys it either way
        if (!devices.empty()) {
            if (flags & BBFMM_FLAG_HOST_ONLY) {
                h->err = "a device list needs devices (BBFMM_FLAG_HOST_ONLY is set)";
                return BBFMM_BAD_ARGUMENT;
            }
            int ndev = 0;
            if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
                h->err = "no HIP device available (the BBFMM passes have no CPU fallback)";
                return BBFMM_DEVICE_ERROR;
            }
            for (int dev : devices)
                if (dev < 0 || dev >= ndev) {
                    h->err = "device " + std::to_string(dev) + " of the device list does not exist (" + std::to_string(ndev) + " visible)";
                    return BBFMM_BAD_ARGUMENT;
                }
            if (devices.size() > static_cast<size_t>(bbfmm::kMaxScatterParts)) {
                h->err = "more parts in the device list than a handle takes";
                return BBFMM_BAD_ARGUMENT;
            }
            (void)hipGetDevice(&cur);
            if (hipSetDevice(devices[0]) != hipSuccess) {
                h->err = "hipSetDevice failed for the first device of the list";
                return BBFMM_DEVICE_ERROR;
            }
        }
        int rc = h->tree.create(pts, n, d, ld, interpolation_order, kernel_type, base_range, total_sill, adaptive_tree != 0, sparse != 0,
                                extents, params, flags);
        if (rc == BBFMM_OK && devices.size() > 1) {
            h->group.reset(new bbfmm::DeviceGroup());
            const bbfmm::GroupCreateArgs a{pts, n, d, ld, interpolation_order, kernel_type, base_range, total_sill, adaptive_tree != 0,
                                           sparse != 0, extents, params, flags};
            rc = h->group->init(&h->tree, a, devices);
            if (rc != BBFMM_OK) {
                h->err = h->group->last_error();
                h->group.reset();
            }
        }
        if (cur >= 0) (void)hipSetDevice(cur); // the caller's current device is not the library's to change
        return rc;
    } catch (const std::exception &e) {
        if (cur >= 0) (void)hipSetDevice(cur);
        if (h) h->err = std::string("exception: ") + e.what();
        return BBFMM_BAD_ARGUMENT;
    } catch (...) {
        if (cur >= 0) (void)hipSetDevice(cur);
        if (h) h->err = "unknown exception";
        return BBFMM_BAD_ARGUMENT;
    }
}

int bbfmm_create(const double *pts, int64_t n, int32_t d, int64_t ld, int32_t interpolation_order,
                 int32_t kernel_type, double base_range, double total_sill, int32_t adaptive_tree, int32_t sparse,
                 const double *extents, const bbfmm_params *params, uint32_t flags, bbfmm_handle **out) {
    // FERREUS_BBFMM_DEVICES: the device list of every handle this process creates through the reference's constructor,
    // which has no argument for it ("0,1,2,3", "all", or "0,0" for logical parts on one device).  Host-only handles
    // (structure tests) ignore it.
    std::vector<int> devices;
    const char *env = std::getenv("FERREUS_BBFMM_DEVICES");
    if (env && *env && !(flags & BBFMM_FLAG_HOST_ONLY)) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
        std::string perr;
        if (!bbfmm::parse_device_list(env, ndev, &devices, &perr)) {
            if (!out) return BBFMM_BAD_ARGUMENT;
            bbfmm_handle *h = new (std::nothrow) bbfmm_handle();
            if (h) h->err = "FERREUS_BBFMM_DEVICES: " + perr;
            *out = h;
            return BBFMM_BAD_ARGUMENT;
        }
    }
    return create_impl(pts, n, d, ld, interpolation_order, kernel_type, base_range, total_sill, adaptive_tree, sparse, extents, params, flags,
                       devices, out);
}

int bbfmm_create_on_devices(const double *pts, int64_t n, int32_t d, int64_t ld, int32_t interpolation_order, int32_t kernel_type,
                            double base_range, double total_sill, int32_t adaptive_tree, int32_t sparse, const double *extents,
                            const bbfmm_params *params, uint32_t flags, const int32_t *devices, int32_t n_devices, bbfmm_handle **out) {
    if (!out) return BBFMM_BAD_ARGUMENT;
    *out = nullptr;
    if (!devices || n_devices < 1) return BBFMM_BAD_ARGUMENT;
    return create_impl(pts, n, d, ld, interpolation_order, kernel_type, base_range, total_sill, adaptive_tree, sparse, extents, params, flags,
                       std::vector<int>(devices, devices + n_devices), out);
}

int32_t bbfmm_device_count(const bbfmm_handle *h) { return !h ? -1 : (h->group ? h->group->n_parts() : 1); }
int32_t bbfmm_part_device(const bbfmm_handle *h, int32_t part) {
    if (!h || part < 0) return -1;
    if (h->group) return part < h->group->n_parts() ? h->group->part_device(part) : -1;
    return part == 0 ? h->tree.device() : -1;
}
int bbfmm_group_bounds(const bbfmm_handle *h, int64_t *bounds_out) {
    if (!h || !h->group || !bounds_out) return BBFMM_BAD_ARGUMENT;
    const std::vector<int64_t> &b = h->group->bounds();
    std::copy(b.begin(), b.end(), bounds_out);
    return BBFMM_OK;
}
int bbfmm_get_part_phase_ms(bbfmm_handle *h, int32_t part, double *ms_out, int64_t *count_out) {
    if (!h || !ms_out) return BBFMM_BAD_ARGUMENT;
    if (h->group) return h->group->part_phase_ms(part, ms_out, count_out);
    return part == 0 ? bbfmm_get_phase_ms(h, ms_out, count_out) : BBFMM_BAD_ARGUMENT;
}

void bbfmm_destroy(bbfmm_handle *h) {
    if (!h) return;
    h->group.reset(); // (its parts end before the primary they lean on)
    delete h;
}

const char *bbfmm_last_error(const bbfmm_handle *h) {
    if (!h) return "null handle";
    if (!h->err.empty()) return h->err.c_str();
    return h->tree.last_error();
}

int bbfmm_set_weights(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw) {
    GUARD(h)
    if (h->group) return group_rc(h, h->group->set_weights(w, rows, k, ldw));
    return h->tree.set_weights(w, rows, k, ldw);
    END_GUARD(h)
}

int bbfmm_set_local_coefficients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw) {
    GUARD(h)
    if (h->group) { // the weights of set_weights: every part stores the whole-tree expansions (Leaves mode over the group)
        bool handled = false;
        int rc = group_rc(h, h->group->set_local_coefficients_all(w, rows, k, ldw, &handled));
        if (rc != BBFMM_OK || handled) return rc;
        rc = group_rc(h, h->group->prepare_primary(false)); // other weights: the primary alone
        if (rc != BBFMM_OK) return rc;
    }
    return h->tree.set_local_coefficients(w, rows, k, ldw);
    END_GUARD(h)
}

int bbfmm_evaluate(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw, const double *x, int64_t m,
                   int64_t ldx, double *out, int64_t ldo, int64_t *bad_point_index) {
    GUARD(h)
    if (h->group) { // targets = sources with the weights of set_weights: partitioned over the group; anything else: the primary
        bool handled = false;
        int rc = group_rc(h, h->group->evaluate_at_sources(w, rows, k, ldw, x, m, ldx, out, ldo, &handled));
        if (rc != BBFMM_OK || handled) return rc;
        rc = h->group->evaluate_rows_of_sources(w, rows, k, ldw, x, m, ldx, out, &handled); // the unchanged caller's matvec_partial
        if (rc != BBFMM_OK || handled) return group_rc(h, rc);
    }
    return evaluate_any(h, w, rows, k, ldw, x, m, ldx, out, ldo, nullptr, 0, false, false, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_with_gradients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw,
                                  const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo, double *grad,
                                  int64_t ldg, int64_t *bad_point_index) {
    GUARD(h) return evaluate_any(h, w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, true, false, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_leaves(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw, const double *x,
                          int64_t m, int64_t ldx, double *out, int64_t ldo, int64_t *bad_point_index) {
    GUARD(h) return evaluate_any(h, w, rows, k, ldw, x, m, ldx, out, ldo, nullptr, 0, false, true, bad_point_index);
    END_GUARD(h)
}

int bbfmm_evaluate_leaves_with_gradients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw,
                                         const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo,
                                         double *grad, int64_t ldg, int64_t *bad_point_index) {
    GUARD(h) return evaluate_any(h, w, rows, k, ldw, x, m, ldx, out, ldo, grad, ldg, true, true, bad_point_index);
    END_GUARD(h)
}

int bbfmm_source_points(const bbfmm_handle *h, double *out, int64_t ld) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    const auto &p = h->tree.source_points();
    const int64_t n = h->tree.tree().n_points;
    const int d = h->tree.tree().d;
    if (ld < n) return BBFMM_BAD_ARGUMENT;
    for (int a = 0; a < d; ++a) std::memcpy(out + a * ld, p.data() + static_cast<size_t>(a) * n, n * sizeof(double));
    return BBFMM_OK;
}

int bbfmm_fast_matrix_vector_product(bbfmm_handle *h, const double *w, int64_t rows, int64_t basis_size,
                                     const int64_t *target_indices, int64_t n_target_indices, const double *poly,
                                     int64_t ldp, double nugget, double *result) {
    GUARD(h)
    if (h->group) {
        if (!target_indices || h->tree.is_identity_subset(target_indices, n_target_indices))
            return group_rc(h, h->group->fast_matrix_vector_product(w, rows, basis_size, poly, ldp, nugget, result));
        // a row subset (matvec_partial, rbf.rs:119-133): every part takes the rows of the set it owns
        return group_rc(h, h->group->fast_matvec_subset(w, rows, basis_size, target_indices, n_target_indices, poly, ldp, nugget, result));
    }
    return h->tree.fast_matrix_vector_product(w, rows, basis_size, target_indices, n_target_indices, poly, ldp, nugget,
                                              result);
    END_GUARD(h)
}

int bbfmm_prepare_target_subset(bbfmm_handle *h, const int64_t *target_indices, int64_t n_target_indices) {
    GUARD(h) return h->tree.prepare_target_subset(target_indices, n_target_indices);
    END_GUARD(h)
}

int bbfmm_matvec_device(bbfmm_handle *h, const double *d_w, int64_t ldw, int32_t k, double *d_out, int64_t ldo,
                        int32_t sync) {
    GUARD(h)
    if (h->group) return group_rc(h, h->group->matvec_device(d_w, ldw, k, d_out, ldo, sync != 0));
    return h->tree.matvec_device(d_w, ldw, k, d_out, ldo, sync != 0);
    END_GUARD(h)
}

void *bbfmm_stream(bbfmm_handle *h) {
    if (!h) return nullptr;
    h->tree.bind_device();
    return static_cast<void *>(h->tree.stream());
}

int bbfmm_target_subset_create(bbfmm_handle *h, const int64_t *target_indices, int64_t n_target_indices,
                               int32_t *subset_id) {
    GUARD(h)
    int id = 0;
    const int rc = h->tree.register_subset(target_indices, n_target_indices, &id);
    if (rc == BBFMM_OK && subset_id) *subset_id = id;
    return rc;
    END_GUARD(h)
}

int bbfmm_matvec_subset_device(bbfmm_handle *h, int32_t subset_id, const double *d_w, double *d_y, int32_t sync) {
    GUARD(h)
    if (h->group) {
        if (subset_id == -1) return group_rc(h, h->group->matvec_device(d_w, h->tree.tree().n_points, 1, d_y, h->tree.tree().n_points, sync != 0));
        h->group->primary_state_changed(); // a registered row subset: the primary alone
    }
    return h->tree.matvec_subset_device(subset_id, d_w, d_y, sync != 0);
    END_GUARD(h)
}

int bbfmm_set_partition(bbfmm_handle *h, int32_t rank, int32_t world) {
    GUARD(h)
    if (refuse_group(h, "the handle spans a device group: its partition is the group's")) return BBFMM_BAD_ARGUMENT;
    return h->tree.set_partition(rank, world);
    END_GUARD(h)
}

int64_t bbfmm_partition_row_count(const bbfmm_handle *h) {
    if (!h) return -1;
    const auto &r = h->tree.partition_rows();
    return h->tree.partitioned() ? static_cast<int64_t>(r.size()) : h->tree.tree().n_points;
}

int bbfmm_partition_rows(const bbfmm_handle *h, int64_t *rows_out) {
    if (!h || !rows_out) return BBFMM_BAD_ARGUMENT;
    const auto &r = h->tree.partition_rows();
    if (!h->tree.partitioned()) {
        for (int64_t i = 0; i < h->tree.tree().n_points; ++i) rows_out[i] = i;
    } else if (!r.empty()) {
        std::memcpy(rows_out, r.data(), r.size() * sizeof(int64_t));
    }
    return BBFMM_OK;
}

int64_t bbfmm_partition_coarse_count(const bbfmm_handle *h) { return h ? h->tree.partition_coarse_count() : -1; }

int bbfmm_matvec_partition_upward(bbfmm_handle *h, const double *d_w, int64_t ldw, int32_t k, double *d_coarse, void *comm_stream) {
    GUARD(h)
    if (refuse_group(h, kExchangeIsTheLibrarys)) return BBFMM_BAD_ARGUMENT;
    return h->tree.matvec_partition_upward(d_w, ldw, k, d_coarse, static_cast<hipStream_t>(comm_stream));
    END_GUARD(h)
}

int32_t bbfmm_partition_world(const bbfmm_handle *h) {
    if (!h) return -1;
    const std::vector<int64_t> &b = h->tree.partition_bounds();
    return b.empty() ? 1 : static_cast<int32_t>(b.size()) - 1;
}
int32_t bbfmm_partition_rank(const bbfmm_handle *h) { return h ? h->tree.partition_rank() : -1; }
int bbfmm_partition_bounds(const bbfmm_handle *h, int32_t world, int64_t *bounds_out) {
    if (!h || !bounds_out) return BBFMM_BAD_ARGUMENT;
    const std::vector<int64_t> &b = h->tree.partition_bounds();
    if (b.empty() || static_cast<size_t>(world) + 1 != b.size()) return BBFMM_BAD_ARGUMENT;
    std::copy(b.begin(), b.end(), bounds_out);
    return BBFMM_OK;
}
int bbfmm_matvec_partition_finish_sorted(bbfmm_handle *h, const double *d_coarse, double *d_seg, int64_t ld, void *comm_stream) {
    GUARD(h)
    if (refuse_group(h, kExchangeIsTheLibrarys)) return BBFMM_BAD_ARGUMENT;
    return h->tree.matvec_partition_finish_sorted(d_coarse, d_seg, ld, static_cast<hipStream_t>(comm_stream));
    END_GUARD(h)
}
int bbfmm_partition_scatter(bbfmm_handle *h, const double *d_all, int32_t first_part, int32_t n_parts, int64_t m_max, int32_t k,
                            double *d_out, int64_t ldo) {
    GUARD(h)
    if (refuse_group(h, kExchangeIsTheLibrarys)) return BBFMM_BAD_ARGUMENT;
    return h->tree.partition_scatter(d_all, first_part, n_parts, m_max, k, d_out, ldo);
    END_GUARD(h)
}
int bbfmm_matvec_partition_finish(bbfmm_handle *h, const double *d_coarse, double *d_out, int64_t ldo, int32_t sync, void *comm_stream) {
    GUARD(h)
    if (refuse_group(h, kExchangeIsTheLibrarys)) return BBFMM_BAD_ARGUMENT;
    return h->tree.matvec_partition_finish(d_coarse, d_out, ldo, sync != 0, static_cast<hipStream_t>(comm_stream));
    END_GUARD(h)
}

int bbfmm_debug_partition_upward_counts(const bbfmm_handle *h, int64_t *counts_out, uint8_t *reads_out, int64_t *info_out) {
    if (!h || !counts_out || !reads_out || !info_out) return BBFMM_BAD_ARGUMENT;
    return h->tree.debug_partition_upward_counts(counts_out, reads_out, info_out);
}

int bbfmm_get_tree_stats(const bbfmm_handle *h, bbfmm_tree_stats *out) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    h->tree.stats(out);
    return BBFMM_OK;
}

int bbfmm_last_evaluate_at_sources(const bbfmm_handle *h) {
    if (!h) return 0;
    if (h->group && h->group->last_path()) return h->group->last_path(); // 1: partitioned at the sources, 3: targets sharded over the parts
    return h->tree.last_evaluate_path();
}
int bbfmm_tree_built_on_device(const bbfmm_handle *h) { return (h && h->tree.tree_built_on_device()) ? 1 : 0; }

int bbfmm_get_cells(const bbfmm_handle *h, uint64_t *keys, uint8_t *is_leaf) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    const auto &t = h->tree.tree();
    if (keys) std::memcpy(keys, t.key.data(), t.key.size() * sizeof(uint64_t));
    if (is_leaf) std::memcpy(is_leaf, t.is_leaf.data(), t.is_leaf.size());
    return BBFMM_OK;
}

int bbfmm_get_leaf_sources(const bbfmm_handle *h, int64_t *ptr, int64_t *idx) {
    if (!h || !ptr || !idx) return BBFMM_BAD_ARGUMENT;
    const auto &t = h->tree.tree();
    const int64_t C = t.n_cells();
    int64_t cur = 0;
    for (int64_t c = 0; c < C; ++c) {
        ptr[c] = cur;
        if (t.is_leaf[c])
            for (int64_t q = t.pt_begin[c]; q < t.pt_end[c]; ++q) idx[cur++] = t.order[q];
    }
    ptr[C] = cur;
    return BBFMM_OK;
}

int bbfmm_get_list(const bbfmm_handle *h, char which, int64_t *ptr, int32_t *idx, int64_t *n_entries) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    const auto &t = h->tree.tree();
    const bbfmm::Csr *l = nullptr;
    switch (which) {
    case 'U': case 'u': l = &t.u; break;
    case 'V': case 'v': l = &t.v; break;
    case 'W': case 'w': l = &t.w; break;
    case 'X': case 'x': l = &t.x; break;
    default: return BBFMM_BAD_ARGUMENT;
    }
    if (n_entries) *n_entries = static_cast<int64_t>(l->idx.size());
    if (ptr) std::memcpy(ptr, l->ptr.data(), l->ptr.size() * sizeof(int64_t));
    if (idx && !l->idx.empty()) std::memcpy(idx, l->idx.data(), l->idx.size() * sizeof(int32_t));
    return BBFMM_OK;
}

int bbfmm_get_m2l_ranks(const bbfmm_handle *h, int32_t *ranks, int32_t *n_ref_out) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    const auto &o = h->tree.ops();
    if (n_ref_out) *n_ref_out = o.n_ref;
    if (ranks)
        for (size_t level = 0; level < o.m2l.size(); ++level)
            for (int r = 0; r < o.n_ref; ++r)
                ranks[level * o.n_ref + r] = o.m2l[level].empty() ? 0 : o.m2l[level][r].rank;
    return BBFMM_OK;
}

int bbfmm_get_m2l_operator(const bbfmm_handle *h, int32_t level, int32_t ref, double *out) {
    if (!h || !out) return BBFMM_BAD_ARGUMENT;
    const auto &o = h->tree.ops();
    if (level < 2 || level >= static_cast<int>(o.m2l.size()) || ref < 0 || ref >= o.n_ref) return BBFMM_BAD_ARGUMENT;
    const auto &op = o.m2l[level][ref];
    const int n = o.n;
    if (op.vt.empty()) {
        std::memcpy(out, op.u.data(), sizeof(double) * n * n);
        return BBFMM_OK;
    }
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int k = 0; k < op.rank; ++k) s += op.u[static_cast<size_t>(k) * n + i] * op.vt[static_cast<size_t>(j) * op.rank + k];
            out[static_cast<size_t>(j) * n + i] = s;
        }
    return BBFMM_OK;
}

int bbfmm_get_m2l_factors(const bbfmm_handle *h, int32_t level, int32_t ref, double *u, double *vt) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    const auto &o = h->tree.ops();
    if (level < 2 || level >= static_cast<int>(o.m2l.size()) || ref < 0 || ref >= o.n_ref) return BBFMM_BAD_ARGUMENT;
    const auto &op = o.m2l[level][ref];
    if (u) std::memcpy(u, op.u.data(), op.u.size() * sizeof(double));
    if (vt && !op.vt.empty()) std::memcpy(vt, op.vt.data(), op.vt.size() * sizeof(double));
    return BBFMM_OK;
}

int bbfmm_get_permutation_tables(const bbfmm_handle *h, int32_t *n_perm, int32_t *perm, int32_t *invperm,
                                 int32_t *perm_lookup, int32_t *ref_lookup) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    const auto &o = h->tree.ops();
    if (n_perm) *n_perm = o.n_perm;
    if (perm) std::memcpy(perm, o.perm.data(), o.perm.size() * sizeof(int32_t));
    if (invperm) std::memcpy(invperm, o.invperm.data(), o.invperm.size() * sizeof(int32_t));
    if (perm_lookup) std::memcpy(perm_lookup, o.perm_lookup.data(), o.perm_lookup.size() * sizeof(int32_t));
    if (ref_lookup) std::memcpy(ref_lookup, o.ref_lookup.data(), o.ref_lookup.size() * sizeof(int32_t));
    return BBFMM_OK;
}

int bbfmm_points_to_leaves(const bbfmm_handle *h, const double *x, int64_t m, int64_t ldx, int32_t *cell_out,
                           int64_t *bad_point_index) {
    if (!h || (m > 0 && (!x || !cell_out)) || ldx < m) return BBFMM_BAD_ARGUMENT;
    const int64_t bad = bbfmm::points_to_leaves(h->tree.tree(), x, m, ldx, cell_out);
    if (bad >= 0) {
        if (bad_point_index) *bad_point_index = bad;
        return BBFMM_POINT_OUTSIDE_TREE;
    }
    return BBFMM_OK;
}

int bbfmm_set_profiling(bbfmm_handle *h, int32_t enable) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    if (h->group) h->group->set_profiling(enable != 0);
    else h->tree.set_profiling(enable != 0);
    return BBFMM_OK;
}

int bbfmm_get_phase_ms(bbfmm_handle *h, double *ms_out, int64_t *count_out) {
    if (!h || !ms_out) return BBFMM_BAD_ARGUMENT;
    h->tree.bind_device();
    std::memcpy(ms_out, h->tree.phase_ms(), sizeof(double) * BBFMM_N_PHASES);
    if (count_out) std::memcpy(count_out, h->tree.phase_count(), sizeof(int64_t) * BBFMM_N_PHASES);
    return BBFMM_OK;
}

int bbfmm_reset_phase_ms(bbfmm_handle *h) {
    if (!h) return BBFMM_BAD_ARGUMENT;
    if (h->group) h->group->reset_phase_ms();
    else h->tree.reset_phase_ms();
    return BBFMM_OK;
}

} // extern "C"
